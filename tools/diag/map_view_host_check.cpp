// Stand-alone check of the host form of the map view (atdn_vslam_amd/csrc/map_view_host.h) for sanitizer builds; needs no input
// file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/map_view_host_check.cpp -o check
//   ./check
// Points, poses and every output sit in exactly sized heap blocks, so a read or write past either end is caught. Closed forms
// (5 x 7, fx = fy = 4, principal point on pixel (3, 2), R = I, size 0.25: a point at z = 2 has hx = splat / 4 before the clamp):
// the half-open footprint with both ends on integers, footprints half outside each border and wholly outside by one pixel, the
// max_splat cap, a footprint larger than the image and an infinite one, near and far and the next doubles outside them, a point
// behind the camera, equal depths (better support, then smaller colour), NaN and infinities in a point and in every slot of a
// pose, M = 0, no colours; then pseudo-random clouds at 5 x 7, 9 x 33 and 47 x 154 rendered in two point orders, which must agree.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/map_view_host.h"

using namespace atdn;

static const float EYE[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

struct Image {
  int B, H, W;
  float* depth;
  unsigned char *colors, *support;
  int64_t* counts;
  Image(int B_, int H_, int W_, bool colored = true) : B(B_), H(H_), W(W_) {
    const size_t n = (size_t)B * H * W;
    depth = new float[n];
    colors = colored ? new unsigned char[3 * n] : nullptr;
    support = new unsigned char[n];
    counts = new int64_t[3 * B];
  }
  ~Image() { delete[] depth; delete[] colors; delete[] support; delete[] counts; }
  bool same(const Image& o) const {
    const size_t n = (size_t)B * H * W;
    return !memcmp(depth, o.depth, 4 * n) && !memcmp(support, o.support, n) && !memcmp(counts, o.counts, 24 * B) &&
           (!colors || !memcmp(colors, o.colors, 3 * n));
  }
  long covered() const { long c = 0; for (size_t i = 0; i < (size_t)B * H * W; ++i) c += depth[i] != 0.0f; return c; }
};

struct Cloud {
  int M;
  float* pts;
  unsigned char* rgb;
  int* n;
  explicit Cloud(int M_) : M(M_), pts(new float[3 * M_]), rgb(new unsigned char[3 * M_]), n(new int[M_]) {
    for (int i = 0; i < M; ++i) { n[i] = 1; rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = 0; }
  }
  ~Cloud() { delete[] pts; delete[] rgb; delete[] n; }
  // the point seen at pixel coordinates (u, v) and depth z by the hand camera
  void at(int i, double u, double v, double z) {
    pts[3 * i] = (float)((u - 3.0) / 4.0 * z);
    pts[3 * i + 1] = (float)((v - 2.0) / 4.0 * z);
    pts[3 * i + 2] = (float)z;
  }
};

static int fail(const char* what) { fprintf(stderr, "FAILED: %s\n", what); return 1; }

static ViewParams hand(double splat = 1.0, int max_splat = 64) {
  return view_params(4.0, 4.0, 3.0, 2.0, 0.25, splat, max_splat, 0.5, 40.0, 1, 5, 7);
}

// renders `c` with the hand camera (or `pose`); true iff exactly the pixels rows r0..r1 x columns c0..c1 are covered
static bool box_is(const Cloud& c, const ViewParams& p, int r0, int r1, int c0, int c1, const float* pose = EYE, int64_t visible = 1) {
  float* P = new float[12];
  memcpy(P, pose, 48);
  Image im(1, 5, 7);
  view_render_host(c.pts, c.rgb, c.n, c.M, P, 1, p, im.depth, im.colors, im.support, im.counts);
  delete[] P;
  bool ok = im.counts[0] == c.M && im.counts[1] == visible;
  long area = 0;
  for (int y = 0; y < 5; ++y)
    for (int x = 0; x < 7; ++x) {
      const bool in = y >= r0 && y <= r1 && x >= c0 && x <= c1;
      area += in;
      ok = ok && (im.depth[y * 7 + x] != 0.0f) == in && (im.support[y * 7 + x] != 0) == in;
    }
  return ok && im.counts[2] == area;
}

static int closed_forms() {
  int bad = 0;
  Cloud one(1);
  one.at(0, 2.5, 1.5, 2.0);
  if (!box_is(one, hand(), 1, 1, 2, 2)) bad += fail("half-open footprint");
  const double border[4][6] = {{0, 2, 1, 3, 0, 1}, {6, 2, 1, 3, 5, 6}, {3, 0, 0, 1, 2, 4}, {3, 4, 3, 4, 2, 4}};
  for (auto& b : border) {
    one.at(0, b[0], b[1], 2.0);
    if (!box_is(one, hand(6.0), (int)b[2], (int)b[3], (int)b[4], (int)b[5])) bad += fail("half outside a border");
  }
  const double outside[4][2] = {{-1, 2}, {7, 2}, {3, -1}, {3, 5}};
  for (auto& o : outside) {
    one.at(0, o[0], o[1], 2.0);
    if (!box_is(one, hand(), 1, 0, 1, 0, EYE, 0)) bad += fail("wholly outside");
  }
  one.at(0, 3.0, 2.0, 2.0);
  if (!box_is(one, hand(6.0, 2), 1, 2, 2, 3)) bad += fail("max_splat");
  if (!box_is(one, hand(100.0), 0, 4, 0, 6)) bad += fail("larger than the image");
  if (!box_is(one, hand(1e300, 1 << 20), 0, 4, 0, 6)) bad += fail("infinite footprint");
  // near, far and the next doubles outside them (R = I: z = (double)p_z - (double)t_z exactly)
  Cloud two(2);
  two.at(0, 3.0, 2.0, 0.5);
  two.at(1, 5.0, 2.0, 40.0);
  {
    float P[12];
    Image im(1, 5, 7);
    const ViewParams p = hand(0.5);
    memcpy(P, EYE, 48);
    view_render_host(two.pts, two.rgb, two.n, 2, P, 1, p, im.depth, im.colors, im.support, im.counts);
    if (im.counts[1] != 2 || im.depth[2 * 7 + 3] != 0.5f || im.depth[2 * 7 + 5] != 40.0f) bad += fail("near and far are inside");
    P[11] = ldexpf(1.0f, -54);
    view_render_host(two.pts, two.rgb, two.n, 2, P, 1, p, im.depth, im.colors, im.support, im.counts);
    if (im.counts[1] != 1 || im.depth[2 * 7 + 3] != 0.0f || im.depth[2 * 7 + 5] != 40.0f) bad += fail("below near");
    P[11] = -ldexpf(1.0f, -47);
    view_render_host(two.pts, two.rgb, two.n, 2, P, 1, p, im.depth, im.colors, im.support, im.counts);
    if (im.counts[1] != 1 || im.depth[2 * 7 + 3] != 0.5f || im.depth[2 * 7 + 5] != 0.0f) bad += fail("above far");
  }
  one.at(0, 3.0, 2.0, -2.0);
  if (!box_is(one, hand(), 1, 0, 1, 0, EYE, 0)) bad += fail("behind the camera");
  // equal depths: the better supported point, then the smaller colour, in either order
  for (int order = 0; order < 2; ++order) {
    Cloud eq(2);
    eq.at(0, 3.0, 2.0, 2.0);
    eq.at(1, 3.0, 2.0, 2.0);
    float* P = new float[12];
    memcpy(P, EYE, 48);
    Image im(1, 5, 7);
    eq.n[order] = 2; eq.n[1 - order] = 5;
    eq.rgb[3 * order] = 1; eq.rgb[3 * (1 - order)] = 9;
    view_render_host(eq.pts, eq.rgb, eq.n, 2, P, 1, hand(), im.depth, im.colors, im.support, im.counts);
    if (im.support[2 * 7 + 3] != 5 || im.colors[2 * 7 + 3] != 9) bad += fail("better support wins");
    eq.n[order] = 300; eq.n[1 - order] = 255;
    eq.rgb[3 * order] = 4; eq.rgb[3 * (1 - order)] = 3; eq.rgb[3 * (1 - order) + 2] = 255;
    view_render_host(eq.pts, eq.rgb, eq.n, 2, P, 1, hand(), im.depth, im.colors, im.support, im.counts);
    if (im.support[2 * 7 + 3] != 255 || im.colors[2 * 7 + 3] != 3 || im.colors[2 * 35 + 2 * 7 + 3] != 255) bad += fail("smaller colour wins");
    delete[] P;
  }
  // NaN and infinities: in a point, and in every slot of a pose
  const float specials[3] = {NAN, INFINITY, -INFINITY};
  for (float s : specials) {
    for (int a = 0; a < 3; ++a) {
      one.at(0, 3.0, 2.0, 2.0);
      one.pts[a] = s;
      if (!box_is(one, hand(), 1, 0, 1, 0, EYE, 0)) bad += fail("special value in a point");
    }
    one.at(0, 3.0, 2.0, 2.0);
    for (int k = 0; k < 12; ++k) {
      float P[12];
      memcpy(P, EYE, 48);
      P[k] = s;
      if (!box_is(one, hand(100.0), 1, 0, 1, 0, P, 0)) bad += fail("special value in a pose");
    }
  }
  // M = 0 and no colours
  {
    float* P = new float[12];
    memcpy(P, EYE, 48);
    Image im(1, 5, 7, false);
    view_render_host(nullptr, nullptr, nullptr, 0, P, 1, hand(), im.depth, nullptr, im.support, im.counts);
    if (im.covered() || im.counts[0] || im.counts[1] || im.counts[2]) bad += fail("M = 0");
    view_render_host(one.pts, nullptr, one.n, 1, P, 1, hand(), im.depth, nullptr, im.support, im.counts);
    if (im.covered() != 1 || im.counts[2] != 1) bad += fail("no colours");
    delete[] P;
  }
  if (!bad) printf("closed forms ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int H, int W, int B) {
  const int M = 4 * H * W;
  Cloud a(M), b(M);
  unsigned r = 977u + (unsigned)(H * W);
  for (int i = 0; i < M; ++i) {
    a.pts[3 * i] = -6.0f + 0.001f * (float)(lcg(r) % 12000);
    a.pts[3 * i + 1] = -2.0f + 0.001f * (float)(lcg(r) % 4000);
    a.pts[3 * i + 2] = -1.0f + 0.01f * (float)(lcg(r) % 4500);
    a.n[i] = 1 + (int)(lcg(r) % 300);
    for (int k = 0; k < 3; ++k) a.rgb[3 * i + k] = (unsigned char)lcg(r);
  }
  for (int i = 0; i < M; ++i) {                                    // the same set in reverse order
    const int j = M - 1 - i;
    memcpy(b.pts + 3 * i, a.pts + 3 * j, 12);
    memcpy(b.rgb + 3 * i, a.rgb + 3 * j, 3);
    b.n[i] = a.n[j];
  }
  float* poses = new float[12 * B];
  for (int k = 0; k < B; ++k) {
    const float P[12] = {1, 0, 0.02f * k, 0.3f * k, 0, 1, 0, -0.1f, -0.02f * k, 0, 1, -2.0f + 0.7f * k};
    memcpy(poses + 12 * k, P, sizeof P);
  }
  int bad = 0;
  for (int min_count = 1; min_count <= 3; min_count += 2)
    for (double splat : {0.5, 1.0, 2.0}) {
      const ViewParams p = view_params(4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 0.25, splat, 64, 0.5, 40.0,
                                       min_count, H, W);
      Image x(B, H, W), y(B, H, W), z(B, H, W, false);
      view_render_host(a.pts, a.rgb, a.n, M, poses, B, p, x.depth, x.colors, x.support, x.counts);
      view_render_host(b.pts, b.rgb, b.n, M, poses, B, p, y.depth, y.colors, y.support, y.counts);
      view_render_host(a.pts, nullptr, a.n, M, poses, B, p, z.depth, nullptr, z.support, z.counts);
      if (!x.same(y)) bad += fail("order invariance");
      if (memcmp(x.depth, z.depth, 4 * (size_t)B * H * W) || x.covered() != x.counts[2] + (B > 1 ? x.counts[5] : 0) + (B > 2 ? x.counts[8] : 0))
        bad += fail("depth without colours, covered count");
      if (min_count == 1 && splat == 1.0)
        printf("random %d x %d, B = %d: camera 0 counts (%ld, %ld, %ld)\n", H, W, B, (long)x.counts[0], (long)x.counts[1], (long)x.counts[2]);
    }
  delete[] poses;
  return bad;
}

int main() {
  int bad = closed_forms();
  bad += random_case(5, 7, 1);
  bad += random_case(9, 33, 3);
  bad += random_case(47, 154, 2);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
