// Stand-alone check of the host form of the two-view rule (atdn_vslam_amd/csrc/two_view_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/two_view_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed forms (6 x 12):
//   R = I, t = (0.5, 0, 0), fx = 64, flow (-4, 0): the plane at depth 8 — H * (W - 4) pixels inside, all inliers, all valid, depth 8;
//   the same with flow (+4, 0): behind the cameras — inliers, no depth;   flow (-4, 2): 2 px off the line — no inliers;
//   t = 0: nothing is an inlier;   a flow that leaves the image: nothing inside;   NaN flow: nothing inside;
//   zero flow, t = (0, 0, 1): parallel rays — inliers except at the epipole, no depth even with min_sin2 = 0.
// Pseudo-random flows at 5 x 7 (B = 1) and 9 x 33 (B = 3: H * W = 297 is odd, so the planes of b = 1, 2 start at odd offsets), with
// and without a mask: the counts are ordered, counts[2] is the number of non-zero depths, masked pixels have none, and the masked
// run equals the unmasked one on the kept pixels.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/two_view_host.h"

using atdn::TwoViewCamera;

static int closed(const char* name, float u, float v, float t0, float t1, float t2, const TwoViewCamera& cam, int want_inside,
                  int want_inlier, int want_valid, float want_depth) {
  const int B = 2, H = 6, W = 12;
  const size_t n = (size_t)H * W;
  float* flow = new float[B * 2 * n];
  float* pose = new float[B * 12];
  float* depth = new float[B * n];
  int* counts = new int[B * 3];
  for (int b = 0; b < B; ++b) {
    for (size_t i = 0; i < n; ++i) { flow[(2 * b) * n + i] = u; flow[(2 * b + 1) * n + i] = v; }
    const float P[12] = {1, 0, 0, t0, 0, 1, 0, t1, 0, 0, 1, t2};
    memcpy(pose + 12 * b, P, sizeof P);
  }
  for (size_t i = 0; i < B * n; ++i) depth[i] = -7.0f;
  for (int i = 0; i < B * 3; ++i) counts[i] = -12345;
  atdn::two_view_depth_host(flow, pose, nullptr, B, H, W, cam, depth, counts);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    if (counts[3 * b] != want_inside || counts[3 * b + 1] != want_inlier || counts[3 * b + 2] != want_valid) {
      fprintf(stderr, "%s b=%d: counts (%d, %d, %d), expected (%d, %d, %d)\n", name, b, counts[3 * b], counts[3 * b + 1],
              counts[3 * b + 2], want_inside, want_inlier, want_valid);
      ++bad;
    }
    int nonzero = 0;
    for (size_t i = 0; i < n; ++i) {
      const float d = depth[b * n + i];
      if (d != 0.0f) {
        ++nonzero;
        if (!(std::fabs(d - want_depth) <= want_depth * 1.2e-7f)) { if (!bad) fprintf(stderr, "%s: depth %g, expected %g\n", name, d, want_depth); ++bad; }
      }
    }
    if (nonzero != want_valid) { fprintf(stderr, "%s b=%d: %d non-zero depths, expected %d\n", name, b, nonzero, want_valid); ++bad; }
  }
  delete[] flow; delete[] pose; delete[] depth; delete[] counts;
  if (!bad) printf("%s: (%d, %d, %d) per image, ok\n", name, want_inside, want_inlier, want_valid);
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int B, int H, int W) {
  const size_t n = (size_t)H * W;
  float* flow = new float[B * 2 * n];
  float* pose = new float[B * 12];
  unsigned char* mask = new unsigned char[B * n];
  float* depth = new float[B * n];
  float* depth_m = new float[B * n];
  int* counts = new int[B * 3];
  int* counts_m = new int[B * 3];
  unsigned s = 12345u + (unsigned)(H * W);
  const TwoViewCamera cam{4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 1.0, 7.6e-7, 80.0};
  for (int b = 0; b < B; ++b) {
    const float P[12] = {1, 0, 0.01f, 0.05f * (b + 1), 0, 1, 0, -0.02f, -0.01f, 0, 1, 1.0f};
    memcpy(pose + 12 * b, P, sizeof P);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        // roughly the radial flow of forward motion over depths of 3 .. 30, plus up to +-0.75 px
        const double z = 3.0 + 27.0 * (lcg(s) % 1000) / 1000.0;
        flow[(2 * b) * n + i] = (float)((x - cam.cx) / (z - 1.0) + ((int)(lcg(s) % 1500) - 750) / 1000.0);
        flow[(2 * b + 1) * n + i] = (float)((y - cam.cy) / (z - 1.0) + ((int)(lcg(s) % 1500) - 750) / 1000.0);
        mask[b * n + i] = (lcg(s) % 10) < 6 ? (unsigned char)(1 + lcg(s) % 255) : 0;
      }
  }
  atdn::two_view_depth_host(flow, pose, nullptr, B, H, W, cam, depth, counts);
  atdn::two_view_depth_host(flow, pose, mask, B, H, W, cam, depth_m, counts_m);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    int nz = 0, nz_m = 0;
    for (size_t i = 0; i < n; ++i) {
      nz += depth[b * n + i] != 0.0f;
      nz_m += depth_m[b * n + i] != 0.0f;
      const float want = mask[b * n + i] ? depth[b * n + i] : 0.0f;
      if (memcmp(&want, &depth_m[b * n + i], 4) != 0) ++bad;
    }
    const int* c = counts + 3 * b;
    const int* m = counts_m + 3 * b;
    if (!(0 <= c[2] && c[2] <= c[1] && c[1] <= c[0] && c[0] <= (int)n) || nz != c[2]) ++bad;
    if (!(0 <= m[2] && m[2] <= m[1] && m[1] <= m[0] && m[0] <= c[0]) || nz_m != m[2] || m[1] > c[1]) ++bad;
    printf("random %d x %d b=%d: counts (%d, %d, %d), masked (%d, %d, %d)\n", H, W, b, c[0], c[1], c[2], m[0], m[1], m[2]);
  }
  delete[] flow; delete[] pose; delete[] mask; delete[] depth; delete[] depth_m; delete[] counts; delete[] counts_m;
  if (bad) fprintf(stderr, "random %d x %d B = %d: %d mismatches\n", H, W, B, bad);
  return bad;
}

int main() {
  int bad = 0;
  const int H = 6, W = 12;
  const TwoViewCamera cam{64.0, 64.0, 5.0, 2.0, 1.0, 7.6e-7, 80.0};
  bad += closed("plane", -4.f, 0.f, 0.5f, 0.f, 0.f, cam, H * (W - 4), H * (W - 4), H * (W - 4), 8.0f);
  bad += closed("behind", 4.f, 0.f, 0.5f, 0.f, 0.f, cam, H * (W - 4), H * (W - 4), 0, 0.0f);
  bad += closed("off-line", -4.f, 2.f, 0.5f, 0.f, 0.f, cam, (H - 2) * (W - 4), 0, 0, 0.0f);
  bad += closed("t=0", -4.f, 0.f, 0.f, 0.f, 0.f, cam, H * (W - 4), 0, 0, 0.0f);
  bad += closed("leaving", (float)W, 0.f, 0.5f, 0.f, 0.f, cam, 0, 0, 0, 0.0f);
  bad += closed("nan", NAN, 0.f, 0.5f, 0.f, 0.f, cam, 0, 0, 0, 0.0f);
  bad += closed("inf", 0.f, INFINITY, 0.5f, 0.f, 0.f, cam, 0, 0, 0, 0.0f);
  TwoViewCamera par = cam;
  par.min_sin2 = 0.0;
  bad += closed("parallel", 0.f, 0.f, 0.f, 0.f, 1.f, par, H * W, H * W - 1, 0, 0.0f);
  bad += random_case(1, 5, 7);
  bad += random_case(3, 9, 33);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
