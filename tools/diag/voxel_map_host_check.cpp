// Stand-alone check of the host form of the voxel map (atdn_vslam_amd/csrc/voxel_map_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/voxel_map_host_check.cpp -o check
//   ./check
// Tables, inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed form (6 x 24,
// fx = fy = 64, integer principal point, R = I): a fronto-parallel wall at depth 8 seen from two cameras one voxel apart gives
// voxels whose z is 8 + (0 + 0.5)/65536 * voxel exactly and whose counts add up to the pixels. Then: special depths (NaN, +-inf, 0,
// negative), a NaN pose (outside), an index list with a repeat and entries outside the bank, stride 3 with mask and pending, a
// table of 4 slots (drops; candidates == inserted + outside + dropped; pending marks the drops), rehash into 256 slots and a
// retry pass that must equal a table that was large from the start, the ends of the key range, extraction with max_out below the
// number of voxels and with min_count 3, and pseudo-random scenes at 5 x 7 and 9 x 33 split over calls in two orders.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/voxel_map_host.h"

using namespace atdn;

struct Table {
  long cap;
  uint64_t* w;
  explicit Table(long c) : cap(c), w(new uint64_t[voxel_table_words(c)]) { voxel_clear_host(w, cap); }
  ~Table() { delete[] w; }
  int64_t cnt(int i) const { return (int64_t)w[i]; }
  bool consistent() const { return cnt(0) == cnt(1) + cnt(2) + cnt(3); }
};

struct Cloud {
  long max_out, n;
  float* pts;
  unsigned char* rgb;
  int* counts;
  int64_t *keys, found;
  Cloud(const Table& t, int min_count, const VoxelParams& c, long max_out_) : max_out(max_out_) {
    pts = new float[3 * max_out];
    rgb = new unsigned char[3 * max_out];
    counts = new int[max_out];
    keys = new int64_t[max_out];
    voxel_extract_host(t.w, t.cap, min_count, c, max_out, pts, rgb, counts, keys, &found);
    n = found < max_out ? found : max_out;
  }
  ~Cloud() { delete[] pts; delete[] rgb; delete[] counts; delete[] keys; }
  bool same(const Cloud& o) const {
    return n == o.n && found == o.found && !memcmp(pts, o.pts, 12 * n) && !memcmp(rgb, o.rgb, 3 * n) && !memcmp(counts, o.counts, 4 * n) &&
           !memcmp(keys, o.keys, 8 * n);
  }
};

struct Scene {
  int N, H, W;
  float *depth, *poses;
  unsigned char* images;
  Scene(int N_, int H_, int W_) : N(N_), H(H_), W(W_) {
    const size_t n = (size_t)H * W;
    depth = new float[N * n];
    poses = new float[N * 12];
    images = new unsigned char[N * 3 * n];
    for (int k = 0; k < N; ++k) {
      const float P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      memcpy(poses + 12 * k, P, sizeof P);
    }
  }
  ~Scene() { delete[] depth; delete[] poses; delete[] images; }
};

static int fail(const char* what) { fprintf(stderr, "FAILED: %s\n", what); return 1; }

static int wall_cases() {
  const int H = 6, W = 24, N = 3;
  const size_t n = (size_t)H * W;
  int bad = 0;
  Scene s(N, H, W);
  for (size_t i = 0; i < N * n; ++i) s.depth[i] = 8.0f;
  for (size_t i = 0; i < N * 3 * n; ++i) s.images[i] = (unsigned char)(i % 251);
  s.poses[12 + 3] = 0.25f;                                         // camera 1 one voxel to the side
  const VoxelParams c = voxel_params(64.0, 64.0, 5.0, 2.0, 1, 0.25, 0.0, 0.0, 0.0, 0.5, 40.0);
  Table t(256);
  unsigned char* pending = new unsigned char[2 * n];
  voxel_integrate_host(s.depth, s.poses, s.images, nullptr, nullptr, N, 2, H, W, c, 0, t.w, t.cap, pending);
  if (t.cnt(0) != (int64_t)(2 * n) || t.cnt(1) != (int64_t)(2 * n) || t.cnt(2) || t.cnt(3) || !t.consistent()) bad += fail("wall counters");
  for (size_t i = 0; i < 2 * n; ++i) if (pending[i]) { bad += fail("wall pending"); break; }
  {
    Cloud cl(t, 1, c, t.cnt(4));
    long total = 0;
    const float z = (float)(0.0 + (32.0 + (0.0 / 1.0 + 0.5) / 65536.0) * 0.25);
    for (long i = 0; i < cl.n; ++i) {
      total += cl.counts[i];
      if (cl.pts[3 * i + 2] != z) { bad += fail("wall z"); break; }
      if (i && !(cl.keys[i - 1] < cl.keys[i])) { bad += fail("key order"); break; }
    }
    if (cl.found != t.cnt(4) || total != (long)(2 * n)) bad += fail("wall counts");
    Cloud few(t, 1, c, 3), three(t, 3, c, t.cnt(4));
    if (few.found != cl.found || few.n != 3 || memcmp(few.keys, cl.keys, 24)) bad += fail("max_out");
    for (long i = 0; i < three.n; ++i) if (three.counts[i] < 3) { bad += fail("min_count"); break; }
  }
  // special depths, a NaN pose, indices with a repeat and entries outside the bank, stride 3 with a mask
  const float special[5] = {NAN, INFINITY, -INFINITY, 0.0f, -1.0f};
  memcpy(s.depth, special, sizeof special);
  s.poses[24 + 7] = NAN;
  const int idx[5] = {0, 2, 0, -1, N};
  unsigned char* mask = new unsigned char[5 * n];
  unsigned char* pend5 = new unsigned char[5 * n];
  for (size_t i = 0; i < 5 * n; ++i) mask[i] = i % 7 != 0;
  Table u(256);
  voxel_integrate_host(s.depth, s.poses, s.images, mask, idx, N, 5, H, W, c, 0, u.w, u.cap, pend5);
  if (!u.consistent() || u.cnt(2) == 0 || u.cnt(3) != 0) bad += fail("special counters");
  Table v(256);
  const VoxelParams c3 = voxel_params(64.0, 64.0, 5.0, 2.0, 3, 0.25, 0.0, 0.0, 0.0, 0.5, 40.0);
  voxel_integrate_host(s.depth, s.poses, nullptr, mask, idx, N, 5, H, W, c3, 0, v.w, v.cap, nullptr);
  if (!v.consistent() || v.cnt(0) >= u.cnt(0)) bad += fail("stride counters");
  // an undersized table, rehash and retry against a table that was large from the start
  s.poses[24 + 7] = 0.0f;
  for (size_t i = 0; i < N * n; ++i) s.depth[i] = 2.0f + 0.01f * (float)(i % 997);
  Table small(4), grown(256), direct(256);
  unsigned char* p1 = new unsigned char[N * n];
  unsigned char* p2 = new unsigned char[N * n];
  voxel_integrate_host(s.depth, s.poses, s.images, nullptr, nullptr, N, N, H, W, c, 0, small.w, small.cap, p1);
  long marked = 0;
  for (size_t i = 0; i < N * n; ++i) marked += p1[i];
  if (!small.consistent() || small.cnt(3) == 0 || small.cnt(4) != 4 || marked != small.cnt(3)) bad += fail("undersized");
  voxel_rehash_host(small.w, small.cap, grown.w, grown.cap);
  voxel_integrate_host(s.depth, s.poses, s.images, p1, nullptr, N, N, H, W, c, 1, grown.w, grown.cap, p2);
  voxel_integrate_host(s.depth, s.poses, s.images, nullptr, nullptr, N, N, H, W, c, 0, direct.w, direct.cap, p1);
  if (memcmp(grown.w, direct.w, 64) || grown.cnt(3) != 0) bad += fail("retry counters");
  {
    Cloud a(grown, 1, c, 256), b(direct, 1, c, 256);
    if (!a.same(b)) bad += fail("growth");
  }
  // the ends of the key range: one pixel at g = -2^20 (inside), 2^20 (outside)
  Scene e(2, 1, 1);
  e.depth[0] = e.depth[1] = 1.0f;
  e.poses[3] = -262144.0f;
  e.poses[12 + 3] = 262144.0f;
  const VoxelParams ce = voxel_params(1.0, 1.0, 0.0, 0.0, 1, 0.25, 0.0, 0.0, 0.0, 0.5, 40.0);
  Table te(2);
  voxel_integrate_host(e.depth, e.poses, nullptr, nullptr, nullptr, 2, 2, 1, 1, ce, 0, te.w, te.cap, nullptr);
  if (te.cnt(0) != 2 || te.cnt(1) != 1 || te.cnt(2) != 1 || te.cnt(4) != 1) bad += fail("key range");
  delete[] pending; delete[] mask; delete[] pend5; delete[] p1; delete[] p2;
  if (!bad) printf("closed forms ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int H, int W) {
  const int N = 4;
  const size_t n = (size_t)H * W;
  Scene s(N, H, W);
  unsigned r = 4321u + (unsigned)(H * W);
  for (int k = 0; k < N; ++k) {
    const float P[12] = {1, 0, 0.01f * k, -3.0f + 0.05f * k, 0, 1, 0, -0.4f, -0.01f * k, 0, 1, -2.0f + 0.7f * k};
    memcpy(s.poses + 12 * k, P, sizeof P);
  }
  for (size_t i = 0; i < N * n; ++i) s.depth[i] = 0.1f * (float)(lcg(r) % 500);
  for (size_t i = 0; i < N * 3 * n; ++i) s.images[i] = (unsigned char)lcg(r);
  const VoxelParams c = voxel_params(4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 1, 0.25, 0.1, -0.2, 0.3, 0.5,
                                     40.0);
  Table whole(1024);
  voxel_integrate_host(s.depth, s.poses, s.images, nullptr, nullptr, N, N, H, W, c, 0, whole.w, whole.cap, nullptr);
  const int order[4] = {2, 0, 3, 1};
  Table* cur = new Table(256);
  for (int i = 0; i < N; ++i) {                                    // one keyframe per call, the table grown before each
    Table* next = new Table(cur->cap * 4);
    voxel_rehash_host(cur->w, cur->cap, next->w, next->cap);
    delete cur;
    cur = next;
    voxel_integrate_host(s.depth, s.poses, s.images, nullptr, order + i, N, 1, H, W, c, 0, cur->w, cur->cap, nullptr);
  }
  int bad = 0;
  if (!whole.consistent() || memcmp(whole.w, cur->w, 40)) bad += fail("split counters");
  {
    Cloud a(whole, 1, c, whole.cnt(4) ? whole.cnt(4) : 1), b(*cur, 1, c, whole.cnt(4) ? whole.cnt(4) : 1);
    if (!a.same(b)) bad += fail("split invariance");
  }
  printf("random %d x %d: counters (%ld, %ld, %ld, %ld, %ld)\n", H, W, (long)whole.cnt(0), (long)whole.cnt(1), (long)whole.cnt(2),
         (long)whole.cnt(3), (long)whole.cnt(4));
  delete cur;
  return bad;
}

int main() {
  int bad = wall_cases();
  bad += random_case(5, 7);
  bad += random_case(9, 33);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
