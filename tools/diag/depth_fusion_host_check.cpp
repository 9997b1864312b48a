// Stand-alone check of the host form of the depth-fusion rule (atdn_vslam_amd/csrc/depth_fusion_host.h) for sanitizer builds; needs
// no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/depth_fusion_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed forms (6 x 12, fx = fy =
// 64, integer principal point, R = I everywhere):
//   a fronto-parallel plane at depth 8 seen by three cameras 0.5 apart sideways (4 px of disparity, everything exact): target 1
//   with sources (0, 2) — columns 4 .. 7 are seen by both, 0 .. 3 and 8 .. 11 by one: views 2 / 1, min_views = 2 keeps H * 4 pixels,
//   fused = 8 —; the same with source 2's plane at depth 8.4 (5 % off: inconsistent, but seen);
//   empty slots (-1, N, the target itself) around the sources: the same outputs; S = 0; a target outside the bank: zeros;
//   a NaN and an infinity in the target's depth: that pixel alone drops out.
// Pseudo-random depths with holes at 5 x 7 and 9 x 33 (N = 4, all targets, small motions): counts ordered, kept = non-zero fused,
// views <= S, no depth where the target has none.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/depth_fusion_host.h"

using atdn::DepthFuseParams;

struct Run {
  int N, B, S, H, W;
  float *bank, *poses, *fused;
  int *targets, *sources, *counts;
  unsigned char* views;
  Run(int N_, int B_, int S_, int H_, int W_) : N(N_), B(B_), S(S_), H(H_), W(W_) {
    const size_t n = (size_t)H * W;
    bank = new float[N * n];
    poses = new float[N * 12];
    targets = new int[B];
    sources = new int[(size_t)B * S];                         // S = 0: a zero-sized block, never read
    fused = new float[B * n];
    views = new unsigned char[B * n];
    counts = new int[B * 3];
    for (int k = 0; k < N; ++k) {
      const float P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      memcpy(poses + 12 * k, P, sizeof P);
    }
  }
  ~Run() { delete[] bank; delete[] poses; delete[] targets; delete[] sources; delete[] fused; delete[] views; delete[] counts; }
  void go(const DepthFuseParams& c) {
    const size_t n = (size_t)H * W;
    for (size_t i = 0; i < B * n; ++i) { fused[i] = -7.0f; views[i] = 99; }
    for (int i = 0; i < B * 3; ++i) counts[i] = -12345;
    atdn::depth_fuse_host(bank, poses, targets, sources, N, B, S, H, W, c, fused, views, counts);
  }
};

static int expect(const char* name, const Run& r, int b, int has, int seen, int kept) {
  const int* c = r.counts + 3 * b;
  if (c[0] == has && c[1] == seen && c[2] == kept) return 0;
  fprintf(stderr, "%s b=%d: counts (%d, %d, %d), expected (%d, %d, %d)\n", name, b, c[0], c[1], c[2], has, seen, kept);
  return 1;
}

static int plane_cases() {
  const int H = 6, W = 12, N = 3;
  const size_t n = (size_t)H * W;
  const DepthFuseParams c = atdn::depth_fuse_params(64.0, 64.0, 5.0, 2.0, 1.0, 0.01, 2, 0.1, 1);
  int bad = 0;
  // sources padded with empty slots: 7 slots, two of them real
  Run r(N, 3, 7, H, W);
  for (int k = 0; k < N; ++k) {
    r.poses[12 * k + 3] = 0.5f * k;
    for (size_t i = 0; i < n; ++i) r.bank[k * n + i] = 8.0f;
  }
  const int src[3][7] = {{-1, 0, N, 1, 2, -5, 1}, {1, 0, -1, 2, N + 3, 1, -1}, {N, N, N, -1, -1, 1, 1}};
  r.targets[0] = 1; r.targets[1] = N; r.targets[2] = 1;
  memcpy(r.sources, src[1], sizeof src[1]);
  memcpy(r.sources + 7, src[0], sizeof src[0]);
  memcpy(r.sources + 14, src[2], sizeof src[2]);
  r.go(c);
  bad += expect("plane", r, 0, H * W, H * W, H * 4);
  bad += expect("outside", r, 1, 0, 0, 0);
  bad += expect("no source", r, 2, H * W, 0, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      const int both = x >= 4 && x <= 7;
      if (r.views[i] != (both ? 2 : 1) || r.fused[i] != (both ? 8.0f : 0.0f)) { if (!bad) fprintf(stderr, "plane: pixel (%d, %d): views %d fused %g\n", x, y, r.views[i], r.fused[i]); ++bad; }
      if (r.views[n + i] != 0 || r.fused[n + i] != 0.0f || r.views[2 * n + i] != 0 || r.fused[2 * n + i] != 0.0f) ++bad;
    }
  // source 2 five per cent off: seen, never consistent; min_views = 1 keeps what source 0 sees
  for (size_t i = 0; i < n; ++i) r.bank[2 * n + i] = 8.4f;
  r.go(atdn::depth_fuse_params(64.0, 64.0, 5.0, 2.0, 1.0, 0.01, 1, 0.1, 0));
  bad += expect("one off", r, 0, H * W, H * W, H * 8);
  // a NaN and an infinity in the target's own depth
  for (size_t i = 0; i < n; ++i) r.bank[2 * n + i] = 8.0f;
  r.bank[n + 2 * W + 5] = NAN;
  r.bank[n + 3 * W + 6] = INFINITY;
  r.go(c);
  bad += expect("nan / inf", r, 0, H * W - 1, H * W - 2, H * 4 - 2);
  // S = 0
  Run z(N, 1, 0, H, W);
  for (size_t i = 0; i < N * n; ++i) z.bank[i] = 8.0f;
  z.targets[0] = 0;
  z.go(c);
  bad += expect("S = 0", z, 0, H * W, 0, 0);
  if (!bad) printf("closed forms ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int H, int W) {
  const int N = 4, S = 5;
  const size_t n = (size_t)H * W;
  Run r(N, N, S, H, W);
  unsigned s = 4321u + (unsigned)(H * W);
  for (int k = 0; k < N; ++k) {
    const float P[12] = {1, 0, 0.01f * k, 0.05f * k, 0, 1, 0, -0.02f, -0.01f * k, 0, 1, 0.02f * k};
    memcpy(r.poses + 12 * k, P, sizeof P);
    for (size_t i = 0; i < n; ++i) r.bank[k * n + i] = (lcg(s) % 10) == 0 ? 0.0f : 10.0f + 0.0005f * (float)(lcg(s) % 100);
    r.targets[k] = k;
    for (int j = 0; j < S; ++j) r.sources[k * S + j] = j - 1 + (int)(lcg(s) % 2) * 3;      // -1 .. 5: empty slots among them
  }
  r.go(atdn::depth_fuse_params(4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 1.0, 0.01, 1, 0.1, 1));
  int bad = 0;
  for (int b = 0; b < N; ++b) {
    int has = 0, kept = 0;
    for (size_t i = 0; i < n; ++i) {
      const float z = r.bank[b * n + i], f = r.fused[b * n + i];
      has += z > 0.0f;
      kept += f != 0.0f;
      if (r.views[b * n + i] > S || (z == 0.0f && (f != 0.0f || r.views[b * n + i] != 0)) || (f != 0.0f && r.views[b * n + i] < 1)) ++bad;
    }
    const int* c = r.counts + 3 * b;
    if (c[0] != has || c[2] != kept || !(0 <= c[2] && c[2] <= c[1] && c[1] <= c[0])) ++bad;
    printf("random %d x %d target %d: counts (%d, %d, %d)\n", H, W, b, c[0], c[1], c[2]);
  }
  if (bad) fprintf(stderr, "random %d x %d: %d mismatches\n", H, W, bad);
  return bad;
}

int main() {
  int bad = plane_cases();
  bad += random_case(5, 7);
  bad += random_case(9, 33);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
