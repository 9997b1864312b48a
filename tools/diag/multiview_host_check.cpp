// Stand-alone check of the host form of the multi-view depth rule (atdn_vslam_amd/csrc/multiview_depth_host.h) for sanitizer
// builds; needs no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/multiview_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed form (6 x 24, fx = fy =
// 64, integer principal point, R = I): a fronto-parallel plane at depth 8 seen from three frames 0.5, 1.0 and 1.5 to the side
// (4, 8 and 12 px of disparity, everything exact). View k sees the columns x >= 4 (k + 1); with min_views = 2 the columns
// x >= 8 are candidates, depth = 8 and info = sum of (8 t_k)^2 over the views that see the pixel: 80 for 8 <= x < 12, 224 beyond.
// The same with empty slots (-1, N) among the views, with an initial depth (right, wrong, a hole), with a NaN and an infinity in
// one view's flow (that view drops out at that pixel: x >= 12 keeps two views, info 224 - (8 t_k)^2), S = 16 with repeated views,
// and pseudo-random flows at 5 x 7 and 9 x 33: counts ordered, valid = non-zero depth = non-zero info, views <= S.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/multiview_depth_host.h"

using atdn::MultiviewParams;

struct Run {
  int N, B, S, H, W;
  float *acc, *poses, *init, *depth, *info;
  unsigned char *alive, *views;
  int *slots, *counts;
  Run(int N_, int B_, int S_, int H_, int W_) : N(N_), B(B_), S(S_), H(H_), W(W_) {
    const size_t n = (size_t)H * W;
    acc = new float[N * 2 * n]();
    alive = new unsigned char[N * n];
    poses = new float[N * 12];
    slots = new int[(size_t)B * S];
    init = new float[B * n]();
    depth = new float[B * n];
    info = new float[B * n];
    views = new unsigned char[B * n];
    counts = new int[B * 3];
    memset(alive, 1, N * n);
    for (int k = 0; k < N; ++k) {
      const float P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      memcpy(poses + 12 * k, P, sizeof P);
    }
  }
  ~Run() {
    delete[] acc; delete[] alive; delete[] poses; delete[] slots; delete[] init; delete[] depth; delete[] info; delete[] views;
    delete[] counts;
  }
  void go(const MultiviewParams& c, bool with_init) {
    const size_t n = (size_t)H * W;
    for (size_t i = 0; i < B * n; ++i) { depth[i] = -7.0f; info[i] = -9.0f; views[i] = 99; }
    for (int i = 0; i < B * 3; ++i) counts[i] = -12345;
    atdn::multiview_depth_host(acc, alive, poses, slots, with_init ? init : nullptr, N, B, S, H, W, c, depth, info, views, counts);
  }
};

static int expect(const char* name, const Run& r, int b, int cand, int solved, int valid) {
  const int* c = r.counts + 3 * b;
  if (c[0] == cand && c[1] == solved && c[2] == valid) return 0;
  fprintf(stderr, "%s b=%d: counts (%d, %d, %d), expected (%d, %d, %d)\n", name, b, c[0], c[1], c[2], cand, solved, valid);
  return 1;
}

static bool close_to(double a, double b, double rel) { return fabs(a - b) <= rel * fabs(b); }

static MultiviewParams params(int H, int W, int iters, int min_views) {
  return atdn::multiview_params(64.0, 64.0, 5.0, 2.0, 4.0, 2.0, 0.1, min_views, 0.25, 80.0, iters, H, W);
}

static int plane_cases() {
  const int H = 6, W = 24, N = 3;
  const size_t n = (size_t)H * W;
  int bad = 0;
  // problem 0: the three views; problem 1: the same among empty slots; problem 2: view 2 alone, twice
  Run r(N, 3, 5, H, W);
  for (int k = 0; k < N; ++k) {
    r.poses[12 * k + 3] = 0.5f * (k + 1);
    for (size_t i = 0; i < n; ++i) r.acc[(2 * k) * n + i] = -4.0f * (k + 1);
  }
  const int slots[3][5] = {{0, 1, 2, -1, -1}, {-1, 0, N, 1, 2}, {2, N + 7, -3, 2, -1}};
  memcpy(r.slots, slots, sizeof slots);
  for (int pass = 0; pass < 2; ++pass) {
    for (size_t i = 0; i < 3 * n; ++i) r.init[i] = i % 3 == 0 ? 8.0f : (i % 3 == 1 ? 2.0f : 0.0f);
    r.go(params(H, W, 4, 2), pass == 1);
    bad += expect("plane", r, 0, H * 16, H * 16, H * 16);
    bad += expect("empty slots", r, 1, H * 16, H * 16, H * 16);
    bad += expect("one view twice", r, 2, H * 12, H * 12, H * 12);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        for (int b = 0; b < 3; ++b) {
          const size_t i = b * n + (size_t)y * W + x;
          const int nv = b == 2 ? (x >= 12 ? 2 : 0) : (x >= 12 ? 3 : (x >= 8 ? 2 : 0));
          const double ri = b == 2 ? 288.0 : (nv == 3 ? 224.0 : 80.0);
          const bool ok = nv == 0 ? (r.depth[i] == 0.0f && r.info[i] == 0.0f && r.views[i] == 0)
                                  : (close_to(r.depth[i], 8.0, 1e-6) && close_to(r.info[i], ri, 1e-6) && r.views[i] == nv);
          if (!ok) { if (!bad) fprintf(stderr, "plane b=%d (%d, %d): depth %g info %g views %d\n", b, x, y, r.depth[i], r.info[i], r.views[i]); ++bad; }
        }
  }
  // a NaN and an infinity in one view's flow: that view drops out there
  r.acc[(2 * 1) * n + 2 * W + 20] = NAN;
  r.acc[(2 * 0 + 1) * n + 3 * W + 21] = INFINITY;
  r.go(params(H, W, 4, 2), false);
  bad += expect("nan / inf", r, 0, H * 16, H * 16, H * 16);
  if (r.views[2 * W + 20] != 2 || !close_to(r.info[2 * W + 20], 224.0 - 64.0, 1e-6) || !close_to(r.depth[2 * W + 20], 8.0, 1e-6)) ++bad;
  if (r.views[3 * W + 21] != 2 || !close_to(r.info[3 * W + 21], 224.0 - 16.0, 1e-6) || !close_to(r.depth[3 * W + 21], 8.0, 1e-6)) ++bad;
  // S = 16: every view several times; iters = 0 and min_views = 16
  Run w(N, 1, 16, H, W);
  memcpy(w.acc, r.acc, sizeof(float) * N * 2 * n);
  memcpy(w.poses, r.poses, sizeof(float) * N * 12);
  w.acc[(2 * 1) * n + 2 * W + 20] = -8.0f;
  w.acc[(2 * 0 + 1) * n + 3 * W + 21] = 0.0f;
  for (int s = 0; s < 16; ++s) w.slots[s] = s % N;
  w.go(params(H, W, 0, 16), false);
  bad += expect("S = 16", w, 0, H * 12, H * 12, H * 12);
  if (!bad) printf("closed forms ok\n");
  return bad;
}

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int random_case(int H, int W) {
  const int N = 5, B = 2, S = 4;
  const size_t n = (size_t)H * W;
  Run r(N, B, S, H, W);
  unsigned s = 4321u + (unsigned)(H * W);
  for (int k = 0; k < N; ++k) {
    const float P[12] = {1, 0, 0.01f * k, 0.05f * k, 0, 1, 0, -0.02f, -0.01f * k, 0, 1, 0.3f * (k + 1)};
    memcpy(r.poses + 12 * k, P, sizeof P);
    for (size_t i = 0; i < 2 * n; ++i) r.acc[2 * k * n + i] = 0.02f * (float)(lcg(s) % 200) - 2.0f;
    for (size_t i = 0; i < n; ++i) r.alive[k * n + i] = (lcg(s) % 8) == 0 ? 0 : (unsigned char)(1 + lcg(s) % 200);
  }
  for (int i = 0; i < B * S; ++i) r.slots[i] = (int)(lcg(s) % (N + 2)) - 1;                      // -1 .. N: empty slots among them
  for (size_t i = 0; i < B * n; ++i) r.init[i] = (lcg(s) % 3) == 0 ? 0.0f : 1.0f + 0.1f * (float)(lcg(s) % 300);
  MultiviewParams c = atdn::multiview_params(4.0 * W / 7.0, 4.0 * W / 7.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2, 4.0, 2.0, 0.1, 1,
                                             50.0, 80.0, 4, H, W);
  r.go(c, true);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    int valid = 0;
    for (size_t i = 0; i < n; ++i) {
      const float z = r.depth[b * n + i], f = r.info[b * n + i];
      valid += z != 0.0f;
      if ((z != 0.0f) != (f != 0.0f) || r.views[b * n + i] > S || (z != 0.0f && (r.views[b * n + i] < 1 || !(z > 0.0f && z <= 80.0f)))) ++bad;
    }
    const int* q = r.counts + 3 * b;
    if (q[2] != valid || !(0 <= q[2] && q[2] <= q[1] && q[1] <= q[0] && q[0] <= (int)n)) ++bad;
    printf("random %d x %d problem %d: counts (%d, %d, %d)\n", H, W, b, q[0], q[1], q[2]);
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
