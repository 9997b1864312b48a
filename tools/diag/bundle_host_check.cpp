// Stand-alone check of the host form of the windowed bundle adjustment (atdn_vslam_amd/csrc/bundle_host.h) for sanitizer
// builds; needs no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/bundle_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. Closed form (12 x 24, fx = fy
// = 64, R = I): a fronto-parallel plane at depth 8 seen from S frames that stand 0.1 (k + 1) to the side and 0.05 (k + 1) ahead,
// flows exact in float64 and rounded to float32. From the true poses the cost stays below 1e-9 per candidate; from poses shifted
// by a few centimetres the cost falls and ends below 1e-6 of where it began. Also: empty slots (-1, N) among the views, stride 1,
// 2 and 5, S = 1 and S = 16 (the full-width system), a mask, a zero translation in the gauge view (outputs = inputs), and
// pseudo-random flows (counts ordered, outputs finite or zero). Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/bundle_host.h"

struct Run {
  int N, B, S, H, W;
  float *acc, *poses, *init, *poses_out, *depth;
  unsigned char *alive, *mask;
  int *slots, *counts;
  double *cost, *sums;
  Run(int N_, int B_, int S_, int H_, int W_) : N(N_), B(B_), S(S_), H(H_), W(W_) {
    const size_t n = (size_t)H * W;
    acc = new float[N * 2 * n]();
    alive = new unsigned char[N * n];
    mask = new unsigned char[B * n];
    poses = new float[N * 12];
    slots = new int[(size_t)B * S];
    init = new float[B * n];
    poses_out = new float[(size_t)B * S * 12];
    depth = new float[B * n];
    cost = new double[B * 2];
    counts = new int[B * 4];
    sums = new double[(size_t)B * atdn::ba_sums(S)];
    memset(alive, 1, N * n);
    memset(mask, 1, B * n);
    for (size_t i = 0; i < B * n; ++i) init[i] = 8.0f;
    for (int b = 0; b < B; ++b)
      for (int s = 0; s < S; ++s) slots[b * S + s] = s % N;
  }
  ~Run() {
    delete[] acc; delete[] alive; delete[] mask; delete[] poses; delete[] slots; delete[] init; delete[] poses_out; delete[] depth;
    delete[] cost; delete[] counts; delete[] sums;
  }
  // the plane at depth 8 seen from frame k at (0.1 (k + 1), 0, 0.05 (k + 1)); `shift` is added to every stored translation
  void plane(double fx, double cx, double cy, float shift) {
    const size_t n = (size_t)H * W;
    for (int k = 0; k < N; ++k) {
      const double tx = 0.1 * (k + 1), tz = 0.05 * (k + 1);
      const float P[12] = {1, 0, 0, (float)tx + shift, 0, 1, 0, shift, 0, 0, 1, (float)tz + shift};
      memcpy(poses + 12 * k, P, sizeof P);
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const double X = 8.0 * (x - cx) / fx - tx, Y = 8.0 * (y - cy) / fx, Z = 8.0 - tz;
          acc[(2 * k) * n + y * W + x] = (float)(fx * X / Z + cx - x);
          acc[(2 * k + 1) * n + y * W + x] = (float)(fx * Y / Z + cy - y);
        }
    }
  }
  void go(const atdn::BundleParams& c, bool masked) {
    const size_t n = (size_t)H * W;
    for (size_t i = 0; i < B * n; ++i) depth[i] = -7.0f;
    for (size_t i = 0; i < (size_t)B * S * 12; ++i) poses_out[i] = -5.0f;
    for (int i = 0; i < B * 4; ++i) counts[i] = -12345;
    atdn::bundle_adjust_host(acc, alive, poses, slots, init, masked ? mask : nullptr, N, B, S, H, W, c, poses_out, depth, cost, counts);
    atdn::bundle_terms_host(acc, alive, poses, slots, init, masked ? mask : nullptr, N, B, S, H, W, c, sums, counts + 0);
    atdn::bundle_adjust_host(acc, alive, poses, slots, init, masked ? mask : nullptr, N, B, S, H, W, c, poses_out, depth, cost, counts);
  }
};

static int fail(const char* what, double a, double b) {
  fprintf(stderr, "%s: %g %g\n", what, a, b);
  return 1;
}

int main() {
  int bad = 0;
  const int H = 12, W = 24;
  const double fx = 64.0, cx = 11.0, cy = 5.0;
  for (int S : {1, 3, 16})
    for (int stride : {1, 2, 5}) {
      const atdn::BundleParams c = atdn::bundle_params(fx, fx, cx, cy, 4.0, 2.0, 0.1, 1, 10, stride, H, W);
      Run r(S, 2, S, H, W);
      r.plane(fx, cx, cy, 0.0f);
      if (S >= 3) { r.slots[1] = -1; r.slots[S + 2] = S; }
      r.go(c, false);
      for (int b = 0; b < 2; ++b) {
        if (r.counts[4 * b] < 1) bad += fail("no candidates", r.counts[4 * b], S);
        if (!(r.cost[2 * b + 1] <= r.cost[2 * b]) || r.cost[2 * b + 1] > 1e-9 * r.counts[4 * b]) bad += fail("exact cost", r.cost[2 * b], r.cost[2 * b + 1]);
      }
      r.plane(fx, cx, cy, 0.03f);
      for (int b = 0; b < 2; ++b)
        for (size_t i = 0; i < (size_t)H * W; i += 7) r.mask[(size_t)b * H * W + i] = 0;
      r.go(c, true);
      for (int b = 0; b < 2; ++b) {
        if (r.counts[4 * b + 3] < 1) bad += fail("no accepted step", b, S);
        if (!(r.cost[2 * b + 1] < 1e-6 * r.cost[2 * b])) bad += fail("shifted cost", r.cost[2 * b], r.cost[2 * b + 1]);
        for (size_t i = 0; i < (size_t)H * W; i += 7)
          if (r.depth[(size_t)b * H * W + i] != 0.0f) bad += fail("masked pixel has a depth", (double)i, r.depth[(size_t)b * H * W + i]);
      }
      // zero translation in the gauge view: nothing is solved
      for (int k = 0; k < r.N; ++k) r.poses[12 * k + 3] = r.poses[12 * k + 7] = r.poses[12 * k + 11] = 0.0f;
      r.go(c, false);
      for (int b = 0; b < 2; ++b) {
        if (r.counts[4 * b + 3] != 0 || r.cost[2 * b] != r.cost[2 * b + 1]) bad += fail("zero gauge", r.counts[4 * b + 3], r.cost[2 * b + 1]);
        for (int s = 0; s < S; ++s) {
          const int k = r.slots[b * S + s];
          for (int i = 0; i < 12; ++i) {
            const float want = k >= 0 && k < r.N ? r.poses[12 * k + i] : 0.0f;
            if (r.poses_out[(b * S + s) * 12 + i] != want) bad += fail("zero gauge pose", s, i);
          }
        }
      }
      // pseudo-random flows and liveness
      unsigned seed = 12345u + 77u * S + stride;
      for (size_t i = 0; i < (size_t)r.N * 2 * H * W; ++i) {
        seed = seed * 1664525u + 1013904223u;
        r.acc[i] = ((int)(seed >> 8) % 2001 - 1000) * 0.01f;
      }
      for (size_t i = 0; i < (size_t)r.N * H * W; ++i) {
        seed = seed * 1664525u + 1013904223u;
        r.alive[i] = (seed >> 12) % 5 != 0;
      }
      r.plane(fx, cx, cy, 0.0f);   // poses again (the flows stay random: plane() rewrites them, so draw them after)
      for (size_t i = 0; i < (size_t)r.N * 2 * H * W; ++i) {
        seed = seed * 1664525u + 1013904223u;
        r.acc[i] += ((int)(seed >> 8) % 601 - 300) * 0.01f;
      }
      r.go(c, true);
      for (int b = 0; b < 2; ++b) {
        const int* n = r.counts + 4 * b;
        if (n[2] > n[1] || n[1] > n[0] * S || n[3] < 0 || n[3] > 10) bad += fail("counts out of order", n[1], n[2]);
        if (!(r.cost[2 * b + 1] <= r.cost[2 * b])) bad += fail("random cost", r.cost[2 * b], r.cost[2 * b + 1]);
        for (size_t i = 0; i < (size_t)H * W; ++i)
          if (!(r.depth[(size_t)b * H * W + i] >= 0.0f)) bad += fail("depth", (double)i, r.depth[(size_t)b * H * W + i]);
      }
    }
  printf(bad ? "FAILED: %d\n" : "bundle host check ok\n", bad);
  return bad ? 1 : 0;
}
