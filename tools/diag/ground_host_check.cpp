// Stand-alone check of the host form of the ground-plane rule (atdn_vslam_amd/csrc/ground_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/ground_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. A road 1.65 m below a camera
// pitched by 2 degrees, under a wall in the upper half of the band, at 5 x 7 (B = 1: one ragged chunk, the default rows), 9 x 33
// (B = 3: odd planes, the band (1, 9)) and 47 x 154 (B = 2: 8 chunks) with a mask, depth holes, a NaN, an infinity and a negative
// depth: from the vote and 8 steps the height must come back within 2 % where the road has enough pixels, ground_terms_host at
// the result must give the solve's sums and counts, ground_classify_host must flag exactly the solve's inliers and leave the rows
// outside the band zero; a plane of zero depth must give q = 0 and zero counts; q_init must give bin -1.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/ground_host.h"

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int run(int B, int H, int W, int y0, int y1, bool accurate) {
  const size_t n = (size_t)H * W;
  float* depth = new float[B * n];
  unsigned char* mask = new unsigned char[B * n];
  double* q = new double[B * 3];
  double* q2 = new double[B * 3];
  double* sums = new double[B * atdn::GROUND_TERMS];
  double* sums2 = new double[B * atdn::GROUND_TERMS];
  int* counts = new int[B * 6];
  int* counts3 = new int[B * 3];
  float* residual = new float[B * n];
  unsigned char* on = new unsigned char[B * n];
  const double fx = 0.58 * W, fy = 0.58 * W, cx = (W - 1) / 2.0 + 0.3, cy = (H - 1) / 2.0 - 0.2;
  const double pitch = 2.0 * 3.14159265358979 / 180.0, ny = std::cos(pitch), nz = std::sin(pitch), h = 1.65;
  const atdn::GroundParams c = atdn::ground_params(fx, fy, cx, cy, 0.05, 0.05, 0.1, 80.0, 0.0, 1.0, 0.0, 3, y0, W);
  unsigned s = 4242u + (unsigned)n;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = b * n + (size_t)y * W + x;
        const double na = ny * (y - cy) / fy + nz;
        double z = na > 1e-6 ? h / na : 1e9;
        if (z > 12.0) z = 12.0 - 0.01 * x;                                // the wall
        depth[i] = (lcg(s) % 10) < 1 ? 0.0f : (float)z;
        mask[i] = (lcg(s) % 10) < 9 ? (unsigned char)(1 + lcg(s) % 255) : 0;
      }
  depth[n - 1] = NAN;
  depth[n - 2] = INFINITY;
  depth[n - 3] = -1.0f;
  if (B > 1) memset(depth + n, 0, n * sizeof(float));                     // plane 1 has no depth at all
  for (int i = 0; i < B * 3; ++i) q[i] = -7.0;
  atdn::ground_solve_host(depth, mask, nullptr, B, H, W, y1, c, 8, q, sums, counts);
  atdn::ground_terms_host(depth, mask, q, B, H, W, y1, c, sums2, counts3);
  atdn::ground_classify_host(depth, mask, q, B, H, W, y1, c, residual, on);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const int* k = counts + 6 * b;
    if (B > 1 && b == 1) {
      if (q[3] != 0.0 || q[4] != 0.0 || q[5] != 0.0 || k[0] || k[1] || k[2] || k[3] || k[4] || k[5]) ++bad;
      continue;
    }
    const double norm = std::sqrt(q[3 * b] * q[3 * b] + q[3 * b + 1] * q[3 * b + 1] + q[3 * b + 2] * q[3 * b + 2]);
    printf("%d x %d b=%d: counts (%d, %d, %d), %d accepted, %d votes in bin %d, height %.4f\n", H, W, b, k[0], k[1], k[2], k[3], k[4],
           k[5], 1.0 / norm);
    if (k[4] < 3 || k[1] <= 0 || k[1] > k[0]) ++bad;
    if (accurate && !(std::fabs(1.0 / norm - h) <= 0.02 * h)) ++bad;
    if (memcmp(sums + atdn::GROUND_TERMS * b, sums2 + atdn::GROUND_TERMS * b, 8 * atdn::GROUND_TERMS) != 0) ++bad;
    if (memcmp(k, counts3 + 3 * b, 12) != 0) ++bad;
    int flagged = 0;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = b * n + (size_t)y * W + x;
        flagged += on[i];
        if ((y < y0 || y >= y1) && (on[i] != 0 || residual[i] != 0.0f)) ++bad;
      }
    if (flagged != k[2]) ++bad;
  }
  for (int b = 0; b < B; ++b) { q2[3 * b] = 0.0; q2[3 * b + 1] = 1.0 / (1.05 * h); q2[3 * b + 2] = 0.01; }
  atdn::ground_solve_host(depth, nullptr, q2, B, H, W, y1, c, 0, q, sums, counts);
  for (int b = 0; b < B; ++b)
    if (memcmp(q + 3 * b, q2 + 3 * b, 24) != 0 || counts[6 * b + 3] != 0 || counts[6 * b + 4] != 0 || counts[6 * b + 5] != -1) ++bad;
  delete[] depth; delete[] mask; delete[] q; delete[] q2; delete[] sums; delete[] sums2; delete[] counts; delete[] counts3;
  delete[] residual; delete[] on;
  if (bad) fprintf(stderr, "%d x %d B = %d: %d mismatches\n", H, W, B, bad);
  return bad;
}

int main() {
  int bad = run(1, 5, 7, 2, 5, false) + run(3, 9, 33, 1, 9, false) + run(2, 47, 154, 0, 47, true);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
