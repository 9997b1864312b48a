// Stand-alone check of the host form of the pose-from-flow rule (atdn_vslam_amd/csrc/epipolar_host.h) for sanitizer builds; needs
// no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/epipolar_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. A scene of depths 5 .. 25 seen
// from two cameras (R = a rotation about y, t = (0.1, -0.05, 0.8)) at 9 x 33 (B = 3: odd planes) and 47 x 154 (B = 2: 8 chunks, a
// ragged last one) with a mask and one NaN flow: from a start 0.02 rad off with t turned towards (0.25, -0.15, 0.9), 16 steps must
// bring the direction of t within 1e-3 degrees of the true one and keep t.t to 1e-6, with every candidate an inlier; a plane whose
// start has t = 0 must return the bits of its start pose; the evaluation alone (iters = 0) must equal epipolar_terms_host.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/epipolar_host.h"

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int run(int B, int H, int W) {
  const size_t n = (size_t)H * W;
  float* flow = new float[B * 2 * n];
  unsigned char* mask = new unsigned char[B * n];
  float* truth = new float[B * 12];
  float* start = new float[B * 12];
  float* out = new float[B * 12];
  double* cost = new double[B];
  int* counts = new int[B * 4];
  double* sums = new double[B * atdn::PLANE_TERMS];
  int* counts3 = new int[B * 3];
  const double fx = 0.58 * W, fy = 0.58 * W, cx = (W - 1) / 2.0 + 0.3, cy = (H - 1) / 2.0 - 0.2;
  const atdn::EpipolarParams cam = atdn::epipolar_params(fx, fy, cx, cy, 2.0, 1.0);
  unsigned s = 777u + (unsigned)n;
  for (int b = 0; b < B; ++b) {
    const double a = 0.01 * (b + 1), a2 = a + 0.02;                    // rotations about y
    const float P[12] = {(float)cos(a), 0, (float)sin(a), 0.1f, 0, 1, 0, -0.05f, (float)-sin(a), 0, (float)cos(a), 0.8f};
    const float S[12] = {(float)cos(a2), 0, (float)sin(a2), 0.25f, 0, 1, 0, -0.15f, (float)-sin(a2), 0, (float)cos(a2), 0.9f};
    memcpy(truth + 12 * b, P, sizeof P);
    memcpy(start + 12 * b, S, sizeof S);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = b * n + (size_t)y * W + x;
        const double z = 5.0 + 20.0 * (lcg(s) % 1000) / 1000.0;
        const double D[3] = {z * (x - cx) / fx - P[3], z * (y - cy) / fy - P[7], z - P[11]};      // X1 - t
        const double X = P[0] * D[0] + P[4] * D[1] + P[8] * D[2], Y = P[1] * D[0] + P[5] * D[1] + P[9] * D[2],
                     Z = P[2] * D[0] + P[6] * D[1] + P[10] * D[2];                                // R^T (X1 - t)
        flow[(2 * b) * n + (size_t)y * W + x] = (float)(fx * X / Z + cx - x);
        flow[(2 * b + 1) * n + (size_t)y * W + x] = (float)(fy * Y / Z + cy - y);
        mask[i] = (lcg(s) % 10) < 8 ? (unsigned char)(1 + lcg(s) % 255) : 0;
      }
    flow[(2 * b) * n + n / 2] = NAN;
  }
  if (B > 1) start[12 + 3] = start[12 + 7] = start[12 + 11] = 0.0f;    // plane 1 starts with t = 0
  for (int i = 0; i < B * 12; ++i) out[i] = -7.0f;
  atdn::epipolar_solve_host(flow, mask, start, B, H, W, cam, 16, out, cost, counts);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const float* o = out + 12 * b;
    if (B > 1 && b == 1) {
      if (memcmp(o, start + 12 * b, 48) != 0 || counts[4 * b + 1] != 0 || counts[4 * b + 3] != 0 || cost[b] != 0.0) {
        printf("%dx%d plane %d: t = 0 did not return the start pose\n", H, W, b);
        ++bad;
      }
      continue;
    }
    const float* p = truth + 12 * b;
    const float* q = start + 12 * b;
    const double c[3] = {(double)o[7] * p[11] - (double)o[11] * p[7], (double)o[11] * p[3] - (double)o[3] * p[11],
                         (double)o[3] * p[7] - (double)o[7] * p[3]};
    const double dot = (double)o[3] * p[3] + (double)o[7] * p[7] + (double)o[11] * p[11];
    const double deg = atan2(sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), dot) * 57.29577951308232;
    const double tt_in = (double)q[3] * q[3] + (double)q[7] * q[7] + (double)q[11] * q[11];
    const double tt_out = (double)o[3] * o[3] + (double)o[7] * o[7] + (double)o[11] * o[11];
    printf("%dx%d plane %d: direction error %.3g deg, t.t %.9g -> %.9g, counts %d %d %d %d, cost %.3g\n", H, W, b, deg, tt_in, tt_out,
           counts[4 * b], counts[4 * b + 1], counts[4 * b + 2], counts[4 * b + 3], cost[b]);
    if (!(deg < 1e-3) || !(fabs(tt_out / tt_in - 1.0) < 1e-6) || counts[4 * b + 2] != counts[4 * b] || counts[4 * b + 3] < 1 ||
        counts[4 * b] <= 0)
      ++bad;
  }
  atdn::epipolar_terms_host(flow, mask, start, B, H, W, cam, sums, counts3);
  atdn::epipolar_solve_host(flow, mask, start, B, H, W, cam, 0, out, cost, counts);
  for (int b = 0; b < B; ++b)
    if (memcmp(out + 12 * b, start + 12 * b, 48) != 0 || memcmp(&cost[b], &sums[atdn::PLANE_TERMS * b + 27], 8) != 0 ||
        memcmp(counts + 4 * b, counts3 + 3 * b, 12) != 0 || counts[4 * b + 3] != 0) {
      printf("%dx%d plane %d: iters = 0 is not the evaluation alone\n", H, W, b);
      ++bad;
    }
  delete[] flow; delete[] mask; delete[] truth; delete[] start; delete[] out; delete[] cost; delete[] counts; delete[] sums;
  delete[] counts3;
  return bad;
}

int main() {
  const int bad = run(3, 9, 33) + run(2, 47, 154);
  printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
