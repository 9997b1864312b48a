// Stand-alone check of the host form of the pose-from-depth rule (atdn_vslam_amd/csrc/pnp_host.h) for sanitizer builds; needs no
// input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/pnp_host_check.cpp -o check
//   ./check
// Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught. A plane of depths 5 .. 25 seen
// from two cameras (R = a rotation about y, t = (0.1, -0.05, 0.8)) at 9 x 33 (B = 3: odd planes), 47 x 154 (B = 2: 8 chunks, a ragged
// last one) with a mask, depth holes and one NaN flow: from a start 0.02 rad and 0.2 m off, 16 steps must come back within 1e-4 m
// of the true translation, with every candidate an inlier; a plane of zero depth must return the bits of its start pose; the
// evaluation alone (iters = 0) must equal pnp_terms_host.
// Exit status 0 = every expectation met and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/pnp_host.h"

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int run(int B, int H, int W) {
  const size_t n = (size_t)H * W;
  float* depth = new float[B * n];
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
  const atdn::PnpParams cam = atdn::pnp_params(fx, fy, cx, cy, 4.0, 2.0, 0.1, H, W);
  unsigned s = 777u + (unsigned)n;
  for (int b = 0; b < B; ++b) {
    const double a = 0.01 * (b + 1), a2 = a + 0.02;                    // rotations about y
    const float P[12] = {(float)cos(a), 0, (float)sin(a), 0.1f, 0, 1, 0, -0.05f, (float)-sin(a), 0, (float)cos(a), 0.8f};
    const float S[12] = {(float)cos(a2), 0, (float)sin(a2), 0.25f, 0, 1, 0, -0.15f, (float)-sin(a2), 0, (float)cos(a2), 0.9f};
    memcpy(truth + 12 * b, P, sizeof P);
    memcpy(start + 12 * b, S, sizeof S);
    double I[12];
    atdn::pnp_internal_pose(P, I);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = b * n + (size_t)y * W + x;
        const float z = (float)(5.0 + 20.0 * (lcg(s) % 1000) / 1000.0);
        const double X1 = z * (x - cx) / fx, Y1 = z * (y - cy) / fy;
        const double X = I[0] * X1 + I[1] * Y1 + I[2] * z + I[9], Y = I[3] * X1 + I[4] * Y1 + I[5] * z + I[10],
                     Z = I[6] * X1 + I[7] * Y1 + I[8] * z + I[11];
        flow[(2 * b) * n + (size_t)y * W + x] = (float)(fx * X / Z + cx - x);
        flow[(2 * b + 1) * n + (size_t)y * W + x] = (float)(fy * Y / Z + cy - y);
        depth[i] = (lcg(s) % 10) < 2 ? 0.0f : z;
        mask[i] = (lcg(s) % 10) < 8 ? (unsigned char)(1 + lcg(s) % 255) : 0;
      }
    flow[(2 * b) * n + n / 2] = NAN;
  }
  if (B > 1) memset(depth + n, 0, n * sizeof(float));                  // plane 1 has no depth at all
  for (int i = 0; i < B * 12; ++i) out[i] = -7.0f;
  atdn::pnp_solve_host(depth, flow, mask, start, B, H, W, cam, 16, out, cost, counts);
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const int* c = counts + 4 * b;
    if (B > 1 && b == 1) {
      if (memcmp(out + 12 * b, start + 12 * b, 48) != 0 || c[0] || c[1] || c[2] || c[3] || cost[b] != 0.0) ++bad;
      continue;
    }
    double e = 0.0;
    for (int i = 0; i < 3; ++i) e += std::pow((double)out[12 * b + 4 * i + 3] - (double)truth[12 * b + 4 * i + 3], 2);
    printf("%d x %d b=%d: counts (%d, %d, %d), %d accepted, translation error %.2e\n", H, W, b, c[0], c[1], c[2], c[3], std::sqrt(e));
    if (!(std::sqrt(e) <= 1e-4) || c[0] <= 0 || c[2] != c[0] || c[1] != c[0] || c[3] < 1) ++bad;
  }
  atdn::pnp_solve_host(depth, flow, mask, start, B, H, W, cam, 0, out, cost, counts);
  atdn::pnp_terms_host(depth, flow, mask, start, B, H, W, cam, sums, counts3);
  for (int b = 0; b < B; ++b) {
    if (memcmp(out + 12 * b, start + 12 * b, 48) != 0 || memcmp(&cost[b], &sums[atdn::PLANE_TERMS * b + 27], 8) != 0) ++bad;
    if (memcmp(counts + 4 * b, counts3 + 3 * b, 12) != 0 || counts[4 * b + 3] != 0) ++bad;
  }
  delete[] depth; delete[] flow; delete[] mask; delete[] truth; delete[] start; delete[] out; delete[] cost; delete[] counts;
  delete[] sums; delete[] counts3;
  if (bad) fprintf(stderr, "%d x %d B = %d: %d mismatches\n", H, W, B, bad);
  return bad;
}

int main() {
  int bad = run(3, 9, 33) + run(2, 47, 154) + run(1, 5, 7);
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
