// Stand-alone check of the host form of the flow-consistency rule (atdn_vslam_amd/csrc/flow_consistency_host.h) for sanitizer
// builds; needs no input file:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/diag/flow_consistency_host_check.cpp -o check
//   ./check
// Cases with counts known in closed form at 5 x 7 (B = 1) and 9 x 33 (B = 3: H * W = 297 is odd, so the planes of b = 1, 2 start
// at odd offsets). Inputs and outputs sit in exactly sized heap blocks, so a read or write past either end is caught.
//   constant flow fw = (dx, dy), bw = -fw: consistent exactly where the target stays inside, (W - |dx|) * (H - |dy|) pixels,
//     also for fractional (dx, dy) — every tap then holds -fw and the interpolation returns it exactly (weights sum to 1 with a
//     power-of-two fraction);
//   zero flows: all ones;  bw = +fw at magnitude 5: all zeros;  fw = NaN everywhere: all zeros.
// Exit status 0 = every count and every mask byte is the expected one and no sanitizer report.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../atdn_vslam_amd/csrc/flow_consistency_host.h"

static int run(int B, int H, int W, float fx, float fy, float bx, float by, int x_lo, int x_hi, int y_lo, int y_hi, const char* name) {
  const size_t n = (size_t)H * W;
  float* fw = new float[B * 2 * n];
  float* bw = new float[B * 2 * n];
  unsigned char* mask = new unsigned char[B * n];
  int* count = new int[B];
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < n; ++i) {
      fw[(2 * b) * n + i] = fx; fw[(2 * b + 1) * n + i] = fy;
      bw[(2 * b) * n + i] = bx; bw[(2 * b + 1) * n + i] = by;
    }
  memset(mask, 0xFF, B * n);
  for (int b = 0; b < B; ++b) count[b] = -12345;
  atdn::flow_consistency_host(fw, bw, B, H, W, 0.01, 0.5, mask, count);
  int bad = 0;
  const int want = (x_hi - x_lo) * (y_hi - y_lo);
  for (int b = 0; b < B; ++b) {
    if (count[b] != want) { fprintf(stderr, "%s %dx%d b=%d: count %d, expected %d\n", name, H, W, b, count[b], want); ++bad; }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int w = x >= x_lo && x < x_hi && y >= y_lo && y < y_hi;
        if (mask[b * n + (size_t)y * W + x] != w) { if (!bad) fprintf(stderr, "%s %dx%d b=%d: mask differs at (%d, %d)\n", name, H, W, b, x, y); ++bad; }
      }
  }
  delete[] fw; delete[] bw; delete[] mask; delete[] count;
  if (!bad) printf("%s %d x %d B = %d: %d ones per image, ok\n", name, H, W, B, want);
  return bad;
}

int main() {
  int bad = 0;
  const int shapes[2][3] = {{1, 5, 7}, {3, 9, 33}};
  for (const auto& s : shapes) {
    const int B = s[0], H = s[1], W = s[2];
    bad += run(B, H, W, 0.f, 0.f, 0.f, 0.f, 0, W, 0, H, "zero");
    bad += run(B, H, W, 3.f, -2.f, -3.f, 2.f, 0, W - 3, 2, H, "const(3,-2)");
    bad += run(B, H, W, -1.5f, 2.25f, 1.5f, -2.25f, 2, W, 0, H - 3, "const(-1.5,2.25)");   // x >= 1.5, y <= H - 1 - 2.25
    bad += run(B, H, W, (float)(W - 1), (float)(H - 1), -(float)(W - 1), -(float)(H - 1), 0, 1, 0, 1, "to-the-corner");
    bad += run(B, H, W, 3.f, 4.f, 3.f, 4.f, 0, 0, 0, 0, "contradicting");
    bad += run(B, H, W, NAN, 0.f, 0.f, 0.f, 0, 0, 0, 0, "nan");
  }
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("all cases ok\n");
  return 0;
}
