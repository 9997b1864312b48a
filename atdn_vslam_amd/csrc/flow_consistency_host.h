// Forward-backward consistency of a pair of flows, the rule in plain C++ float64 (no HIP needed): flow_consistent_pixel is the
// rule for one pixel, flow_consistency_host the host form behind atdn_flow_consistency_host (flow_consistency.hip), which serves CPU
// tensors. The kernel of flow_consistency.hip evaluates the same function, so the two cannot drift apart; the independent
// statement the tests compare both with is tests/flow_consistency_ref.py (NumPy).
//
// The check is the one of UnFlow (Meister et al., AAAI 2018, eq. 2) and ARFlow: follow the forward flow from (x, y), read the
// backward flow there (bilinear), and ask that the round trip returns to the start within alpha1 * (|fw|^2 + |bw|^2) + alpha2.
//
// flow_fw, flow_bw [2, H, W] float32, channel 0 = x. For pixel (x, y), everything in float64, every operation rounded on its
// own (fp contraction off), in exactly this order:
//   x1 = x + fw_x, y1 = y + fw_y                                  (exact in float64)
//   inside, b = bilinear_flow(flow_bw at (x1, y1))                (pixel_rule.h states it line by line: the closed inside test,
//                                                                  four taps always read, the order of the products and sums);
//                                                                  not inside: mask 0, nothing more is read
//   sx = fw_x + b_x, sy = fw_y + b_y, diff = sx*sx + sy*sy
//   mag = (fw_x*fw_x + fw_y*fw_y) + (b_x*b_x + b_y*b_y), thr = alpha1*mag + alpha2
//   mask = inside && diff <= thr && diff <= DBL_MAX               (plain comparisons: any NaN gives 0)
// The last clause only matters for an infinite flow_bw tap of non-zero weight, where diff = thr = +inf and `diff <= thr` alone
// would call the pixel consistent; with finite float32 inputs diff is finite (|v| < 3.5e38, squares < 1.2e77) and the clause is
// always true.
#pragma once
#include <cfloat>
#include <cmath>

#include "pixel_rule.h"

namespace atdn {

// fw_x, fw_y: the forward flow at (x, y); bx, by: the two planes [H * W] of the backward flow.
ATDN_HD inline bool flow_consistent_pixel(float fw_x, float fw_y, const float* bx, const float* by, int H, int W, int x, int y,
                                          double alpha1, double alpha2) {
#pragma clang fp contract(off)
  const double fx = (double)fw_x, fy = (double)fw_y;
  const double x1 = (double)x + fx, y1 = (double)y + fy;
  double b[2];
  if (!bilinear_flow(x1, y1, bx, by, H, W, b)) return false;
  const double sx = fx + b[0], sy = fy + b[1];
  const double sxx = sx * sx, syy = sy * sy;
  const double diff = sxx + syy;
  const double fxx = fx * fx, fyy = fy * fy, bxx = b[0] * b[0], byy = b[1] * b[1];
  const double mf = fxx + fyy, mb = bxx + byy;
  const double mag = mf + mb;
  const double scaled = alpha1 * mag;
  const double thr = scaled + alpha2;
  return diff <= thr && diff <= DBL_MAX;
}

// mask [B, 1, H, W] uint8 (1 = consistent), count [B] = the number of ones of each mask.
inline void flow_consistency_host(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                                  unsigned char* mask, int* count) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    const float* fx = flow_fw + (long)b * 2 * n;
    const float* fy = fx + n;
    const float* bx = flow_bw + (long)b * 2 * n;
    const float* by = bx + n;
    unsigned char* m = mask + (long)b * n;
    int ones = 0;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long i = (long)y * W + x;
        const bool ok = flow_consistent_pixel(fx[i], fy[i], bx, by, H, W, x, y, alpha1, alpha2);
        m[i] = ok ? 1 : 0;
        ones += ok ? 1 : 0;
      }
    count[b] = ones;
  }
}

}  // namespace atdn
