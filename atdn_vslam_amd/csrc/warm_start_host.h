// Forward interpolation of a flow field along itself, host form (plain C++, no HIP): the rules of warm_start.hip in float64.
// atdn_flow_forward_interpolate_host (warm_start.hip) is this function behind argument checks; it serves CPU tensors and is what the
// CPU tests compare with the recorded outputs of the GMA wheel's forward_interpolate (whl:GMA/core/utils/utils.py:28-56).
//
// For one flow [2, h, w] (channel 0 = dx, 1 = dy) and the row-major source index i = y * w + x:
//   source point   (x1, y1) = (x + dx_i, y + dy_i), formed in float64
//   valid          0 < x1 < w and 0 < y1 < h, all four strict (NaN and infinite flows are invalid)
//   output (qx,qy) (dx_j, dy_j) of the valid source j with the smallest (qx - x1_j)^2 + (qy - y1_j)^2 in float64, each product
//                  and the sum rounded separately (no fused multiply-add: the ordering is the one numpy's float64 gives);
//                  equal distances go to the lowest j; without any valid source the output is all zeros
// Outputs are bit copies of input values. Batches are independent.
#pragma once
#include <limits>
#include <vector>

namespace atdn {

inline void forward_interpolate_host(const float* flow, int B, int h, int w, float* out) {
#pragma clang fp contract(off)
  const long n = (long)h * w;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> sx((size_t)n), sy((size_t)n);
  for (int b = 0; b < B; ++b) {
    const float* fx = flow + (long)b * 2 * n;
    const float* fy = fx + n;
    float* ox = out + (long)b * 2 * n;
    float* oy = ox + n;
    for (long j = 0; j < n; ++j) {
      const double x1 = (double)(j % w) + (double)fx[j], y1 = (double)(j / w) + (double)fy[j];
      const bool valid = x1 > 0.0 && x1 < (double)w && y1 > 0.0 && y1 < (double)h;
      sx[j] = valid ? x1 : inf;   // an invalid source is infinitely far from every query
      sy[j] = valid ? y1 : 0.0;
    }
    for (long q = 0; q < n; ++q) {
      const double qx = (double)(q % w), qy = (double)(q / w);
      double best = inf;
      long bj = -1;
      for (long j = 0; j < n; ++j) {
        const double ex = qx - sx[j], ey = qy - sy[j];
        const double xx = ex * ex, yy = ey * ey;
        const double d = xx + yy;
        if (d < best) { best = d; bj = j; }   // strict: the first (lowest) index keeps an equal distance
      }
      ox[q] = bj >= 0 ? fx[bj] : 0.0f;
      oy[q] = bj >= 0 ? fy[bj] : 0.0f;
    }
  }
}

}  // namespace atdn
