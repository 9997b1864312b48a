// What the per-pixel float64 rules (flow_consistency_host.h, two_view_host.h, flow_track_host.h, depth_fusion_host.h) share, in plain C++ (no HIP
// needed): the host/device marker of a function that the kernel and the host form both call, and the bilinear read of a flow (and of one plane: bilinear_plane).
//
// bilinear_flow reads a two-plane float32 field [2, H, W] at (x1, y1). Everything in float64, every operation rounded on its own
// (fp contraction off), in exactly this order:
//   inside = 0 <= x1 <= W-1 && 0 <= y1 <= H-1                     (closed; a NaN fails); not inside: nothing is read
//   x0 = floor(x1), ax = x1 - x0; y0 = floor(y1), ay = y1 - y0
//   taps at (x0, y0), (min(x0+1, W-1), y0), (x0, min(y0+1, H-1)), (min(x0+1, W-1), min(y0+1, H-1)): all four are always read,
//   zero-weight ones too (a NaN or an infinity there reaches the result)
//   per plane: top = t00*(1-ax) + t10*ax, bot = t01*(1-ax) + t11*ax, s = top*(1-ay) + bot*ay
// The bits of kernel, host form and NumPy restatement agree because this order is written once, here.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ATDN_HD __host__ __device__
#else
#define ATDN_HD
#endif

namespace atdn {

// px, py: the two planes [H * W]. Returns `inside`; s[0], s[1] = the values of the two planes at (x1, y1), set only when inside.
ATDN_HD inline bool bilinear_flow(double x1, double y1, const float* px, const float* py, int H, int W, double s[2]) {
#pragma clang fp contract(off)
  const bool inside = x1 >= 0.0 && x1 <= (double)(W - 1) && y1 >= 0.0 && y1 <= (double)(H - 1);
  if (!inside) return false;
  const double xf = floor(x1), yf = floor(y1);
  const double ax = x1 - xf, ay = y1 - yf;
  const int x0 = (int)xf, y0 = (int)yf;                       // in [0, W-1] x [0, H-1]: inside
  const int xn = x0 + 1 < W ? x0 + 1 : W - 1, yn = y0 + 1 < H ? y0 + 1 : H - 1;
  const long r0 = (long)y0 * W, r1 = (long)yn * W;
  const double wx = 1.0 - ax, wy = 1.0 - ay;
  for (int c = 0; c < 2; ++c) {
    const float* p = c ? py : px;
    const double t00 = (double)p[r0 + x0], t10 = (double)p[r0 + xn], t01 = (double)p[r1 + x0], t11 = (double)p[r1 + xn];
    const double top_l = t00 * wx, top_r = t10 * ax, bot_l = t01 * wx, bot_r = t11 * ax;
    const double top = top_l + top_r, bot = bot_l + bot_r;
    const double up = top * wy, dn = bot * ay;
    s[c] = up + dn;
  }
  return true;
}

// The one-plane sibling (depth_fusion_host.h): p [H * W] at (x1, y1), the same tests, taps, weights and order of operations as one
// plane of bilinear_flow. Returns `inside`; *s = the value and *positive = "all four taps > 0" (a NaN tap fails), both set only when
// inside. All four taps are always read.
ATDN_HD inline bool bilinear_plane(double x1, double y1, const float* p, int H, int W, double* s, bool* positive) {
#pragma clang fp contract(off)
  const bool inside = x1 >= 0.0 && x1 <= (double)(W - 1) && y1 >= 0.0 && y1 <= (double)(H - 1);
  if (!inside) return false;
  const double xf = floor(x1), yf = floor(y1);
  const double ax = x1 - xf, ay = y1 - yf;
  const int x0 = (int)xf, y0 = (int)yf;                       // in [0, W-1] x [0, H-1]: inside
  const int xn = x0 + 1 < W ? x0 + 1 : W - 1, yn = y0 + 1 < H ? y0 + 1 : H - 1;
  const long r0 = (long)y0 * W, r1 = (long)yn * W;
  const double wx = 1.0 - ax, wy = 1.0 - ay;
  const float f00 = p[r0 + x0], f10 = p[r0 + xn], f01 = p[r1 + x0], f11 = p[r1 + xn];
  const double t00 = (double)f00, t10 = (double)f10, t01 = (double)f01, t11 = (double)f11;
  const double top_l = t00 * wx, top_r = t10 * ax, bot_l = t01 * wx, bot_r = t11 * ax;
  const double top = top_l + top_r, bot = bot_l + bot_r;
  const double up = top * wy, dn = bot * ay;
  *s = up + dn;
  *positive = f00 > 0.0f && f10 > 0.0f && f01 > 0.0f && f11 > 0.0f;
  return true;
}

}  // namespace atdn
