// One step of a flow track, the rule in plain C++ float64 (no HIP needed): flow_track_pixel is the rule for one pixel,
// flow_track_step_host the host form behind atdn_flow_track_step_host (flow_track.hip), which serves CPU tensors. The kernel of
// flow_track.hip evaluates the same function, so the two cannot drift apart; the independent statement the tests compare both with
// is tests/flow_track_ref.py (NumPy).
//
// A track follows every pixel of an anchor frame through the frames after it: acc [2, H, W] is the flow from the anchor to frame k
// on the anchor's grid, and a step composes it with the flow k -> k+1, read bilinearly where the track stands: p(k+1) = p(k) +
// flow_k(p(k)). The composed flow is a correspondence over the whole interval, and with the accumulated pose anchor <- frame k+1
// the two-view rule (two_view_host.h) triangulates it over the whole baseline.
//
// flow [2, H, W] float32, channel 0 = x, on frame k's grid; mask [H, W] uint8 or null, on frame k's grid; (acc_x, acc_y) and
// alive_in the state of pixel (x, y) of the anchor. Everything in float64, every operation rounded on its own (fp contraction off),
// in exactly this order:
//   alive_in == 0: dead                                           (dead: alive_out = 0, acc_out = acc_in bit for bit, depth untouched,
//                                                                  counted nowhere)
//   x1 = x + acc_x, y1 = y + acc_y                                (exact in float64)
//   inside, s = bilinear_flow(flow at (x1, y1))                   (pixel_rule.h states it line by line: the closed inside test,
//                                                                  four taps always read, the order of the products and sums);
//                                                                  not inside: dead, nothing more is read
//   n_x = acc_x + s_x, n_y = acc_y + s_y, finite = |n_x| <= DBL_MAX && |n_y| <= DBL_MAX
//   trusted = mask == null || mask[floor(y1 + 0.5)][floor(x1 + 0.5)] != 0       (inside the image, given `inside`)
//   alive_out = inside && finite && trusted && neither n_x nor n_y rounds to a float32 infinity; otherwise dead
//   acc_out = ((float)n_x, (float)n_y)                            (one rounding each)
//   with a pose: two_view_pixel (two_view_host.h) of pixel (x, y) with the flow acc_out — the float32 values —, no mask:
//   its inside, inlier and valid are counted, and valid: depth = (float)z1; otherwise depth untouched
// |n| rounds to a float32 infinity exactly when |n| >= 2^128 - 2^103 (the midpoint between FLT_MAX and 2^128 goes to the even
// neighbour, 2^128), so that is a comparison and no out-of-range conversion is ever made.
#pragma once
#include <cfloat>
#include <cmath>

#include "two_view_host.h"

namespace atdn {

enum { FT_ALIVE = 8 };   // beside TV_INSIDE, TV_INLIER, TV_VALID

// (acc_x, acc_y), alive_in: the state of pixel (x, y); fx, fy: the two planes [H * W] of the flow; mask [H * W] or null. Returns
// FT_ALIVE | the TV_* bits of the pixel; *out_x, *out_y = acc_out (the input's bits when dead); *z = the depth where TV_VALID is
// set, untouched otherwise. DEPTH = false is the chain-only form: P and cam are not read, no TV_* bit is set.
template <bool DEPTH>
ATDN_HD inline int flow_track_pixel(float acc_x, float acc_y, bool alive_in, const float* fx, const float* fy,
                                    const unsigned char* mask, int H, int W, int x, int y, const TwoViewPose* P,
                                    const TwoViewCamera* cam, float* out_x, float* out_y, float* z) {
#pragma clang fp contract(off)
  *out_x = acc_x;
  *out_y = acc_y;
  if (!alive_in) return 0;
  const double ux = (double)acc_x, uy = (double)acc_y;
  const double x1 = (double)x + ux, y1 = (double)y + uy;
  double s[2];
  if (!bilinear_flow(x1, y1, fx, fy, H, W, s)) return 0;
  const double nx = ux + s[0], ny = uy + s[1];
  const bool finite = fabs(nx) <= DBL_MAX && fabs(ny) <= DBL_MAX;
  bool trusted = true;
  if (mask) {
    const double xr = x1 + 0.5, yr = y1 + 0.5;
    const int xm = (int)floor(xr), ym = (int)floor(yr);        // <= W-1, H-1: x1 + 0.5 <= W - 0.5
    trusted = mask[(long)ym * W + xm] != 0;
  }
  const double to_inf = 0x1.ffffffp+127;                       // 2^128 - 2^103: from here a double rounds to a float32 infinity
  if (!(finite && trusted && fabs(nx) < to_inf && fabs(ny) < to_inf)) return 0;
  const float ox = (float)nx, oy = (float)ny;
  *out_x = ox;
  *out_y = oy;
  int flags = FT_ALIVE;
  if (DEPTH) {
    int tv = 0;
    const float d = two_view_pixel(ox, oy, *P, *cam, H, W, x, y, &tv);
    if (tv & TV_VALID) *z = d;
    flags |= tv;
  }
  return flags;
}

// flow [B, 2, H, W], mask [B, H, W] or null, acc [B, 2, H, W], alive [B, H, W], pose [B, 12] or null, depth [B, 1, H, W] (null
// without a pose), counts [B, 4] = (alive, inside, inliers, valid). acc_out == acc_in and alive_out == alive_in are allowed: a
// pixel's own state is read before it is written, and no other pixel's is read.
inline void flow_track_step_host(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in,
                                 int B, int H, int W, float* acc_out, unsigned char* alive_out, const float* pose,
                                 const TwoViewCamera& cam, float* depth, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    const float* fx = flow + (long)b * 2 * n;
    const float* fy = fx + n;
    const unsigned char* m = mask ? mask + (long)b * n : nullptr;
    const float* ix = acc_in + (long)b * 2 * n;
    const float* iy = ix + n;
    float* ox = acc_out + (long)b * 2 * n;
    float* oy = ox + n;
    const unsigned char* li = alive_in + (long)b * n;
    unsigned char* lo = alive_out + (long)b * n;
    float* d = pose ? depth + (long)b * n : nullptr;
    TwoViewPose P{};
    if (pose) P = two_view_load_pose(pose + 12L * b);
    int sum[4] = {0, 0, 0, 0};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long i = (long)y * W + x;
        float px, py, z = 0.0f;
        const int flags = pose ? flow_track_pixel<true>(ix[i], iy[i], li[i] != 0, fx, fy, m, H, W, x, y, &P, &cam, &px, &py, &z)
                               : flow_track_pixel<false>(ix[i], iy[i], li[i] != 0, fx, fy, m, H, W, x, y, nullptr, nullptr, &px,
                                                         &py, &z);
        ox[i] = px;
        oy[i] = py;
        lo[i] = (flags & FT_ALIVE) ? 1 : 0;
        if (flags & TV_VALID) d[i] = z;
        sum[0] += (flags & FT_ALIVE) ? 1 : 0;
        sum[1] += (flags & TV_INSIDE) ? 1 : 0;
        sum[2] += (flags & TV_INLIER) ? 1 : 0;
        sum[3] += (flags & TV_VALID) ? 1 : 0;
      }
    for (int k = 0; k < 4; ++k) counts[4 * b + k] = sum[k];
  }
}

}  // namespace atdn
