// Two-view geometry of a flow and a relative pose, the rule in plain C++ float64 (no HIP needed): two_view_pixel is the rule for
// one pixel, two_view_depth_host the host form behind atdn_flow_two_view_depth_host (two_view.hip), which serves CPU tensors. The
// kernel of two_view.hip evaluates the same function, so the two cannot drift apart; the independent statement the tests compare
// both with is tests/two_view_ref.py (NumPy). The epipolar part of the pixel rule (x2 .. epi2) is two_view_epipolar, which
// epipolar_host.h (pose from flow alone) calls too.
//
// Given the calibration (fx, fy, cx, cy; no skew), the flow of pixel (x, y) of image 1 names its correspondence (x2, y2) in image 2,
// and the relative pose [R|t] (X1 = R X2 + t, what `transform(rot, tr)` of the pose head returns) names the epipolar line of (x, y)
// in image 2. The rule gives the squared pixel distance of (x2, y2) from that line, and — by the least-squares intersection of the
// two viewing rays (the midpoint method; Hartley & Zisserman, Multiple View Geometry, 12.1) — the depth of the pixel in camera 1.
//
// flow [2, H, W] float32, channel 0 = x; pose = 12 float32, the rows of [R|t]: r_ij = pose[4*i + j], t_i = pose[4*i + 3]. For pixel
// (x, y), everything in float64, every operation rounded on its own (fp contraction off), in exactly this order:
//   x2 = x + u, y2 = y + v                                        (exact in float64)
//   inside = 0 <= x2 <= W-1 && 0 <= y2 <= H-1                     (closed; a NaN fails); not inside: depth 0, counted nowhere
//   a0 = (x - cx)/fx, a1 = (y - cy)/fy                            (the ray of the pixel, a2 = 1)
//   q0 = (x2 - cx)/fx, q1 = (y2 - cy)/fy                          (the ray of its correspondence in camera 2, q2 = 1)
//   b_i = (r_i0*q0 + r_i1*q1) + r_i2                   i = 0,1,2  (b = R q: that ray in camera 1's axes)
//   n0 = t1 - t2*a1, n1 = t2*a0 - t0, n2 = t0*a1 - t1*a0          (n = t x a: the normal of the epipolar plane)
//   res = (n0*b0 + n1*b1) + n2*b2
//   m0 = (r00*n0 + r10*n1) + r20*n2, m1 = (r01*n0 + r11*n1) + r21*n2, l0 = m0/fx, l1 = m1/fy     (the line in pixels of image 2)
//   epi2 = (res*res) / (l0*l0 + l1*l1)                            squared pixel distance of (x2, y2) from its epipolar line
//   inlier = epi2 <= max_epipolar*max_epipolar                    (plain comparison: 0/0 from t = 0 is NaN and fails)
//   aa = (a0*a0 + a1*a1) + 1, bb = (b0*b0 + b1*b1) + b2*b2, ab = (a0*b0 + a1*b1) + b2
//   at = (a0*t0 + a1*t1) + t2, bt = (b0*t0 + b1*t1) + b2*t2
//   p = aa*bb, det = p - ab*ab, sin2 = det/p                      sin^2 of the angle between the two rays
//   z1 = (bb*at - ab*bt)/det, z2 = (ab*at - aa*bt)/det            least-squares solution of z1*a - z2*b = t
//   valid = inlier && sin2 >= min_sin2 && z1 >= FLT_MIN && z2 > 0 && z1 <= max_depth
//   depth = valid ? (float)z1 : 0
// `z1 >= FLT_MIN` (2^-126, as a double) stands where `z1 > 0` would: a positive z1 below it rounds to a float32 zero or
// subnormal, and a pixel counted valid would then carry the depth that means "no depth". With it every valid depth is a normal
// positive float32, and counts[2] is the number of non-zero depths. Parallel rays give det = 0, sin2 = 0 and z1 = +-inf or NaN, which
// fails `z1 <= max_depth` whatever min_sin2 is; any NaN fails every comparison it reaches.
#pragma once
#include <cfloat>
#include <cmath>

#include "pixel_rule.h"

namespace atdn {

struct TwoViewCamera {
  double fx, fy, cx, cy, max_epipolar, min_sin2, max_depth;
};

struct TwoViewPose {   // X1 = R X2 + t
  double r[3][3], t[3];
};

ATDN_HD inline TwoViewPose two_view_load_pose(const float* pose12) {
  TwoViewPose P;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P.r[i][j] = (double)pose12[4 * i + j];
    P.t[i] = (double)pose12[4 * i + 3];
  }
  return P;
}

enum { TV_INSIDE = 1, TV_INLIER = 2, TV_VALID = 4 };

// The epipolar part of the rule for one pixel — x2 .. epi2 above, in that order —, written once for two_view_pixel and for
// epipolar_pixel (epipolar_host.h: pose from flow alone), so that the two cannot drift apart.
struct TwoViewEpi {
  double x2, y2, a0, a1, b[3], n0, n1, n2, res, l0, l1, ll, epi2;
};

// Returns `inside`; e is set only when inside.
ATDN_HD inline bool two_view_epipolar(float u, float v, const TwoViewPose& P, double fx, double fy, double cx, double cy, int H,
                                      int W, int x, int y, TwoViewEpi& e) {
#pragma clang fp contract(off)
  const double xd = (double)x, yd = (double)y;
  const double x2 = xd + (double)u, y2 = yd + (double)v;
  const bool inside = x2 >= 0.0 && x2 <= (double)(W - 1) && y2 >= 0.0 && y2 <= (double)(H - 1);
  if (!inside) return false;
  const double dx = xd - cx, dy = yd - cy;
  const double a0 = dx / fx, a1 = dy / fy;
  const double ex = x2 - cx, ey = y2 - cy;
  const double q0 = ex / fx, q1 = ey / fy;
  double b[3];
  for (int i = 0; i < 3; ++i) {
    const double s0 = P.r[i][0] * q0, s1 = P.r[i][1] * q1;
    const double s = s0 + s1;
    b[i] = s + P.r[i][2];
  }
  const double t0 = P.t[0], t1 = P.t[1], t2 = P.t[2];
  const double t2a1 = t2 * a1, t2a0 = t2 * a0, t0a1 = t0 * a1, t1a0 = t1 * a0;
  const double n0 = t1 - t2a1, n1 = t2a0 - t0, n2 = t0a1 - t1a0;
  const double nb0 = n0 * b[0], nb1 = n1 * b[1], nb2 = n2 * b[2];
  const double nb01 = nb0 + nb1;
  const double res = nb01 + nb2;
  double m[2];
  for (int j = 0; j < 2; ++j) {
    const double s0 = P.r[0][j] * n0, s1 = P.r[1][j] * n1, s2 = P.r[2][j] * n2;
    const double s = s0 + s1;
    m[j] = s + s2;
  }
  const double l0 = m[0] / fx, l1 = m[1] / fy;
  const double rr = res * res, l00 = l0 * l0, l11 = l1 * l1;
  const double ll = l00 + l11;
  e.x2 = x2; e.y2 = y2; e.a0 = a0; e.a1 = a1;
  e.b[0] = b[0]; e.b[1] = b[1]; e.b[2] = b[2];
  e.n0 = n0; e.n1 = n1; e.n2 = n2;
  e.res = res; e.l0 = l0; e.l1 = l1; e.ll = ll;
  e.epi2 = rr / ll;
  return true;
}

// u, v: the flow at (x, y). Returns the depth (0 = none) and sets `flags` to the TV_* bits of the pixel.
ATDN_HD inline float two_view_pixel(float u, float v, const TwoViewPose& P, const TwoViewCamera& c, int H, int W, int x, int y,
                                    int* flags) {
#pragma clang fp contract(off)
  *flags = 0;
  TwoViewEpi e;
  if (!two_view_epipolar(u, v, P, c.fx, c.fy, c.cx, c.cy, H, W, x, y, e)) return 0.0f;
  const double a0 = e.a0, a1 = e.a1, epi2 = e.epi2;
  const double b[3] = {e.b[0], e.b[1], e.b[2]};
  const double t0 = P.t[0], t1 = P.t[1], t2 = P.t[2];
  const double thr = c.max_epipolar * c.max_epipolar;
  const bool inlier = epi2 <= thr;
  const double a00 = a0 * a0, a11 = a1 * a1, b00 = b[0] * b[0], b11 = b[1] * b[1], b22 = b[2] * b[2];
  const double asum = a00 + a11, bsum = b00 + b11;
  const double aa = asum + 1.0, bb = bsum + b22;
  const double a0b0 = a0 * b[0], a1b1 = a1 * b[1];
  const double absum = a0b0 + a1b1;
  const double ab = absum + b[2];
  const double a0t0 = a0 * t0, a1t1 = a1 * t1;
  const double atsum = a0t0 + a1t1;
  const double at = atsum + t2;
  const double b0t0 = b[0] * t0, b1t1 = b[1] * t1, b2t2 = b[2] * t2;
  const double btsum = b0t0 + b1t1;
  const double bt = btsum + b2t2;
  const double p = aa * bb, abab = ab * ab;
  const double det = p - abab;
  const double sin2 = det / p;
  const double bbat = bb * at, abbt = ab * bt, abat = ab * at, aabt = aa * bt;
  const double num1 = bbat - abbt, num2 = abat - aabt;
  const double z1 = num1 / det, z2 = num2 / det;
  const bool valid = inlier && sin2 >= c.min_sin2 && z1 >= (double)FLT_MIN && z2 > 0.0 && z1 <= c.max_depth;
  *flags = TV_INSIDE | (inlier ? TV_INLIER : 0) | (valid ? TV_VALID : 0);
  return valid ? (float)z1 : 0.0f;
}

// flow [B, 2, H, W], pose [B, 12], mask [B, H, W] uint8 or null -> depth [B, 1, H, W], counts [B, 3] = (inside, inliers, valid).
inline void two_view_depth_host(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W,
                                const TwoViewCamera& cam, float* depth, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    const float* fu = flow + (long)b * 2 * n;
    const float* fv = fu + n;
    const unsigned char* m = mask ? mask + (long)b * n : nullptr;
    float* d = depth + (long)b * n;
    const TwoViewPose P = two_view_load_pose(pose + 12L * b);
    int sum[3] = {0, 0, 0};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long i = (long)y * W + x;
        int flags = 0;
        d[i] = (m && m[i] == 0) ? 0.0f : two_view_pixel(fu[i], fv[i], P, cam, H, W, x, y, &flags);
        sum[0] += (flags & TV_INSIDE) ? 1 : 0;
        sum[1] += (flags & TV_INLIER) ? 1 : 0;
        sum[2] += (flags & TV_VALID) ? 1 : 0;
      }
    for (int k = 0; k < 3; ++k) counts[3 * b + k] = sum[k];
  }
}

}  // namespace atdn
