// Multi-view consistency filter of the keyframe depths (the geometric-consistency fusion of multi-view stereo: COLMAP, MVSNet),
// the rule in plain C++ float64 (no HIP needed): depth_fuse_relative composes the pose of a (target, source) pair,
// depth_fuse_source is the rule for one pixel and one source, depth_fuse_result the pixel's outcome, depth_fuse_host the host form
// behind atdn_depth_fuse_host (depth_fusion.hip), which serves CPU tensors. The kernel of depth_fusion.hip calls the same functions, so the
// two cannot drift apart; the independent statement the tests compare both with is tests/depth_fusion_ref.py (NumPy).
//
// bank [N, H, W] float32 (0 = no depth), poses [N, 12] float32 (rows of [R|t], world <- camera). For target i and source j, in
// float64 from the float32 rows, every operation rounded on its own (fp contraction off), every dot product (p0 + p1) + p2:
//   R = R_j^T R_i:  R_kl = (rj_0k*ri_0l + rj_1k*ri_1l) + rj_2k*ri_2l
//   d_m = ti_m - tj_m,  t = R_j^T d:  t_k = (rj_0k*d_0 + rj_1k*d_1) + rj_2k*d_2                  (X_j = R X_i + t)
// Pixel (x, y) of the target with z = bank[i][y][x]: has = z > 0; a0 = (x - cx)/fx, a1 = (y - cy)/fy, X = (z*a0, z*a1, z).
// Per source, in list order (a slot with j < 0, j >= N or j == i is skipped and reads nothing):
//   Xs_k = ((R_k0*X0 + R_k1*X1) + R_k2*X2) + t_k
//   front = Xs_2 >= min_z                                          not front: the source is not ok, nothing is read
//   u = fx*(Xs_0/Xs_2) + cx, v = fy*(Xs_1/Xs_2) + cy
//   inside = 0 <= u <= W-1 && 0 <= v <= H-1                        (closed; a NaN fails); not inside: not ok, nothing is read
//   ds = the source's depth at (u, v), bilinear_plane of pixel_rule.h; ok = front && inside && all four taps > 0
//   q0 = (u - cx)/fx, q1 = (v - cy)/fy, Y = (ds*q0 - t0, ds*q1 - t1, ds - t2)
//   Yt_k = (R_0k*Y0 + R_1k*Y1) + R_2k*Y2                           (the source's surface point in the target camera)
//   back = ok && Yt_2 >= min_z
//   xr = fx*(Yt_0/Yt_2) + cx, yr = fy*(Yt_1/Yt_2) + cy
//   e2 = (xr - x)*(xr - x) + (yr - y)*(yr - y),  rd = |Yt_2 - z| / z
//   consistent = back && e2 <= max_reproj*max_reproj && rd <= max_rel_depth
//   consistent: n += 1, zsum += Yt_2                               (zsum starts at z, n at 0)
// Result: views = n; kept = has && n >= min_views; fused = kept ? (float)(average ? zsum/(n + 1) : z) : 0;
// counts = (has, seen, kept), seen = ok for at least one source. Any NaN fails every comparison it reaches.
#pragma once
#include <cmath>
#include <vector>

#include "pixel_rule.h"

namespace atdn {

struct DepthFuseParams {
  double fx, fy, cx, cy, max_reproj2, max_rel_depth, min_z;
  int min_views, average;
};

inline DepthFuseParams depth_fuse_params(double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth,
                                         int min_views, double min_z, int average) {
  return DepthFuseParams{fx, fy, cx, cy, max_reproj * max_reproj, max_rel_depth, min_z, min_views, average != 0};
}

enum { DF_HAS = 1, DF_SEEN = 2, DF_KEPT = 4 };
constexpr int DF_REL = 12;   // float64 per relative pose: R row-major (9), then t (3)

// pi, pj: the 12 float32 of target and source -> rel[DF_REL]
ATDN_HD inline void depth_fuse_relative(const float* pi, const float* pj, double* rel) {
#pragma clang fp contract(off)
  double d[3];
  for (int m = 0; m < 3; ++m) d[m] = (double)pi[4 * m + 3] - (double)pj[4 * m + 3];
  for (int k = 0; k < 3; ++k) {
    const double j0 = (double)pj[k], j1 = (double)pj[4 + k], j2 = (double)pj[8 + k];
    for (int l = 0; l < 3; ++l) {
      const double p0 = j0 * (double)pi[l], p1 = j1 * (double)pi[4 + l], p2 = j2 * (double)pi[8 + l];
      const double s = p0 + p1;
      rel[3 * k + l] = s + p2;
    }
    const double p0 = j0 * d[0], p1 = j1 * d[1], p2 = j2 * d[2];
    const double s = p0 + p1;
    rel[9 + k] = s + p2;
  }
}

// One source for one pixel with a depth: X = the pixel's point in the target camera, z its depth, src the source's plane [H * W].
// Returns `consistent` and then *zt = Yt_2; *ok as in the rule.
ATDN_HD inline bool depth_fuse_source(const double* rel, const float* src, const double X[3], double z, int x, int y,
                                      const DepthFuseParams& c, int H, int W, bool* ok, double* zt) {
#pragma clang fp contract(off)
  *ok = false;
  double Xs[3];
  for (int k = 0; k < 3; ++k) {
    const double p0 = rel[3 * k] * X[0], p1 = rel[3 * k + 1] * X[1], p2 = rel[3 * k + 2] * X[2];
    const double s01 = p0 + p1;
    const double s = s01 + p2;
    Xs[k] = s + rel[9 + k];
  }
  if (!(Xs[2] >= c.min_z)) return false;
  const double nu = Xs[0] / Xs[2], nv = Xs[1] / Xs[2];
  const double fu = c.fx * nu, fv = c.fy * nv;
  const double u = fu + c.cx, v = fv + c.cy;
  double ds;
  bool positive;
  if (!bilinear_plane(u, v, src, H, W, &ds, &positive)) return false;
  if (!positive) return false;
  *ok = true;
  const double eu = u - c.cx, ev = v - c.cy;
  const double q0 = eu / c.fx, q1 = ev / c.fy;
  const double dq0 = ds * q0, dq1 = ds * q1;
  const double Y0 = dq0 - rel[9], Y1 = dq1 - rel[10], Y2 = ds - rel[11];
  double Yt[3];
  for (int k = 0; k < 3; ++k) {
    const double p0 = rel[k] * Y0, p1 = rel[3 + k] * Y1, p2 = rel[6 + k] * Y2;
    const double s = p0 + p1;
    Yt[k] = s + p2;
  }
  if (!(Yt[2] >= c.min_z)) return false;
  const double nx = Yt[0] / Yt[2], ny = Yt[1] / Yt[2];
  const double fxr = c.fx * nx, fyr = c.fy * ny;
  const double xr = fxr + c.cx, yr = fyr + c.cy;
  const double ex = xr - (double)x, ey = yr - (double)y;
  const double exx = ex * ex, eyy = ey * ey;
  const double e2 = exx + eyy;
  const double dz = Yt[2] - z;
  const double rd = fabs(dz) / z;
  *zt = Yt[2];
  return e2 <= c.max_reproj2 && rd <= c.max_rel_depth;
}

// X of a pixel with depth z
ATDN_HD inline void depth_fuse_point(double z, int x, int y, const DepthFuseParams& c, double X[3]) {
#pragma clang fp contract(off)
  const double dx = (double)x - c.cx, dy = (double)y - c.cy;
  const double a0 = dx / c.fx, a1 = dy / c.fy;
  X[0] = z * a0;
  X[1] = z * a1;
  X[2] = z;
}

// The outcome of a pixel after its sources: returns the fused depth and sets the DF_* bits (`seen`: ok for at least one source).
ATDN_HD inline float depth_fuse_result(float zf, int n, double zsum, bool seen, const DepthFuseParams& c, int* flags) {
#pragma clang fp contract(off)
  const bool has = zf > 0.0f;
  const bool kept = has && n >= c.min_views;
  *flags = (has ? DF_HAS : 0) | (has && seen ? DF_SEEN : 0) | (kept ? DF_KEPT : 0);
  if (!kept) return 0.0f;
  return c.average ? (float)(zsum / (double)(n + 1)) : zf;
}

// bank [N, H, W], poses [N, 12], targets [B], sources [B, S] -> fused [B, 1, H, W], views [B, H, W] uint8, counts [B, 3]
inline void depth_fuse_host(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S, int H,
                            int W, const DepthFuseParams& c, float* fused, unsigned char* views, int* counts) {
  const long n = (long)H * W;
  std::vector<double> rel_buf((size_t)S * DF_REL);
  std::vector<int> src_buf((size_t)S);
  double* rel = rel_buf.data();
  int* src = src_buf.data();
  for (int b = 0; b < B; ++b) {
    float* f = fused + (long)b * n;
    unsigned char* vw = views + (long)b * n;
    int sum[3] = {0, 0, 0};
    const int i = targets[b];
    if (i < 0 || i >= N) {
      for (long p = 0; p < n; ++p) { f[p] = 0.0f; vw[p] = 0; }
      for (int k = 0; k < 3; ++k) counts[3 * b + k] = 0;
      continue;
    }
    for (int s = 0; s < S; ++s) {
      const int j = sources[(long)b * S + s];
      src[s] = (j < 0 || j >= N || j == i) ? -1 : j;
      if (src[s] >= 0) depth_fuse_relative(poses + 12L * i, poses + 12L * j, rel + (long)s * DF_REL);
    }
    const float* zi = bank + (long)i * n;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long p = (long)y * W + x;
        const float zf = zi[p];
        int cnt = 0, flags = 0;
        bool seen = false;
        double zsum = (double)zf;
        if (zf > 0.0f) {
          double X[3];
          depth_fuse_point((double)zf, x, y, c, X);
          for (int s = 0; s < S; ++s) {
            if (src[s] < 0) continue;
            bool ok;
            double zt;
            if (depth_fuse_source(rel + (long)s * DF_REL, bank + (long)src[s] * n, X, (double)zf, x, y, c, H, W, &ok, &zt)) {
              ++cnt;
              zsum = zsum + zt;
            }
            seen = seen || ok;
          }
        }
        f[p] = depth_fuse_result(zf, cnt, zsum, seen, c, &flags);
        vw[p] = (unsigned char)cnt;
        sum[0] += (flags & DF_HAS) ? 1 : 0;
        sum[1] += (flags & DF_SEEN) ? 1 : 0;
        sum[2] += (flags & DF_KEPT) ? 1 : 0;
      }
    for (int k = 0; k < 3; ++k) counts[3 * b + k] = sum[k];
  }
}

}  // namespace atdn
