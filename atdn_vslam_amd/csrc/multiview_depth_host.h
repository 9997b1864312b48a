// Multi-view keyframe depth: per anchor pixel, the inverse depth that best explains its correspondences in up to
// MV_MAX_VIEWS later frames with known poses (the depth half of bundle adjustment, the batch form of a depth filter), by
// Levenberg-Marquardt on the reprojection error under the Geman-McClure loss, with the information of the result. The rule in
// plain C++ float64 (no HIP needed): multiview_pixel is the whole rule for one pixel, multiview_depth_host the host form behind
// atdn_multiview_depth_host (multiview_depth.hip), which serves CPU tensors. The kernel of multiview_depth.hip calls the same function, so
// the two cannot drift apart; the independent statement the tests compare both with is tests/multiview_ref.py (NumPy). The rule
// is stated in full in include/atdn_hip.h, atdn_multiview_depth; only + - * / and comparisons, every operation rounded on its
// own (fp contraction off). The robust loss, the cost of a point behind a camera, the internal pose and the damping constants
// are those of the PnP solver (pnp_host.h, lm6.h).
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/atdn_hip.h"
#include "pnp_host.h"

namespace atdn {

constexpr int MV_MAX_VIEWS = ATDN_MULTIVIEW_MAX_VIEWS;
constexpr int MV_POSE = 12;   // float64 per listed view: Rc row-major (9), then tc (3): the internal pose of pnp_host.h
enum { MV_CAND = 1, MV_SOLVED = 2, MV_VALID = 4 };

struct MultiviewParams {
  double fx, fy, cx, cy;
  double c2;             // scale_px * scale_px
  double thr;            // inlier_px * inlier_px
  double min_z;
  double rho_behind;     // the cost of a view the point is behind: the loss at e2 = (H + W)^2
  double min_rel_info;   // 1 / (max_rel_sigma * max_rel_sigma)
  double max_depth;
  int min_views, iters;
};

inline MultiviewParams multiview_params(double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z,
                                        int min_views, double max_rel_sigma, double max_depth, int iters, int H, int W) {
#pragma clang fp contract(off)
  const PnpParams p = pnp_params(fx, fy, cx, cy, scale_px, inlier_px, min_z, H, W);
  const double s2 = max_rel_sigma * max_rel_sigma;
  return MultiviewParams{fx, fy, cx, cy, p.c2, p.thr, min_z, p.rho_behind, 1.0 / s2, max_depth, min_views, iters};
}

// The views of one problem: slot[s] = the bank index of listed view s, or -1 for a skipped one (k < 0 or k >= N), whose pose is
// not written. slots_b: the S entries of the problem; pose [S * MV_POSE].
ATDN_HD inline void multiview_view(const float* poses, const int* slots_b, int N, int s, int* slot, double* pose) {
  const int k = slots_b[s];
  const bool use = k >= 0 && k < N;
  slot[s] = use ? k : -1;
  if (use) pnp_internal_pose(poses + 12L * k, pose + (long)s * MV_POSE);
}

// In the kernel: the ray of a pixel is opaque to the compiler at the head of every evaluation and no LDS read moves across it.
// Without it the per-view terms that do not depend on rho (the poses out of LDS, m, kx, ky: 34 registers per view) are hoisted
// out of the evaluation loop and held for all MV_MAX_VIEWS views: 256 + 126 registers and one wave per SIMD; recomputing them is
// 20 of an evaluation's operations per view beside four divisions. No instruction, the same values.
ATDN_HD inline void multiview_per_evaluation(double& a0, double& a1) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(a0), "+v"(a1) : : "memory");
#else
  (void)a0;
  (void)a1;
#endif
}

// Pixel (x, y) = flat index p of a plane of n = H * W: acc_bank [N, 2, n], alive_bank [N, n], slot [S] and pose [S * MV_POSE] of
// multiview_view, z0 the initial depth (0: none). Returns the MV_* bits; *depth, *info and *views are always written.
// The per-view inputs are read once into arrays of MV_MAX_VIEWS walked with unrolled constant indices: in the kernel they stay
// in registers over all evaluations.
ATDN_HD inline int multiview_pixel(const float* acc_bank, const unsigned char* alive_bank, const int* slot, const double* pose, int S,
                                   long n, long p, int x, int y, int H, int W, float z0, const MultiviewParams& c, float* depth,
                                   float* info, int* views) {
#pragma clang fp contract(off)
  *depth = 0.0f;
  *info = 0.0f;
  *views = 0;
  const double xd = (double)x, yd = (double)y;
  const double dx = xd - c.cx, dy = yd - c.cy;
  double a0 = dx / c.fx, a1 = dy / c.fy;
  float u[MV_MAX_VIEWS], v[MV_MAX_VIEWS];
  unsigned obs = 0;
  int n_obs = 0;
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int s = 0; s < MV_MAX_VIEWS; ++s) {
    u[s] = 0.0f;
    v[s] = 0.0f;
    if (s < S && slot[s] >= 0) {
      const long k = slot[s];
      const float* a = acc_bank + 2 * k * n + p;
      u[s] = a[0];
      v[s] = a[n];
      const bool alive = alive_bank[k * n + p] != 0;
      const double x2 = xd + (double)u[s], y2 = yd + (double)v[s];
      const bool inside = x2 >= 0.0 && x2 <= (double)(W - 1) && y2 >= 0.0 && y2 <= (double)(H - 1);
      if (alive && inside) {
        const double* P = pose + s * MV_POSE;
        const double m0 = (P[0] * a0 + P[1] * a1) + P[2];
        const double m1 = (P[3] * a0 + P[4] * a1) + P[5];
        const double m2 = (P[6] * a0 + P[7] * a1) + P[8];
        const double xt = x2 - c.cx, yt = y2 - c.cy;
        const double Ax = c.fx * P[9] - xt * P[11], Bx = xt * m2 - c.fx * m0;
        const double Ay = c.fy * P[10] - yt * P[11], By = yt * m2 - c.fy * m1;
        num = num + (Ax * Bx + Ay * By);
        den = den + (Ax * Ax + Ay * Ay);
        obs |= 1u << s;
        ++n_obs;
      }
    }
  }
  if (n_obs < c.min_views) return 0;
  const double rho_lin = num / den;
  const bool lin_ok = rho_lin > 0.0 && rho_lin <= DBL_MAX;
  const double z0d = (double)z0;
  const bool init_ok = z0d > 0.0 && z0d <= (double)FLT_MAX;
  const double rho_0 = 1.0 / z0d;
  // evaluation 0 is E(rho_lin), 1 is E(rho_0), 2 .. iters + 1 are the trials of the steps: one site for the view loop
  double rho = 0.0, g = 0.0, h = 0.0, cost = 0.0, lambda = 1e-3;
  int n_in = 0;
  bool solved = false;
  for (int e = 0; e < c.iters + 2; ++e) {
    double r_t;
    if (e == 0) {
      if (!lin_ok) continue;
      r_t = rho_lin;
    } else if (e == 1) {
      if (!init_ok) continue;
      r_t = rho_0;
    } else {
      if (!solved) break;
      const double lh = lambda * h;
      const double dn = h + lh;
      const double st = g / dn;
      r_t = rho - st;
      if (!(r_t > 0.0 && r_t <= DBL_MAX)) {
        lambda = lm_lambda(lambda, false);
        continue;
      }
    }
    multiview_per_evaluation(a0, a1);
    double g_t = 0.0, h_t = 0.0, cost_t = 0.0;
    int n_t = 0;
    const double zlim = c.min_z * r_t;
#pragma unroll
    for (int s = 0; s < MV_MAX_VIEWS; ++s) {
      if (!((obs >> s) & 1u)) continue;
      const double* P = pose + s * MV_POSE;
      const double m0 = (P[0] * a0 + P[1] * a1) + P[2];
      const double m1 = (P[3] * a0 + P[4] * a1) + P[5];
      const double m2 = (P[6] * a0 + P[7] * a1) + P[8];
      const double P0 = m0 + r_t * P[9], P1 = m1 + r_t * P[10], P2 = m2 + r_t * P[11];
      if (!(P2 >= zlim)) {
        cost_t = cost_t + c.rho_behind;
        continue;
      }
      const double kx = c.fx * (P[9] * m2 - m0 * P[11]);
      const double ky = c.fy * (P[10] * m2 - m1 * P[11]);
      const double x2 = xd + (double)u[s], y2 = yd + (double)v[s];
      const double iz = 1.0 / P2;
      const double px = (c.fx * P0) * iz, py = (c.fy * P1) * iz;
      const double rx = (px + c.cx) - x2, ry = (py + c.cy) - y2;
      const double e2 = rx * rx + ry * ry;
      const double sc = 1.0 + e2 / c.c2;
      const double w = 1.0 / (sc * sc);
      const double r = (0.5 * e2) / sc;
      const double Jx = (kx * iz) * iz, Jy = (ky * iz) * iz;
      const double wx = w * Jx, wy = w * Jy;
      g_t = g_t + (wx * rx + wy * ry);
      h_t = h_t + (wx * Jx + wy * Jy);
      cost_t = cost_t + r;
      n_t += e2 <= c.thr ? 1 : 0;
    }
    // the linear start is taken as it comes; the initial depth replaces it only with a smaller cost; a trial likewise
    const bool accept = !solved || cost_t < cost;
    if (e >= 2) lambda = lm_lambda(lambda, accept);
    if (accept) {
      rho = r_t; g = g_t; h = h_t; cost = cost_t; n_in = n_t;
      solved = true;
    }
  }
  if (!solved) return MV_CAND;
  const double z = 1.0 / rho;
  const double ri = (h * rho) * rho;
  *views = n_in;
  const bool valid = n_in >= c.min_views && ri >= c.min_rel_info && z >= (double)FLT_MIN && z <= c.max_depth;
  if (!valid) return MV_CAND | MV_SOLVED;
  *depth = (float)z;
  *info = (float)(ri < (double)FLT_MAX ? ri : (double)FLT_MAX);
  return MV_CAND | MV_SOLVED | MV_VALID;
}

// acc_bank [N,2,H,W], alive_bank [N,H,W], poses [N,12], slots [B,S], depth_init [B,1,H,W] or null ->
// depth, info [B,1,H,W], views [B,H,W] uint8, counts [B,3]
inline void multiview_depth_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                                 const float* depth_init, int N, int B, int S, int H, int W, const MultiviewParams& c, float* depth,
                                 float* info, unsigned char* views, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    int slot[MV_MAX_VIEWS];
    double pose[MV_MAX_VIEWS * MV_POSE];
    for (int s = 0; s < S; ++s) multiview_view(poses, slots + (long)b * S, N, s, slot, pose);
    int sum[3] = {0, 0, 0};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long p = (long)y * W + x;
        int vw;
        const int flags = multiview_pixel(acc_bank, alive_bank, slot, pose, S, n, p, x, y, H, W, depth_init ? depth_init[b * n + p] : 0.0f,
                                          c, depth + b * n + p, info + b * n + p, &vw);
        views[b * n + p] = (unsigned char)vw;
        sum[0] += (flags & MV_CAND) ? 1 : 0;
        sum[1] += (flags & MV_SOLVED) ? 1 : 0;
        sum[2] += (flags & MV_VALID) ? 1 : 0;
      }
    for (int k = 0; k < 3; ++k) counts[3 * b + k] = sum[k];
  }
}

}  // namespace atdn
