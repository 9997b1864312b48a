// Pose from depth and flow (robust PnP), the rule in plain C++ float64 (no HIP needed). A depth map of image 1 gives a 3-D point
// per pixel, the flow image 1 -> image 2 gives that point's pixel in image 2: pnp_pixel is the contribution of one pixel to the
// Gauss-Newton normal equations of the reprojection error under the Geman-McClure loss, pnp_plane_host the fixed-order sum of
// a plane, pnp_lm_step one Levenberg-Marquardt step (the 28 terms, the chunks, the state and the decision are those of
// plane_lm.h, shared with epipolar_host.h; the 6 x 6 algebra, the Cayley matrix and the damping constants are those of lm6.h, shared with the pose graph; the composition from the left is
// PnP's own), pnp_terms_host / pnp_solve_host the host forms behind atdn_pnp_terms_host / atdn_pnp_solve_host (pnp.hip), which
// serve CPU tensors. The kernels of pnp.hip call the same functions, so the two cannot drift apart; the independent statement
// the tests compare both with is tests/pnp_ref.py (NumPy). The rule is stated in full in include/atdn_hip.h, atdn_pnp_terms and
// atdn_pnp_solve; only + - * / and comparisons, every operation rounded on its own (fp contraction off).
#pragma once
#include <cfloat>
#include <cmath>

#include "plane_lm.h"

namespace atdn {

enum { PNP_CAND = 1, PNP_USED = 2, PNP_INLIER = 4 };

struct PnpParams {
  double fx, fy, cx, cy;
  double c2;           // scale_px * scale_px
  double thr;          // inlier_px * inlier_px
  double min_z;
  double rho_behind;   // the cost of a candidate behind the camera: rho at e2 = (H + W)^2
};

inline PnpParams pnp_params(double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, int H,
                            int W) {
#pragma clang fp contract(off)
  PnpParams p{fx, fy, cx, cy, scale_px * scale_px, inlier_px * inlier_px, min_z, 0.0};
  const double eb = (double)(H + W);
  const double e2 = eb * eb;
  const double q = e2 / p.c2;
  const double s = 1.0 + q;
  const double h = 0.5 * e2;
  p.rho_behind = h / s;
  return p;
}

// The poses of the solver's state (PlaneLmState) are INTERNAL: p[0..8] = Rc (row-major), p[9..11] = tc, X2 = Rc X1 + tc.
// public pose (12 float32, rows of [R|t], X1 = R X2 + t) -> internal pose
ATDN_HD inline void pnp_internal_pose(const float* pose12, double p[12]) {
#pragma clang fp contract(off)
  double r[3][3], t[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r[i][j] = (double)pose12[4 * i + j];
    t[i] = (double)pose12[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) p[3 * i + j] = r[j][i];
    p[9 + i] = -dot3(r[0][i], t[0], r[1][i], t[1], r[2][i], t[2]);
  }
}

// internal pose -> public pose, rounded to float32
ATDN_HD inline void pnp_public_pose(const double p[12], float* pose12) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose12[4 * i + j] = (float)p[3 * j + i];
    pose12[4 * i + 3] = (float)(-dot3(p[i], p[9], p[3 + i], p[10], p[6 + i], p[11]));
  }
}

// The 28 terms of pixel (x, y): z its depth, (u, v) its flow, keep its mask. Returns the PNP_* bits; t is always written
// (+0.0 where the pixel contributes nothing).
ATDN_HD inline int pnp_pixel(float zf, float u, float v, bool keep, const double* P, const PnpParams& c, int H, int W, int x,
                             int y, double t[PLANE_TERMS]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < PLANE_TERMS; ++i) t[i] = 0.0;
  const double xd = (double)x, yd = (double)y, z = (double)zf;
  const double x2 = xd + (double)u, y2 = yd + (double)v;
  const bool inside = x2 >= 0.0 && x2 <= (double)(W - 1) && y2 >= 0.0 && y2 <= (double)(H - 1);
  const bool cand = keep && z > 0.0 && z <= (double)FLT_MAX && inside;
  if (!cand) return 0;
  const double dx = xd - c.cx, dy = yd - c.cy;
  const double zx = z * dx, zy = z * dy;
  const double X1 = zx / c.fx, Y1 = zy / c.fy;
  double Xc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) Xc[i] = dot3(P[3 * i], X1, P[3 * i + 1], Y1, P[3 * i + 2], z) + P[9 + i];
  const double X = Xc[0], Y = Xc[1], Z = Xc[2];
  if (!(Z >= c.min_z)) {
    t[27] = c.rho_behind;
    return PNP_CAND;
  }
  const double iz = 1.0 / Z;
  const double fX = c.fx * X, fY = c.fy * Y;
  const double px = fX * iz, py = fY * iz;
  const double pxc = px + c.cx, pyc = py + c.cy;
  const double rx = pxc - x2, ry = pyc - y2;
  const double rxx = rx * rx, ryy = ry * ry;
  const double e2 = rxx + ryy;
  const double q = e2 / c.c2;
  const double s = 1.0 + q;
  const double ss = s * s;
  const double w = 1.0 / ss;
  const double he = 0.5 * e2;
  const double rho = he / s;
  const double a = c.fx * iz, k = c.fy * iz;
  const double pxiz = px * iz, pyiz = py * iz;
  const double b = -pxiz, d = -pyiz;
  const double aZ = a * Z, bX = b * X, aY = a * Y, dY = d * Y, kZ = k * Z, dX = d * X;
  const double Jx[6] = {b * Y, aZ - bX, -aY, a, 0.0, b};
  const double Jy[6] = {dY - kZ, -dX, k * X, 0.0, k, d};
  int n = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wx = w * Jx[i], wy = w * Jy[i];
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const double hx = wx * Jx[j], hy = wy * Jy[j];
      t[n++] = hx + hy;
    }
    const double gx = wx * rx, gy = wy * ry;
    t[21 + i] = gx + gy;
  }
  t[27] = rho;
  return PNP_CAND | PNP_USED | (e2 <= c.thr ? PNP_INLIER : 0);
}

// The damped step from the accepted point: s.trial = retract(s.acc, delta), or s.acc again where the factorisation fails.
ATDN_HD inline void pnp_lm_step(PlaneLmState& s) {
#pragma clang fp contract(off)
  double A[36], F[21], b[6], dl[6], E[9];
  int n = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) A[6 * i + j] = A[6 * j + i] = s.sums[n++];
  for (int i = 0; i < 6; ++i) {
    const double l = s.lambda * A[7 * i];
    A[7 * i] = A[7 * i] + l;
    b[i] = -s.sums[21 + i];
  }
  const bool ok = ldl6_factor(A, F);
  ldl6_solve(F, b, dl);
  if (!(ok && finite6(dl))) {
    for (int i = 0; i < 12; ++i) s.trial[i] = s.acc[i];
    return;
  }
  cayley3(dl, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) s.trial[3 * i + j] = dot3(E[3 * i], s.acc[j], E[3 * i + 1], s.acc[3 + j], E[3 * i + 2], s.acc[6 + j]);
    s.trial[9 + i] = dot3(E[3 * i], s.acc[9], E[3 * i + 1], s.acc[10], E[3 * i + 2], s.acc[11]) + dl[3 + i];
  }
}

// The outputs of a finished solve.
ATDN_HD inline void pnp_output(const PlaneLmState& s, const float* pose_in, float* pose_out, double* cost, int* counts4) {
  if (s.accepted == 0) {
    for (int i = 0; i < 12; ++i) pose_out[i] = pose_in[i];
  } else {
    pnp_public_pose(s.acc, pose_out);
  }
  *cost = s.sums[27];
  for (int i = 0; i < 3; ++i) counts4[i] = s.counts[i];
  counts4[3] = s.accepted;
}

// The sums of one plane at the internal pose P, in the order of plane_sum_host (plane_lm.h).
inline void pnp_plane_host(const float* depth, const float* fu, const float* fv, const unsigned char* mask, const double* P,
                           const PnpParams& c, int H, int W, double sums[PLANE_TERMS], int counts[3]) {
  plane_sum_host((long)H * W, [&](long i, double* t) {
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    return pnp_pixel(depth[i], fu[i], fv[i], mask ? mask[i] != 0 : true, P, c, H, W, x, y, t);
  }, sums, counts);
}

// depth [B,H,W], flow [B,2,H,W], mask [B,H,W] uint8 or null, pose [B,12] -> sums [B,28], counts [B,3]
inline void pnp_terms_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                           const PnpParams& c, double* sums, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    double P[12];
    pnp_internal_pose(pose + 12L * b, P);
    pnp_plane_host(depth + b * n, flow + 2 * b * n, flow + (2 * b + 1) * n, mask ? mask + b * n : nullptr, P, c, H, W,
                   sums + (long)PLANE_TERMS * b, counts + 3L * b);
  }
}

// what plane_finalise_kernel (plane_sum.h) and plane_solve_host (plane_lm.h) run for this solver
struct PnpSolver {
  ATDN_HD static void load_pose(const float* pose12, double p[12]) { pnp_internal_pose(pose12, p); }
  ATDN_HD static void lm_step(PlaneLmState& s) { pnp_lm_step(s); }
  ATDN_HD static void output(const PlaneLmState& s, const float* pose_in, float* pose_out, double* cost, int* counts4) {
    pnp_output(s, pose_in, pose_out, cost, counts4);
  }
};

// iters Levenberg-Marquardt steps (iters + 1 evaluations) from pose_init -> pose_out [B,12], cost [B], counts [B,4]
inline void pnp_solve_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose_init, int B, int H,
                           int W, const PnpParams& c, int iters, float* pose_out, double* cost, int* counts) {
  const long n = (long)H * W;
  plane_solve_host<PnpSolver>(B, iters, [&](int b, const double* P, double* sums, int* cnt) {
    pnp_plane_host(depth + b * n, flow + 2 * b * n, flow + (2 * b + 1) * n, mask ? mask + b * n : nullptr, P, c, H, W, sums, cnt);
  }, pose_init, pose_out, cost, counts);
}

}  // namespace atdn
