// Pose from flow alone (epipolar refinement), the rule in plain C++ float64 (no HIP needed). The flow image 1 -> image 2 gives
// every pixel a correspondence, a relative pose [R|t] (X1 = R X2 + t) gives it an epipolar line: epipolar_pixel is the contribution
// of one pixel to the Gauss-Newton normal equations of the signed pixel distance from that line under the Geman-McClure loss,
// over the step (dw, dth) with R <- C(dw) R and t <- C(dth) t (C = cayley3 of lm6.h: the translation is ROTATED, never added to,
// so |t| — which two views do not show — is kept without a square root). epipolar_lm_step is one damped step with the gauge term
// that gives the unobservable direction dth || t the mean curvature of its block; the 28 terms, the plane sum, the state and
// the decision are those of plane_lm.h (shared with PnP), the per-pixel prefix up to epi2 is two_view_epipolar of
// two_view_host.h (shared with two_view_pixel). epipolar_terms_host / epipolar_solve_host are the host forms behind
// atdn_epipolar_terms_host / atdn_epipolar_solve_host (epipolar.hip); the kernels of epipolar.hip call the same functions. The
// independent statement the tests compare both with is tests/epipolar_ref.py (NumPy). The rule is stated in full in
// include/atdn_hip.h, atdn_epipolar_terms and atdn_epipolar_solve; only + - * / and comparisons, every operation rounded on
// its own (fp contraction off).
#pragma once
#include <cfloat>

#include "plane_lm.h"
#include "two_view_host.h"

namespace atdn {

enum { EPI_CAND = 1, EPI_USED = 2, EPI_INLIER = 4 };

struct EpipolarParams {
  double fx, fy, cx, cy;
  double c2;    // scale_px * scale_px
  double thr;   // inlier_px * inlier_px
};

inline EpipolarParams epipolar_params(double fx, double fy, double cx, double cy, double scale_px, double inlier_px) {
#pragma clang fp contract(off)
  return EpipolarParams{fx, fy, cx, cy, scale_px * scale_px, inlier_px * inlier_px};
}

// The state's pose (PlaneLmState::acc / trial) is the PUBLIC one in float64: p[0..8] = R (row-major), p[9..11] = t.
ATDN_HD inline void epipolar_load_pose(const float* pose12, double p[12]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) p[3 * i + j] = (double)pose12[4 * i + j];
    p[9 + i] = (double)pose12[4 * i + 3];
  }
}

ATDN_HD inline TwoViewPose epipolar_pose(const double p[12]) {
  TwoViewPose P;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P.r[i][j] = p[3 * i + j];
    P.t[i] = p[9 + i];
  }
  return P;
}

// a*b - c*d, each product and the difference rounded on its own
ATDN_HD inline double diff2(double a, double b, double c, double d) {
#pragma clang fp contract(off)
  const double ab = a * b, cd = c * d;
  return ab - cd;
}

// The 28 terms of pixel (x, y): (u, v) its flow, keep its mask. Returns the EPI_* bits; t is always written (+0.0 where the
// pixel contributes nothing).
ATDN_HD inline int epipolar_pixel(float u, float v, bool keep, const TwoViewPose& P, const EpipolarParams& c, int H, int W, int x,
                                  int y, double t[PLANE_TERMS]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < PLANE_TERMS; ++i) t[i] = 0.0;
  TwoViewEpi e;
  const bool inside = two_view_epipolar(u, v, P, c.fx, c.fy, c.cx, c.cy, H, W, x, y, e);
  if (!(keep && inside)) return 0;
  const bool used = e.ll > 0.0 && e.epi2 <= DBL_MAX;
  if (!used) return EPI_CAND;
  const double q = e.epi2 / c.c2;
  const double s = 1.0 + q;
  const double ss = s * s;
  const double w = 1.0 / ss;
  const double he = 0.5 * e.epi2;
  const double rho = he / s;
  const double a0 = e.a0, a1 = e.a1, b0 = e.b[0], b1 = e.b[1], b2 = e.b[2], n0 = e.n0, n1 = e.n1, n2 = e.n2;
  const double t0 = P.t[0], t1 = P.t[1], t2 = P.t[2];
  double jr[6];   // the Jacobian of res: (b x n, t x (a x b))
  jr[0] = diff2(b1, n2, b2, n1);
  jr[1] = diff2(b2, n0, b0, n2);
  jr[2] = diff2(b0, n1, b1, n0);
  const double a1b2 = a1 * b2, a0b2 = a0 * b2;
  const double k0 = a1b2 - b1, k1 = b0 - a0b2, k2 = diff2(a0, b1, a1, b0);     // a x b with a2 = 1
  jr[3] = diff2(t1, k2, t2, k1);
  jr[4] = diff2(t2, k0, t0, k2);
  jr[5] = diff2(t0, k1, t1, k0);
  const double a0t0 = a0 * t0, a1t1 = a1 * t1;
  const double ats = a0t0 + a1t1;
  const double at = ats + t2;
  const double e0 = e.l0 / c.fx, e1 = e.l1 / c.fy;
  double dm[2][6];   // the Jacobian of m = R^T n: (column j of R) x n, and (column j of R . t) a - (a . t) (row i of R)_j
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double r0 = P.r[0][j], r1 = P.r[1][j], r2 = P.r[2][j];
    dm[j][0] = diff2(r1, n2, r2, n1);
    dm[j][1] = diff2(r2, n0, r0, n2);
    dm[j][2] = diff2(r0, n1, r1, n0);
    const double rt = dot3(r0, t0, r1, t1, r2, t2);
    dm[j][3] = diff2(rt, a0, at, r0);
    dm[j][4] = diff2(rt, a1, at, r1);
    const double atr2 = at * r2;
    dm[j][5] = rt - atr2;
  }
  const double ll2 = 2.0 * e.ll;
  const double kk = e.res / ll2;
  const double ww = w / e.ll;
  double jd[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double p0 = e0 * dm[0][i], p1 = e1 * dm[1][i];
    const double ps = p0 + p1;
    const double dll = 2.0 * ps;
    const double kd = kk * dll;
    jd[i] = jr[i] - kd;
  }
  int n = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wj = ww * jd[i];
#pragma unroll
    for (int j = i; j < 6; ++j) t[n++] = wj * jd[j];
    t[21 + i] = wj * e.res;
  }
  t[27] = rho;
  return EPI_CAND | EPI_USED | (e.epi2 <= c.thr ? EPI_INLIER : 0);
}

// The damped step from the accepted point: s.trial = (C(dw) R, C(dth) t), or s.acc again where the gauge term or the
// factorisation fails.
ATDN_HD inline void epipolar_lm_step(PlaneLmState& s) {
#pragma clang fp contract(off)
  double A[36], F[21], b[6], dl[6], E[9], G[9];
  int n = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) A[6 * i + j] = A[6 * j + i] = s.sums[n++];
  const double* tv = s.acc + 9;
  const double tt = dot3(tv[0], tv[0], tv[1], tv[1], tv[2], tv[2]);
  const double h34 = A[21] + A[28];
  const double tr = h34 + A[35];
  const double gamma = tr / tt;
  for (int i = 0; i < 3; ++i) {
    const double gt = gamma * tv[i];
    for (int j = 0; j < 3; ++j) {
      const double gtt = gt * tv[j];
      A[6 * (3 + i) + 3 + j] = A[6 * (3 + i) + 3 + j] + gtt;
    }
  }
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
  cayley3(dl + 3, G);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) s.trial[3 * i + j] = dot3(E[3 * i], s.acc[j], E[3 * i + 1], s.acc[3 + j], E[3 * i + 2], s.acc[6 + j]);
    s.trial[9 + i] = dot3(G[3 * i], tv[0], G[3 * i + 1], tv[1], G[3 * i + 2], tv[2]);
  }
}

// The outputs of a finished solve.
ATDN_HD inline void epipolar_output(const PlaneLmState& s, const float* pose_in, float* pose_out, double* cost, int* counts4) {
  if (s.accepted == 0) {
    for (int i = 0; i < 12; ++i) pose_out[i] = pose_in[i];
  } else {
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose_out[4 * i + j] = (float)s.acc[3 * i + j];
      pose_out[4 * i + 3] = (float)s.acc[9 + i];
    }
  }
  *cost = s.sums[27];
  for (int i = 0; i < 3; ++i) counts4[i] = s.counts[i];
  counts4[3] = s.accepted;
}

inline void epipolar_plane_host(const float* fu, const float* fv, const unsigned char* mask, const double* pose, const EpipolarParams& c,
                                int H, int W, double sums[PLANE_TERMS], int counts[3]) {
  const TwoViewPose P = epipolar_pose(pose);
  plane_sum_host((long)H * W, [&](long i, double* t) {
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    return epipolar_pixel(fu[i], fv[i], mask ? mask[i] != 0 : true, P, c, H, W, x, y, t);
  }, sums, counts);
}

// flow [B,2,H,W], mask [B,H,W] uint8 or null, pose [B,12] -> sums [B,28], counts [B,3]
inline void epipolar_terms_host(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                                const EpipolarParams& c, double* sums, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    double p[12];
    epipolar_load_pose(pose + 12L * b, p);
    epipolar_plane_host(flow + 2 * b * n, flow + (2 * b + 1) * n, mask ? mask + b * n : nullptr, p, c, H, W,
                        sums + (long)PLANE_TERMS * b, counts + 3L * b);
  }
}

// what plane_finalise_kernel (plane_sum.h) and plane_solve_host (plane_lm.h) run for this solver
struct EpipolarSolver {
  ATDN_HD static void load_pose(const float* pose12, double p[12]) { epipolar_load_pose(pose12, p); }
  ATDN_HD static void lm_step(PlaneLmState& s) { epipolar_lm_step(s); }
  ATDN_HD static void output(const PlaneLmState& s, const float* pose_in, float* pose_out, double* cost, int* counts4) {
    epipolar_output(s, pose_in, pose_out, cost, counts4);
  }
};

// iters Levenberg-Marquardt steps (iters + 1 evaluations) from pose_init -> pose_out [B,12], cost [B], counts [B,4]
inline void epipolar_solve_host(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W,
                                const EpipolarParams& c, int iters, float* pose_out, double* cost, int* counts) {
  const long n = (long)H * W;
  plane_solve_host<EpipolarSolver>(B, iters, [&](int b, const double* p, double* sums, int* cnt) {
    epipolar_plane_host(flow + 2 * b * n, flow + (2 * b + 1) * n, mask ? mask + b * n : nullptr, p, c, H, W, sums, cnt);
  }, pose_init, pose_out, cost, counts);
}

}  // namespace atdn
