// Windowed dense bundle adjustment over a flow bank: the joint Levenberg-Marquardt refinement of the poses of up to
// BA_MAX_VIEWS listed views and of the inverse depths of the anchor's candidate pixels, the depths eliminated by the Schur
// complement (the other half of multiview_depth_host.h, and the coupling of the two). The rule in plain C++ float64 (no HIP
// needed): ba_view is what one view of one candidate contributes, ba_backsub the depth step of a candidate, ba_decide /
// ba_system_entry / ldln_* / ba_retract_view the step on the reduced 6S x 6S system, bundle_terms_host / bundle_adjust_host the
// host forms behind atdn_bundle_terms_host / atdn_bundle_adjust_host (bundle.hip), which serve CPU tensors. The kernels of
// bundle.hip call the same functions, so the two cannot drift apart; the independent statement the tests compare both with is
// tests/bundle_ref.py (NumPy). The rule is stated in full in include/atdn_hip.h, atdn_bundle_adjust; only + - * / and
// comparisons, every operation rounded on its own (fp contraction off). The robust loss, the cost of a point behind a camera and
// the internal pose are those of pnp_host.h, the Cayley matrix and the damping constants those of lm6.h, the observation test
// that of multiview_pixel.
//
// ORDER OF THE SUMS (part of the rule). The candidate positions are the pixels of the strided grid, position q = ys * Ws + xs
// (Ws = ceil(W / stride)) standing for pixel (xs * stride, ys * stride). Over the views of a candidate: ascending list index s,
// starting from +0.0. Over candidates: the positions are cut into chunks of BA_CHUNK consecutive q; every sum of a chunk starts
// from +0.0 and takes the chunk's candidates in ascending q; the chunk sums are added in chunk order, starting from +0.0.
// The sums of one evaluation, ba_sums(S) float64 with n = 6 S:
//   [0, n (n + 1) / 2)   T0, upper triangle row by row: entry (i, j), i <= j, takes (E_i * ic) * E_j of a candidate, ic = 1 / c
//   then n               v0: entry i takes E_i * (b * ic)
//   then 27 S            per view the 21 upper-triangle entries of H_s row by row, then the 6 of g_s
//   then 1               the cost: per candidate the sum over its observed views (rho_behind for a view it is behind)
// A candidate whose c is not > 0 contributes to the cost alone.
#pragma once
#include <cfloat>
#include <cmath>
#include <vector>

#include "../../include/atdn_hip.h"
#include "multiview_depth_host.h"

namespace atdn {

constexpr int BA_MAX_VIEWS = MV_MAX_VIEWS;
constexpr int BA_MAX_N = 6 * BA_MAX_VIEWS;   // unknowns of the reduced system
constexpr int BA_CHUNK = 512;                // candidate positions per chunk (one workgroup of the terms kernel)
constexpr int BA_VIEW_TERMS = 27;            // 21 of H_s, 6 of g_s
enum { BA_FRONT = 1, BA_INLIER = 2 };

struct BundleParams {
  double fx, fy, cx, cy;
  double c2;            // scale_px * scale_px
  double thr;           // inlier_px * inlier_px
  double min_z;
  double rho_behind;    // the cost of a view the point is behind: the loss at e2 = (H + W)^2
  int min_views, iters, stride;
};

inline BundleParams bundle_params(double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z,
                                  int min_views, int iters, int stride, int H, int W) {
  const PnpParams p = pnp_params(fx, fy, cx, cy, scale_px, inlier_px, min_z, H, W);
  return BundleParams{fx, fy, cx, cy, p.c2, p.thr, min_z, p.rho_behind, min_views, iters, stride};
}

ATDN_HD inline int ba_tri(int n) { return n * (n + 1) / 2; }
ATDN_HD inline int ba_ut(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }   // i <= j
ATDN_HD inline int ba_sums(int S) { return ba_tri(6 * S) + 6 * S + BA_VIEW_TERMS * S + 1; }
ATDN_HD inline int ba_grid(int extent, int stride) { return (extent + stride - 1) / stride; }
ATDN_HD inline long ba_positions(int H, int W, int stride) { return (long)ba_grid(H, stride) * ba_grid(W, stride); }
ATDN_HD inline long ba_chunks(int H, int W, int stride) { return (ba_positions(H, W, stride) + BA_CHUNK - 1) / BA_CHUNK; }

// The solver's state of one problem. Poses are INTERNAL (pnp_host.h), 12 float64 per listed view.
struct BundleState {
  double acc[BA_MAX_VIEWS * MV_POSE];     // the accepted poses
  double trial[BA_MAX_VIEWS * MV_POSE];   // the poses of the next (or the current) evaluation
  double dxi[BA_MAX_N];                   // the pose step that leads from acc to trial
  double lambda;                          // the damping of that step
  double cost, cost0;                     // the accepted and the initial cost
  int counts[3];                          // candidates, observations in front, those within inlier_px, at the accepted state
  int accepted;                           // number of accepted steps
  int last_accept;                        // whether the last evaluation was accepted: rho trial becomes rho accepted
  int step_ok;                            // whether dxi is a step (otherwise trial = acc and rho stays)
  int held;                               // the held gauge unknown, -1: none (nothing is solved)
  int slot[BA_MAX_VIEWS];                 // bank index per listed view, -1: empty
};

// Whether view k observes flat index p = pixel (x, y): alive and its correspondence inside (multiview_pixel's test).
ATDN_HD inline bool ba_observe(const float* acc_bank, const unsigned char* alive_bank, long k, long n, long p, int x, int y, int H,
                               int W, double* x2, double* y2) {
#pragma clang fp contract(off)
  const float* a = acc_bank + 2 * k * n + p;
  const float u = a[0], v = a[n];
  const bool alive = alive_bank[k * n + p] != 0;
  *x2 = (double)x + (double)u;
  *y2 = (double)y + (double)v;
  return alive && *x2 >= 0.0 && *x2 <= (double)(W - 1) && *y2 >= 0.0 && *y2 <= (double)(H - 1);
}

ATDN_HD inline void ba_ray(int x, int y, const BundleParams& c, double* a0, double* a1) {
#pragma clang fp contract(off)
  const double dx = (double)x - c.cx, dy = (double)y - c.cy;
  *a0 = dx / c.fx;
  *a1 = dy / c.fy;
}

// One observed view of a candidate at internal pose P and inverse depth rho: t[27] = H_s (21, upper triangle row by row) and g_s
// (6), E[6] = w J_pose^T J_rho, *cs = w J_rho^T J_rho, *bs = w J_rho^T r, *cost. Returns the BA_* bits. Behind the camera: all
// terms +0.0 and the cost rho_behind.
ATDN_HD inline int ba_view(const double* P, double a0, double a1, double rho, double x2, double y2, const BundleParams& c, double* t,
                           double* E, double* cs, double* bs, double* cost) {
#pragma clang fp contract(off)
  const double m0 = (P[0] * a0 + P[1] * a1) + P[2];
  const double m1 = (P[3] * a0 + P[4] * a1) + P[5];
  const double m2 = (P[6] * a0 + P[7] * a1) + P[8];
  const double r0 = rho * P[9], r1 = rho * P[10], r2 = rho * P[11];
  const double P0 = m0 + r0, P1 = m1 + r1, P2 = m2 + r2;
  const double zlim = c.min_z * rho;
  if (!(P2 >= zlim)) {
#pragma unroll
    for (int i = 0; i < BA_VIEW_TERMS; ++i) t[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) E[i] = 0.0;
    *cs = 0.0;
    *bs = 0.0;
    *cost = c.rho_behind;
    return 0;
  }
  const double iz = 1.0 / P2;
  const double fX = c.fx * P0, fY = c.fy * P1;
  const double px = fX * iz, py = fY * iz;
  const double pxc = px + c.cx, pyc = py + c.cy;
  const double rx = pxc - x2, ry = pyc - y2;
  const double rxx = rx * rx, ryy = ry * ry;
  const double e2 = rxx + ryy;
  const double q = e2 / c.c2;
  const double sc = 1.0 + q;
  const double ss = sc * sc;
  const double w = 1.0 / ss;
  const double he = 0.5 * e2;
  const double ax = c.fx * iz, ay = c.fy * iz;
  const double pxiz = px * iz, pyiz = py * iz;
  const double bx = -pxiz, by = -pyiz;               // A = [[ax, 0, bx], [0, ay, by]]
  const double bxm1 = bx * m1, bxm0 = bx * m0, axm2 = ax * m2, axm1 = ax * m1;
  const double bym1 = by * m1, bym0 = by * m0, aym2 = ay * m2, aym0 = ay * m0;
  const double Jx[6] = {bxm1, axm2 - bxm0, -axm1, rho * ax, 0.0, rho * bx};      // -A [m]x, rho A
  const double Jy[6] = {bym1 - aym2, -bym0, aym0, 0.0, rho * ay, rho * by};
  const double jx0 = ax * P[9], jx2 = bx * P[11], jy1 = ay * P[10], jy2 = by * P[11];
  const double jrx = jx0 + jx2, jry = jy1 + jy2;      // A tc
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
    const double ex = wx * jrx, ey = wy * jry;
    E[i] = ex + ey;
  }
  const double wrx = w * jrx, wry = w * jry;
  const double cx_ = wrx * jrx, cy_ = wry * jry;
  *cs = cx_ + cy_;
  const double bx_ = wrx * rx, by_ = wry * ry;
  *bs = bx_ + by_;
  *cost = he / sc;
  return BA_FRONT | (e2 <= c.thr ? BA_INLIER : 0);
}

// E . d over the six pose unknowns of a view, ascending
ATDN_HD inline double ba_dot6(const double* E, const double* d) {
#pragma clang fp contract(off)
  double v = E[0] * d[0];
#pragma unroll
  for (int i = 1; i < 6; ++i) {
    const double p = E[i] * d[i];
    v = v + p;
  }
  return v;
}

// The depth step of a candidate from its sums at the accepted state: c, b, e = E . dxi. The accepted rho is kept where c is
// not > 0 or where the trial is not in (0, DBL_MAX].
ATDN_HD inline double ba_backsub(double c, double b, double e, double lambda, double rho) {
#pragma clang fp contract(off)
  if (!(c > 0.0)) return rho;
  const double num = b + e;
  const double opl = 1.0 + lambda;
  const double den = c * opl;
  const double st = num / den;
  const double rt = rho - st;
  return rt > 0.0 && rt <= DBL_MAX ? rt : rho;
}

// Evaluation 0 of a problem: the internal poses of the listed views and the held gauge unknown.
ATDN_HD inline void ba_init_state(BundleState& s, const float* poses, const int* slots_b, int N, int S) {
  int g = -1;
  for (int v = 0; v < BA_MAX_VIEWS; ++v) {
    s.slot[v] = -1;
    for (int i = 0; i < MV_POSE; ++i) s.trial[v * MV_POSE + i] = s.acc[v * MV_POSE + i] = 0.0;
  }
  for (int v = 0; v < S; ++v) {
    multiview_view(poses, slots_b, N, v, s.slot, s.trial);
    if (s.slot[v] >= 0) g = v;
  }
  for (int i = 0; i < BA_MAX_N; ++i) s.dxi[i] = 0.0;
  s.held = -1;
  if (g >= 0) {
    const double* tc = s.trial + g * MV_POSE + 9;
    int j = 0;
    double best = tc[0] < 0.0 ? -tc[0] : tc[0];
    for (int i = 1; i < 3; ++i) {
      const double a = tc[i] < 0.0 ? -tc[i] : tc[i];
      if (a > best) { best = a; j = i; }
    }
    if (best > 0.0) s.held = 6 * g + 3 + j;
  }
  s.step_ok = 0;
  s.last_accept = 0;
}

// After evaluation k with cost `cost` and counts `cnt` at s.trial: the decision of plane_lm_update. Returns it.
ATDN_HD inline bool ba_decide(BundleState& s, double cost, const int* cnt, int k) {
#pragma clang fp contract(off)
  const bool accept = k == 0 || cost < s.cost;
  if (accept) {
    for (int i = 0; i < BA_MAX_VIEWS * MV_POSE; ++i) s.acc[i] = s.trial[i];
    s.cost = cost;
    for (int i = 0; i < 3; ++i) s.counts[i] = cnt[i];
  }
  if (k == 0) {
    s.lambda = 1e-3;
    s.accepted = 0;
    s.cost0 = cost;
  } else {
    s.lambda = lm_lambda(s.lambda, accept);
    if (accept) s.accepted += 1;
  }
  s.last_accept = accept ? 1 : 0;
  return accept;
}

ATDN_HD inline bool ba_is_held(const BundleState& s, int i) { return s.slot[i / 6] < 0 || i == s.held; }

// Entry (i, j), i <= j, of S_lambda from the accepted sums: H + lambda diag(H) - T0 / (1 + lambda), held unknowns as identity.
ATDN_HD inline double ba_system_entry(const double* sums, const BundleState& s, int S, int i, int j) {
#pragma clang fp contract(off)
  const int n = 6 * S;
  if (ba_is_held(s, i) || ba_is_held(s, j)) return i == j ? 1.0 : 0.0;
  const int vi = i / 6, vj = j / 6;
  double h = 0.0;
  if (vi == vj) h = sums[ba_tri(n) + n + BA_VIEW_TERMS * vi + ba_ut(6, i - 6 * vi, j - 6 * vi)];
  const double opl = 1.0 + s.lambda;
  const double d = sums[ba_ut(n, i, j)] / opl;
  if (i == j) {
    const double l = s.lambda * h;
    const double hl = h + l;
    return hl - d;
  }
  return h - d;
}

// Entry i of the right-hand side of the step: -(g - v0 / (1 + lambda)), +0.0 for a held unknown.
ATDN_HD inline double ba_rhs_entry(const double* sums, const BundleState& s, int S, int i) {
#pragma clang fp contract(off)
  const int n = 6 * S;
  if (ba_is_held(s, i)) return 0.0;
  const int vi = i / 6;
  const double g = sums[ba_tri(n) + n + BA_VIEW_TERMS * vi + 21 + (i - 6 * vi)];
  const double opl = 1.0 + s.lambda;
  const double d = sums[ba_tri(n) + i] / opl;
  const double r = g - d;
  return -r;
}

// LDL^T without pivoting of a symmetric n x n matrix in packed upper storage U (entry (j, i), j <= i, at ba_ut(n, j, i), standing
// for A_ij and then L_ij), ldl6_factor's term order: ldln_col is A_ij - sum_k L_ik (L_jk d_k), k < j ascending, term by term;
// for i == j that is the pivot d_j, otherwise L_ij is the value divided by d_j.
ATDN_HD inline double ldln_col(const double* U, const double* D, int n, int i, int j) {
#pragma clang fp contract(off)
  double a = U[ba_ut(n, j, i)];
  int k = 0;
  // blocks of eight: the products do not depend on the running value, so their reads are in flight together; the
  // subtractions stay one after the other in ascending k
  for (; k + 8 <= j; k += 8) {
    double lld[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double ld = U[ba_ut(n, k + u, j)] * D[k + u];
      lld[u] = U[ba_ut(n, k + u, i)] * ld;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) a = a - lld[u];
  }
  for (; k < j; ++k) {
    const double ld = U[ba_ut(n, k, j)] * D[k];
    const double lld = U[ba_ut(n, k, i)] * ld;
    a = a - lld;
  }
  return a;
}

// x = A^-1 x for the factor (U, D), ldl6_solve's order.
ATDN_HD inline void ldln_solve(const double* U, const double* D, int n, double* x) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; ++i) {
    double v = x[i];
    int k = 0;
    for (; k + 8 <= i; k += 8) {                  // blocks of eight, as in ldln_col
      double ly[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) ly[u] = U[ba_ut(n, k + u, i)] * x[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) v = v - ly[u];
    }
    for (; k < i; ++k) {
      const double ly = U[ba_ut(n, k, i)] * x[k];
      v = v - ly;
    }
    x[i] = v;
  }
  for (int i = 0; i < n; ++i) x[i] = x[i] / D[i];
  for (int i = n - 1; i >= 0; --i) {
    double v = x[i];
    int k = i + 1;
    for (; k + 8 <= n; k += 8) {
      double ly[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) ly[u] = U[ba_ut(n, i, k + u)] * x[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) v = v - ly[u];
    }
    for (; k < n; ++k) {
      const double ly = U[ba_ut(n, i, k)] * x[k];
      v = v - ly;
    }
    x[i] = v;
  }
}

// After the solve: whether x (n values) is a step. ok: every pivot was positive. Writes s.dxi and s.step_ok.
ATDN_HD inline void ba_take_step(BundleState& s, const double* x, int n, bool ok) {
  ok = ok && s.held >= 0;
  for (int i = 0; i < n; ++i) ok = ok && x[i] >= -DBL_MAX && x[i] <= DBL_MAX;
  for (int i = 0; i < n; ++i) s.dxi[i] = ok ? x[i] : 0.0;
  s.step_ok = ok ? 1 : 0;
}

// The trial pose of listed view v: Rc <- cayley3(dw) Rc, tc <- tc + dt; the accepted pose where there is no step.
ATDN_HD inline void ba_retract_view(BundleState& s, int v) {
#pragma clang fp contract(off)
  const double* a = s.acc + v * MV_POSE;
  double* t = s.trial + v * MV_POSE;
  if (!s.step_ok || s.slot[v] < 0) {
    for (int i = 0; i < MV_POSE; ++i) t[i] = a[i];
    return;
  }
  const double* d = s.dxi + 6 * v;
  double E[9];
  cayley3(d, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) t[3 * i + j] = dot3(E[3 * i], a[j], E[3 * i + 1], a[3 + j], E[3 * i + 2], a[6 + j]);
    t[9 + i] = a[9 + i] + d[3 + i];
  }
}

// The pose row of listed view v of a finished solve.
ATDN_HD inline void ba_output_pose(const BundleState& s, const float* poses, int v, float* out12) {
  if (s.slot[v] < 0) {
    for (int i = 0; i < 12; ++i) out12[i] = 0.0f;
  } else if (s.accepted == 0) {
    for (int i = 0; i < 12; ++i) out12[i] = poses[12L * s.slot[v] + i];
  } else {
    pnp_public_pose(s.acc + v * MV_POSE, out12);
  }
}

ATDN_HD inline void ba_output_scalars(const BundleState& s, double* cost2, int* counts4) {
  cost2[0] = s.cost0;
  cost2[1] = s.cost;
  for (int i = 0; i < 3; ++i) counts4[i] = s.counts[i];
  counts4[3] = s.accepted;
}

// the depth of a position from its final rho (0: no candidate)
ATDN_HD inline float ba_output_depth(double rho) {
#pragma clang fp contract(off)
  return rho > 0.0 ? (float)(1.0 / rho) : 0.0f;
}

// ------------------------------------------------------------------ host forms
// One evaluation of problem b: poses `Pt` (trial), and for back = true first the depth step from `Pa` (accepted), dxi, lambda.
// rho_acc / rho_trial [positions]; first: rho accepted is 1 / depth_init; commit: rho trial becomes rho accepted first.
inline void bundle_eval_host(const float* acc_bank, const unsigned char* alive_bank, const float* z0, const unsigned char* mask,
                             const BundleState& s, int S, int H, int W, const BundleParams& c, bool first, double* rho_acc,
                             double* rho_trial, double* sums, int* cnt) {
#pragma clang fp contract(off)
  const long n = (long)H * W;
  const int nu = 6 * S, NS = ba_sums(S);
  const int Ws = ba_grid(W, c.stride);
  const long npos = ba_positions(H, W, c.stride), chunks = ba_chunks(H, W, c.stride);
  std::vector<double> cs((size_t)NS);
  for (int e = 0; e < NS; ++e) sums[e] = 0.0;
  cnt[0] = cnt[1] = cnt[2] = 0;
  for (long ch = 0; ch < chunks; ++ch) {
    for (int e = 0; e < NS; ++e) cs[e] = 0.0;
    for (long q = ch * BA_CHUNK; q < (ch + 1) * BA_CHUNK && q < npos; ++q) {
      const int y = (int)(q / Ws) * c.stride, x = (int)(q % Ws) * c.stride;
      const long p = (long)y * W + x;
      double x2[BA_MAX_VIEWS], y2[BA_MAX_VIEWS];
      bool obs[BA_MAX_VIEWS];
      int n_obs = 0;
      for (int v = 0; v < S; ++v) {
        obs[v] = s.slot[v] >= 0 && ba_observe(acc_bank, alive_bank, s.slot[v], n, p, x, y, H, W, x2 + v, y2 + v);
        n_obs += obs[v] ? 1 : 0;
      }
      const double zd = (double)z0[p];
      const bool cand = (mask ? mask[p] != 0 : true) && zd > 0.0 && zd <= (double)FLT_MAX && n_obs >= c.min_views;
      if (!cand) {
        rho_acc[q] = 0.0;
        rho_trial[q] = 0.0;
        continue;
      }
      double a0, a1;
      ba_ray(x, y, c, &a0, &a1);
      double ra = first ? 1.0 / zd : (s.last_accept ? rho_trial[q] : rho_acc[q]);
      double rt = ra;
      double t[BA_MAX_VIEWS][BA_VIEW_TERMS], E[6 * BA_MAX_VIEWS], cv, bv, costv;
      if (!first && s.step_ok) {
        double cc = 0.0, bb = 0.0, ee = 0.0;
        for (int v = 0; v < S; ++v) {
          if (!obs[v]) continue;
          ba_view(s.acc + v * MV_POSE, a0, a1, ra, x2[v], y2[v], c, t[v], E + 6 * v, &cv, &bv, &costv);
          const double ev = ba_dot6(E + 6 * v, s.dxi + 6 * v);
          cc = cc + cv;
          bb = bb + bv;
          ee = ee + ev;
        }
        rt = ba_backsub(cc, bb, ee, s.lambda, ra);
      }
      rho_acc[q] = ra;
      rho_trial[q] = rt;
      double cc = 0.0, bb = 0.0, cost = 0.0;
      for (int v = 0; v < S; ++v) {
        if (!obs[v]) {
          for (int i = 0; i < BA_VIEW_TERMS; ++i) t[v][i] = 0.0;
          for (int i = 0; i < 6; ++i) E[6 * v + i] = 0.0;
          continue;
        }
        const int f = ba_view(s.trial + v * MV_POSE, a0, a1, rt, x2[v], y2[v], c, t[v], E + 6 * v, &cv, &bv, &costv);
        cc = cc + cv;
        bb = bb + bv;
        cost = cost + costv;
        cnt[1] += (f & BA_FRONT) ? 1 : 0;
        cnt[2] += (f & BA_INLIER) ? 1 : 0;
      }
      cnt[0] += 1;
      cs[NS - 1] = cs[NS - 1] + cost;
      if (!(cc > 0.0)) continue;
      const double ic = 1.0 / cc;
      const double bc = bb * ic;
      int e = 0;
      for (int i = 0; i < nu; ++i) {
        const double F = E[i] * ic;
        for (int j = i; j < nu; ++j, ++e) {
          const double f = F * E[j];
          cs[e] = cs[e] + f;
        }
      }
      for (int i = 0; i < nu; ++i, ++e) {
        const double f = E[i] * bc;
        cs[e] = cs[e] + f;
      }
      for (int v = 0; v < S; ++v)
        for (int i = 0; i < BA_VIEW_TERMS; ++i, ++e) cs[e] = cs[e] + t[v][i];
    }
    for (int e = 0; e < NS; ++e) sums[e] = sums[e] + cs[e];
  }
}

// The step on the reduced system from the accepted sums (destroyed): dxi, step_ok and the trial poses of s.
inline void bundle_step_host(BundleState& s, double* sums, int S) {
  const int n = 6 * S;
  double D[BA_MAX_N], x[BA_MAX_N];
  for (int i = 0; i < n; ++i) x[i] = ba_rhs_entry(sums, s, S, i);
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) sums[ba_ut(n, i, j)] = ba_system_entry(sums, s, S, i, j);
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    const double d = ldln_col(sums, D, n, j, j);
    D[j] = d;
    ok = ok && d > 0.0;
    for (int i = j + 1; i < n; ++i) sums[ba_ut(n, j, i)] = ldln_col(sums, D, n, i, j) / d;
  }
  ldln_solve(sums, D, n, x);
  ba_take_step(s, x, n, ok);
  for (int v = 0; v < S; ++v) ba_retract_view(s, v);
}

// acc_bank [N,2,H,W], alive_bank [N,H,W], poses [N,12], slots [B,S], depth [B,1,H,W], mask [B,H,W] or null ->
// sums [B, ba_sums(S)], counts [B,3]
inline void bundle_terms_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                              const float* depth, const unsigned char* mask, int N, int B, int S, int H, int W,
                              const BundleParams& c, double* sums, int* counts) {
  const long n = (long)H * W, npos = ba_positions(H, W, c.stride);
  std::vector<double> ra((size_t)npos), rt((size_t)npos);
  for (int b = 0; b < B; ++b) {
    BundleState s;
    ba_init_state(s, poses, slots + (long)b * S, N, S);
    bundle_eval_host(acc_bank, alive_bank, depth + b * n, mask ? mask + b * n : nullptr, s, S, H, W, c, true, ra.data(), rt.data(),
                     sums + (long)b * ba_sums(S), counts + 3L * b);
  }
}

// -> poses_out [B,S,12], depth [B,1,H,W], cost [B,2], counts [B,4]
inline void bundle_adjust_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                               const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W,
                               const BundleParams& c, float* poses_out, float* depth, double* cost, int* counts) {
  const long n = (long)H * W, npos = ba_positions(H, W, c.stride);
  const int NS = ba_sums(S), Ws = ba_grid(W, c.stride);
  std::vector<double> ra((size_t)npos), rt((size_t)npos), sums((size_t)NS), acc_sums((size_t)NS);
  for (int b = 0; b < B; ++b) {
    BundleState s;
    ba_init_state(s, poses, slots + (long)b * S, N, S);
    for (int k = 0; k <= c.iters; ++k) {
      int cnt[3];
      bundle_eval_host(acc_bank, alive_bank, depth_init + b * n, mask ? mask + b * n : nullptr, s, S, H, W, c, k == 0, ra.data(),
                       rt.data(), sums.data(), cnt);
      if (ba_decide(s, sums[NS - 1], cnt, k)) acc_sums = sums;
      if (k < c.iters) {
        sums = acc_sums;
        bundle_step_host(s, sums.data(), S);
      }
    }
    for (int v = 0; v < S; ++v) ba_output_pose(s, poses, v, poses_out + ((long)b * S + v) * 12);
    ba_output_scalars(s, cost + 2L * b, counts + 4L * b);
    for (long p = 0; p < n; ++p) depth[b * n + p] = 0.0f;
    for (long q = 0; q < npos; ++q) {
      const long p = (long)((q / Ws) * c.stride) * W + (q % Ws) * c.stride;
      depth[b * n + p] = ba_output_depth(s.last_accept ? rt[q] : ra[q]);
    }
  }
}

}  // namespace atdn
