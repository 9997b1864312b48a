// What the float64 pose solvers (pnp_host.h, pose_graph_host.h) share, in plain C++ (no HIP needed): the algebra of one damped
// 6 x 6 Levenberg-Marquardt step over a pose increment (dw, dt). Everything in float64, only + - * / and comparisons, every
// operation rounded on its own (fp contraction off), in exactly this order:
//   dot3         (a0 b0 + a1 b1) + a2 b2
//   ldl6_factor  A = L D L^T without pivoting, column j = 0 .. 5: d_j = A_jj - sum_k L_jk (L_jk d_k) and, for i > j,
//                L_ij = (A_ij - sum_k L_ik (L_jk d_k)) / d_j, each sum subtracted term by term in ascending k < j
//   ldl6_solve   forward y_i = b_i - sum_{k<i} L_ik y_k, then y_i / d_i, then backward x_i = y_i - sum_{k>i} L_ki x_k from i = 5 down,
//                each sum subtracted term by term in ascending k
//   cayley3      the rotation (I - K)^-1 (I + K) of the step w, K = [w / 2]x: with h = w / 2, n2 = (h0^2 + h1^2) + h2^2 and
//                f = 2 / (1 + n2): C_ii = 1 + f (h_i^2 - n2), C_ij = f (K_ij + h_i h_j); orthogonal for every w, no trigonometry
//   ldl3_factor / ldl3_solve   the same two recurrences for a 3 x 3 system (the ground plane's step, ground_host.h)
//   lm_lambda    the damping after a decision: / 3 and not below 1e-9 on acceptance, * 4 and not above 1e6 on rejection
// On which side a solver multiplies the Cayley matrix onto its pose is the solver's own business (PnP: from the left, the pose
// graph: from the right). The bits of kernel, host form and NumPy restatement agree because this order is written once, here.
#pragma once
#include <cfloat>

#include "pixel_rule.h"

namespace atdn {

ATDN_HD inline double dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
#pragma clang fp contract(off)
  const double x = a0 * b0, y = a1 * b1, z = a2 * b2;
  const double xy = x + y;
  return xy + z;
}

// A: symmetric, flat row-major; only the diagonal and the lower triangle are read. F: L rows 1 .. 5 (15 values, row i at
// i (i - 1) / 2), then the 6 pivots. Returns false on a non-positive pivot. No early exit: after a failed pivot the remaining
// values are garbage that is computed and never used.
ATDN_HD inline bool ldl6_factor(const double* A, double* F) {
#pragma clang fp contract(off)
  double L[6][6], D[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[7 * j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double ld = L[j][k] * D[k];
      const double lld = L[j][k] * ld;
      dj = dj - lld;
    }
    ok = ok && dj > 0.0;
    D[j] = dj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double l = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const double ld = L[j][k] * D[k];
        const double lld = L[i][k] * ld;
        l = l - lld;
      }
      L[i][j] = l / dj;
    }
  }
#pragma unroll
  for (int i = 1; i < 6; ++i)
#pragma unroll
    for (int k = 0; k < i; ++k) F[i * (i - 1) / 2 + k] = L[i][k];
#pragma unroll
  for (int i = 0; i < 6; ++i) F[15 + i] = D[i];
  return ok;
}

// x = A^-1 b for the factor F of A; x may be b.
ATDN_HD inline void ldl6_solve(const double* F, const double* b, double* x) {
#pragma clang fp contract(off)
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) {
      const double ly = F[i * (i - 1) / 2 + k] * y[k];
      v = v - ly;
    }
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = y[i] / F[15 + i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) {
      const double ly = F[k * (k - 1) / 2 + i] * y[k];
      v = v - ly;
    }
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = y[i];
}

// The same factorisation and solve for a 3 x 3 system (the ground plane's step, ground_host.h): the recurrences of ldl6_factor /
// ldl6_solve with 6 replaced by 3. A: flat row-major, diagonal and lower triangle read. F: L rows 1 .. 2 (3 values, row i at
// i (i - 1) / 2), then the 3 pivots.
ATDN_HD inline bool ldl3_factor(const double* A, double* F) {
#pragma clang fp contract(off)
  double L[3][3], D[3];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double dj = A[4 * j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double ld = L[j][k] * D[k];
      const double lld = L[j][k] * ld;
      dj = dj - lld;
    }
    ok = ok && dj > 0.0;
    D[j] = dj;
#pragma unroll
    for (int i = j + 1; i < 3; ++i) {
      double l = A[3 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const double ld = L[j][k] * D[k];
        const double lld = L[i][k] * ld;
        l = l - lld;
      }
      L[i][j] = l / dj;
    }
  }
  F[0] = L[1][0]; F[1] = L[2][0]; F[2] = L[2][1];
#pragma unroll
  for (int i = 0; i < 3; ++i) F[3 + i] = D[i];
  return ok;
}

// x = A^-1 b for the factor F (ldl3_factor) of A; x may be b.
ATDN_HD inline void ldl3_solve(const double* F, const double* b, double* x) {
#pragma clang fp contract(off)
  double y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) {
      const double ly = F[i * (i - 1) / 2 + k] * y[k];
      v = v - ly;
    }
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = y[i] / F[3 + i];
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 3; ++k) {
      const double ly = F[k * (k - 1) / 2 + i] * y[k];
      v = v - ly;
    }
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = y[i];
}

ATDN_HD inline bool finite3(const double* v) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && v[k] >= -DBL_MAX && v[k] <= DBL_MAX;
  return ok;
}

// C (3 x 3, row-major) = the Cayley matrix of the rotation step w[0..2]
ATDN_HD inline void cayley3(const double* w, double* C) {
#pragma clang fp contract(off)
  const double h[3] = {0.5 * w[0], 0.5 * w[1], 0.5 * w[2]};
  const double h00 = h[0] * h[0], h11 = h[1] * h[1], h22 = h[2] * h[2];
  const double h01 = h00 + h11;
  const double n2 = h01 + h22;
  const double den = 1.0 + n2;
  const double f = 2.0 / den;
  const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double hh = h[i] * h[j];
      const double m = i == j ? hh - n2 : K[3 * i + j] + hh;
      const double fm = f * m;
      C[3 * i + j] = i == j ? 1.0 + fm : fm;
    }
}

// whether every entry of the step v[0..5] is a finite number (a NaN fails)
ATDN_HD inline bool finite6(const double* v) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) ok = ok && v[k] >= -DBL_MAX && v[k] <= DBL_MAX;
  return ok;
}

ATDN_HD inline double lm_lambda(double lambda, bool accept) {
#pragma clang fp contract(off)
  if (accept) {
    const double l = lambda / 3.0;
    return l > 1e-9 ? l : 1e-9;
  }
  const double l = 4.0 * lambda;
  return l < 1e6 ? l : 1e6;
}

}  // namespace atdn
