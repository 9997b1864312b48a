// Composite pose term of CLVO_Loss (odometry/loss.py:60-101) and its hand-derived gradient: the per-item arithmetic of
// clvo_loss_composite_kernel (train_kernels.hip), in double. Plain C++ (host and device), no memory traffic of its own.
//
// A pose (Euler "yxz" angles r, translation t) is the affine map P = [R(r) t; 0 0 0 1] (transforms.py:79-81,97-119); a
// window's product C = P_j ... P_{j+w-1} is converted back as matrix2euler does (transforms.py:41-44):
//   a = atan2(C02, C22),  b = atan2(-C12, sqrt(1 - C12^2)),  g = atan2(C10, C11),  translation C[:3,3]
// and the window loss is l = |dt|^2 + 100 |d euler|^2 against the same quantities of the targets (no angle wrapping).
//
// Clamps (the only departures from the reference, and only where it returns NaN): the radicand 1 - C12^2 is clamped at 0
// from below for the value and at FLT_EPSILON in the derivative db/dC12 = -1/sqrt(1 - C12^2); the squared radii
// C02^2 + C22^2 and C10^2 + C11^2 in the atan2 derivatives are clamped at DBL_MIN (both vanish only at pitch +-pi/2).
#pragma once
#include <cfloat>
#include <cmath>

#include "pixel_rule.h"   // ATDN_HD

namespace atdn {
namespace composite {

constexpr double kDelta = 1.0, kKhi = 100.0;   // loss.py:20-21

struct Affine {   // [r t; 0 0 0 1], r row-major 3x3. Also holds dl/dC (the bottom row of C is constant)
  double r[9];
  double t[3];
};

ATDN_HD inline Affine identity() {
  Affine a;
  for (int i = 0; i < 9; ++i) a.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
  a.t[0] = a.t[1] = a.t[2] = 0.0;
  return a;
}

ATDN_HD inline Affine mul(const Affine& a, const Affine& b) {
  Affine c;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) c.r[i * 3 + j] = a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j] + a.r[i * 3 + 2] * b.r[6 + j];
    c.t[i] = a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1] + a.r[i * 3 + 2] * b.t[2] + a.t[i];
  }
  return c;
}

ATDN_HD inline Affine from_pose(const float* rot, const float* tr) {
  const double c1 = cos((double)rot[0]), c2 = cos((double)rot[1]), c3 = cos((double)rot[2]);
  const double s1 = sin((double)rot[0]), s2 = sin((double)rot[1]), s3 = sin((double)rot[2]);
  Affine p;
  p.r[0] = c1 * c3 + s1 * s2 * s3; p.r[1] = c3 * s1 * s2 - c1 * s3; p.r[2] = c2 * s1;
  p.r[3] = c2 * s3;                p.r[4] = c2 * c3;                p.r[5] = -s2;
  p.r[6] = c1 * s2 * s3 - c3 * s1; p.r[7] = c1 * c3 * s2 + s1 * s3; p.r[8] = c1 * c2;
  p.t[0] = (double)tr[0]; p.t[1] = (double)tr[1]; p.t[2] = (double)tr[2];
  return p;
}

// p[first] p[first+1] ... p[first+count-1]; the identity for count == 0
ATDN_HD inline Affine chain(const Affine* p, int first, int count) {
  if (count <= 0) return identity();
  Affine c = p[first];
  for (int i = 1; i < count; ++i) c = mul(c, p[first + i]);
  return c;
}

ATDN_HD inline void to_euler(const Affine& c, double e[3]) {
  const double rad = 1.0 - c.r[5] * c.r[5];
  e[0] = atan2(c.r[2], c.r[8]);
  e[1] = atan2(-c.r[5], sqrt(rad > 0.0 ? rad : 0.0));
  e[2] = atan2(c.r[3], c.r[4]);
}

// Loss of one window from the two products; g (optional) receives dl/dC of the predicted product.
ATDN_HD inline double window_loss(const Affine& cp, const Affine& ct, Affine* g) {
  double ep[3], et[3];
  to_euler(cp, ep);
  to_euler(ct, et);
  const double ea = ep[0] - et[0], eb = ep[1] - et[1], eg = ep[2] - et[2];
  const double d0 = cp.t[0] - ct.t[0], d1 = cp.t[1] - ct.t[1], d2 = cp.t[2] - ct.t[2];
  if (g) {
    for (int i = 0; i < 9; ++i) g->r[i] = 0.0;
    double n = cp.r[2] * cp.r[2] + cp.r[8] * cp.r[8];
    n = n > DBL_MIN ? n : DBL_MIN;
    g->r[2] = 2.0 * kKhi * ea * (cp.r[8] / n);
    g->r[8] = 2.0 * kKhi * ea * (-cp.r[2] / n);
    double rad = 1.0 - cp.r[5] * cp.r[5];
    rad = rad > (double)FLT_EPSILON ? rad : (double)FLT_EPSILON;
    g->r[5] = 2.0 * kKhi * eb * (-1.0 / sqrt(rad));
    n = cp.r[3] * cp.r[3] + cp.r[4] * cp.r[4];
    n = n > DBL_MIN ? n : DBL_MIN;
    g->r[3] = 2.0 * kKhi * eg * (cp.r[4] / n);
    g->r[4] = 2.0 * kKhi * eg * (-cp.r[3] / n);
    g->t[0] = 2.0 * kDelta * d0; g->t[1] = 2.0 * kDelta * d1; g->t[2] = 2.0 * kDelta * d2;
  }
  return kDelta * (d0 * d0 + d1 * d1 + d2 * d2) + kKhi * (ea * ea + eb * eb + eg * eg);
}

// d L_com / d (rot_i, tr_i) of one clip: p[0..T) its predicted transforms, g[0..T-w] its windows' dl/dC. Step i sits in the
// windows j = max(0, i-w+1) .. min(i, T-w), summed in ascending j. With A = P_j..P_{i-1} and S = P_{i+1}..P_{j+w-1},
// C = A P_i S and the top three rows of dl/dP_i = A^T G S^T are  M = Ra^T G  ->  dR = M[:, :3] Rs^T + M[:, 3] ts^T,  dt = M[:, 3].
ATDN_HD inline void step_gradient(const Affine* p, const Affine* g, int T, int w, int i, const float* rot, double d_rot[3],
                                  double d_tr[3]) {
  double dR[9], dt[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < 9; ++k) dR[k] = 0.0;
  const int j0 = i - w + 1 > 0 ? i - w + 1 : 0, j1 = i < T - w ? i : T - w;
  for (int j = j0; j <= j1; ++j) {
    const Affine A = chain(p, j, i - j), S = chain(p, i + 1, j + w - 1 - i);
    const Affine& G = g[j];
    double M[9], m[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) M[r * 3 + c] = A.r[r] * G.r[c] + A.r[3 + r] * G.r[3 + c] + A.r[6 + r] * G.r[6 + c];
      m[r] = A.r[r] * G.t[0] + A.r[3 + r] * G.t[1] + A.r[6 + r] * G.t[2];
    }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        dR[r * 3 + c] += M[r * 3] * S.r[c * 3] + M[r * 3 + 1] * S.r[c * 3 + 1] + M[r * 3 + 2] * S.r[c * 3 + 2] + m[r] * S.t[c];
      dt[r] += m[r];
    }
  }
  const double c1 = cos((double)rot[0]), c2 = cos((double)rot[1]), c3 = cos((double)rot[2]);
  const double s1 = sin((double)rot[0]), s2 = sin((double)rot[1]), s3 = sin((double)rot[2]);
  // entries of dR/d(angle) of the yxz matrix, row-major
  const double q1[9] = {-s1 * c3 + c1 * s2 * s3, c3 * c1 * s2 + s1 * s3, c2 * c1,
                        0.0, 0.0, 0.0,
                        -s1 * s2 * s3 - c3 * c1, -s1 * c3 * s2 + c1 * s3, -s1 * c2};
  const double q2[9] = {s1 * c2 * s3, c3 * s1 * c2, -s2 * s1,
                        -s2 * s3, -s2 * c3, -c2,
                        c1 * c2 * s3, c1 * c3 * c2, -c1 * s2};
  const double q3[9] = {-c1 * s3 + s1 * s2 * c3, -s3 * s1 * s2 - c1 * c3, 0.0,
                        c2 * c3, -c2 * s3, 0.0,
                        c1 * s2 * c3 + s3 * s1, -c1 * s3 * s2 + s1 * c3, 0.0};
  d_rot[0] = d_rot[1] = d_rot[2] = 0.0;
  for (int k = 0; k < 9; ++k) {
    d_rot[0] += q1[k] * dR[k];
    d_rot[1] += q2[k] * dR[k];
    d_rot[2] += q3[k] * dR[k];
  }
  d_tr[0] = dt[0]; d_tr[1] = dt[1]; d_tr[2] = dt[2];
}

}  // namespace composite
}  // namespace atdn
