// The ground plane of a depth map, the rule in plain C++ float64 (no HIP needed). A camera of known height over a road sees a
// plane n . X = h; with q = n / h and the ray a = ((x - cx) / fx, (y - cy) / fy, 1) of a pixel of depth z the RELATIVE depth
// residual e = z (q . a) - 1 is linear in q, dimensionless, and meaningful when the scale of the depth is wrong — the case the fit
// exists for: the fitted height is (scale error) x (true height). n . X = h (1 + e), so a pixel stands -h e above the road.
//   ground_pixel     the 10 terms of one pixel under the Geman-McClure loss: the 6 upper-triangle entries of the 3 x 3
//                    Gauss-Newton Hessian, row by row, the 3 gradient entries and the cost
//   ground_vote_bin  the bin of a pixel in the start vote: nothing lies below the road, so under a prior normal n0 the ground
//                    pixels share one height z (n0 . a) and everything else spreads over smaller ones; the bin is the exponent and
//                    the top 5 mantissa bits of that float64 (an integer operation on the bit pattern)
//   ground_mode_better / ground_start_vote   the mode of the smoothed 320 bins and the start q of its centre
//   ground_lm_update / ground_lm_step   the decision of plane_lm_update (plane_lm.h) on a 3-vector, and the damped 3 x 3 step
//                    (ldl3_factor / ldl3_solve of lm6.h)
//   ground_classify_pixel   e as float32 and the inlier flag of one pixel
// The plane sum is plane_sum_host<10> of plane_lm.h: the chunks, the 4-sum, the tree and the chunk order of the pose solvers over
// 10 terms. ground_terms_host / ground_solve_host / ground_classify_host are the host forms behind atdn_ground_*_host (ground.hip),
// which serve CPU tensors. The kernels of ground.hip call the same functions, so the two cannot drift apart; the independent
// statement the tests compare both with is tests/ground_ref.py (NumPy). The rule is stated in full in include/atdn_hip.h,
// atdn_ground_terms and atdn_ground_solve; only + - * /, comparisons and integer operations, every operation rounded on its own
// (fp contraction off), no square root: normal and height are formed by the caller from q.
#pragma once
#include <cstdint>

#include "plane_lm.h"

namespace atdn {

constexpr int GROUND_TERMS = 10;          // H00 H01 H02 H11 H12 H22, g0 g1 g2, the cost
constexpr int GROUND_BINS = 320;          // 10 octaves [2^-4, 2^6) x 32 bins
constexpr int GROUND_BIN0 = 1019 * 32;    // (bits of 2^-4) >> 47
enum { GROUND_CAND = 1, GROUND_USED = 2, GROUND_INLIER = 4 };

struct GroundParams {
  double fx, fy, cx, cy;
  double c2;            // scale_rel * scale_rel
  double thr;           // inlier_rel * inlier_rel
  double min_z, max_depth;
  double n0[3];         // the prior normal (any length; the vote divides it by a height)
  int y0, W;            // the band starts at row y0: flat index i of the band is pixel (i % W, y0 + i / W)
  int min_votes;
};

inline GroundParams ground_params(double fx, double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z,
                                  double max_depth, double nx, double ny, double nz, int min_votes, int y0, int W) {
#pragma clang fp contract(off)
  return GroundParams{fx, fy, cx, cy, scale_rel * scale_rel, inlier_rel * inlier_rel, min_z, max_depth, {nx, ny, nz}, y0, W,
                      min_votes};
}

// The solver's state of one problem.
struct GroundState {
  double acc[3];               // the accepted q
  double trial[3];             // the q of the next (or the current) evaluation
  double sums[GROUND_TERMS];   // H, g and cost at the accepted q
  double lambda;
  int counts[3];               // the three counts at the accepted q
  int accepted;                // number of accepted steps
  int votes, bin;              // of the start vote (0, -1 with q_init)
  int plane;                   // 0: the vote found no plane, the outputs are zeros
  int pad;
};

// ray and depth of a pixel; returns whether the candidate is used
ATDN_HD inline bool ground_ray(float zf, const GroundParams& c, int x, int y, double a[2], double* z) {
#pragma clang fp contract(off)
  const double dx = (double)x - c.cx, dy = (double)y - c.cy;
  a[0] = dx / c.fx;
  a[1] = dy / c.fy;
  *z = (double)zf;
  return *z >= c.min_z && *z <= c.max_depth;       // a NaN fails; max_depth is finite
}

// The 10 terms of pixel (x, y) at q: zf its depth, keep its mask. Returns the GROUND_* bits; t is always written (+0.0 where the
// pixel contributes nothing).
ATDN_HD inline int ground_pixel(float zf, bool keep, const double* q, const GroundParams& c, int x, int y,
                                double t[GROUND_TERMS]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < GROUND_TERMS; ++i) t[i] = 0.0;
  if (!keep) return 0;
  double a[2], z;
  if (!ground_ray(zf, c, x, y, a, &z)) return GROUND_CAND;
  const double qa = dot3(q[0], a[0], q[1], a[1], q[2], 1.0);
  const double zq = z * qa;
  const double e = zq - 1.0;
  const double e2 = e * e;
  const double r = e2 / c.c2;
  const double s = 1.0 + r;
  const double ss = s * s;
  const double w = 1.0 / ss;
  const double he = 0.5 * e2;
  const double J[3] = {z * a[0], z * a[1], z};
  int n = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 3; ++j) t[n++] = wj * J[j];
    t[6 + i] = wj * e;
  }
  t[9] = he / s;
  return GROUND_CAND | GROUND_USED | (e2 <= c.thr ? GROUND_INLIER : 0);
}

// The vote bin of pixel (x, y), or -1: not kept, not used, or a height outside [2^-4, 2^6).
ATDN_HD inline int ground_vote_bin(float zf, bool keep, const GroundParams& c, int x, int y) {
#pragma clang fp contract(off)
  if (!keep) return -1;
  double a[2], z;
  if (!ground_ray(zf, c, x, y, a, &z)) return -1;
  const double na = dot3(c.n0[0], a[0], c.n0[1], a[1], c.n0[2], 1.0);
  const double h = z * na;
  uint64_t bits;
  __builtin_memcpy(&bits, &h, 8);
  const int64_t k = (int64_t)(bits >> 47) - GROUND_BIN0;     // a negative h, a NaN or an infinity lands far above 320
  return k >= 0 && k < GROUND_BINS ? (int)k : -1;
}

// smoothed count of bin k of the histogram c
ATDN_HD inline int ground_smoothed(const int* c, int k) {
  return (k > 0 ? c[k - 1] : 0) + c[k] + (k + 1 < GROUND_BINS ? c[k + 1] : 0);
}

// the centre of bin k: its lower edge with the next mantissa bit set
ATDN_HD inline double ground_bin_centre(int k) {
  const uint64_t bits = ((uint64_t)(k + GROUND_BIN0) << 47) | ((uint64_t)1 << 46);
  double h;
  __builtin_memcpy(&h, &bits, 8);
  return h;
}

// The start of a solve from the mode (bin, votes) of the vote: s.trial = n0 / centre, or no plane.
ATDN_HD inline void ground_start_vote(GroundState& s, const GroundParams& c, int bin, int votes) {
#pragma clang fp contract(off)
  s.votes = votes;
  s.bin = bin;
  s.plane = votes >= c.min_votes ? 1 : 0;
  const double h = ground_bin_centre(bin);
  for (int i = 0; i < 3; ++i) s.trial[i] = s.plane ? c.n0[i] / h : 0.0;
}

ATDN_HD inline void ground_start_init(GroundState& s, const double* q_init) {
  s.votes = 0;
  s.bin = -1;
  s.plane = 1;
  for (int i = 0; i < 3; ++i) s.trial[i] = q_init[i];
}

// After evaluation k (k = 0: the start) with the plane sums and counts at s.trial: the decision of plane_lm_update.
ATDN_HD inline void ground_lm_update(GroundState& s, const double* sums, const int* counts, int k) {
#pragma clang fp contract(off)
  const bool accept = k == 0 || sums[9] < s.sums[9];
  if (accept) {
    for (int i = 0; i < 3; ++i) s.acc[i] = s.trial[i];
    for (int i = 0; i < GROUND_TERMS; ++i) s.sums[i] = sums[i];
    for (int i = 0; i < 3; ++i) s.counts[i] = counts[i];
  }
  if (k == 0) {
    s.lambda = 1e-3;
    s.accepted = 0;
  } else {
    s.lambda = lm_lambda(s.lambda, accept);
    if (accept) s.accepted += 1;
  }
}

// The damped step from the accepted point: s.trial = s.acc + delta, or s.acc again where the factorisation fails.
ATDN_HD inline void ground_lm_step(GroundState& s) {
#pragma clang fp contract(off)
  double A[9], F[6], b[3], dl[3];
  int n = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) A[3 * i + j] = A[3 * j + i] = s.sums[n++];
  for (int i = 0; i < 3; ++i) {
    const double l = s.lambda * A[4 * i];
    A[4 * i] = A[4 * i] + l;
    b[i] = -s.sums[6 + i];
  }
  const bool ok = ldl3_factor(A, F);
  ldl3_solve(F, b, dl);
  const bool step = ok && finite3(dl);
  for (int i = 0; i < 3; ++i) s.trial[i] = step ? s.acc[i] + dl[i] : s.acc[i];
}

// The outputs of a finished solve: q [3], sums [10], counts [6] = (candidates, used, inliers, accepted steps, votes, bin).
ATDN_HD inline void ground_output(const GroundState& s, double* q, double* sums, int* counts6) {
  for (int i = 0; i < 3; ++i) q[i] = s.plane ? s.acc[i] : 0.0;
  for (int i = 0; i < GROUND_TERMS; ++i) sums[i] = s.plane ? s.sums[i] : 0.0;
  for (int i = 0; i < 3; ++i) counts6[i] = s.plane ? s.counts[i] : 0;
  counts6[3] = s.plane ? s.accepted : 0;
  counts6[4] = s.plane ? s.votes : 0;
  counts6[5] = s.plane ? s.bin : 0;
}

// e (float32, 0 where the pixel is not used) and the inlier flag of pixel (x, y) at q
ATDN_HD inline int ground_classify_pixel(float zf, bool keep, const double* q, const GroundParams& c, int x, int y, float* e32) {
#pragma clang fp contract(off)
  *e32 = 0.0f;
  if (!keep) return 0;
  double a[2], z;
  if (!ground_ray(zf, c, x, y, a, &z)) return 0;
  const double qa = dot3(q[0], a[0], q[1], a[1], q[2], 1.0);
  const double zq = z * qa;
  const double e = zq - 1.0;
  const double e2 = e * e;
  *e32 = (float)e;
  return e2 <= c.thr ? 1 : 0;
}

// The sums of the band of one plane at q, in the order of plane_sum_host. depth, mask: the plane's row 0.
inline void ground_plane_host(const float* depth, const unsigned char* mask, const double* q, const GroundParams& c, int y1,
                              double sums[GROUND_TERMS], int counts[3]) {
  const long off = (long)c.y0 * c.W;
  plane_sum_host<GROUND_TERMS>((long)(y1 - c.y0) * c.W, [&](long i, double* t) {
    const int r = (int)(i / c.W), x = (int)(i - (long)r * c.W);
    return ground_pixel(depth[off + i], mask ? mask[off + i] != 0 : true, q, c, x, c.y0 + r, t);
  }, sums, counts);
}

// Whether bin k with (smoothed count v, own count c) beats the mode so far: the larger smoothed count, among equals the larger own
// count (a single populated bin k has the same smoothed count at k - 1, k and k + 1: the mode is k), among equals the lower bin.
ATDN_HD inline bool ground_mode_better(int v, int c, int k, int votes, int own, int bin) {
  return v > votes || (v == votes && (c > own || (c == own && k < bin)));
}

// The start vote of the band of one plane: the mode of the smoothed histogram.
inline void ground_vote_host(const float* depth, const unsigned char* mask, const GroundParams& c, int y1, int* bin, int* votes) {
  int hist[GROUND_BINS];
  for (int k = 0; k < GROUND_BINS; ++k) hist[k] = 0;
  const long off = (long)c.y0 * c.W, n = (long)(y1 - c.y0) * c.W;
  for (long i = 0; i < n; ++i) {
    const int r = (int)(i / c.W), x = (int)(i - (long)r * c.W);
    const int k = ground_vote_bin(depth[off + i], mask ? mask[off + i] != 0 : true, c, x, c.y0 + r);
    if (k >= 0) hist[k] += 1;
  }
  *bin = 0;
  *votes = ground_smoothed(hist, 0);
  for (int k = 1; k < GROUND_BINS; ++k) {
    const int v = ground_smoothed(hist, k);
    if (ground_mode_better(v, hist[k], k, *votes, hist[*bin], *bin)) { *votes = v; *bin = k; }
  }
}

// depth [B,H,W], mask [B,H,W] uint8 or null, q [B,3] -> sums [B,10], counts [B,3] over the rows [y0, y1)
inline void ground_terms_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y1,
                              const GroundParams& c, double* sums, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b)
    ground_plane_host(depth + b * n, mask ? mask + b * n : nullptr, q + 3L * b, c, y1, sums + (long)GROUND_TERMS * b,
                      counts + 3L * b);
}

// The vote (q_init null) or q_init, then iters Levenberg-Marquardt steps (iters + 1 evaluations) -> q [B,3], sums [B,10] at it,
// counts [B,6]
inline void ground_solve_host(const float* depth, const unsigned char* mask, const double* q_init, int B, int H, int W, int y1,
                              const GroundParams& c, int iters, double* q, double* sums, int* counts) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b) {
    const float* d = depth + b * n;
    const unsigned char* m = mask ? mask + b * n : nullptr;
    GroundState s;
    if (q_init) {
      ground_start_init(s, q_init + 3L * b);
    } else {
      int bin, votes;
      ground_vote_host(d, m, c, y1, &bin, &votes);
      ground_start_vote(s, c, bin, votes);
    }
    for (int k = 0; s.plane && k <= iters; ++k) {
      double S[GROUND_TERMS];
      int cnt[3];
      ground_plane_host(d, m, s.trial, c, y1, S, cnt);
      ground_lm_update(s, S, cnt, k);
      if (k < iters) ground_lm_step(s);
    }
    ground_output(s, q + 3L * b, sums + (long)GROUND_TERMS * b, counts + 6L * b);
  }
}

// residual [B,H,W] float32 and on_ground [B,H,W] uint8 at q [B,3]; zeros outside the rows [y0, y1)
inline void ground_classify_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y1,
                                 const GroundParams& c, float* residual, unsigned char* on_ground) {
  const long n = (long)H * W;
  for (int b = 0; b < B; ++b)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long i = b * n + (long)y * W + x;
        float e = 0.0f;
        int in = 0;
        if (y >= c.y0 && y < y1) in = ground_classify_pixel(depth[i], mask ? mask[i] != 0 : true, q + 3L * b, c, x, y, &e);
        residual[i] = e;
        on_ground[i] = (unsigned char)in;
      }
}

}  // namespace atdn
