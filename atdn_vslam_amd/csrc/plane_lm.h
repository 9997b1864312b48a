// What the two dense pose solvers (pnp_host.h: pose from depth and flow; epipolar_host.h: pose from flow alone) share, in plain
// C++ float64 (no HIP needed): 28 terms per pixel — the 21 upper-triangle entries of a 6 x 6 Gauss-Newton Hessian, row by row, the
// 6 gradient entries and the cost —, their order-fixed sum over a plane, the solver's state of one problem and the
// Levenberg-Marquardt decision on it, and the loop of a solve (plane_solve_host). What a pixel contributes, and how a step is
// taken from the accepted terms, is each solver's own: a stateless struct `Solver` (PnpSolver, EpipolarSolver) names its
// load_pose, lm_step and output. Every operation rounded on its own (fp contraction off).
//   plane sum    a plane is cut into chunks of 1024 consecutive flat indices; inside a chunk, thread j = 0 .. 255 owns the indices
//                4j .. 4j + 3 and forms ((t0 + t1) + t2) + t3 (an index past the plane contributes +0.0), the 256 values go through
//                the binary tree of strides 1 .. 128 (v[i] += v[i + stride] for i a multiple of 2 * stride); the chunk sums are
//                added in chunk order, starting from chunk 0's. The three counts are integer sums of the flag bits 1, 2, 4.
//   decision     evaluation 0 always becomes the accepted point, with lambda = 1e-3; evaluation k >= 1 is accepted iff its cost is
//                below the accepted one (a NaN fails); lambda by lm_lambda of lm6.h.
// The kernels (plane_sum.h) walk the same tree, so kernel, host form and NumPy restatement give the same bits.
// The plane sum takes the number of terms as a template parameter (28 unless given): the ground plane (ground_host.h) sums its 10
// terms over the same chunks, 4-sums, tree and chunk order.
#pragma once
#include <vector>

#include "lm6.h"

namespace atdn {

constexpr int PLANE_TERMS = 28;          // 21 upper-triangle Hessian entries (row-major), 6 gradient entries, the cost
constexpr int PLANE_CHUNK = 1024;        // flat indices per chunk: 256 threads x 4
constexpr int PLANE_CHUNK_THREADS = 256;

// The solver's state of one problem; what the 12 values of a pose mean is the solver's own.
struct PlaneLmState {
  double acc[12];              // the accepted pose
  double trial[12];            // the pose of the next (or the current) evaluation
  double sums[PLANE_TERMS];    // H, g and cost at the accepted pose
  double lambda;
  int counts[3];               // the three counts at the accepted pose
  int accepted;                // number of accepted steps
};

// After evaluation k (k = 0: the initial pose) with the plane sums `sums` and counts `counts` at s.trial: accept or reject.
ATDN_HD inline void plane_lm_update(PlaneLmState& s, const double* sums, const int* counts, int k) {
#pragma clang fp contract(off)
  const bool accept = k == 0 || sums[27] < s.sums[27];
  if (accept) {
    for (int i = 0; i < 12; ++i) s.acc[i] = s.trial[i];
    for (int i = 0; i < PLANE_TERMS; ++i) s.sums[i] = sums[i];
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

// The sums of one plane of n flat indices: pixel(i, t) writes the TERMS terms of index i < n and returns its flag bits. TERMS is
// 28 for the two pose solvers and 10 for the ground plane (ground_host.h): the chunks, the 4-sum, the tree and the chunk order
// do not depend on it.
template <int TERMS = PLANE_TERMS, class Pixel>
inline void plane_sum_host(long n, Pixel pixel, double* sums, int counts[3]) {
#pragma clang fp contract(off)
  const long chunks = (n + PLANE_CHUNK - 1) / PLANE_CHUNK;
  std::vector<double> v((size_t)PLANE_CHUNK_THREADS * TERMS);
  double t[TERMS];
  counts[0] = counts[1] = counts[2] = 0;
  for (long ch = 0; ch < chunks; ++ch) {
    for (int j = 0; j < PLANE_CHUNK_THREADS; ++j) {
      double* a = &v[(size_t)j * TERMS];
      for (int k = 0; k < 4; ++k) {
        const long i = ch * PLANE_CHUNK + 4 * j + k;
        int flags = 0;
        if (i < n) {
          flags = pixel(i, t);
        } else {
          for (int e = 0; e < TERMS; ++e) t[e] = 0.0;
        }
        for (int e = 0; e < TERMS; ++e) a[e] = k == 0 ? t[e] : a[e] + t[e];
        counts[0] += (flags & 1) ? 1 : 0;
        counts[1] += (flags & 2) ? 1 : 0;
        counts[2] += (flags & 4) ? 1 : 0;
      }
    }
    for (int stride = 1; stride < PLANE_CHUNK_THREADS; stride *= 2)
      for (int i = 0; i < PLANE_CHUNK_THREADS; i += 2 * stride)
        for (int e = 0; e < TERMS; ++e)
          v[(size_t)i * TERMS + e] = v[(size_t)i * TERMS + e] + v[(size_t)(i + stride) * TERMS + e];
    for (int e = 0; e < TERMS; ++e) sums[e] = ch == 0 ? v[e] : sums[e] + v[e];
  }
}

// The solve of B problems: iters Levenberg-Marquardt steps (iters + 1 evaluations) from pose_init -> pose_out [B,12], cost [B],
// counts [B,4]. plane(b, pose, sums, counts) writes the sums of plane b at the solver's pose.
template <class Solver, class Plane>
inline void plane_solve_host(int B, int iters, Plane plane, const float* pose_init, float* pose_out, double* cost, int* counts) {
  for (int b = 0; b < B; ++b) {
    PlaneLmState s;
    Solver::load_pose(pose_init + 12L * b, s.trial);
    for (int k = 0; k <= iters; ++k) {
      double sums[PLANE_TERMS];
      int cnt[3];
      plane(b, s.trial, sums, cnt);
      plane_lm_update(s, sums, cnt, k);
      if (k < iters) Solver::lm_step(s);
    }
    Solver::output(s, pose_init + 12L * b, pose_out + 12L * b, cost + b, counts + 4L * b);
  }
}

}  // namespace atdn
