// The device side of plane_lm.h, shared by the two dense pose solvers (pnp.hip, epipolar.hip): the workspace of a solve, the
// fixed binary tree that takes the 28 sums of a workgroup's threads to its slot of the workspace, and the order-fixed sum of the
// slots of a plane. The terms kernels run (chunks, B) workgroups of pixel_quads.h with off = 0 — workgroup c of plane b owns the
// flat indices 1024 c .. 1024 c + 1023, a thread four consecutive ones —; the finalise kernel (plane_finalise_kernel<Solver>, one
// for both) one wave per problem; plane_run is the launch sequence of their entry points. No memset
// and no atomics: every workgroup writes its own slot (store-and-sum: cdna_hip_programming.md, Guideline 12).
// The tree and the ordered sum take the number of terms as a template parameter (28 unless given): ground.hip walks the same
// tree over its 10 terms, with a workspace of its own.
#pragma once
#include "pixel_quads.h"
#include "plane_lm.h"

namespace atdn {

static_assert(PLANE_CHUNK == 4 * PQ_THREADS && PLANE_CHUNK_THREADS == PQ_THREADS, "a chunk is one workgroup of pixel_quads.h");
static_assert(sizeof(PlaneLmState) % 8 == 0, "the chunk sums follow the states in the workspace");

constexpr int PLANE_FIN_THREADS = 64;

struct PlaneWorkspace {
  PlaneLmState* state;   // [B]
  double* sums;          // [B, chunks, 28]
  int* counts;           // [B, chunks, 4] (three used)
};

inline long plane_chunks(int H, int W) { return cdivl((long)H * W, PLANE_CHUNK); }

inline size_t plane_workspace_size(int B, int H, int W) {
  const size_t chunks = (size_t)plane_chunks(H, W);
  return (size_t)B * (sizeof(PlaneLmState) + chunks * (PLANE_TERMS * sizeof(double) + 4 * sizeof(int)));
}

inline PlaneWorkspace plane_carve(void* workspace, int B, int H, int W) {
  const size_t chunks = (size_t)plane_chunks(H, W);
  PlaneWorkspace ws;
  ws.state = (PlaneLmState*)workspace;
  ws.sums = (double*)(ws.state + B);
  ws.counts = (int*)(ws.sums + (size_t)B * chunks * PLANE_TERMS);
  return ws;
}

// acc: the thread's TERMS sums (28 for the pose solvers, 10 for the ground plane: the tree does not depend on it); cnt: the WAVE's
// three counts, in every lane. Every thread of workgroup (blockIdx.x, b) calls it, once.
template <int TERMS = PLANE_TERMS>
__device__ __forceinline__ void plane_chunk_reduce(double* acc, const int cnt[3], int b, double* __restrict__ csums,
                                                   int* __restrict__ ccounts) {
#pragma clang fp contract(off)
  static_assert(TERMS <= 32, "threads 32 .. 34 carry the counts");
  __shared__ double part[PQ_WAVES][TERMS];
  __shared__ int ipart[PQ_WAVES][3];
  // strides 1 .. 32 inside the wave: lane i (a multiple of 2 * stride) takes v[i] + v[i + stride]; the other lanes hold values
  // that nobody reads
#pragma unroll
  for (int e = 0; e < TERMS; ++e) {
#pragma unroll
    for (int stride = 1; stride < 64; stride *= 2) acc[e] = acc[e] + __shfl_down(acc[e], stride, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int e = 0; e < TERMS; ++e) part[wave][e] = acc[e];
#pragma unroll
    for (int j = 0; j < 3; ++j) ipart[wave][j] = cnt[j];
  }
  __syncthreads();
  const long slot = (long)b * gridDim.x + blockIdx.x;
  if (threadIdx.x < TERMS) {
    const int e = threadIdx.x;
    const double lo = part[0][e] + part[1][e], hi = part[2][e] + part[3][e];     // strides 64 and 128
    csums[slot * TERMS + e] = lo + hi;
  } else if (threadIdx.x >= 32 && threadIdx.x < 35) {
    const int j = threadIdx.x - 32;
    ccounts[slot * 4 + j] = (ipart[0][j] + ipart[1][j]) + (ipart[2][j] + ipart[3][j]);
  }
}

// One wave per problem b: thread e < TERMS adds the chunk sums of term e in chunk order (coalesced: the terms of a chunk are
// contiguous), threads 32 .. 34 the integer counts; after the barrier inside, S and Cn (in LDS) hold the plane's.
template <int TERMS = PLANE_TERMS>
__device__ __forceinline__ void plane_ordered_sum(const double* __restrict__ csums, const int* __restrict__ ccounts, int chunks,
                                                  int b, double* S, int* Cn) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t < TERMS) {
    const double* p = csums + (long)b * chunks * TERMS + t;
    double s = p[0];
    int ch = 1;
    for (; ch + 8 <= chunks; ch += 8) {                        // eight loads in flight, the adds in chunk order
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = p[(long)(ch + i) * TERMS];
#pragma unroll
      for (int i = 0; i < 8; ++i) s = s + v[i];
    }
    for (; ch < chunks; ++ch) s = s + p[(long)ch * TERMS];
    S[t] = s;
  } else if (t >= 32 && t < 35) {
    const int* p = ccounts + (long)b * chunks * 4 + (t - 32);
    int s = 0;
    for (int ch = 0; ch < chunks; ++ch) s += p[(long)ch * 4];
    Cn[t - 32] = s;
  }
  __syncthreads();
}

// One wave per problem; Solver is PnpSolver or EpipolarSolver. k < 0: one evaluation (the plane sums go to sums_out /
// counts_out). k >= 0: evaluation k of a solve of `iters` steps: thread 0 takes the Levenberg-Marquardt decision and then either
// the next step or, after the last evaluation, writes the outputs.
template <class Solver>
__global__ __launch_bounds__(PLANE_FIN_THREADS) void plane_finalise_kernel(const double* __restrict__ csums,
                                                                          const int* __restrict__ ccounts, int chunks, int k,
                                                                          int iters, PlaneLmState* __restrict__ state,
                                                                          const float* __restrict__ pose_init,
                                                                          double* __restrict__ sums_out, int* __restrict__ counts_out,
                                                                          float* __restrict__ pose_out, double* __restrict__ cost_out) {
#pragma clang fp contract(off)
  __shared__ double S[PLANE_TERMS];
  __shared__ int Cn[3];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  plane_ordered_sum(csums, ccounts, chunks, b, S, Cn);
  if (k < 0) {
    if (t < PLANE_TERMS) sums_out[(long)b * PLANE_TERMS + t] = S[t];
    if (t < 3) counts_out[3 * b + t] = Cn[t];
    return;
  }
  if (t != 0) return;
  PlaneLmState& s = state[b];
  if (k == 0) Solver::load_pose(pose_init + 12 * b, s.trial);
  plane_lm_update(s, S, Cn, k);
  if (k < iters)
    Solver::lm_step(s);
  else
    Solver::output(s, pose_init + 12 * b, pose_out + 12 * b, cost_out + b, counts_out + 4 * b);
}

// The launches of an entry point: launch_terms(pose32, ws) is the solver's terms kernel at the float32 poses `pose32`, or at the
// trial poses of the state where pose32 is null. iters < 0: one evaluation, sums [B,28] and counts [B,3] (2 launches). Otherwise a
// solve of `iters` steps from `pose`: pose_out [B,12], cost [B], counts [B,4] (2 (iters + 1) launches).
template <class Solver, class LaunchTerms>
inline void plane_run(LaunchTerms launch_terms, void* workspace, int B, int H, int W, int iters, const float* pose, double* sums,
                      int* counts, float* pose_out, double* cost, hipStream_t stream) {
  const PlaneWorkspace ws = plane_carve(workspace, B, H, W);
  const bool solve = iters >= 0;
  for (int k = 0; k <= (solve ? iters : 0); ++k) {
    launch_terms(k == 0 ? pose : nullptr, ws);
    hipLaunchKernelGGL(plane_finalise_kernel<Solver>, dim3((unsigned)B), dim3(PLANE_FIN_THREADS), 0, stream, ws.sums, ws.counts,
                       (int)plane_chunks(H, W), solve ? k : -1, solve ? iters : 0, ws.state, pose, sums, counts, pose_out, cost);
    ATDN_HIP(hipGetLastError());
  }
}

}  // namespace atdn
