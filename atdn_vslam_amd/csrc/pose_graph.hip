// Pose-graph optimisation on the device: atdn_pose_graph_terms (one evaluation) and atdn_pose_graph_solve (Levenberg-Marquardt
// with a block-tridiagonal-preconditioned conjugate gradient), batched over graphs, and their host twins. The rule — float64,
// every operation rounded on its own, the order of every sum fixed — and the solver over it, pg_solve, are pose_graph_host.h;
// the kernel and the host form run that one function, each with its own executor, so they evaluate one function
// (include/atdn_hip.h): the same bits on every call and on both paths. This file holds the workgroup's executor, PgBlockExec.
//
// ONE launch, one workgroup of 256 threads per graph (grid = B), the whole solve inside it. A solve is 10^3 .. 10^4 short
// dependent phases; between them stands a workgroup barrier, the cheapest synchronisation there is, where a launch per phase
// would be all launch overhead. The batch is what occupies the chip. No atomics, no memset, no host synchronisation, nothing
// waited for outside the workgroup, every loop bound an argument; capturable on one stream.
//   each, over edges    classify once; per evaluation the residual and cost term, per linearisation the 122 values of the
//                       edge's slot (store-and-sum: cdna_hip_programming.md, Guideline 12)
//   each, over nodes    node n belongs to thread n % 256: incidence lists (built here, once per solve, by a scan of the edge
//                       list in ascending edge number, so no caller's list can send the kernel out of bounds), the gather of
//                       a node's blocks in edge order, A p, the vector updates, the retraction
//   sum                 wave shuffles for the strides 1 .. 32 of the fixed tree, LDS for (w0 + w1) + (w2 + w3), the chunks of
//                       256 nodes in order; every thread forms the same total, so every scalar of the solver is uniform
//   serial              thread 0: the block LDL^T of the preconditioner and its two sweeps per CG iteration (operands loaded a
//                       node ahead, the running vector carried in registers; S^-1 y between the sweeps is per node)
// All state lives in the workspace (L2-resident: 1.5 KB per node, 1 KB per edge); LDS holds only the partial sums.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "pose_graph_host.h"

namespace atdn {

static_assert(PG_MAX_N % PG_THREADS == 0 && PG_THREADS == 256, "four waves, eight chunks of nodes at most");
constexpr int PG_CHUNKS = PG_MAX_N / PG_THREADS;

struct PgArgs {
  const float* poses;
  const int* index;
  const float* meas;
  const double* weight;
  const unsigned char* robust;
  const unsigned char* fixed;
  int N, E, iters, cg_iters;
  double q, tol2;
  float* poses_out;
  double* cost;
  double* edge_chi2;
  int* counts;
  char* workspace;
  size_t graph_bytes;
};

// The executor of pg_solve for one workgroup of PG_THREADS threads, thread t taking i = t, t + 256, ... Every primitive ends in a
// workgroup barrier with workgroup-scope fences (__syncthreads, or the __syncthreads_and / _count / _or reductions, which contain
// one), and sum reads everything its terms need before its barrier: whatever follows a primitive may overwrite what it read.
struct PgBlockExec {
  double* part;   // LDS: two buffers of [chunk][wave] used in turn, so one barrier per sum is enough
  int flip;

  template <class F>
  __device__ __forceinline__ void each(int n, F f) {
    for (int i = threadIdx.x; i < n; i += PG_THREADS) f(i);
    __syncthreads();
  }

  template <class F>
  __device__ __forceinline__ bool serial(F f) {
    int ok = 1;
    if (threadIdx.x == 0) ok = f() ? 1 : 0;
    return __syncthreads_and(ok) != 0;
  }

  template <class F>
  __device__ __forceinline__ double sum(int n, F value) {
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double* buf = part + flip * (4 * PG_CHUNKS);
    flip ^= 1;
    const int chunks = (n + PG_THREADS - 1) / PG_THREADS;
    for (int c = 0; c < chunks; ++c) {
      const int i = c * PG_THREADS + t;
      double v = i < n ? value(i) : 0.0;
#pragma unroll
      for (int stride = 1; stride < 64; stride *= 2) v = v + __shfl_down(v, stride, 64);
      if (lane == 0) buf[4 * c + wave] = v;
    }
    __syncthreads();
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) {
      const double lo = buf[4 * c] + buf[4 * c + 1], hi = buf[4 * c + 2] + buf[4 * c + 3];
      const double s = lo + hi;
      total = c == 0 ? s : total + s;
    }
    return total;
  }

  template <class F>
  __device__ __forceinline__ int count(int n, F f) {
    int total = 0;
    for (int c = 0; c * PG_THREADS < n; ++c) {
      const int i = c * PG_THREADS + threadIdx.x;
      total += __syncthreads_count(i < n && f(i));
    }
    __syncthreads();
    return total;
  }

  template <class F>
  __device__ __forceinline__ bool all(int n, F f) {
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += PG_THREADS) bad |= f(i) ? 0 : 1;
    const bool ok = __syncthreads_or(bad) == 0;
    __syncthreads();
    return ok;
  }
};

// iters < 0: one evaluation (atdn_pose_graph_terms)
__global__ __launch_bounds__(PG_THREADS) void pose_graph_kernel(PgArgs a) {
  __shared__ double part[2 * 4 * PG_CHUNKS];
  const size_t b = blockIdx.x, N = a.N, E = a.E;
  PgProblem P;
  P.poses = a.poses + 12 * N * b;
  P.index = a.index + 2 * E * b;
  P.meas = a.meas + 12 * E * b;
  P.weight = a.weight + 2 * E * b;
  P.robust = a.robust ? a.robust + E * b : nullptr;
  P.fixed = a.fixed ? a.fixed + N * b : nullptr;
  P.N = a.N;
  P.E = a.E;
  P.q = a.q;
  const bool solve = a.iters >= 0;
  PgBlockExec x{part, 0};
  pg_solve(P, pg_carve(a.workspace + a.graph_bytes * b, a.N, a.E), a.iters, a.cg_iters, a.tol2,
           solve ? a.poses_out + 12 * N * b : nullptr, a.cost + (solve ? 2 : 1) * b, a.edge_chi2 + E * b,
           a.counts + (solve ? 4 : 2) * b, x);
}

struct PgCall {
  const float* poses;
  const int* index;
  const float* meas;
  const double* weight;
  const unsigned char* robust;
  const unsigned char* fixed;
  int B, N, E;
  double robust_scale;
};

// Argument rules shared by the device and the host entry points. out[i] of out_bytes[i]: the outputs (a workspace among them),
// none of which may overlap an input or another output.
static void pg_check_args(const PgCall& c, const void* const* out, const long* out_bytes, int n_out) {
  ATDN_CHECK(c.B >= 1 && c.B <= PG_MAX_B, "B must be in [1, 1024]");
  ATDN_CHECK(c.N >= 2 && c.N <= PG_MAX_N, "N must be in [2, 2048]");
  ATDN_CHECK(c.E >= 1 && c.E <= PG_MAX_E, "E must be in [1, 8192]");
  ATDN_CHECK(std::isfinite(c.robust_scale) && c.robust_scale > 0.0, "robust_scale must be finite and > 0");
  ATDN_CHECK(c.poses && c.index && c.meas && c.weight, "null argument");
  ATDN_CHECK(((uintptr_t)c.weight & 7) == 0, "edge_weight must be 8-byte aligned");
  for (int i = 0; i < n_out; ++i) ATDN_CHECK(out[i], "null argument");
  const long B = c.B, N = c.N, E = c.E;
  const void* in[6] = {c.poses, c.index, c.meas, c.weight, c.robust, c.fixed};
  const long in_bytes[6] = {B * N * 48, B * E * 8, B * E * 48, B * E * 16, B * E, B * N};
  check_disjoint(in, in_bytes, 6, out, out_bytes, n_out);
}

static void pg_check_solver(int iters, int cg_iters, double cg_tol) {
  ATDN_CHECK(iters >= 0 && iters <= PG_MAX_ITERS, "iters must be in [0, 32]");
  ATDN_CHECK(cg_iters >= 1 && cg_iters <= PG_MAX_CG, "cg_iters must be in [1, 128]");
  ATDN_CHECK(std::isfinite(cg_tol) && cg_tol > 0.0, "cg_tol must be finite and > 0");
}

static void pg_launch(const PgCall& c, int iters, int cg_iters, double cg_tol, float* poses_out, double* cost, double* edge_chi2,
                      int* counts, void* workspace, void* stream) {
  PgArgs a;
  a.poses = c.poses;
  a.index = c.index;
  a.meas = c.meas;
  a.weight = c.weight;
  a.robust = c.robust;
  a.fixed = c.fixed;
  a.N = c.N;
  a.E = c.E;
  a.iters = iters;
  a.cg_iters = cg_iters;
  a.q = c.robust_scale * c.robust_scale;
  a.tol2 = cg_tol * cg_tol;
  a.poses_out = poses_out;
  a.cost = cost;
  a.edge_chi2 = edge_chi2;
  a.counts = counts;
  a.workspace = (char*)workspace;
  a.graph_bytes = pg_graph_bytes(c.N, c.E);
  hipLaunchKernelGGL(pose_graph_kernel, dim3((unsigned)c.B), dim3(PG_THREADS), 0, (hipStream_t)stream, a);
  ATDN_HIP(hipGetLastError());
}

static void pg_run_host(const PgCall& c, int iters, int cg_iters, double cg_tol, float* poses_out, double* cost, double* edge_chi2,
                        int* counts) {
  const size_t N = c.N, E = c.E;
  for (size_t b = 0; b < (size_t)c.B; ++b) {
    PgProblem P;
    P.poses = c.poses + 12 * N * b;
    P.index = c.index + 2 * E * b;
    P.meas = c.meas + 12 * E * b;
    P.weight = c.weight + 2 * E * b;
    P.robust = c.robust ? c.robust + E * b : nullptr;
    P.fixed = c.fixed ? c.fixed + N * b : nullptr;
    P.N = c.N;
    P.E = c.E;
    P.q = c.robust_scale * c.robust_scale;
    const bool solve = iters >= 0;
    pose_graph_run_host(P, iters, cg_iters, cg_tol, solve ? poses_out + 12 * N * b : nullptr, cost + (solve ? 2 : 1) * b,
                        edge_chi2 + E * b, counts + (solve ? 4 : 2) * b);
  }
}

}  // namespace atdn

using namespace atdn;

long atdn_pose_graph_workspace_bytes(int B, int N, int E) {
  if (B < 1 || B > PG_MAX_B || N < 2 || N > PG_MAX_N || E < 1 || E > PG_MAX_E) return 0;
  return (long)((size_t)B * pg_graph_bytes(N, E));
}

int atdn_pose_graph_terms(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                          const unsigned char* edge_robust, int B, int N, int E, double robust_scale, double* cost,
                          double* edge_chi2, int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const PgCall c{poses, edge_index, edge_pose, edge_weight, edge_robust, nullptr, B, N, E, robust_scale};
  const void* out[4] = {cost, edge_chi2, counts, workspace};
  const long out_bytes[4] = {(long)B * 8, (long)B * E * 8, (long)B * 8, atdn_pose_graph_workspace_bytes(B, N, E)};
  pg_check_args(c, out, out_bytes, 4);
  ATDN_CHECK((((uintptr_t)workspace | (uintptr_t)cost | (uintptr_t)edge_chi2) & 7) == 0,
             "workspace, cost and edge_chi2 must be 8-byte aligned");
  pg_launch(c, -1, 1, 1.0, nullptr, cost, edge_chi2, counts, workspace, stream);
  ATDN_API_END
}

int atdn_pose_graph_solve(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                          const unsigned char* edge_robust, const unsigned char* fixed, int B, int N, int E, double robust_scale,
                          int iters, int cg_iters, double cg_tol, float* poses_out, double* cost, double* edge_chi2, int* counts,
                          void* workspace, void* stream) {
  ATDN_API_BEGIN
  const PgCall c{poses, edge_index, edge_pose, edge_weight, edge_robust, fixed, B, N, E, robust_scale};
  const void* out[5] = {poses_out, cost, edge_chi2, counts, workspace};
  const long out_bytes[5] = {(long)B * N * 48, (long)B * 16, (long)B * E * 8, (long)B * 16,
                             atdn_pose_graph_workspace_bytes(B, N, E)};
  pg_check_args(c, out, out_bytes, 5);
  pg_check_solver(iters, cg_iters, cg_tol);
  ATDN_CHECK((((uintptr_t)workspace | (uintptr_t)cost | (uintptr_t)edge_chi2) & 7) == 0,
             "workspace, cost and edge_chi2 must be 8-byte aligned");
  pg_launch(c, iters, cg_iters, cg_tol, poses_out, cost, edge_chi2, counts, workspace, stream);
  ATDN_API_END
}

int atdn_pose_graph_terms_host(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                               const unsigned char* edge_robust, int B, int N, int E, double robust_scale, double* cost,
                               double* edge_chi2, int* counts) {
  ATDN_API_BEGIN
  const PgCall c{poses, edge_index, edge_pose, edge_weight, edge_robust, nullptr, B, N, E, robust_scale};
  const void* out[3] = {cost, edge_chi2, counts};
  const long out_bytes[3] = {(long)B * 8, (long)B * E * 8, (long)B * 8};
  pg_check_args(c, out, out_bytes, 3);
  pg_run_host(c, -1, 1, 1.0, nullptr, cost, edge_chi2, counts);
  ATDN_API_END
}

int atdn_pose_graph_solve_host(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                               const unsigned char* edge_robust, const unsigned char* fixed, int B, int N, int E,
                               double robust_scale, int iters, int cg_iters, double cg_tol, float* poses_out, double* cost,
                               double* edge_chi2, int* counts) {
  ATDN_API_BEGIN
  const PgCall c{poses, edge_index, edge_pose, edge_weight, edge_robust, fixed, B, N, E, robust_scale};
  const void* out[4] = {poses_out, cost, edge_chi2, counts};
  const long out_bytes[4] = {(long)B * N * 48, (long)B * 16, (long)B * E * 8, (long)B * 16};
  pg_check_args(c, out, out_bytes, 4);
  pg_check_solver(iters, cg_iters, cg_tol);
  pg_run_host(c, iters, cg_iters, cg_tol, poses_out, cost, edge_chi2, counts);
  ATDN_API_END
}
