// Pose-graph optimisation on the device: atdn_pose_graph_terms (one evaluation) and atdn_pose_graph_solve (Levenberg-Marquardt
// with a block-tridiagonal-preconditioned conjugate gradient), batched over graphs, and their host twins. The rule — float64,
// every operation rounded on its own, the order of every sum fixed — is the per-edge and per-node functions of
// pose_graph_host.h, which this kernel calls phase by phase in the order of pose_graph_run_host, so the kernel and the host
// form evaluate one function (include/atdn_hip.h): the same bits on every call and on both paths.
//
// ONE launch, one workgroup of 256 threads per graph (grid = B), the whole solve inside it. A solve is 10^3 .. 10^4 short
// dependent phases; between them stands a workgroup barrier, the cheapest synchronisation there is, where a launch per phase
// would be all launch overhead. The batch is what occupies the chip. No atomics, no memset, no host synchronisation, nothing
// waited for outside the workgroup, every loop bound an argument; capturable on one stream.
//   edges, thread-strided   classify once; per evaluation the residual and cost term, per linearisation the 122 values of the
//                           edge's slot (store-and-sum: cdna_hip_programming.md, Guideline 12)
//   nodes, thread-strided   node n belongs to thread n % 256: incidence lists (built here, once per solve, by a scan of the edge
//                           list in ascending edge number, so no caller's list can send the kernel out of bounds), the gather of
//                           a node's blocks in edge order, A p, the vector updates, the retraction
//   sums over nodes         wave shuffles for the strides 1 .. 32 of the fixed tree, LDS for (w0 + w1) + (w2 + w3), the chunks of
//                           256 nodes in order; every thread forms the same total, so every scalar of the solver is uniform
//   thread 0                the serial part: the block LDL^T of the preconditioner and its two sweeps per CG iteration (operands
//                           loaded a node ahead, the running vector carried in registers; S^-1 y between the sweeps is per node)
// All state lives in the workspace (L2-resident: 1.5 KB per node, 1 KB per edge); LDS holds only the partial sums.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "common.h"
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

// The fixed-order sum over i = 0 .. n-1 of value(i), thread t supplying i = 256 c + t; the result in every thread. `part` is
// two buffers of [chunk][wave] used in turn, so one barrier per sum is enough.
template <class F>
__device__ __forceinline__ double pg_block_sum(double* part, int& flip, int n, F value) {
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

__device__ __forceinline__ double pg_block_cost(const PgProblem& P, const PgView& V, const double* X, double* part, int& flip) {
  for (int e = threadIdx.x; e < P.E; e += PG_THREADS) pg_edge_phase(P, V, X, e, false);
  __syncthreads();
  return pg_block_sum(part, flip, P.N, [&](int n) {
    pg_node_cost(V, n);
    return V.costn[n];
  });
}

__device__ __forceinline__ void pg_block_sweeps(const PgView& V, int N) {
  __syncthreads();
  if (threadIdx.x == 0) pg_sweep_forward_all(V, N);
  __syncthreads();
  for (int n = threadIdx.x; n < N; n += PG_THREADS) pg_node_pivot_solve(V, n);
  __syncthreads();
  if (threadIdx.x == 0) pg_sweep_backward_all(V, N);
  __syncthreads();
}

// iters < 0: one evaluation (atdn_pose_graph_terms)
__global__ __launch_bounds__(PG_THREADS) void pose_graph_kernel(PgArgs a) {
#pragma clang fp contract(off)
  __shared__ double part[2 * 4 * PG_CHUNKS];
  int flip = 0;
  const int b = blockIdx.x, t = threadIdx.x;
  const int N = a.N, E = a.E;
  PgProblem P;
  P.poses = a.poses + 12 * (size_t)N * b;
  P.index = a.index + 2 * (size_t)E * b;
  P.meas = a.meas + 12 * (size_t)E * b;
  P.weight = a.weight + 2 * (size_t)E * b;
  P.robust = a.robust ? a.robust + (size_t)E * b : nullptr;
  P.fixed = a.fixed ? a.fixed + (size_t)N * b : nullptr;
  P.N = N;
  P.E = E;
  P.q = a.q;
  const PgView V = pg_carve(a.workspace + a.graph_bytes * b, N, E);

  int valid = 0;
  for (int c = 0; c * PG_THREADS < E; ++c) {
    const int e = c * PG_THREADS + t;
    int kind = PG_ABSENT;
    if (e < E) {
      kind = pg_edge_kind(P, e, &V.ei[e], &V.ej[e]);
      V.kind[e] = kind;
    }
    valid += __syncthreads_count(kind != PG_ABSENT);
  }
  for (int n = t; n < N; n += PG_THREADS) V.deg[n] = pg_node_incidence(V, E, n, false);
  __syncthreads();
  if (t == 0) {
    int o = 0;
    for (int n = 0; n < N; ++n) {
      V.off[n] = o;
      o += V.deg[n];
    }
    V.off[N] = o;
  }
  __syncthreads();
  for (int n = t; n < N; n += PG_THREADS) {
    pg_node_incidence(V, E, n, true);
    V.free_[n] = V.deg[n] > 0 && !(P.fixed && P.fixed[n] != 0);
    pg_internal_pose(P.poses + 12 * (size_t)n, V.acc + 12 * (size_t)n);
  }
  __syncthreads();

  double cost_acc = pg_block_cost(P, V, V.acc, part, flip);
  const double cost0 = cost_acc;
  double lambda = 1e-3;
  int accepted = 0, cg_total = 0;
  bool fresh = false;
  for (int k = 0; k < a.iters; ++k) {
    if (!fresh) {
      for (int e = t; e < E; e += PG_THREADS) pg_edge_phase(P, V, V.acc, e, true);
      __syncthreads();
      for (int n = t; n < N; n += PG_THREADS) pg_node_gather(V, N, n);
      __syncthreads();
      fresh = true;
    }
    int okf = 1;
    if (t == 0) {
      for (int n = 0; n < N; ++n)
        if (!pg_factor_node(V, N, n, lambda)) {
          okf = 0;
          break;
        }
    }
    bool ok = __syncthreads_and(okf) != 0;
    if (ok) {
      for (int n = t; n < N; n += PG_THREADS)
        for (int c = 0; c < 6; ++c) {
          const size_t i = 6 * (size_t)n + c;
          V.x[i] = 0.0;
          V.r[i] = V.free_[n] ? -V.g[i] : 0.0;
          V.z[i] = 0.0;
          V.Ap[i] = 0.0;
        }
      pg_block_sweeps(V, N);
      for (int n = t; n < N; n += PG_THREADS)
        for (int c = 0; c < 6; ++c) V.p[6 * (size_t)n + c] = V.z[6 * (size_t)n + c];
      double rz = pg_block_sum(part, flip, N, [&](int n) { return pg_dot6(V.r, V.z, n); });
      const double thr = a.tol2 * rz;
      if (rz > 0.0) {
        for (int it = 0; it < a.cg_iters; ++it) {
          for (int n = t; n < N; n += PG_THREADS) pg_apply_node(V, n, lambda);
          const double pAp = pg_block_sum(part, flip, N, [&](int n) { return pg_dot6(V.p, V.Ap, n); });
          if (!(pAp > 0.0)) break;
          const double alpha = rz / pAp;
          for (int n = t; n < N; n += PG_THREADS)
            for (int c = 0; c < 6; ++c) {
              const size_t i = 6 * (size_t)n + c;
              const double ap = alpha * V.p[i], aAp = alpha * V.Ap[i];
              V.x[i] = V.x[i] + ap;
              V.r[i] = V.r[i] - aAp;
            }
          ++cg_total;
          pg_block_sweeps(V, N);
          const double rz_new = pg_block_sum(part, flip, N, [&](int n) { return pg_dot6(V.r, V.z, n); });
          if (!(rz_new > thr)) break;
          const double beta = rz_new / rz;
          for (int n = t; n < N; n += PG_THREADS)
            for (int c = 0; c < 6; ++c) {
              const size_t i = 6 * (size_t)n + c;
              const double bp = beta * V.p[i];
              V.p[i] = V.z[i] + bp;
            }
          rz = rz_new;
          __syncthreads();
        }
      }
      int bad = 0;
      for (int n = t; n < N; n += PG_THREADS) bad |= pg_retract_node(V, n) ? 0 : 1;
      ok = __syncthreads_or(bad) == 0;
    }
    bool accept = false;
    if (ok) {
      const double c = pg_block_cost(P, V, V.trial, part, flip);
      accept = c < cost_acc;
      if (accept) {
        for (int n = t; n < N; n += PG_THREADS)
          for (int i = 0; i < 12; ++i) V.acc[12 * (size_t)n + i] = V.trial[12 * (size_t)n + i];
        cost_acc = c;
        accepted += 1;
        fresh = false;
        __syncthreads();
      }
    }
    lambda = pg_lambda(lambda, accept);
  }

  const float* final_poses = P.poses;
  if (a.iters >= 0) {
    float* out = a.poses_out + 12 * (size_t)N * b;
    for (int n = t; n < N; n += PG_THREADS) {
      float* o = out + 12 * (size_t)n;
      if (accepted > 0 && V.free_[n]) {
        pg_public_pose(V.acc + 12 * (size_t)n, o);
      } else {
        for (int i = 0; i < 12; ++i) o[i] = P.poses[12 * (size_t)n + i];
      }
    }
    final_poses = out;
    __syncthreads();
  }
  for (int e = t; e < E; e += PG_THREADS) a.edge_chi2[(size_t)E * b + e] = pg_edge_chi2(P, V, final_poses, e);
  if (t == 0) {
    if (a.iters >= 0) {
      a.cost[2 * b] = cost0;
      a.cost[2 * b + 1] = cost_acc;
      int* cn = a.counts + 4 * b;
      cn[0] = valid;
      cn[1] = E - valid;
      cn[2] = accepted;
      cn[3] = cg_total;
    } else {
      a.cost[b] = cost0;
      a.counts[2 * b] = valid;
      a.counts[2 * b + 1] = E - valid;
    }
  }
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
  for (int i = 0; i < n_out; ++i) {
    for (int k = 0; k < 6; ++k)
      if (in[k]) ATDN_CHECK(disjoint(in[k], in_bytes[k], out[i], out_bytes[i]), "an output overlaps an input");
    for (int j = 0; j < i; ++j) ATDN_CHECK(disjoint(out[j], out_bytes[j], out[i], out_bytes[i]), "two outputs overlap");
  }
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
