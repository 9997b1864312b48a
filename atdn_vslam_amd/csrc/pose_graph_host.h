// Pose-graph optimisation of a keyframe map, the rule in plain C++ float64 (no HIP needed). Nodes are poses world <- camera,
// an edge (i, j) measures T_i^-1 T_j with separate rotation and translation weights and an optional Geman-McClure loss;
// Levenberg-Marquardt over the graph with a conjugate-gradient solve preconditioned by the block-tridiagonal part of the system.
// pg_edge_residual / pg_edge_blocks are one edge's residual and its contribution to the normal equations, pg_node_gather a
// node's sums over its incident edges, pg_factor_node / pg_sweep_*_all / pg_node_pivot_solve the block LDL^T of the
// preconditioner and its sweeps, pg_apply_node one block row of A p, pg_retract_node the retraction from the right, pg_tree_sum
// the fixed-order sum over nodes; the 6 x 6 factorisation, the Cayley matrix and the damping constants are those of lm6.h, shared
// with PnP. pg_solve is the solver itself, written once: every phase from the classification of the edges to the last output,
// over an executor that says how a phase reaches all edges or nodes. pose_graph_run_host runs it with plain loops (PgHostExec)
// behind atdn_pose_graph_terms_host / atdn_pose_graph_solve_host, the kernel of pose_graph.hip with a workgroup, so the two
// cannot drift apart; the independent statement the tests compare both with is tests/pose_graph_ref.py (NumPy and plain Python
// floats). The rule is stated in full in include/atdn_hip.h, atdn_pose_graph_solve; only + - * / and comparisons, every
// operation rounded on its own.
#pragma once
#include <cfloat>
#include <vector>

#include "lm6.h"

namespace atdn {

constexpr int PG_THREADS = 256;        // the chunk of the fixed binary tree, and the kernel's workgroup
constexpr int PG_EDGE_DOUBLES = 122;   // A_ii 36, A_jj 36, A_ij 36, g_i 6, g_j 6, the cost term, c_e
constexpr int PG_AII = 0, PG_AJJ = 36, PG_AIJ = 72, PG_GI = 108, PG_GJ = 114, PG_COST = 120, PG_CHI2 = 121;
constexpr int PG_NODE_DOUBLES = 24 + 36 + 6 + 1 + 36 + 21 + 36 + 30;
constexpr int PG_MAX_B = 1024, PG_MAX_N = 2048, PG_MAX_E = 8192, PG_MAX_ITERS = 32, PG_MAX_CG = 128;
enum { PG_ABSENT = 0, PG_IDLE = 1, PG_ACTIVE = 2 };   // an edge: not there; there with both weights zero; contributing

// One graph's inputs.
struct PgProblem {
  const float* poses;            // [N,12]
  const int* index;              // [2,E]: the i's, then the j's
  const float* meas;             // [E,12]
  const double* weight;          // [E,2] = (w_rot, w_tr)
  const unsigned char* robust;   // [E] or null
  const unsigned char* fixed;    // [N] or null
  int N, E;
  double q;                      // robust_scale * robust_scale
};

// One graph's working arrays (the kernel's workspace, a std::vector on the host).
struct PgView {
  double *acc, *trial;           // [N,12] internal poses: R row-major, then t
  double* edge;                  // [E,122]
  double *D, *g, *costn, *U;     // [N,36], [N,6], [N], [N,36]: diagonal block, gradient, cost share, block (n, n+1)
  double *F, *W;                 // [N,21], [N,36]: L (15, rows 1..5) and pivots (6) of S_n; W_n = S_n^-1 U_n
  double *x, *r, *z, *p, *Ap;    // [N,6]
  int *ei, *ej, *kind;           // [E]
  int *deg, *off, *inc, *free_;  // [N], [N+1], [2E], [N]; inc = 2 * edge + side (0: the node is the edge's i)
};

inline size_t pg_graph_bytes(int N, int E) {
  const size_t ints = 5 * (size_t)E + 3 * (size_t)N + 1;
  return ((size_t)N * PG_NODE_DOUBLES + (size_t)E * PG_EDGE_DOUBLES) * 8 + (ints + 1) / 2 * 8;
}

ATDN_HD inline PgView pg_carve(void* base, int N, int E) {
  PgView v;
  double* d = (double*)base;
  v.acc = d; d += 12 * (size_t)N;
  v.trial = d; d += 12 * (size_t)N;
  v.D = d; d += 36 * (size_t)N;
  v.g = d; d += 6 * (size_t)N;
  v.costn = d; d += N;
  v.U = d; d += 36 * (size_t)N;
  v.F = d; d += 21 * (size_t)N;
  v.W = d; d += 36 * (size_t)N;
  v.x = d; d += 6 * (size_t)N;
  v.r = d; d += 6 * (size_t)N;
  v.z = d; d += 6 * (size_t)N;
  v.p = d; d += 6 * (size_t)N;
  v.Ap = d; d += 6 * (size_t)N;
  v.edge = d; d += (size_t)PG_EDGE_DOUBLES * E;
  int* i = (int*)d;
  v.ei = i; i += E;
  v.ej = i; i += E;
  v.kind = i; i += E;
  v.inc = i; i += 2 * (size_t)E;
  v.deg = i; i += N;
  v.free_ = i; i += N;
  v.off = i;
  return v;
}

// out = A^T B (3 x 3, row-major)
ATDN_HD inline void pg_atb(const double* A, const double* B, double* out) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) out[3 * a + b] = dot3(A[a], B[b], A[3 + a], B[3 + b], A[6 + a], B[6 + b]);
}

// public pose (12 float32, rows of [R|t]) -> internal (R row-major, t)
ATDN_HD inline void pg_internal_pose(const float* p12, double* X) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) X[3 * a + b] = (double)p12[4 * a + b];
    X[9 + a] = (double)p12[4 * a + 3];
  }
}

ATDN_HD inline void pg_public_pose(const double* X, float* p12) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) p12[4 * a + b] = (float)X[3 * a + b];
    p12[4 * a + 3] = (float)X[9 + a];
  }
}

// The class of edge e, and its endpoints (0, 0 for an absent edge, so that nothing is read out of range).
ATDN_HD inline int pg_edge_kind(const PgProblem& P, int e, int* i, int* j) {
  const int a = P.index[e], b = P.index[P.E + e];
  const double wr = P.weight[2 * e], wt = P.weight[2 * e + 1];
  const bool ok = a >= 0 && a < P.N && b >= 0 && b < P.N && a != b && wr >= 0.0 && wr <= DBL_MAX && wt >= 0.0 && wt <= DBL_MAX;
  *i = ok ? a : 0;
  *j = ok ? b : 0;
  return !ok ? PG_ABSENT : (wr > 0.0 || wt > 0.0) ? PG_ACTIVE : PG_IDLE;
}

struct PgRes {
  double Rz[9], Re[9], tm[3], r[6];
  double c, cost, omega;
};

// The residual of an edge with measurement Z between the internal poses Xi, Xj.
ATDN_HD inline void pg_edge_residual(const double* Xi, const double* Xj, const float* Z, double wr, double wt, bool robust, double q,
                                     PgRes& o) {
#pragma clang fp contract(off)
  double tz[3], M[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) o.Rz[3 * a + b] = (double)Z[4 * a + b];
    tz[a] = (double)Z[4 * a + 3];
  }
  pg_atb(Xi, Xj, M);
  pg_atb(o.Rz, M, o.Re);
  const double d0 = Xj[9] - Xi[9], d1 = Xj[10] - Xi[10], d2 = Xj[11] - Xi[11];
#pragma unroll
  for (int a = 0; a < 3; ++a) o.tm[a] = dot3(Xi[a], d0, Xi[3 + a], d1, Xi[6 + a], d2);
  const double u0 = o.tm[0] - tz[0], u1 = o.tm[1] - tz[1], u2 = o.tm[2] - tz[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) o.r[3 + a] = dot3(o.Rz[a], u0, o.Rz[3 + a], u1, o.Rz[6 + a], u2);
  const double s0 = o.Re[7] - o.Re[5], s1 = o.Re[2] - o.Re[6], s2 = o.Re[3] - o.Re[1];
  o.r[0] = 0.5 * s0;
  o.r[1] = 0.5 * s1;
  o.r[2] = 0.5 * s2;
  const double aa = dot3(o.r[0], o.r[0], o.r[1], o.r[1], o.r[2], o.r[2]);
  const double tt = dot3(o.r[3], o.r[3], o.r[4], o.r[4], o.r[5], o.r[5]);
  const double ca = wr * aa, ct = wt * tt;
  o.c = ca + ct;
  if (robust) {
    const double s = q + o.c;
    const double f = q / s;
    const double qc = q * o.c;
    o.omega = f * f;
    o.cost = qc / s;
  } else {
    o.omega = 1.0;
    o.cost = o.c;
  }
}

// out[a][b] = sum over k = 0..5, in that order, of (w[k] * X[k][a]) * Y[k][b]; `sym`: a <= b computed, the rest mirrored
ATDN_HD inline void pg_jtwj(const double* X, const double* w, const double* Y, bool sym, double* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      if (sym && b < a) continue;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double wx = w[k] * X[6 * k + a];
        const double t = wx * Y[6 * k + b];
        s = k == 0 ? t : s + t;
      }
      out[6 * a + b] = s;
      if (sym) out[6 * b + a] = s;
    }
}

// The contribution of an edge to the normal equations -> its slot (122 values).
ATDN_HD inline void pg_edge_blocks(const PgRes& o, double wr, double wt, double* slot) {
#pragma clang fp contract(off)
  const double* Re = o.Re;
  const double* Rz = o.Rz;
  const double t01 = Re[0] + Re[4];
  const double tr = t01 + Re[8];
  double Ji[36], Jj[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) Ji[k] = Jj[k] = 0.0;
  double G[9];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double dg = tr - Re[4 * a];
      G[3 * a + b] = a == b ? dg : -Re[3 * a + b];
      Jj[6 * a + b] = a == b ? 0.5 * dg : -0.5 * Re[3 * b + a];
      Jj[6 * (3 + a) + 3 + b] = Re[3 * a + b];
    }
  const double S[9] = {0.0, -o.tm[2], o.tm[1], o.tm[2], 0.0, -o.tm[0], -o.tm[1], o.tm[0], 0.0};
  double Pm[9];
  pg_atb(Rz, S, Pm);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double gr = dot3(G[3 * a], Rz[3 * b], G[3 * a + 1], Rz[3 * b + 1], G[3 * a + 2], Rz[3 * b + 2]);
      Ji[6 * a + b] = -0.5 * gr;
      Ji[6 * (3 + a) + b] = Pm[3 * a + b];
      Ji[6 * (3 + a) + 3 + b] = -Rz[3 * b + a];
    }
  const double owr = o.omega * wr, owt = o.omega * wt;
  const double w[6] = {owr, owr, owr, owt, owt, owt};
  pg_jtwj(Ji, w, Ji, true, slot + PG_AII);
  pg_jtwj(Jj, w, Jj, true, slot + PG_AJJ);
  pg_jtwj(Ji, w, Jj, false, slot + PG_AIJ);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double si = 0.0, sj = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double wi = w[k] * Ji[6 * k + a], wj = w[k] * Jj[6 * k + a];
      const double ti = wi * o.r[k], tj = wj * o.r[k];
      si = k == 0 ? ti : si + ti;
      sj = k == 0 ? tj : sj + tj;
    }
    slot[PG_GI + a] = si;
    slot[PG_GJ + a] = sj;
  }
  slot[PG_COST] = o.cost;
  slot[PG_CHI2] = o.c;
}

// Edge e at the poses X [N,12]: the cost term alone, or the whole slot. Idle and absent edges write nothing.
ATDN_HD inline void pg_edge_phase(const PgProblem& P, const PgView& V, const double* X, int e, bool blocks) {
  if (V.kind[e] != PG_ACTIVE) return;
  PgRes o;
  const double wr = P.weight[2 * e], wt = P.weight[2 * e + 1];
  pg_edge_residual(X + 12 * (size_t)V.ei[e], X + 12 * (size_t)V.ej[e], P.meas + 12 * (size_t)e, wr, wt,
                   P.robust && P.robust[e] != 0, P.q, o);
  double* slot = V.edge + (size_t)PG_EDGE_DOUBLES * e;
  if (blocks)
    pg_edge_blocks(o, wr, wt, slot);
  else
    slot[PG_COST] = o.cost;
}

// c_e of edge e at the public poses p32 [N,12]; +0.0 for an absent edge.
ATDN_HD inline double pg_edge_chi2(const PgProblem& P, const PgView& V, const float* p32, int e) {
  if (V.kind[e] == PG_ABSENT) return 0.0;
  double Xi[12], Xj[12];
  pg_internal_pose(p32 + 12 * (size_t)V.ei[e], Xi);
  pg_internal_pose(p32 + 12 * (size_t)V.ej[e], Xj);
  PgRes o;
  pg_edge_residual(Xi, Xj, P.meas + 12 * (size_t)e, P.weight[2 * e], P.weight[2 * e + 1], false, P.q, o);
  return o.c;
}

// The number of active edges at node n, and with `fill` their codes into the node's list, in ascending edge number.
ATDN_HD inline int pg_node_incidence(const PgView& V, int E, int n, bool fill) {
  int k = 0;
  int* list = fill ? V.inc + V.off[n] : nullptr;
  for (int e = 0; e < E; ++e) {
    if (V.kind[e] != PG_ACTIVE) continue;
    const bool a = V.ei[e] == n, b = V.ej[e] == n;
    if (!(a || b)) continue;
    if (fill) list[k] = 2 * e + (a ? 0 : 1);
    ++k;
  }
  return k;
}

// The cost share of node n: the cost terms of the edges whose i it is, in ascending edge number (+0.0 without one).
ATDN_HD inline void pg_node_cost(const PgView& V, int n) {
#pragma clang fp contract(off)
  double c = 0.0;
  bool first = true;
  for (int s = V.off[n]; s < V.off[n + 1]; ++s) {
    const int code = V.inc[s];
    if (code & 1) continue;
    const double t = V.edge[(size_t)PG_EDGE_DOUBLES * (code >> 1) + PG_COST];
    c = first ? t : c + t;
    first = false;
  }
  V.costn[n] = c;
}

// Node n's diagonal block, gradient and block (n, n+1), summed over its incident edges in ascending edge number.
ATDN_HD inline void pg_node_gather(const PgView& V, int N, int n) {
#pragma clang fp contract(off)
  if (!V.free_[n]) return;
  const bool link = n + 1 < N && V.free_[n + 1];
  double D[36], U[36], g[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) D[k] = U[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = 0.0;
  bool first = true, ufirst = true;
  for (int s = V.off[n]; s < V.off[n + 1]; ++s) {
    const int code = V.inc[s], e = code >> 1, side = code & 1;
    const double* slot = V.edge + (size_t)PG_EDGE_DOUBLES * e;
    const double* blk = slot + (side ? PG_AJJ : PG_AII);
    const double* gr = slot + (side ? PG_GJ : PG_GI);
#pragma unroll
    for (int k = 0; k < 36; ++k) D[k] = first ? blk[k] : D[k] + blk[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = first ? gr[k] : g[k] + gr[k];
    first = false;
    const int other = side ? V.ei[e] : V.ej[e];
    if (link && other == n + 1) {
      const double* Cm = slot + PG_AIJ;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          const double t = side ? Cm[6 * b + a] : Cm[6 * a + b];
          U[6 * a + b] = ufirst ? t : U[6 * a + b] + t;
        }
      ufirst = false;
    }
  }
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    V.D[36 * (size_t)n + k] = D[k];
    V.U[36 * (size_t)n + k] = U[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) V.g[6 * (size_t)n + k] = g[k];
}

// Step n of the block LDL^T of the damped block-tridiagonal part. Returns false on a non-positive pivot.
ATDN_HD inline bool pg_factor_node(const PgView& V, int N, int n, double lambda) {
#pragma clang fp contract(off)
  if (!V.free_[n]) return true;
  double A[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) A[k] = V.D[36 * (size_t)n + k];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double l = lambda * A[7 * a];
    A[7 * a] = A[7 * a] + l;
  }
  if (n > 0 && V.free_[n - 1]) {
    const double* U = V.U + 36 * (size_t)(n - 1);
    const double* W = V.W + 36 * (size_t)(n - 1);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double t = U[6 * c + a] * W[6 * c + b];
          s = c == 0 ? t : s + t;
        }
        A[6 * a + b] = A[6 * a + b] - s;
      }
  }
  double* F = V.F + 21 * (size_t)n;
  const bool ok = ldl6_factor(A, F);
  if (ok && n + 1 < N && V.free_[n + 1]) {
    const double* U = V.U + 36 * (size_t)n;
    double* W = V.W + 36 * (size_t)n;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double col[6], x[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) col[a] = U[6 * a + b];
      ldl6_solve(F, col, x);
#pragma unroll
      for (int a = 0; a < 6; ++a) W[6 * a + b] = x[a];
    }
  }
  return ok;
}

// z = M^-1 r in three passes. The forward sweep, serial over the nodes: y_n = r_n - W_{n-1}^T y_{n-1}, written to z. The operands
// of node n + 1 are loaded before node n is computed and y is carried in registers, so that the one lane that walks the chain
// waits for arithmetic, not for memory.
ATDN_HD inline void pg_sweep_forward_all(const PgView& V, int N) {
#pragma clang fp contract(off)
  double yp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Wn[36], rn[6];
  bool linked = false;
  int fn = V.free_[0];
#pragma unroll
  for (int k = 0; k < 36; ++k) Wn[k] = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) rn[a] = V.r[a];
  for (int n = 0; n < N; ++n) {
    double Wc[36], y[6];
    const int fc = fn;
#pragma unroll
    for (int k = 0; k < 36; ++k) Wc[k] = Wn[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) y[a] = rn[a];
    if (n + 1 < N) {
      fn = V.free_[n + 1];
#pragma unroll
      for (int k = 0; k < 36; ++k) Wn[k] = V.W[36 * (size_t)n + k];
#pragma unroll
      for (int a = 0; a < 6; ++a) rn[a] = V.r[6 * (size_t)(n + 1) + a];
    }
    if (!fc) {
      linked = false;
      continue;
    }
    if (linked) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double t = Wc[6 * c + a] * yp[c];
          s = c == 0 ? t : s + t;
        }
        y[a] = y[a] - s;
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      V.z[6 * (size_t)n + a] = y[a];
      yp[a] = y[a];
    }
    linked = true;
  }
}

// The middle pass, every node on its own: z_n = S_n^-1 z_n
ATDN_HD inline void pg_node_pivot_solve(const PgView& V, int n) {
  if (!V.free_[n]) return;
  double y[6], v[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) y[a] = V.z[6 * (size_t)n + a];
  ldl6_solve(V.F + 21 * (size_t)n, y, v);
#pragma unroll
  for (int a = 0; a < 6; ++a) V.z[6 * (size_t)n + a] = v[a];
}

// The backward sweep, serial over the nodes: z_n = z_n - W_n z_{n+1}, loads ahead and z carried as in the forward sweep.
ATDN_HD inline void pg_sweep_backward_all(const PgView& V, int N) {
#pragma clang fp contract(off)
  double zp[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Wn[36], vn[6];
  bool linked = false;
  int fn = V.free_[N - 1];
#pragma unroll
  for (int k = 0; k < 36; ++k) Wn[k] = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) vn[a] = V.z[6 * (size_t)(N - 1) + a];
  for (int n = N - 1; n >= 0; --n) {
    double Wc[36], v[6];
    const int fc = fn;
#pragma unroll
    for (int k = 0; k < 36; ++k) Wc[k] = Wn[k];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = vn[a];
    if (n > 0) {
      fn = V.free_[n - 1];
#pragma unroll
      for (int k = 0; k < 36; ++k) Wn[k] = V.W[36 * (size_t)(n - 1) + k];
#pragma unroll
      for (int a = 0; a < 6; ++a) vn[a] = V.z[6 * (size_t)(n - 1) + a];
    }
    if (!fc) {
      linked = false;
      continue;
    }
    if (linked) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const double t = Wc[6 * a + c] * zp[c];
          s = c == 0 ? t : s + t;
        }
        v[a] = v[a] - s;
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) V.z[6 * (size_t)n + a] = v[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) zp[a] = v[a];
    linked = true;
  }
}

// Ap_n = (D_n + lambda diag D_n) p_n + the off-diagonal blocks of n's edges to free nodes times their p, in edge order
ATDN_HD inline void pg_apply_node(const PgView& V, int n, double lambda) {
#pragma clang fp contract(off)
  if (!V.free_[n]) return;
  const double* D = V.D + 36 * (size_t)n;
  double pn[6], y[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) pn[a] = V.p[6 * (size_t)n + a];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double d = D[6 * a + b];
      if (a == b) {
        const double l = lambda * d;
        d = d + l;
      }
      const double t = d * pn[b];
      s = b == 0 ? t : s + t;
    }
    y[a] = s;
  }
  for (int s = V.off[n]; s < V.off[n + 1]; ++s) {
    const int code = V.inc[s], e = code >> 1, side = code & 1;
    const int other = side ? V.ei[e] : V.ej[e];
    if (!V.free_[other]) continue;
    const double* Cm = V.edge + (size_t)PG_EDGE_DOUBLES * e + PG_AIJ;
    double po[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) po[a] = V.p[6 * (size_t)other + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double t = 0.0;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const double m = (side ? Cm[6 * b + a] : Cm[6 * a + b]) * po[b];
        t = b == 0 ? m : t + m;
      }
      y[a] = y[a] + t;
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) V.Ap[6 * (size_t)n + a] = y[a];
}

// the six products of node n of a . b, summed in index order
ATDN_HD inline double pg_dot6(const double* a, const double* b, int n) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double t = a[6 * (size_t)n + k] * b[6 * (size_t)n + k];
    s = k == 0 ? t : s + t;
  }
  return s;
}

// trial_n = acc_n . [C(dw) | dt] with the step x_n = (dw, dt) and its Cayley matrix C; a node that is not free is copied.
// Returns whether the step is finite.
ATDN_HD inline bool pg_retract_node(const PgView& V, int n) {
#pragma clang fp contract(off)
  const double* A = V.acc + 12 * (size_t)n;
  double* T = V.trial + 12 * (size_t)n;
  if (!V.free_[n]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = A[k];
    return true;
  }
  double dl[6], Em[9];
#pragma unroll
  for (int k = 0; k < 6; ++k) dl[k] = V.x[6 * (size_t)n + k];
  cayley3(dl, Em);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) T[3 * a + b] = dot3(A[3 * a], Em[b], A[3 * a + 1], Em[3 + b], A[3 * a + 2], Em[6 + b]);
    const double rt = dot3(A[3 * a], dl[3], A[3 * a + 1], dl[4], A[3 * a + 2], dl[5]);
    T[9 + a] = rt + A[9 + a];
  }
  return finite6(dl);
}

// The fixed-order sum of v[0..n): chunks of 256 values (+0.0 beyond n), in a chunk the binary tree of strides 1 .. 128
// (v[i] += v[i + stride] for i a multiple of 2 * stride), the chunk sums added in chunk order (the tree of pnp_plane_host).
inline double pg_tree_sum(const double* v, int n) {
#pragma clang fp contract(off)
  double total = 0.0;
  double w[PG_THREADS];
  for (int c = 0; c * PG_THREADS < n; ++c) {
    for (int t = 0; t < PG_THREADS; ++t) w[t] = c * PG_THREADS + t < n ? v[c * PG_THREADS + t] : 0.0;
    for (int stride = 1; stride < PG_THREADS; stride *= 2)
      for (int i = 0; i < PG_THREADS; i += 2 * stride) w[i] = w[i] + w[i + stride];
    total = c == 0 ? w[0] : total + w[0];
  }
  return total;
}

// The solver, written once. It reaches all edges or nodes only through the executor x:
//   x.each(n, f)    f(i) for every i < n; what it wrote is visible to all afterwards
//   x.serial(f)     f() once, after everything before it; its result is known to all
//   x.sum(n, f)     the fixed-order sum (pg_tree_sum) of f(i), i < n, the same value for all
//   x.count(n, f)   how many i < n have f(i)
//   x.all(n, f)     whether all i < n have f(i); every f(i) is evaluated
// Where "all" are the threads of a workgroup, every one of them runs this function: its control flow depends only on its
// arguments and on what the primitives return, so all take the same path, and no primitive stands inside an f.
// iters < 0 is one evaluation (atdn_pose_graph_terms: cost[0] and counts[0..1] only, poses_out unused).
template <class X>
ATDN_HD inline void pg_solve(const PgProblem& P, const PgView& V, int iters, int cg_iters, double tol2, float* poses_out,
                             double* cost, double* edge_chi2, int* counts, X& x) {
#pragma clang fp contract(off)
  const int N = P.N, E = P.E;
  const int valid = x.count(E, [&](int e) {
    const int kind = pg_edge_kind(P, e, &V.ei[e], &V.ej[e]);
    V.kind[e] = kind;
    return kind != PG_ABSENT;
  });
  x.each(N, [&](int n) { V.deg[n] = pg_node_incidence(V, E, n, false); });
  x.serial([&] {
    V.off[0] = 0;
    for (int n = 0; n < N; ++n) V.off[n + 1] = V.off[n] + V.deg[n];
    return true;
  });
  x.each(N, [&](int n) {
    pg_node_incidence(V, E, n, true);
    V.free_[n] = V.deg[n] > 0 && !(P.fixed && P.fixed[n] != 0);
    pg_internal_pose(P.poses + 12 * (size_t)n, V.acc + 12 * (size_t)n);
  });
  const auto cost_at = [&](const double* poses) {
    x.each(E, [&](int e) { pg_edge_phase(P, V, poses, e, false); });
    return x.sum(N, [&](int n) {
      pg_node_cost(V, n);
      return V.costn[n];
    });
  };
  const auto dot = [&](const double* a, const double* b) { return x.sum(N, [&](int n) { return pg_dot6(a, b, n); }); };
  const auto precondition = [&] {   // z = M^-1 r
    x.serial([&] {
      pg_sweep_forward_all(V, N);
      return true;
    });
    x.each(N, [&](int n) { pg_node_pivot_solve(V, n); });
    x.serial([&] {
      pg_sweep_backward_all(V, N);
      return true;
    });
  };
  double cost_acc = cost_at(V.acc);
  const double cost0 = cost_acc;
  double lambda = 1e-3;
  int accepted = 0, cg_total = 0;
  bool fresh = false;
  for (int k = 0; k < iters; ++k) {
    if (!fresh) {
      x.each(E, [&](int e) { pg_edge_phase(P, V, V.acc, e, true); });
      x.each(N, [&](int n) { pg_node_gather(V, N, n); });
      fresh = true;
    }
    bool ok = x.serial([&] {
      for (int n = 0; n < N; ++n)
        if (!pg_factor_node(V, N, n, lambda)) return false;
      return true;
    });
    if (ok) {
      x.each(N, [&](int n) {
        for (size_t i = 6 * (size_t)n; i < 6 * (size_t)n + 6; ++i) {
          V.x[i] = 0.0;
          V.r[i] = V.free_[n] ? -V.g[i] : 0.0;
          V.z[i] = 0.0;
          V.Ap[i] = 0.0;
        }
      });
      precondition();
      x.each(N, [&](int n) {
        for (size_t i = 6 * (size_t)n; i < 6 * (size_t)n + 6; ++i) V.p[i] = V.z[i];
      });
      double rz = dot(V.r, V.z);
      const double thr = tol2 * rz;
      if (rz > 0.0) {
        for (int it = 0; it < cg_iters; ++it) {
          x.each(N, [&](int n) { pg_apply_node(V, n, lambda); });
          const double pAp = dot(V.p, V.Ap);
          if (!(pAp > 0.0)) break;
          const double alpha = rz / pAp;
          x.each(N, [&](int n) {
#pragma clang fp contract(off)
            for (size_t i = 6 * (size_t)n; i < 6 * (size_t)n + 6; ++i) {
              const double ap = alpha * V.p[i], aAp = alpha * V.Ap[i];
              V.x[i] = V.x[i] + ap;
              V.r[i] = V.r[i] - aAp;
            }
          });
          ++cg_total;
          precondition();
          const double rz_new = dot(V.r, V.z);
          if (!(rz_new > thr)) break;
          const double beta = rz_new / rz;
          x.each(N, [&](int n) {
#pragma clang fp contract(off)
            for (size_t i = 6 * (size_t)n; i < 6 * (size_t)n + 6; ++i) {
              const double bp = beta * V.p[i];
              V.p[i] = V.z[i] + bp;
            }
          });
          rz = rz_new;
        }
      }
      ok = x.all(N, [&](int n) { return pg_retract_node(V, n); });
    }
    bool accept = false;
    if (ok) {
      const double c = cost_at(V.trial);
      accept = c < cost_acc;
      if (accept) {
        x.each(N, [&](int n) {
          for (size_t i = 12 * (size_t)n; i < 12 * (size_t)n + 12; ++i) V.acc[i] = V.trial[i];
        });
        cost_acc = c;
        accepted += 1;
        fresh = false;
      }
    }
    lambda = lm_lambda(lambda, accept);
  }
  const float* final_poses = P.poses;
  if (iters >= 0) {
    x.each(N, [&](int n) {
      float* o = poses_out + 12 * (size_t)n;
      if (accepted > 0 && V.free_[n])
        pg_public_pose(V.acc + 12 * (size_t)n, o);
      else
        for (int k = 0; k < 12; ++k) o[k] = P.poses[12 * (size_t)n + k];
    });
    final_poses = poses_out;
  }
  x.each(E, [&](int e) { edge_chi2[e] = pg_edge_chi2(P, V, final_poses, e); });
  x.serial([&] {
    cost[0] = cost0;
    counts[0] = valid;
    counts[1] = E - valid;
    if (iters >= 0) {
      cost[1] = cost_acc;
      counts[2] = accepted;
      counts[3] = cg_total;
    }
    return true;
  });
}

// The executor of the host form: plain loops.
struct PgHostExec {
  std::vector<double> tmp;   // [N]: the terms of a sum
  template <class F> void each(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
  template <class F> bool serial(F f) { return f(); }
  template <class F> double sum(int n, F f) {
    for (int i = 0; i < n; ++i) tmp[i] = f(i);
    return pg_tree_sum(tmp.data(), n);
  }
  template <class F> int count(int n, F f) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += f(i) ? 1 : 0;
    return c;
  }
  template <class F> bool all(int n, F f) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = f(i) && ok;
    return ok;
  }
};

// One graph on the host, its working arrays in a std::vector.
inline void pose_graph_run_host(const PgProblem& P, int iters, int cg_iters, double cg_tol, float* poses_out, double* cost,
                                double* edge_chi2, int* counts) {
#pragma clang fp contract(off)
  std::vector<double> mem(pg_graph_bytes(P.N, P.E) / 8);
  PgHostExec x{std::vector<double>(P.N)};
  pg_solve(P, pg_carve(mem.data(), P.N, P.E), iters, cg_iters, cg_tol * cg_tol, poses_out, cost, edge_chi2, counts, x);
}

}  // namespace atdn
