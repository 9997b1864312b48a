// Windowed dense bundle adjustment on the device: the terms of one evaluation (atdn_bundle_terms) and the Levenberg-Marquardt
// solve over the poses of the listed views and the inverse depths of the anchor's candidates (atdn_bundle_adjust), batched over
// problems. The rule — float64, every operation rounded on its own, no matrix instructions — is written once in bundle_host.h,
// whose functions these kernels call, and the ORDER of every sum is part of it: the same bits on every call and on both paths.
//
// Two launches per evaluation, nothing else on the stream (no memset, no atomics, no host synchronisation; capturable):
//   ba_terms_kernel     (chunks, B) workgroups of 256 threads; workgroup ch of problem b owns the candidate positions
//                       512 ch .. 512 ch + 511 and walks them in sub-chunks of PS = 192 / S positions. PIXEL PHASE: thread
//                       (position, view) reads its correspondence, the views of a position meet in LDS for the candidate test,
//                       for the depth step from the accepted state (c, b, E . dxi summed over the views in list order) and for c,
//                       b and the cost at the trial state; each thread then stages its view's 27 terms and 6 values of E, the
//                       position its 1 / c, b / c and cost: 36 S float64 per position, 55 KiB per sub-chunk. ENTRY PHASE: every
//                       thread owns output entries in registers and walks the sub-chunk's positions in ascending order — the
//                       first S (S + 1) / 2 threads a 6 x 6 view-pair block of T0 each (12 LDS reads and one multiply for E / c
//                       per 36 multiply-adds; 13 KB of LDS reads per position at S = 16, not the 74 KB of one entry per thread),
//                       the others up to five of the 33 S + 1 small sums (v0, H_s, g_s, cost) each. The accumulators live across
//                       the sub-chunks; at the end the workgroup stores them in ITS slot of the workspace (store-and-sum:
//                       cdna_hip_programming.md, Guideline 12). 62 KiB of static LDS: two workgroups per CU.
//   ba_finalise_kernel  one workgroup of 1024 threads per problem: entry e is summed over the chunks in chunk order (coalesced,
//                       eight reads in flight per thread: the sum is bound by what one CU can read), thread 0 takes
//                       the decision, the accepted sums are kept in the workspace; S_lambda is built in place of T0 in LDS, the
//                       n x n LDL^T runs column by column with one thread per row (two barriers per column), thread 0 solves,
//                       one thread per view retracts. After the last evaluation it writes the outputs, the depth plane included.
// Evaluation 0 reads the caller's poses and depth; later ones the state, rho accepted and rho trial of the workspace, all of
// which evaluation 0 has written: the workspace carries nothing from one call to the next.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "bundle_host.h"
#include "flow_args.h"

namespace atdn {

constexpr int BA_THREADS = 256;
constexpr int BA_FIN_THREADS = 1024;    // the finalise workgroup: the ordered chunk sum is one workgroup's memory traffic
constexpr int BA_SUB_THREADS = 192;     // (position, view) pairs of a sub-chunk
constexpr int BA_STAGE = 36;            // float64 staged per pair: 27 terms, 6 of E, 3 scratch (c_s, b_s, cost_s or E_s . dxi_s)
constexpr int BA_SMALL = 5;             // small sums per thread: (33 S + 1) / (256 - S (S + 1) / 2) <= 4.41 for S <= 16
static_assert(BA_CHUNK % 2 == 0 && BA_SUB_THREADS >= BA_MAX_VIEWS, "chunk shape");
static_assert(33 * BA_MAX_VIEWS + 1 <= BA_SMALL * (BA_THREADS - BA_MAX_VIEWS * (BA_MAX_VIEWS + 1) / 2), "small sums do not fit");

struct BaWorkspace {
  BundleState* state;   // [B]
  double* acc_sums;     // [B, NS] the sums at the accepted state
  double* csums;        // [B, chunks, NS]
  double* rho_acc;      // [B, positions]
  double* rho_trial;    // [B, positions]
  int* ccounts;         // [B, chunks, 4]
};

static size_t ba_workspace_size(int B, int S, int H, int W, int stride) {
  const size_t npos = (size_t)ba_positions(H, W, stride), chunks = (size_t)ba_chunks(H, W, stride), NS = (size_t)ba_sums(S);
  return (size_t)B * (sizeof(BundleState) + NS * 8 + chunks * NS * 8 + 2 * npos * 8 + chunks * 16);
}

static BaWorkspace ba_carve(void* workspace, int B, int S, int H, int W, int stride) {
  static_assert(sizeof(BundleState) % 8 == 0, "state size");
  const size_t npos = (size_t)ba_positions(H, W, stride), chunks = (size_t)ba_chunks(H, W, stride), NS = (size_t)ba_sums(S);
  BaWorkspace ws;
  ws.state = (BundleState*)workspace;
  ws.acc_sums = (double*)(ws.state + B);
  ws.csums = ws.acc_sums + (size_t)B * NS;
  ws.rho_acc = ws.csums + (size_t)B * chunks * NS;
  ws.rho_trial = ws.rho_acc + (size_t)B * npos;
  ws.ccounts = (int*)(ws.rho_trial + (size_t)B * npos);
  return ws;
}

// The sums of the three scratch values of the S views of one position in list order, from +0.0: four views' reads in flight,
// the additions one after the other. base: the position's first pair in the staging area.
__device__ inline void ba_fold_views(const double* base, int S, double& s0, double& s1, double& s2) {
#pragma clang fp contract(off)
  s0 = 0.0;
  s1 = 0.0;
  s2 = 0.0;
  for (int v0 = 0; v0 < S; v0 += 4) {
    double x[4][3];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double* o = base + (v0 + u < S ? v0 + u : S - 1) * BA_STAGE;
      x[u][0] = o[33];
      x[u][1] = o[34];
      x[u][2] = o[35];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v0 + u < S) {
        s0 = s0 + x[u][0];
        s1 = s1 + x[u][1];
        s2 = s2 + x[u][2];
      }
  }
}

// k == 0: evaluation at the caller's poses and depth_init; k >= 1: at the state's trial poses, after the depth step
__global__ __launch_bounds__(BA_THREADS) void ba_terms_kernel(const float* __restrict__ acc_bank,
                                                              const unsigned char* __restrict__ alive_bank,
                                                              const float* __restrict__ poses, const int* __restrict__ slots,
                                                              const float* __restrict__ depth_init,
                                                              const unsigned char* __restrict__ mask, int N, int S, int H, int W,
                                                              BundleParams c, int k, const BundleState* __restrict__ state,
                                                              double* __restrict__ rho_acc, double* __restrict__ rho_trial,
                                                              double* __restrict__ csums, int* __restrict__ ccounts) {
#pragma clang fp contract(off)
  __shared__ double stage[BA_SUB_THREADS * BA_STAGE];
  __shared__ double pix[3 * BA_SUB_THREADS];                    // per position: 1 / c, b / c, cost
  __shared__ double Pt[BA_MAX_VIEWS * MV_POSE], Pa[BA_MAX_VIEWS * MV_POSE], dxi[BA_MAX_N];
  __shared__ int slot[BA_MAX_VIEWS];
  __shared__ unsigned char obsf[BA_SUB_THREADS];
  const int t = threadIdx.x, b = blockIdx.y, ch = blockIdx.x;
  const long n = (long)H * W;
  const int nu = 6 * S, NS = ba_sums(S);
  const int Ws = ba_grid(W, c.stride);
  const long npos = ba_positions(H, W, c.stride);
  const BundleState& st = state[b];
  if (k == 0) {
    if (t < S) multiview_view(poses, slots + (long)b * S, N, t, slot, Pt);
  } else {
    if (t < S) slot[t] = st.slot[t];
    if (t < S * MV_POSE) {
      Pt[t] = st.trial[t];
      Pa[t] = st.acc[t];
    }
    if (t < nu) dxi[t] = st.dxi[t];
  }
  const bool back = k > 0 && st.step_ok != 0;
  const bool commit = k > 0 && st.last_accept != 0;
  const double lambda = k > 0 ? st.lambda : 0.0;
  __syncthreads();

  // the entries this thread owns
  const int NP = S * (S + 1) / 2;
  int si = 0, sj = 0;
  if (t < NP) {
    int r = t;
    while (r >= S - si) { r -= S - si; ++si; }
    sj = si + r;
  }
  int soff[BA_SMALL], skind[BA_SMALL], sidx[BA_SMALL];          // kind 0: E * (b / c), 1: staged term, 2: cost, -1: none
  for (int i = 0; i < BA_SMALL; ++i) {
    const int e = t < NP ? -1 : (t - NP) + i * (BA_THREADS - NP);
    skind[i] = -1;
    soff[i] = 0;
    sidx[i] = 0;
    if (e >= 0 && e < nu) {
      skind[i] = 0;
      soff[i] = (e / 6) * BA_STAGE + 27 + e % 6;
      sidx[i] = ba_tri(nu) + e;
    } else if (e >= nu && e < nu + BA_VIEW_TERMS * S) {
      const int r = e - nu;
      skind[i] = 1;
      soff[i] = (r / BA_VIEW_TERMS) * BA_STAGE + r % BA_VIEW_TERMS;
      sidx[i] = ba_tri(nu) + e;
    } else if (e == nu + BA_VIEW_TERMS * S) {
      skind[i] = 2;
      sidx[i] = NS - 1;
    }
  }
  double accu[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) accu[i] = 0.0;
  int cnt0 = 0, cnt1 = 0, cnt2 = 0;

  const int PS = BA_SUB_THREADS / S;                            // positions per sub-chunk
  const int pl = t / S, s = t - pl * S;
  const bool active = pl < PS;
  const long q_begin = (long)ch * BA_CHUNK;
  const long q_end = q_begin + BA_CHUNK < npos ? q_begin + BA_CHUNK : npos;
  double* mine = stage + (active ? t : 0) * BA_STAGE;
  for (long q0 = q_begin; q0 < q_end; q0 += PS) {
    // ---- pixel phase
    const long q = q0 + pl;
    const bool inpos = active && q < q_end;
    int x = 0, y = 0;
    long p = 0;
    double x2 = 0.0, y2 = 0.0;
    bool obs = false, allowed = true;
    float z0 = 0.0f;
    double r_in = 0.0;
    if (inpos) {
      y = (int)(q / Ws) * c.stride;
      x = (int)(q % Ws) * c.stride;
      p = (long)y * W + x;
      // every read of the position is issued here, so that one memory latency covers them all (a position that is no
      // candidate holds 0 in both rho planes since evaluation 0)
      z0 = depth_init[b * n + p];
      if (mask) allowed = mask[b * n + p] != 0;
      if (k > 0) r_in = commit ? rho_trial[b * npos + q] : rho_acc[b * npos + q];
      if (slot[s] >= 0) obs = ba_observe(acc_bank, alive_bank, slot[s], n, p, x, y, H, W, &x2, &y2);
    }
    if (active) obsf[t] = obs ? 1 : 0;
    __syncthreads();
    bool cand = false;
    double ra = 0.0, a0 = 0.0, a1 = 0.0;
    if (inpos) {
      int n_obs = 0;
      for (int v = 0; v < S; ++v) n_obs += obsf[pl * S + v];
      const double zd = (double)z0;
      cand = allowed && zd > 0.0 && zd <= (double)FLT_MAX && n_obs >= c.min_views;
      if (cand) {
        ra = k == 0 ? 1.0 / zd : r_in;
        ba_ray(x, y, c, &a0, &a1);
      }
    }
    double rt = ra;
    double tt[BA_VIEW_TERMS], E[6], cv, bv, costv;
    if (back) {
      if (active) {
        double ev = 0.0;
        cv = 0.0;
        bv = 0.0;
        if (cand && obs) {
          ba_view(Pa + s * MV_POSE, a0, a1, ra, x2, y2, c, tt, E, &cv, &bv, &costv);
          ev = ba_dot6(E, dxi + 6 * s);
        }
        mine[33] = cv;
        mine[34] = bv;
        mine[35] = ev;
      }
      __syncthreads();
      if (cand) {
        double cc, bb, ee;
        ba_fold_views(stage + pl * S * BA_STAGE, S, cc, bb, ee);
        rt = ba_backsub(cc, bb, ee, lambda, ra);
      }
      __syncthreads();
    }
    int flags = 0;
    cv = 0.0;
    bv = 0.0;
    costv = 0.0;
    if (cand && obs) {
      flags = ba_view(Pt + s * MV_POSE, a0, a1, rt, x2, y2, c, tt, E, &cv, &bv, &costv);
    } else {
#pragma unroll
      for (int i = 0; i < BA_VIEW_TERMS; ++i) tt[i] = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) E[i] = 0.0;
    }
    if (active) {
      mine[33] = cv;
      mine[34] = bv;
      mine[35] = costv;
    }
    cnt1 += (flags & BA_FRONT) ? 1 : 0;
    cnt2 += (flags & BA_INLIER) ? 1 : 0;
    __syncthreads();
    if (active) {
      double cc, bb, cost;
      ba_fold_views(stage + pl * S * BA_STAGE, S, cc, bb, cost);
      const bool valid = cand && cc > 0.0;
#pragma unroll
      for (int i = 0; i < BA_VIEW_TERMS; ++i) mine[i] = valid ? tt[i] : 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) mine[27 + i] = valid ? E[i] : 0.0;
      if (s == 0) {
        double ic = 0.0, bc = 0.0;
        if (valid) {
          ic = 1.0 / cc;
          bc = bb * ic;
        }
        pix[pl] = ic;
        pix[BA_SUB_THREADS + pl] = bc;
        pix[2 * BA_SUB_THREADS + pl] = cand ? cost : 0.0;
        if (inpos) {
          rho_acc[b * npos + q] = cand ? ra : 0.0;
          rho_trial[b * npos + q] = cand ? rt : 0.0;
        }
        cnt0 += cand ? 1 : 0;
      }
    }
    __syncthreads();
    // ---- entry phase: the positions of the sub-chunk in ascending order
    if (t < NP) {
      for (int pp = 0; pp < PS; ++pp) {
        const double* o = stage + pp * S * BA_STAGE;
        const double ic = pix[pp];
        double F[6], G[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          F[i] = o[si * BA_STAGE + 27 + i] * ic;
          G[i] = o[sj * BA_STAGE + 27 + i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const double f = F[i] * G[j];
            accu[6 * i + j] = accu[6 * i + j] + f;
          }
      }
    } else {
      for (int pp = 0; pp < PS; ++pp) {
        const double* o = stage + pp * S * BA_STAGE;
        const double bc = pix[BA_SUB_THREADS + pp], cost = pix[2 * BA_SUB_THREADS + pp];
#pragma unroll
        for (int i = 0; i < BA_SMALL; ++i) {
          if (skind[i] < 0) continue;
          double f;
          if (skind[i] == 0)
            f = o[soff[i]] * bc;
          else if (skind[i] == 1)
            f = o[soff[i]];
          else
            f = cost;
          accu[i] = accu[i] + f;
        }
      }
    }
    __syncthreads();
  }
  // ---- the chunk's sums to the chunk's slot
  double* out = csums + ((long)b * gridDim.x + ch) * NS;
  if (t < NP) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (si < sj || i <= j) out[ba_ut(nu, 6 * si + i, 6 * sj + j)] = accu[6 * i + j];
  } else {
#pragma unroll
    for (int i = 0; i < BA_SMALL; ++i)
      if (skind[i] >= 0) out[sidx[i]] = accu[i];
  }
  int* ic = (int*)stage;
  ic[t] = cnt0;
  ic[BA_THREADS + t] = cnt1;
  ic[2 * BA_THREADS + t] = cnt2;
  __syncthreads();
  if (t < 3) {
    int v = 0;
    for (int i = 0; i < BA_THREADS; ++i) v += ic[t * BA_THREADS + i];
    ccounts[((long)b * gridDim.x + ch) * 4 + t] = v;
  }
}

// k < 0: atdn_bundle_terms (the sums go to sums_out / counts_out). k >= 0: evaluation k of a solve of `iters` steps.
__global__ __launch_bounds__(BA_FIN_THREADS) void ba_finalise_kernel(const double* __restrict__ csums, const int* __restrict__ ccounts,
                                                                 int chunks, int k, int iters, int N, int S, int H, int W,
                                                                 int stride, BundleState* __restrict__ state,
                                                                 double* __restrict__ acc_sums, const double* __restrict__ rho_acc,
                                                                 const double* __restrict__ rho_trial,
                                                                 const float* __restrict__ poses, const int* __restrict__ slots,
                                                                 double* __restrict__ sums_out, int* __restrict__ counts_out,
                                                                 float* __restrict__ poses_out, float* __restrict__ depth,
                                                                 double* __restrict__ cost_out) {
#pragma clang fp contract(off)
  __shared__ double T[BA_MAX_N * (BA_MAX_N + 1) / 2 + 33 * BA_MAX_VIEWS + 1];
  __shared__ double D[BA_MAX_N], xs[BA_MAX_N];
  __shared__ BundleState st;
  __shared__ int Cn[3];
  __shared__ int flag;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = 6 * S, NS = ba_sums(S);
  for (int e = t; e < NS; e += BA_FIN_THREADS) {
    const double* src = csums + (long)b * chunks * NS + e;
    double v = 0.0;
    int ch = 0;
    for (; ch + 8 <= chunks; ch += 8) {          // eight reads in flight, the additions one after the other in chunk order
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = src[(long)(ch + u) * NS];
#pragma unroll
      for (int u = 0; u < 8; ++u) v = v + x[u];
    }
    for (; ch < chunks; ++ch) v = v + src[(long)ch * NS];
    T[e] = v;
  }
  if (t < 3) {
    int v = 0;
    for (int ch = 0; ch < chunks; ++ch) v += ccounts[((long)b * chunks + ch) * 4 + t];
    Cn[t] = v;
  }
  if (k > 0) {
    const int* src = (const int*)(state + b);
    int* dst = (int*)&st;
    for (int i = t; i < (int)(sizeof(BundleState) / 4); i += BA_FIN_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  if (k < 0) {
    for (int e = t; e < NS; e += BA_FIN_THREADS) sums_out[(long)b * NS + e] = T[e];
    if (t < 3) counts_out[3 * b + t] = Cn[t];
    return;
  }
  if (t == 0) {
    if (k == 0) ba_init_state(st, poses, slots + (long)b * S, N, S);
    flag = ba_decide(st, T[NS - 1], Cn, k) ? 1 : 0;
  }
  __syncthreads();
  const bool accept = flag != 0;
  double* as = acc_sums + (long)b * NS;
  for (int e = t; e < NS; e += BA_FIN_THREADS) {
    if (accept)
      as[e] = T[e];
    else
      T[e] = as[e];
  }
  __syncthreads();
  if (k < iters) {
    if (t < n) xs[t] = ba_rhs_entry(T, st, S, t);
    for (int idx = t; idx < n * n; idx += BA_FIN_THREADS) {
      const int i = idx / n, j = idx - i * n;
      if (i <= j) T[ba_ut(n, i, j)] = ba_system_entry(T, st, S, i, j);
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      double v = 0.0;
      if (t >= j && t < n) v = ldln_col(T, D, n, t, j);
      if (t == j) D[j] = v;
      __syncthreads();
      if (t > j && t < n) T[ba_ut(n, j, t)] = v / D[j];
      __syncthreads();
    }
    if (t == 0) {
      bool ok = true;
      for (int j = 0; j < n; ++j) ok = ok && D[j] > 0.0;
      ldln_solve(T, D, n, xs);
      ba_take_step(st, xs, n, ok);
    }
    __syncthreads();
    if (t < S) ba_retract_view(st, t);
  } else {
    if (t < S) ba_output_pose(st, poses, t, poses_out + ((long)b * S + t) * 12);
    if (t == 0) ba_output_scalars(st, cost_out + 2L * b, counts_out + 4L * b);
    const long np = (long)H * W, npos = ba_positions(H, W, stride);
    const int Ws = ba_grid(W, stride);
    const double* rho = (st.last_accept ? rho_trial : rho_acc) + (long)b * npos;
    for (long p = t; p < np; p += BA_FIN_THREADS) {
      const int y = (int)(p / W), x = (int)(p - (long)y * W);
      float z = 0.0f;
      if (x % stride == 0 && y % stride == 0) z = ba_output_depth(rho[(long)(y / stride) * Ws + x / stride]);
      depth[(long)b * np + p] = z;
    }
  }
  __syncthreads();
  {
    int* dst = (int*)(state + b);
    const int* src = (const int*)&st;
    for (int i = t; i < (int)(sizeof(BundleState) / 4); i += BA_FIN_THREADS) dst[i] = src[i];
  }
}

struct BundleCall {
  const float* acc_bank;
  const unsigned char* alive_bank;
  const float* poses;
  const int* slots;
  const float* depth_init;
  const unsigned char* mask;   // may be null
  int N, B, S, H, W;
  double fx, fy, cx, cy;
  int stride, iters;
  double scale_px, inlier_px, min_z;
  int min_views;
};

// What the sizes of the outputs rest on, checked before they are formed. The device form (`device`) limits B to gridDim.y.
static void bundle_check_sizes(const BundleCall& c, bool device) {
  ATDN_CHECK(c.S >= 1 && c.S <= BA_MAX_VIEWS && c.stride >= 1, "S must be in [1, ATDN_MULTIVIEW_MAX_VIEWS] and stride >= 1");
  check_plane_batch(c.B, c.H, c.W, device);
}

// Argument rules of an entry pair, after bundle_check_sizes. out[i] of out_bytes[i]: the outputs (the device form's workspace
// among them), none of which may be null or overlap an input or another output. Returns the parameters of the call.
static BundleParams bundle_check_args(const BundleCall& c, bool device, const void* const* out, const long* out_bytes, int n_out) {
  ATDN_CHECK(c.acc_bank && c.alive_bank && c.poses && c.slots, "null argument");
  ATDN_CHECK(c.depth_init, "depth_init is mandatory");
  check_plane_solver(c.B, c.H, c.W, device, c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, out, n_out);
  ATDN_CHECK(c.N >= 1, "the bank is empty (N >= 1)");
  ATDN_CHECK(c.S >= 1 && c.S <= BA_MAX_VIEWS, "S must be in [1, ATDN_MULTIVIEW_MAX_VIEWS]");
  ATDN_CHECK(c.min_views >= 1 && c.min_views <= c.S, "min_views must be in [1, S]");
  ATDN_CHECK(c.stride >= 1, "stride must be >= 1");
  ATDN_CHECK(c.iters >= 0 && c.iters <= 16, "iters must be in [0, 16]");
  ATDN_CHECK(std::isfinite(c.min_z) && c.min_z > 0.0, "min_z must be finite and > 0");
  const long n = (long)c.H * c.W;
  const void* in[6] = {c.acc_bank, c.alive_bank, c.poses, c.slots, c.depth_init, c.mask};
  const long in_bytes[6] = {(long)c.N * 2 * n * 4, (long)c.N * n, (long)c.N * 48, (long)c.B * c.S * 4, (long)c.B * n * 4,
                            (long)c.B * n};
  check_disjoint(in, in_bytes, 6, out, out_bytes, n_out);
  return bundle_params(c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, c.min_z, c.min_views, c.iters, c.stride, c.H, c.W);
}

// Both forms of atdn_bundle_terms (iters of the call: 0)
static BundleParams bundle_terms_args(const BundleCall& c, double* sums, int* counts, bool device, void* workspace) {
  bundle_check_sizes(c, device);
  const void* out[3] = {sums, counts, workspace};
  const long out_bytes[3] = {(long)c.B * ba_sums(c.S) * 8, (long)c.B * 12,
                             (long)ba_workspace_size(c.B, c.S, c.H, c.W, c.stride)};
  return bundle_check_args(c, device, out, out_bytes, device ? 3 : 2);
}

// Both forms of atdn_bundle_adjust
static BundleParams bundle_adjust_args(const BundleCall& c, float* poses_out, float* depth, double* cost, int* counts, bool device,
                                       void* workspace) {
  bundle_check_sizes(c, device);
  const void* out[5] = {poses_out, depth, cost, counts, workspace};
  const long out_bytes[5] = {(long)c.B * c.S * 48, (long)c.B * c.H * c.W * 4, (long)c.B * 16, (long)c.B * 16,
                             (long)ba_workspace_size(c.B, c.S, c.H, c.W, c.stride)};
  return bundle_check_args(c, device, out, out_bytes, device ? 5 : 4);
}

static void ba_launch_terms(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                            const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W,
                            const BundleParams& c, int k, const BaWorkspace& ws, hipStream_t stream) {
  hipLaunchKernelGGL(ba_terms_kernel, dim3((unsigned)ba_chunks(H, W, c.stride), (unsigned)B), dim3(BA_THREADS), 0, stream, acc_bank,
                     alive_bank, poses, slots, depth_init, mask, N, S, H, W, c, k, ws.state, ws.rho_acc, ws.rho_trial, ws.csums,
                     ws.ccounts);
  ATDN_HIP(hipGetLastError());
}

}  // namespace atdn

using namespace atdn;

long atdn_bundle_workspace_bytes(int B, int S, int H, int W, int stride) {
  if (B < 1 || S < 1 || S > BA_MAX_VIEWS || H < 1 || W < 1 || stride < 1 || (long)H * W > (1L << 24)) return 0;
  return (long)ba_workspace_size(B, S, H, W, stride);
}

int atdn_bundle_terms(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                      const float* depth, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                      double cx, double cy, int stride, double scale_px, double inlier_px, double min_z, int min_views, double* sums,
                      int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const BundleCall a{acc_bank, alive_bank, poses, slots, depth, mask, N, B, S, H, W, fx, fy, cx, cy, stride, 0,
                     scale_px, inlier_px, min_z, min_views};
  const BundleParams c = bundle_terms_args(a, sums, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "workspace and sums must be 8-byte aligned");
  const BaWorkspace ws = ba_carve(workspace, B, S, H, W, stride);
  ba_launch_terms(acc_bank, alive_bank, poses, slots, depth, mask, N, B, S, H, W, c, 0, ws, (hipStream_t)stream);
  hipLaunchKernelGGL(ba_finalise_kernel, dim3((unsigned)B), dim3(BA_FIN_THREADS), 0, (hipStream_t)stream, ws.csums, ws.ccounts,
                     (int)ba_chunks(H, W, stride), -1, 0, N, S, H, W, stride, ws.state, ws.acc_sums, ws.rho_acc, ws.rho_trial, poses,
                     slots, sums, counts, (float*)nullptr, (float*)nullptr, (double*)nullptr);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_bundle_terms_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                           const float* depth, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                           double cx, double cy, int stride, double scale_px, double inlier_px, double min_z, int min_views,
                           double* sums, int* counts) {
  ATDN_API_BEGIN
  const BundleCall a{acc_bank, alive_bank, poses, slots, depth, mask, N, B, S, H, W, fx, fy, cx, cy, stride, 0,
                     scale_px, inlier_px, min_z, min_views};
  const BundleParams c = bundle_terms_args(a, sums, counts, false, nullptr);
  bundle_terms_host(acc_bank, alive_bank, poses, slots, depth, mask, N, B, S, H, W, c, sums, counts);
  ATDN_API_END
}

int atdn_bundle_adjust(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                       const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                       double cx, double cy, int stride, int iters, double scale_px, double inlier_px, double min_z, int min_views,
                       float* poses_out, float* depth, double* cost, int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const BundleCall a{acc_bank, alive_bank, poses, slots, depth_init, mask, N, B, S, H, W, fx, fy, cx, cy, stride, iters,
                     scale_px, inlier_px, min_z, min_views};
  const BundleParams c = bundle_adjust_args(a, poses_out, depth, cost, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)cost & 7) == 0, "workspace and cost must be 8-byte aligned");
  const BaWorkspace ws = ba_carve(workspace, B, S, H, W, stride);
  for (int k = 0; k <= iters; ++k) {
    ba_launch_terms(acc_bank, alive_bank, poses, slots, depth_init, mask, N, B, S, H, W, c, k, ws, (hipStream_t)stream);
    hipLaunchKernelGGL(ba_finalise_kernel, dim3((unsigned)B), dim3(BA_FIN_THREADS), 0, (hipStream_t)stream, ws.csums, ws.ccounts,
                       (int)ba_chunks(H, W, stride), k, iters, N, S, H, W, stride, ws.state, ws.acc_sums, ws.rho_acc, ws.rho_trial,
                       poses, slots, (double*)nullptr, counts, poses_out, depth, cost);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}

int atdn_bundle_adjust_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                            const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W, double fx,
                            double fy, double cx, double cy, int stride, int iters, double scale_px, double inlier_px, double min_z,
                            int min_views, float* poses_out, float* depth, double* cost, int* counts) {
  ATDN_API_BEGIN
  const BundleCall a{acc_bank, alive_bank, poses, slots, depth_init, mask, N, B, S, H, W, fx, fy, cx, cy, stride, iters,
                     scale_px, inlier_px, min_z, min_views};
  const BundleParams c = bundle_adjust_args(a, poses_out, depth, cost, counts, false, nullptr);
  bundle_adjust_host(acc_bank, alive_bank, poses, slots, depth_init, mask, N, B, S, H, W, c, poses_out, depth, cost, counts);
  ATDN_API_END
}
