// The ground plane of a depth map on the device: the terms of a plane q = n / h (atdn_ground_terms), the start vote with a
// Levenberg-Marquardt solve over the terms (atdn_ground_solve) and the per-pixel classification (atdn_ground_classify), batched
// over problems. The rule — float64, every operation rounded on its own — is ground_pixel, ground_vote_bin, ground_start_vote,
// ground_lm_update, ground_lm_step and ground_output of ground_host.h (over ldl3_* of lm6.h), which these kernels call, so the
// kernels and the host form evaluate one function, and the ORDER of every sum is part of the rule (include/atdn_hip.h): the
// same bits on every call and on both paths.
//
// The pixels are a band of rows [y0, y1): a contiguous range of every plane, so the kernels walk the band as a plane of
// (y1 - y0) * W flat indices whose first row is y0 (y0 only enters the ray). Launches on the stream, nothing else (no memset, no
// global atomics, no host synchronisation; capturable):
//   ground_vote_kernel      (at most 32, B) workgroups, each over the chunks c, c + gridDim.x, ..: the bin of every pixel is
//                           counted into a 320-bin histogram in LDS (integer adds: the sum does not depend on the order), which
//                           the workgroup stores in ITS slot of the workspace
//   ground_terms_kernel     (chunks, B) workgroups of pixel_quads.h with off = 0: workgroup c of plane b owns the flat indices
//                           1024 c .. 1024 c + 1023 of the band, a thread four consecutive ones. It streams 4 or 5 bytes per pixel
//                           (depth, mask), keeps the 10 sums of its pixels in registers, reduces them by the fixed binary tree of
//                           plane_sum.h and stores them in its slot
//   ground_finalise_kernel  one wave per problem. GROUND_FIN_VOTE: adds the histogram slots, smooths, finds the mode (shuffles;
//                           ground_mode_better) and writes the start of the solve. GROUND_FIN_TERMS: the ordered sums, written
//                           out. k >= 0: the ordered sums, then the Levenberg-Marquardt decision and the next step (3 x 3 LDL^T,
//                           in registers) on the problem's GroundState, or the outputs after the last evaluation
//   ground_classify_kernel  the whole plane in quads: e as float32 and the inlier byte, zeros outside the band
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "ground_host.h"
#include "plane_sum.h"

namespace atdn {

constexpr int GROUND_VOTE_GROUPS = 32;
constexpr int GROUND_FIN_VOTE = -2, GROUND_FIN_TERMS = -1;
static_assert(sizeof(GroundState) % 8 == 0, "the chunk sums follow the states in the workspace");
static_assert(GROUND_BINS == 5 * PLANE_FIN_THREADS, "the finalise wave owns five bins per lane");

struct GroundWorkspace {
  GroundState* state;   // [B]
  double* sums;         // [B, chunks, 10]
  int* counts;          // [B, chunks, 4] (three used)
  int* hist;            // [B, vote groups, 320]
};

// sized for the whole plane: a band has no more chunks
static size_t ground_workspace_size(int B, int H, int W) {
  const size_t chunks = (size_t)plane_chunks(H, W);
  const size_t groups = chunks < (size_t)GROUND_VOTE_GROUPS ? chunks : (size_t)GROUND_VOTE_GROUPS;
  return (size_t)B * (sizeof(GroundState) + chunks * (GROUND_TERMS * sizeof(double) + 4 * sizeof(int)) +
                      groups * GROUND_BINS * sizeof(int));
}

static GroundWorkspace ground_carve(void* workspace, int B, int H, int W) {
  const size_t chunks = (size_t)plane_chunks(H, W);
  GroundWorkspace ws;
  ws.state = (GroundState*)workspace;
  ws.sums = (double*)(ws.state + B);
  ws.counts = (int*)(ws.sums + (size_t)B * chunks * GROUND_TERMS);
  ws.hist = ws.counts + (size_t)B * chunks * 4;
  return ws;
}

// plane: H * W; nb: the flat indices of the band. q_in != nullptr: the caller's q [B,3]; otherwise the trial of the state.
template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void ground_terms_kernel(const float* __restrict__ depth,
                                                                  const unsigned char* __restrict__ mask,
                                                                  const double* __restrict__ q_in,
                                                                  const GroundState* __restrict__ state, long plane, int nb,
                                                                  GroundParams c, double* __restrict__ csums,
                                                                  int* __restrict__ ccounts) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const long base = (long)b * plane + (long)c.y0 * c.W;
  const Quad qd = quad_of(nb, 0);
  double q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = q_in ? q_in[3 * b + i] : state[b].trial[i];
  float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool keep[4] = {true, true, true, true};
  if (qd.lo < qd.hi) {
    quad_load(qd, depth + base, z);
    if (MASKED) quad_load(qd, mask + base, keep);
  }
  const int r = qd.lo / c.W;
  int x = qd.lo - r * c.W, y = c.y0 + r;                       // of index lo; the quad may cross the end of a row
  double acc[GROUND_TERMS];
  int cnt[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double t[GROUND_TERMS];
    int flags = 0;
    if (qd.has(k)) {
      flags = ground_pixel(z[k], keep[k], q, c, x, y, t);
      if (++x == c.W) { x = 0; ++y; }
    } else {
#pragma unroll
      for (int e = 0; e < GROUND_TERMS; ++e) t[e] = 0.0;
    }
#pragma unroll
    for (int e = 0; e < GROUND_TERMS; ++e) acc[e] = k == 0 ? t[e] : acc[e] + t[e];   // ((t0 + t1) + t2) + t3
#pragma unroll
    for (int j = 0; j < 3; ++j) cnt[j] += __popcll(__ballot(flags & (1 << j)));      // the wave's count, in every lane
  }
  plane_chunk_reduce<GROUND_TERMS>(acc, cnt, b, csums, ccounts);
}

template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void ground_vote_kernel(const float* __restrict__ depth,
                                                                 const unsigned char* __restrict__ mask, long plane, int nb,
                                                                 int chunks, GroundParams c, int* __restrict__ hist_out) {
  __shared__ int hist[GROUND_BINS];
  for (int k = threadIdx.x; k < GROUND_BINS; k += PQ_THREADS) hist[k] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const long base = (long)b * plane + (long)c.y0 * c.W;
  for (int ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const Quad qd = quad_at(nb, 0, (unsigned)ch);
    if (qd.lo >= qd.hi) continue;
    float z[4];
    bool keep[4] = {true, true, true, true};
    quad_load(qd, depth + base, z);
    if (MASKED) quad_load(qd, mask + base, keep);
    const int r = qd.lo / c.W;
    int x = qd.lo - r * c.W, y = c.y0 + r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (qd.has(k)) {
        const int bin = ground_vote_bin(z[k], keep[k], c, x, y);
        if (bin >= 0) atomicAdd(&hist[bin], 1);                 // LDS, integer
        if (++x == c.W) { x = 0; ++y; }
      }
    }
  }
  __syncthreads();
  int* out = hist_out + ((long)b * gridDim.x + blockIdx.x) * GROUND_BINS;
  for (int k = threadIdx.x; k < GROUND_BINS; k += PQ_THREADS) out[k] = hist[k];
}

// mode GROUND_FIN_VOTE: `groups` histogram slots per problem. GROUND_FIN_TERMS: sums_out [B,10], counts_out [B,3]. k = mode >= 0:
// evaluation k of a solve of `iters` steps; q_init (may be null: the vote has set the start) is read at k = 0.
__global__ __launch_bounds__(PLANE_FIN_THREADS) void ground_finalise_kernel(const double* __restrict__ csums,
                                                                           const int* __restrict__ ccounts,
                                                                           const int* __restrict__ hist, int chunks, int groups,
                                                                           int mode, int iters, GroundParams c,
                                                                           GroundState* __restrict__ state,
                                                                           const double* __restrict__ q_init,
                                                                           double* __restrict__ q_out, double* __restrict__ sums_out,
                                                                           int* __restrict__ counts_out) {
#pragma clang fp contract(off)
  __shared__ double S[GROUND_TERMS];
  __shared__ int Cn[3];
  __shared__ int tot[GROUND_BINS];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  if (mode == GROUND_FIN_VOTE) {
    const int* p = hist + (long)b * groups * GROUND_BINS;
    int s[5] = {0, 0, 0, 0, 0};
    for (int g = 0; g < groups; ++g) {
#pragma unroll
      for (int j = 0; j < 5; ++j) s[j] += p[(long)g * GROUND_BINS + 64 * j + t];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) tot[64 * j + t] = s[j];
    __syncthreads();
    int votes = -1, own = -1, bin = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int k = 64 * j + t, v = ground_smoothed(tot, k);
      if (ground_mode_better(v, tot[k], k, votes, own, bin)) { votes = v; own = tot[k]; bin = k; }
    }
#pragma unroll
    for (int stride = 1; stride < 64; stride *= 2) {             // a total order: every lane ends with the same mode
      const int v = __shfl_xor(votes, stride, 64), c = __shfl_xor(own, stride, 64), k = __shfl_xor(bin, stride, 64);
      if (ground_mode_better(v, c, k, votes, own, bin)) { votes = v; own = c; bin = k; }
    }
    if (t == 0) ground_start_vote(state[b], c, bin, votes);
    return;
  }
  plane_ordered_sum<GROUND_TERMS>(csums, ccounts, chunks, b, S, Cn);
  if (mode == GROUND_FIN_TERMS) {
    if (t < GROUND_TERMS) sums_out[(long)b * GROUND_TERMS + t] = S[t];
    if (t < 3) counts_out[3 * b + t] = Cn[t];
    return;
  }
  if (t != 0) return;
  const int k = mode;
  GroundState& s = state[b];
  if (k == 0 && q_init) ground_start_init(s, q_init + 3 * b);
  ground_lm_update(s, S, Cn, k);
  if (k < iters)
    ground_lm_step(s);
  else
    ground_output(s, q_out + 3 * b, sums_out + (long)GROUND_TERMS * b, counts_out + 6 * b);
}

template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void ground_classify_kernel(const float* __restrict__ depth,
                                                                     const unsigned char* __restrict__ mask,
                                                                     const double* __restrict__ q_in, int n, int y1, GroundParams c,
                                                                     float* __restrict__ residual,
                                                                     unsigned char* __restrict__ on_ground) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const long base = (long)b * n;
  const Quad qd = quad_of(n, 0);
  if (qd.lo >= qd.hi) return;
  double q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = q_in[3 * b + i];
  float z[4];
  bool keep[4] = {true, true, true, true};
  quad_load(qd, depth + base, z);
  if (MASKED) quad_load(qd, mask + base, keep);
  int y = qd.lo / c.W, x = qd.lo - y * c.W;
  float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int in[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (qd.has(k)) {
      if (y >= c.y0 && y < y1) in[k] = ground_classify_pixel(z[k], keep[k], q, c, x, y, &e[k]);
      if (++x == c.W) { x = 0; ++y; }
    }
  }
  quad_store(qd, residual + base, e);
  quad_store(qd, on_ground + base, in, 1);
}

struct GroundCall {
  const float* depth;
  const unsigned char* mask;
  const double* q;
  int B, H, W, y0, y1;
  double fx, fy, cx, cy, scale_rel, inlier_rel, min_z, max_depth;
};

// Argument rules of an entry pair. q may be null only where `q_optional`. out[i] of out_bytes[i]: the outputs, none of which may
// be null or overlap an input or another output. The device form (`device`) limits B to gridDim.y before anything else, and its
// workspace, where it has one, is one more output.
static void ground_check_args(const GroundCall& c, bool q_optional, bool device, const void* const* out, const long* out_bytes,
                              int n_out) {
  if (device) check_plane_batch(c.B, c.H, c.W);
  ATDN_CHECK(c.depth && (c.q || q_optional), "null argument");
  for (int i = 0; i < n_out; ++i) ATDN_CHECK(out[i], "null argument");
  check_plane_batch(c.B, c.H, c.W, device);
  ATDN_CHECK(c.y0 >= 0 && c.y0 < c.y1 && c.y1 <= c.H, "the rows must satisfy 0 <= y0 < y1 <= H");
  check_pinhole(c.fx, c.fy, c.cx, c.cy);
  ATDN_CHECK(std::isfinite(c.scale_rel) && c.scale_rel > 0.0, "scale_rel must be finite and > 0");
  ATDN_CHECK(std::isfinite(c.inlier_rel) && c.inlier_rel > 0.0, "inlier_rel must be finite and > 0");
  ATDN_CHECK(std::isfinite(c.min_z) && c.min_z > 0.0, "min_z must be finite and > 0");
  ATDN_CHECK(std::isfinite(c.max_depth) && c.max_depth > 0.0, "max_depth must be finite and > 0");
  ATDN_CHECK(!c.q || ((uintptr_t)c.q & 7) == 0, "q must be 8-byte aligned");
  const long n = (long)c.H * c.W;
  const void* in[3] = {c.depth, c.mask, c.q};
  const long in_bytes[3] = {(long)c.B * n * 4, (long)c.B * n, (long)c.B * 24};
  check_disjoint(in, in_bytes, 3, out, out_bytes, n_out);
}

// Both forms of atdn_ground_terms: the checks and the parameters
static GroundParams ground_terms_args(const GroundCall& c, double* sums, int* counts, bool device, void* workspace) {
  const void* out[3] = {sums, counts, workspace};
  const long out_bytes[3] = {(long)c.B * GROUND_TERMS * 8, (long)c.B * 12, (long)ground_workspace_size(c.B, c.H, c.W)};
  ground_check_args(c, false, device, out, out_bytes, device ? 3 : 2);
  return ground_params(c.fx, c.fy, c.cx, c.cy, c.scale_rel, c.inlier_rel, c.min_z, c.max_depth, 0.0, 1.0, 0.0, 1, c.y0, c.W);
}

// Both forms of atdn_ground_solve
static GroundParams ground_solve_args(const GroundCall& c, double nx, double ny, double nz, int min_votes, int iters, double* q,
                                      double* sums, int* counts, bool device, void* workspace) {
  const void* out[4] = {q, sums, counts, workspace};
  const long out_bytes[4] = {(long)c.B * 24, (long)c.B * GROUND_TERMS * 8, (long)c.B * 24,
                             (long)ground_workspace_size(c.B, c.H, c.W)};
  ground_check_args(c, true, device, out, out_bytes, device ? 4 : 3);
  ATDN_CHECK(std::isfinite(nx) && std::isfinite(ny) && std::isfinite(nz) && (nx != 0.0 || ny != 0.0 || nz != 0.0),
             "the prior normal must be finite and not zero");
  ATDN_CHECK(min_votes >= 1, "min_votes must be >= 1");
  ATDN_CHECK(iters >= 0 && iters <= 64, "iters must be in [0, 64]");
  return ground_params(c.fx, c.fy, c.cx, c.cy, c.scale_rel, c.inlier_rel, c.min_z, c.max_depth, nx, ny, nz, min_votes, c.y0, c.W);
}

// Both forms of atdn_ground_classify (which build the call with scale_rel = 1.0)
static GroundParams ground_classify_args(const GroundCall& c, float* residual, unsigned char* on_ground, bool device) {
  const long n = (long)c.H * c.W;
  const void* out[2] = {residual, on_ground};
  const long out_bytes[2] = {(long)c.B * n * 4, (long)c.B * n};
  ground_check_args(c, false, device, out, out_bytes, 2);
  return ground_params(c.fx, c.fy, c.cx, c.cy, c.scale_rel, c.inlier_rel, c.min_z, c.max_depth, 0.0, 1.0, 0.0, 1, c.y0, c.W);
}

static void ground_launch_terms(const float* depth, const unsigned char* mask, const double* q, const GroundWorkspace& ws, int B,
                                int H, int W, int y1, const GroundParams& c, hipStream_t stream) {
  const int nb = (y1 - c.y0) * W;
  const dim3 grid((unsigned)cdivl(nb, PLANE_CHUNK), (unsigned)B);
  if (mask)
    hipLaunchKernelGGL(ground_terms_kernel<true>, grid, dim3(PQ_THREADS), 0, stream, depth, mask, q, ws.state, (long)H * W, nb, c,
                       ws.sums, ws.counts);
  else
    hipLaunchKernelGGL(ground_terms_kernel<false>, grid, dim3(PQ_THREADS), 0, stream, depth, mask, q, ws.state, (long)H * W, nb, c,
                       ws.sums, ws.counts);
  ATDN_HIP(hipGetLastError());
}

static void ground_launch_finalise(const GroundWorkspace& ws, int B, int chunks, int groups, int mode, int iters,
                                   const GroundParams& c, const double* q_init, double* q_out, double* sums, int* counts,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(ground_finalise_kernel, dim3((unsigned)B), dim3(PLANE_FIN_THREADS), 0, stream, ws.sums, ws.counts, ws.hist,
                     chunks, groups, mode, iters, c, ws.state, q_init, q_out, sums, counts);
  ATDN_HIP(hipGetLastError());
}

}  // namespace atdn

using namespace atdn;

long atdn_ground_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long)H * W > (1L << 24)) return 0;
  return (long)ground_workspace_size(B, H, W);
}

int atdn_ground_terms(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1, double fx,
                      double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z, double max_depth,
                      double* sums, int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q, B, H, W, y0, y1, fx, fy, cx, cy, scale_rel, inlier_rel, min_z, max_depth};
  const GroundParams c = ground_terms_args(a, sums, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "workspace and sums must be 8-byte aligned");
  const GroundWorkspace ws = ground_carve(workspace, B, H, W);
  ground_launch_terms(depth, mask, q, ws, B, H, W, y1, c, (hipStream_t)stream);
  ground_launch_finalise(ws, B, (int)cdivl((long)(y1 - y0) * W, PLANE_CHUNK), 0, GROUND_FIN_TERMS, 0, c, nullptr, nullptr, sums,
                         counts, (hipStream_t)stream);
  ATDN_API_END
}

int atdn_ground_terms_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                           double fx, double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z,
                           double max_depth, double* sums, int* counts) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q, B, H, W, y0, y1, fx, fy, cx, cy, scale_rel, inlier_rel, min_z, max_depth};
  ground_terms_host(depth, mask, q, B, H, W, y1, ground_terms_args(a, sums, counts, false, nullptr), sums, counts);
  ATDN_API_END
}

int atdn_ground_solve(const float* depth, const unsigned char* mask, const double* q_init, int B, int H, int W, int y0, int y1,
                      double fx, double fy, double cx, double cy, double nx, double ny, double nz, double scale_rel,
                      double inlier_rel, double min_z, double max_depth, int min_votes, int iters, double* q, double* sums,
                      int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q_init, B, H, W, y0, y1, fx, fy, cx, cy, scale_rel, inlier_rel, min_z, max_depth};
  const GroundParams c = ground_solve_args(a, nx, ny, nz, min_votes, iters, q, sums, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)q & 7) == 0,
             "workspace, q and sums must be 8-byte aligned");
  const GroundWorkspace ws = ground_carve(workspace, B, H, W);
  const hipStream_t st = (hipStream_t)stream;
  const int nb = (y1 - y0) * W;
  const int chunks = (int)cdivl(nb, PLANE_CHUNK);
  if (!q_init) {
    const int groups = chunks < GROUND_VOTE_GROUPS ? chunks : GROUND_VOTE_GROUPS;
    const dim3 grid((unsigned)groups, (unsigned)B);
    if (mask)
      hipLaunchKernelGGL(ground_vote_kernel<true>, grid, dim3(PQ_THREADS), 0, st, depth, mask, (long)H * W, nb, chunks, c, ws.hist);
    else
      hipLaunchKernelGGL(ground_vote_kernel<false>, grid, dim3(PQ_THREADS), 0, st, depth, mask, (long)H * W, nb, chunks, c, ws.hist);
    ATDN_HIP(hipGetLastError());
    ground_launch_finalise(ws, B, chunks, groups, GROUND_FIN_VOTE, iters, c, nullptr, nullptr, nullptr, nullptr, st);
  }
  for (int k = 0; k <= iters; ++k) {
    ground_launch_terms(depth, mask, k == 0 ? q_init : nullptr, ws, B, H, W, y1, c, st);
    ground_launch_finalise(ws, B, chunks, 0, k, iters, c, q_init, q, sums, counts, st);
  }
  ATDN_API_END
}

int atdn_ground_solve_host(const float* depth, const unsigned char* mask, const double* q_init, int B, int H, int W, int y0, int y1,
                           double fx, double fy, double cx, double cy, double nx, double ny, double nz, double scale_rel,
                           double inlier_rel, double min_z, double max_depth, int min_votes, int iters, double* q, double* sums,
                           int* counts) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q_init, B, H, W, y0, y1, fx, fy, cx, cy, scale_rel, inlier_rel, min_z, max_depth};
  const GroundParams c = ground_solve_args(a, nx, ny, nz, min_votes, iters, q, sums, counts, false, nullptr);
  ground_solve_host(depth, mask, q_init, B, H, W, y1, c, iters, q, sums, counts);
  ATDN_API_END
}

int atdn_ground_classify(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                         double fx, double fy, double cx, double cy, double inlier_rel, double min_z, double max_depth,
                         float* residual, unsigned char* on_ground, void* stream) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q, B, H, W, y0, y1, fx, fy, cx, cy, 1.0, inlier_rel, min_z, max_depth};
  const GroundParams c = ground_classify_args(a, residual, on_ground, true);
  const long n = (long)H * W;
  const dim3 grid(quad_blocks(n, false), (unsigned)B);
  if (mask)
    hipLaunchKernelGGL(ground_classify_kernel<true>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, depth, mask, q, (int)n, y1, c,
                       residual, on_ground);
  else
    hipLaunchKernelGGL(ground_classify_kernel<false>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, depth, mask, q, (int)n, y1, c,
                       residual, on_ground);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_ground_classify_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                              double fx, double fy, double cx, double cy, double inlier_rel, double min_z, double max_depth,
                              float* residual, unsigned char* on_ground) {
  ATDN_API_BEGIN
  const GroundCall a{depth, mask, q, B, H, W, y0, y1, fx, fy, cx, cy, 1.0, inlier_rel, min_z, max_depth};
  ground_classify_host(depth, mask, q, B, H, W, y1, ground_classify_args(a, residual, on_ground, false), residual, on_ground);
  ATDN_API_END
}
