// Map view on the device: a point cloud rendered into B cameras with a z-buffer — the inverse of the voxel map's integration and
// the library's second scatter primitive. The rule — float64, every operation rounded on its own — is view_point, view_word and
// view_resolve of map_view_host.h, which these kernels call, so the kernels and the host form evaluate one set of functions. The
// combining operation is an unsigned 64-bit min: it commutes, so the images do not depend on thread order or launch geometry.
//
// Launches on the caller's stream, nothing else (no host synchronisation, no memset; capturable):
//   view_clear_kernel    a thread per word of the workspace (all ones) and per counter (0)
//   view_splat_kernel    blockIdx.y is the camera, a lane projects one point (the pose is wave-uniform). The visible lanes are
//                        balloted; for each of them, in lane order, its box and word are read by lane and the wave's 64 lanes
//                        cover the box as runs of consecutive pixels along x: a run is `pitch` = the box's width rounded up to a
//                        power of two (at most 64) lanes, 64 / pitch rows per step — contiguous 8-byte words, whole lines per
//                        wave instruction. A lane reads its pixel's word with a plain load and issues the atomic min (agent
//                        scope, its result unused) only where the new word is smaller: words only ever decrease, so a stale
//                        read costs an atomic and never correctness. No lock and no retry; the trip counts are bounded by
//                        64 visible lanes, H and W. The two counters go through LDS: two global atomics per workgroup
//                        (per-wave atomics on one address serialise behind each other), issued before the splat, so the
//                        workgroup's only barriers come before any footprint and no wave is held behind a long one.
//   view_resolve_kernel  blockIdx.y is the camera, a workgroup owns `iters` (an argument) runs of 256 pixels, a thread a pixel of
//                        each: word -> depth, support, colours; covered pixels counted through LDS, one atomic per workgroup.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "map_view_host.h"

namespace atdn {

constexpr int VIEW_THREADS = 256;
constexpr int VIEW_RESOLVE_ITERS = 8;                              // 2048 pixels per workgroup: one counter atomic for them all
typedef unsigned long long view_u64;
static_assert(sizeof(view_u64) == 8, "64-bit atomics");

__device__ inline void view_count(int64_t* p, int v) {
  (void)__hip_atomic_fetch_add((view_u64*)p, (view_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void view_min(uint64_t* p, uint64_t word) {
  view_u64* q = (view_u64*)p;
  if ((view_u64)word < __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    (void)__hip_atomic_fetch_min(q, (view_u64)word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(VIEW_THREADS) void view_clear_kernel(uint64_t* __restrict__ ws, long words,
                                                                  int64_t* __restrict__ counts_out, int counters) {
  const long i = (long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (i < words) ws[i] = VIEW_EMPTY;
  else if (i < words + counters) counts_out[i - words] = 0;
}

__global__ __launch_bounds__(VIEW_THREADS) void view_splat_kernel(const float* __restrict__ points,
                                                                  const unsigned char* __restrict__ colors,
                                                                  const int* __restrict__ counts, int M,
                                                                  const float* __restrict__ poses, ViewParams c,
                                                                  uint64_t* __restrict__ ws, int64_t* __restrict__ counts_out) {
  __shared__ unsigned blk[2];
  if (threadIdx.x < 2) blk[threadIdx.x] = 0;
  __syncthreads();
  const int b = (int)blockIdx.y;
  const int i = (int)(blockIdx.x * VIEW_THREADS + threadIdx.x);   // < M + 256 <= 2^31 (checked by the entry point)
  const int lane = (int)(threadIdx.x & 63);
  uint64_t* plane = ws + (long)b * c.H * c.W;
  bool cand = false, vis = false;
  int box[4] = {0, 0, 0, 0};
  uint64_t word = 0;
  if (i < M) {
    const int n = counts[i];
    cand = n >= c.min_count;
    if (cand) {
      uint32_t zbits;
      vis = view_point(points + 3L * i, poses + 12L * b, c, box, &zbits);
      if (vis) word = view_word(zbits, n, colors ? colors + 3L * i : nullptr);
    }
  }
  const view_u64 cm = __ballot(cand);
  view_u64 todo = __ballot(vis);
  if (lane == 0) {
    if (cm) atomicAdd(&blk[0], (unsigned)__popcll(cm));
    if (todo) atomicAdd(&blk[1], (unsigned)__popcll(todo));
  }
  __syncthreads();                                                // before the splat: no wave is held back behind a long one
  if (threadIdx.x < 2 && blk[threadIdx.x]) view_count(counts_out + 3L * b + threadIdx.x, (int)blk[threadIdx.x]);
  for (int round = 0; round < 64; ++round) {
    if (!todo) break;                                             // the same in every lane
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int x0 = __builtin_amdgcn_readlane(box[0], L), x1 = __builtin_amdgcn_readlane(box[1], L);
    const int y0 = __builtin_amdgcn_readlane(box[2], L), y1 = __builtin_amdgcn_readlane(box[3], L);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, L);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(word >> 32), L);
    const uint64_t wl = ((uint64_t)hi << 32) | lo;
    const int w = x1 - x0 + 1;
    int sh = 0;                                                   // pitch = 2^sh >= min(w, 64)
    while (sh < 6 && (1 << sh) < w) ++sh;
    const int rx = lane & ((1 << sh) - 1), ry = lane >> sh, rows = 64 >> sh;
    for (int y = y0 + ry; y <= y1; y += rows)
      for (int x = x0 + rx; x <= x1; x += 64) view_min(plane + (long)y * c.W + x, wl);
  }
}

__global__ __launch_bounds__(VIEW_THREADS) void view_resolve_kernel(const uint64_t* __restrict__ ws, int H, int W, int iters,
                                                                    float* __restrict__ depth,
                                                                    unsigned char* __restrict__ colors_out,
                                                                    unsigned char* __restrict__ support,
                                                                    int64_t* __restrict__ counts_out) {
  __shared__ unsigned blk;
  if (threadIdx.x == 0) blk = 0;
  __syncthreads();
  const int b = (int)blockIdx.y;
  const long n = (long)H * W;
  unsigned mine = 0;
  for (int it = 0; it < iters; ++it) {
    const long i = ((long)blockIdx.x * iters + it) * VIEW_THREADS + threadIdx.x;
    if (i < n) {
      uint32_t bits;
      unsigned char s, rgb[3];
      mine += view_resolve(ws[(long)b * n + i], &bits, &s, rgb);
      depth[(long)b * n + i] = __uint_as_float(bits);
      support[(long)b * n + i] = s;
      if (colors_out) {
#pragma unroll
        for (int a = 0; a < 3; ++a) colors_out[((long)b * 3 + a) * n + i] = rgb[a];
      }
    }
  }
  if (mine) atomicAdd(&blk, mine);
  __syncthreads();
  if (threadIdx.x == 0 && blk) view_count(counts_out + 3L * b + 2, (int)blk);
}

// ---- argument rules, shared by the device entry point and its host twin (colors and colors_out may be null; workspace is null
// for the host form)

static bool view_size_ok(int B, int H, int W) {
  return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && (long)B * H * W < (1L << 31);
}

static void view_check(const float* points, const uint8_t* colors, const int* counts, int M, const float* poses, int B, int H, int W,
                       double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near, double far,
                       int min_count, const float* depth, const uint8_t* colors_out, const uint8_t* support, const int64_t* counts_out,
                       const void* workspace, bool device) {
  ATDN_CHECK(poses && depth && support && counts_out, "null argument");
  ATDN_CHECK(M >= 0 && M <= (1 << 30), "M must be in [0, 2^30]");
  ATDN_CHECK(M == 0 || (points && counts), "null argument");
  ATDN_CHECK(view_size_ok(B, H, W), "bad batch or image size (B <= 65535, B * H * W < 2^31)");
  check_pinhole(fx, fy, cx, cy);
  ATDN_CHECK(std::isfinite(size) && size > 0.0, "size must be finite and > 0");
  ATDN_CHECK(std::isfinite(splat) && splat > 0.0, "splat must be finite and > 0");
  ATDN_CHECK(max_splat >= 1, "max_splat must be >= 1");
  ATDN_CHECK(near > 0.0 && near <= far && std::isfinite(far) && (double)(float)far == far,
             "0 < near <= far, far finite and representable in fp32");
  ATDN_CHECK(min_count >= 1, "min_count must be >= 1");
  ATDN_CHECK(((uintptr_t)points & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)poses & 3) == 0 && ((uintptr_t)depth & 3) == 0,
             "points, counts, poses and depth must be 4-byte aligned");
  ATDN_CHECK(((uintptr_t)counts_out & 7) == 0, "counts_out must be 8-byte aligned");
  if (device) {
    ATDN_CHECK(workspace, "null argument");
    ATDN_CHECK(((uintptr_t)workspace & 7) == 0, "the workspace must be 8-byte aligned");
  }
  const long n = (long)B * H * W;
  const void* in[4] = {M ? points : nullptr, M ? colors : nullptr, M ? counts : nullptr, poses};
  const long in_bytes[4] = {(long)M * 12, (long)M * 3, (long)M * 4, (long)B * 48};
  const void* out[5] = {depth, support, counts_out, nullptr, nullptr};
  long out_bytes[5] = {n * 4, n, (long)B * 24, 0, 0};
  int n_out = 3;
  if (colors_out) {
    out[n_out] = colors_out;
    out_bytes[n_out++] = 3 * n;
  }
  if (device) {
    out[n_out] = workspace;
    out_bytes[n_out++] = 8 * n;
  }
  check_disjoint(in, in_bytes, 4, out, out_bytes, n_out);
}

}  // namespace atdn

using namespace atdn;

long atdn_view_workspace_bytes(int B, int H, int W) { return view_size_ok(B, H, W) ? 8L * B * H * W : 0; }

int atdn_view_render(const float* points, const uint8_t* colors, const int* counts, int M, const float* poses, int B, int H, int W,
                     double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near, double far,
                     int min_count, float* depth, uint8_t* colors_out, uint8_t* support, int64_t* counts_out, void* workspace,
                     void* stream) {
  ATDN_API_BEGIN
  view_check(points, colors, counts, M, poses, B, H, W, fx, fy, cx, cy, size, splat, max_splat, near, far, min_count, depth, colors_out,
             support, counts_out, workspace, true);
  const long words = (long)B * H * W;
  const ViewParams c = view_params(fx, fy, cx, cy, size, splat, max_splat, near, far, min_count, H, W);
  hipLaunchKernelGGL(view_clear_kernel, dim3((unsigned)cdivl(words + 3L * B, VIEW_THREADS)), dim3(VIEW_THREADS), 0, (hipStream_t)stream,
                     (uint64_t*)workspace, words, counts_out, 3 * B);
  ATDN_HIP(hipGetLastError());
  hipLaunchKernelGGL(view_splat_kernel, dim3((unsigned)cdivl(M > 0 ? M : 1, VIEW_THREADS), (unsigned)B), dim3(VIEW_THREADS), 0,
                     (hipStream_t)stream, points, colors, counts, M, poses, c, (uint64_t*)workspace, counts_out);
  ATDN_HIP(hipGetLastError());
  hipLaunchKernelGGL(view_resolve_kernel, dim3((unsigned)cdivl((long)H * W, VIEW_THREADS * VIEW_RESOLVE_ITERS), (unsigned)B),
                     dim3(VIEW_THREADS), 0, (hipStream_t)stream, (const uint64_t*)workspace, H, W, VIEW_RESOLVE_ITERS, depth, colors_out,
                     support, counts_out);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_view_render_host(const float* points, const uint8_t* colors, const int* counts, int M, const float* poses, int B, int H,
                          int W, double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near,
                          double far, int min_count, float* depth, uint8_t* colors_out, uint8_t* support, int64_t* counts_out) {
  ATDN_API_BEGIN
  view_check(points, colors, counts, M, poses, B, H, W, fx, fy, cx, cy, size, splat, max_splat, near, far, min_count, depth, colors_out,
             support, counts_out, nullptr, false);
  view_render_host(points, colors, counts, M, poses, B, view_params(fx, fy, cx, cy, size, splat, max_splat, near, far, min_count, H, W),
                   depth, colors_out, support, counts_out);
  ATDN_API_END
}
