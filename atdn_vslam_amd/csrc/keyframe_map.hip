// Keyframe map kernels: the relocalisation map of NeuralSLAM kept in HBM (atdn_vslam_amd/keyframe_map.py).
//
// * atdn_map_search: L2 distance of Q query embeddings to every row of the embedding bank in one launch, then the topk
//   nearest rows per query — the per-keyframe `torch.norm(kf.embedding - mu, p=2)` loop, `torch.stack` and `argmin` of
//   slam_framework/neural_slam.py:374-383.
// * atdn_map_gather_images_u8: uint8 keyframe images of the image bank -> the fp32 [n,3,H,W] batch the VAE encoder and the
//   flow network read (`torch.load(rgb_file).to(device).float()`, neural_slam.py:386-390).
//
// The search is a streaming reduction with a FIXED summation order, so that dist[q][k] depends on the contents of row k and
// query q alone (not on Q, K, the row's slot, the other queries or how the launch was cut):
//   lane t of a 256-lane workgroup owns the 16-byte vectors t, t + 256, t + 512, ... of a row; it forms the difference first
//   and accumulates d * d with one fused multiply-add per element into ONE accumulator per (row, query), in element order;
//   after MS_SEG = 16 vectors (64 sequential FMAs) the accumulator is added to a running total and restarted (rows of up to
//   16,384 floats are one such partial sum); the 64 lanes of a wave are summed by a butterfly of 6 shuffle levels, the 4 waves
//   through LDS as (w0 + w1) + (w2 + w3); the square root is correctly rounded.
// Every term is non-negative, so the relative error of d^2 is at most (64 + 8 + ceil(D / 16384) - 1 + 1) * 2^-24 (the last
// one is the rounding of the difference, counted twice for the square); a row equal to the query gives exactly 0.
//
// A workgroup takes R bank rows and up to 16 queries: per 16-byte column position the lane loads its query vectors once and
// uses them for the R rows, so the bank is read once per launch and the queries R times less often than the rows ask for.
// R is chosen on the host from K alone so that a few hundred keyframes still make a workgroup per CU; it changes no bit.
#include "../../include/atdn_hip.h"

#include <algorithm>
#include <vector>

#include "common.h"

namespace atdn {

constexpr int MS_THREADS = 256;
constexpr int MS_SEG = 16;       // 16-byte vectors per lane and partial sum: 64 sequential FMAs
constexpr int MS_QMAX = 16;      // queries per launch

// the inner loop: 4 subtractions and 4 fused multiply-adds per 16 bytes of a row and query, in element order. Plain fp32: a
// build with v_pk_add_f32 / v_pk_fma_f32 (two accumulators per pair) was timed beside this one and was no faster at 1 to 8
// queries and 1.4x slower at 16 (the second accumulator set costs the occupancy): profiles/reloc_search_variants.txt.
__device__ __forceinline__ void ms_acc(float& a, const float4 r, const float4 q) {
  const float dx = r.x - q.x, dy = r.y - q.y, dz = r.z - q.z, dw = r.w - q.w;
  a = __builtin_fmaf(dx, dx, a);
  a = __builtin_fmaf(dy, dy, a);
  a = __builtin_fmaf(dz, dz, a);
  a = __builtin_fmaf(dw, dw, a);
}

template <int R, int QB>
__device__ __forceinline__ void ms_step(const float4* __restrict__ rows, const long (&roff)[R], const float4* __restrict__ qs, long n4,
                                        int i, float (&acc)[R][QB], const int (&qsel)[QB]) {
  // every load of the step is issued before the first use: R + QB 16-byte loads in flight per lane
  float4 rv[R], qv[QB];
#pragma unroll
  for (int r = 0; r < R; ++r) rv[r] = rows[roff[r] + i];
#pragma unroll
  for (int q = 0; q < QB; ++q) qv[q] = qs[(long)qsel[q] * n4 + i];
#pragma unroll
  for (int q = 0; q < QB; ++q)
#pragma unroll
    for (int r = 0; r < R; ++r) ms_acc(acc[r][q], rv[r], qv[q]);
}

// grid: ceil(K / R) workgroups; queries q0 .. q0 + nq - 1 (nq <= QB) of the [Q][D] array; dist [Q][K]
template <int R, int QB>
__global__ __launch_bounds__(MS_THREADS) void map_search_kernel(const float* __restrict__ bank, int K, int D,
                                                                const float* __restrict__ queries, int q0, int nq,
                                                                float* __restrict__ dist) {
  constexpr int UNR = (R * QB >= 16) ? 1 : 4;
  const long n4 = D >> 2;
  const int t = threadIdx.x;
  const int k0 = blockIdx.x * R;
  const float4* rows = reinterpret_cast<const float4*>(bank);
  const float4* qs = reinterpret_cast<const float4*>(queries) + (long)q0 * n4;
  long roff[R];
  int qsel[QB];
#pragma unroll
  for (int r = 0; r < R; ++r) roff[r] = (long)min(k0 + r, K - 1) * n4;   // (rows past the end: a duplicate, never stored)
#pragma unroll
  for (int q = 0; q < QB; ++q) qsel[q] = min(q, nq - 1);

  float tot[R][QB], acc[R][QB];
  const int nfull = (int)(n4 / MS_THREADS);                 // iterations in which every lane has a vector
  const int niter = (int)((n4 + MS_THREADS - 1) / MS_THREADS);
  for (int j0 = 0; j0 < niter; j0 += MS_SEG) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < QB; ++q) acc[r][q] = 0.0f;
    const int jend = min(j0 + MS_SEG, nfull);
#pragma unroll UNR
    for (int j = j0; j < jend; ++j) ms_step<R, QB>(rows, roff, qs, n4, j * MS_THREADS + t, acc, qsel);
    if (jend < min(j0 + MS_SEG, niter)) {                   // the one partial iteration of the row falls into this segment
      const int i = nfull * MS_THREADS + t;
      if (i < n4) ms_step<R, QB>(rows, roff, qs, n4, i, acc, qsel);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int q = 0; q < QB; ++q) tot[r][q] = (j0 == 0) ? acc[r][q] : tot[r][q] + acc[r][q];
  }

  __shared__ float red[MS_THREADS / 64][R * QB];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      float v = tot[r][q];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((t & 63) == 0) red[t >> 6][r * QB + q] = v;
    }
  __syncthreads();
  if (t < R * QB) {
    const int r = t / QB, q = t % QB;
    const float s = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    if (k0 + r < K && q < nq) dist[(long)(q0 + q) * K + k0 + r] = sqrtf(s);
  }
}

// one workgroup per query: the topk smallest of dist[q][0..K), ascending, equal values by the lower index. A key is
// (bits of the non-negative distance, index): unsigned order of the bits is the order of the values, a NaN sorts last.
// Pass n takes the smallest key above the one pass n - 1 chose. A lane reads 4 independent values per trip: with one
// dependent read per trip the 16,384 distances of a large map cost 26 us per pass in load latency alone.
constexpr int TK_THREADS = 1024;
__device__ __forceinline__ unsigned long long tk_key(float d, int i) {
  return ((unsigned long long)(__float_as_uint(d) & 0x7FFFFFFFu) << 32) | (unsigned)i;
}
__global__ __launch_bounds__(TK_THREADS) void map_topk_kernel(const float* __restrict__ dist, int K, int topk, int* __restrict__ idx) {
  const float* d = dist + (long)blockIdx.x * K;
  const int t = threadIdx.x;
  __shared__ unsigned long long red[TK_THREADS / 64];
  __shared__ unsigned long long chosen;
  unsigned long long prev = 0;
  for (int n = 0; n < topk; ++n) {
    unsigned long long best = ~0ull;
    for (int i0 = t; i0 < K; i0 += 4 * TK_THREADS) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = d[min(i0 + u * TK_THREADS, K - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TK_THREADS;
        const unsigned long long key = tk_key(v[u], i);
        if (i < K && (n == 0 || key > prev) && key < best) best = key;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o < best ? o : best;
    }
    if ((t & 63) == 0) red[t >> 6] = best;
    __syncthreads();
    if (t == 0) {
      unsigned long long m = red[0];
#pragma unroll
      for (int w = 1; w < TK_THREADS / 64; ++w) m = red[w] < m ? red[w] : m;
      idx[(long)blockIdx.x * topk + n] = (int)(unsigned)(m & 0xFFFFFFFFull);
      chosen = m;
    }
    __syncthreads();
    prev = chosen;
    __syncthreads();
  }
}

// one launch covers up to MAP_GATHER_MAX output images; the table of bank slots travels by value in the kernel arguments
constexpr int MAP_GATHER_MAX = 512;
struct MapGatherTable {
  int slot[MAP_GATHER_MAX];
};

__device__ __forceinline__ float4 u8x4_to_f32(unsigned w) {
  return make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24));
}

__global__ __launch_bounds__(256) void map_gather_u8_kernel(const uint8_t* __restrict__ bank, long plane_bytes, const MapGatherTable tab,
                                                            float* __restrict__ out) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;   // 16-byte vector within the image
  if (v * 16 >= plane_bytes) return;
  const uint4 p = *reinterpret_cast<const uint4*>(bank + (long)tab.slot[blockIdx.y] * plane_bytes + v * 16);
  float4* o = reinterpret_cast<float4*>(out + (long)blockIdx.y * plane_bytes + v * 16);
  o[0] = u8x4_to_f32(p.x);
  o[1] = u8x4_to_f32(p.y);
  o[2] = u8x4_to_f32(p.z);
  o[3] = u8x4_to_f32(p.w);
}

template <int R>
static void launch_search(int QB, dim3 grid, hipStream_t st, const float* bank, int K, int D, const float* queries, int q0, int nq,
                          float* dist) {
  switch (QB) {
    case 1: hipLaunchKernelGGL((map_search_kernel<R, 1>), grid, dim3(MS_THREADS), 0, st, bank, K, D, queries, q0, nq, dist); break;
    case 2: hipLaunchKernelGGL((map_search_kernel<R, 2>), grid, dim3(MS_THREADS), 0, st, bank, K, D, queries, q0, nq, dist); break;
    case 4: hipLaunchKernelGGL((map_search_kernel<R, 4>), grid, dim3(MS_THREADS), 0, st, bank, K, D, queries, q0, nq, dist); break;
    case 8: hipLaunchKernelGGL((map_search_kernel<R, 8>), grid, dim3(MS_THREADS), 0, st, bank, K, D, queries, q0, nq, dist); break;
    default: hipLaunchKernelGGL((map_search_kernel<R, 16>), grid, dim3(MS_THREADS), 0, st, bank, K, D, queries, q0, nq, dist); break;
  }
}

}  // namespace atdn

using namespace atdn;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int atdn_map_search(const float* bank, int K, int D, const float* queries, int Q, int topk, float* dist, int* idx, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(K >= 1, "the map holds no keyframe");
  ATDN_CHECK(Q >= 1, "no query");
  ATDN_CHECK(D >= 4 && D % 4 == 0, "the embedding length must be a multiple of 4 (16-byte vectors)");
  ATDN_CHECK(topk >= 1 && topk <= K && topk <= 16, "topk must be in [1, min(K, 16)]");
  ATDN_CHECK(bank && queries && dist && idx, "null pointer");
  ATDN_CHECK(aligned16(bank) && aligned16(queries), "bank and queries must be 16-byte aligned");
  ATDN_CHECK(((uintptr_t)dist & 3) == 0 && ((uintptr_t)idx & 3) == 0, "dist and idx must be 4-byte aligned");
  // rows per workgroup from K alone: a workgroup per CU (256) and more before the queries are shared between rows
  const int R = K >= 2048 ? 4 : K >= 512 ? 2 : 1;
  const dim3 grid((unsigned)cdiv(K, R));
  hipStream_t st = (hipStream_t)stream;
  for (int q0 = 0; q0 < Q; q0 += MS_QMAX) {
    const int nq = std::min(MS_QMAX, Q - q0);
    int QB = 1;
    while (QB < nq) QB <<= 1;
    if (R == 4) launch_search<4>(QB, grid, st, bank, K, D, queries, q0, nq, dist);
    else if (R == 2) launch_search<2>(QB, grid, st, bank, K, D, queries, q0, nq, dist);
    else launch_search<1>(QB, grid, st, bank, K, D, queries, q0, nq, dist);
    ATDN_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(map_topk_kernel, dim3((unsigned)Q), dim3(TK_THREADS), 0, st, dist, K, topk, idx);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_map_gather_images_u8(const uint8_t* bank, int K, long plane_bytes, const int* index_host, int n, float* out, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(bank && index_host && out, "null pointer");
  ATDN_CHECK(K >= 1 && n >= 1, "bad argument");
  ATDN_CHECK(plane_bytes >= 16 && plane_bytes % 16 == 0, "the image size in bytes must be a multiple of 16");
  ATDN_CHECK(aligned16(bank) && aligned16(out), "bank and output must be 16-byte aligned");
  // every index is checked on the host before anything is launched: no slot outside the bank can reach the device
  for (int j = 0; j < n; ++j) {
    if (index_host[j] < 0 || index_host[j] >= K) {
      char msg[160];
      snprintf(msg, sizeof msg, "image %d: keyframe index %d outside [0, %d)", j, index_host[j], K);
      throw Error(msg);
    }
  }
  const unsigned gx = (unsigned)cdivl(plane_bytes / 16, 256);
  for (int j0 = 0; j0 < n; j0 += MAP_GATHER_MAX) {
    const int nj = std::min(MAP_GATHER_MAX, n - j0);
    MapGatherTable tab;
    for (int j = 0; j < MAP_GATHER_MAX; ++j) tab.slot[j] = j < nj ? index_host[j0 + j] : 0;
    hipLaunchKernelGGL(map_gather_u8_kernel, dim3(gx, (unsigned)nj), dim3(256), 0, (hipStream_t)stream, bank, plane_bytes, tab,
                       out + (long)j0 * plane_bytes);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}
