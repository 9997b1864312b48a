// Range probe (range_probe.h): one pass over a strided 2-D fp32 view that reduces it to the largest finite magnitude, the number
// of finite values beyond the split-f16 limit and the number of non-finite values. A pure read, bound by memory bandwidth.
//
// Shape. Every row is cut into [head | body | tail]: the body is the run of whole 16-byte groups that starts at the first
// 16-byte boundary of the row (the same cut for every row, because the pitch is a multiple of four floats whenever the body is
// used with more than one row), head and tail are the up to 3 + 3 values around it. A view without pitch padding is one long row.
// The body is read with 16-byte loads, four in flight per lane (a tile = 256 lanes x 4 loads = 16 KB); rows wider than a tile
// are cut into tiles, rows narrower than a tile share one (a power-of-two number of lane slots per row, so that a lane finds
// its row with a shift). Head and tail go through 4-byte loads in a second sweep, which is also the whole kernel for a view whose
// pitch rules 16-byte loads out. Everything is integer arithmetic on the bit patterns: |x| is the pattern without its sign,
// non-negative floats order like their patterns (denormals included, no flushing), "non-finite" is an all-ones exponent.
// Reduction: registers over the grid-stride loop, the wave by lane exchange, the block's four waves through LDS, then at most
// three atomics per block (a maximum and two 64-bit sums; the sums only when non-zero). Maxima and integer sums are exact and
// order-free: the result does not depend on the grid.
#include "range_probe.h"

#include <algorithm>
#include <cstdint>

namespace atdn {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int kTile = kThreads * kUnroll;       // lane slots of one tile (16-byte groups in the body sweep, values in the edge sweep)
constexpr int kMaxBlocks = 2048;                // 256 CUs x 8 resident blocks: a memory-bound grid is capped there and strides
constexpr unsigned kLimitBits = 0x477FE000u;    // 65504.0f, the largest finite f16
constexpr unsigned kInfBits = 0x7F800000u;

struct ProbeGeom {
  long rows, ld;
  // body sweep
  long nvec;       // 16-byte groups per row
  long head;       // values in front of the body
  long vtiles;     // tiles of the body sweep
  long tpr;        // wide rows (nvec >= kTile): tiles per row
  int lgv;         // narrow rows: log2 of the lane slots per row (>= nvec)
  int wide;
  // edge sweep: the `en` values of a row that the body leaves out; value e is column e (e < head) or e + 4 * nvec
  long en;
  long etiles;
  int lge;         // log2 of the lane slots per row (>= en)
};

// Lanes without work in a tile load from a valid address of the view (its first body group / first value) and discard the
// value: the loads carry no predicate, so all four of a lane are issued before the first is waited for. (With a branch around
// each load the compiler waits for every load inside its branch: one in flight per lane.)
__global__ __launch_bounds__(kThreads) void range_probe_kernel(const float* __restrict__ x, ProbeGeom g,
                                                               RangeSlot* __restrict__ slot) {
  unsigned mx = 0, over = 0, nonf = 0;   // (a lane sees < 2^32 values: the grid has 2,048 blocks wherever the view is large)
  auto take = [&](float v) {
    const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
    const bool nf = b >= kInfBits;
    nonf += nf ? 1u : 0u;
    over += (!nf && b > kLimitBits) ? 1u : 0u;
    mx = max(mx, nf ? 0u : b);
  };
  const int tid = threadIdx.x;

  // ---- body: 16-byte loads
  for (long t = blockIdx.x; t < g.vtiles; t += gridDim.x) {
    long o[kUnroll];    // offset of the lane's group, in floats
    bool ok[kUnroll];
    if (g.wide) {
      const long r = t / g.tpr;               // uniform: once per 16 KB
      const long c0 = (t - r * g.tpr) * kTile;
      const long row = r * g.ld + g.head;
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const long c = c0 + u * kThreads + tid;
        ok[u] = c < g.nvec;
        o[u] = ok[u] ? row + 4 * c : g.head;
      }
    } else {
      const long r0 = t << (10 - g.lgv);      // kTile >> lgv rows per tile
      const int mask = (1 << g.lgv) - 1;
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int j = u * kThreads + tid;
        const long r = r0 + (j >> g.lgv);
        const int c = j & mask;
        ok[u] = r < g.rows && c < g.nvec;
        o[u] = ok[u] ? r * g.ld + g.head + 4 * c : g.head;
      }
    }
    float4 v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = *reinterpret_cast<const float4*>(x + o[u]);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const float4 w = keep_if(ok[u], v[u]);
      take(w.x); take(w.y); take(w.z); take(w.w);
    }
  }

  // ---- edges (and views that cannot be read 16 bytes at a time): 4-byte loads
  const long emask = (1L << g.lge) - 1;
  for (long t = blockIdx.x; t < g.etiles; t += gridDim.x) {
    float v[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long i = t * kTile + u * kThreads + tid;
      const long r = i >> g.lge, e = i & emask;
      ok[u] = r < g.rows && e < g.en;
      const long c = e < g.head ? e : e + 4 * g.nvec;
      v[u] = x[ok[u] ? r * g.ld + c : 0];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) take(ok[u] ? v[u] : 0.f);
  }

  // ---- wave, block, device
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
    over += (unsigned)__shfl_xor((int)over, off);
    nonf += (unsigned)__shfl_xor((int)nonf, off);
  }
  __shared__ unsigned part[kThreads / 64][3];
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { part[wave][0] = mx; part[wave][1] = over; part[wave][2] = nonf; }
  __syncthreads();
  if (tid == 0) {
    unsigned bm = 0;
    unsigned long long bo = 0, bn = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { bm = max(bm, part[w][0]); bo += part[w][1]; bn += part[w][2]; }
    if (bm) atomicMax(&slot->max_bits, bm);
    if (bo) atomicAdd(&slot->over, bo);
    if (bn) atomicAdd(&slot->nonfinite, bn);
  }
}

int ceil_log2(long n) {
  int l = 0;
  while ((1L << l) < n) ++l;
  return l;
}

}  // namespace

void launch_range_probe(const float* x, long rows, long cols, long ld, RangeSlot* slot, hipStream_t st) {
  ATDN_CHECK(x && slot, "range probe: null pointer");
  ATDN_CHECK(rows >= 0 && cols >= 0 && (rows <= 1 || ld >= cols), "range probe: the row pitch must cover the row");
  ATDN_CHECK((reinterpret_cast<uintptr_t>(x) & 3) == 0, "range probe: the view must start on a 4-byte boundary");
  if (rows == 0 || cols == 0) return;
  if (rows > 1 && ld == cols) { cols *= rows; rows = 1; }   // no pitch padding: one long row
  if (rows == 1) ld = cols;
  ATDN_CHECK(rows < (1L << 40) && cols < (1L << 40), "range probe: view too large");
  ProbeGeom g{};
  g.rows = rows; g.ld = ld;
  const bool vec = rows == 1 || (ld & 3) == 0;   // else every row has another phase against the 16-byte grid
  if (vec) {
    const long a = (long)((reinterpret_cast<uintptr_t>(x) >> 2) & 3);   // floats past a 16-byte boundary
    g.head = std::min(cols, (4 - a) & 3);
    g.nvec = (cols - g.head) / 4;
  } else {
    g.head = cols;
    g.nvec = 0;
  }
  g.en = cols - 4 * g.nvec;
  g.wide = g.nvec >= kTile;
  if (g.wide) {
    g.tpr = cdivl(g.nvec, kTile);
    g.vtiles = rows * g.tpr;
  } else if (g.nvec > 0) {
    g.lgv = ceil_log2(g.nvec);                   // <= 10
    g.vtiles = cdivl(rows, kTile >> g.lgv);
  }
  g.lge = ceil_log2(std::max(g.en, 1L));
  ATDN_CHECK(ceil_log2(rows) + g.lge < 62, "range probe: view too large");
  g.etiles = g.en > 0 ? cdivl(rows << g.lge, kTile) : 0;
  const long blocks = std::min<long>(std::max(g.vtiles, g.etiles), kMaxBlocks);
  hipLaunchKernelGGL(range_probe_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, g, slot);
  ATDN_HIP(hipGetLastError());
}

}  // namespace atdn
