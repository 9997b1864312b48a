// The frame of the per-pixel rule kernels (flow_consistency.hip, two_view.hip, flow_track.hip): a launch of (workgroups, B)
// workgroups of PQ_THREADS walks the planes [B, H * W] of its buffers, plane blockIdx.y, four consecutive flat indices per thread.
//
// The quads are cut on an ADDRESS offset, not on the index: with off = (address of the kernel's anchor plane) & 3 — or 0 — quad q
// holds the indices 4q - off .. 4q - off + 3 of the plane, so that a byte plane chosen as the anchor is one aligned dword per
// quad whatever H * W and the plane base of b >= 1 are. Every access of a quad is a vector access (float4, or a dword of four
// bytes) only where the quad is whole and its own address is aligned — the same answer for every quad of a plane, since a quad
// advances every address by a multiple of its vector size —; the ragged quads at the head and the tail of a plane, and a plane
// that is off its grid, take scalar accesses of the indices inside [lo, hi) only. A thread touches no index outside its quad.
//
// The pixel (x, y) of index lo is (lo % W, lo / W), and a quad may cross the end of a row; the kernels walk it with
//   int y = q.lo / W, x = q.lo - y * W;   ...   if (++x == W) { x = 0; ++y; }      (after every index inside the plane)
//
// Everything works on arrays of four with unrolled constant indices, so that they stay in registers (see keep_if in common.h).
#pragma once
#include <cstdint>

#include "common.h"

namespace atdn {

constexpr int PQ_THREADS = 256;   // four waves
constexpr int PQ_WAVES = PQ_THREADS / 64;

// Workgroups along x for planes of n indices. `anchored`: the kernel cuts its quads on an address, and off <= 3 moves the last
// index into one more quad at most.
inline unsigned quad_blocks(long n, bool anchored) { return (unsigned)cdivl(cdivl(n, 4) + (anchored ? 1 : 0), PQ_THREADS); }

struct Quad {
  int s0;       // first index of the quad: -3 .. n + 4 * PQ_THREADS (n <= 2^24)
  int lo, hi;   // the indices of the quad inside the plane: [lo, hi), empty past the end of the plane
  bool full;    // all four
  __device__ __forceinline__ bool has(int k) const { return s0 + k >= lo && s0 + k < hi; }
};

// the quad of this thread in workgroup `block` of the plane (a kernel whose workgroups walk several: ground.hip's vote)
__device__ __forceinline__ Quad quad_at(int n, int off, unsigned block) {
  Quad q;
  q.s0 = 4 * (int)(block * PQ_THREADS + threadIdx.x) - off;
  q.lo = q.s0 > 0 ? q.s0 : 0;
  q.hi = q.s0 + 4 < n ? q.s0 + 4 : n;
  q.full = q.hi - q.lo == 4;
  return q;
}

__device__ __forceinline__ Quad quad_of(int n, int off) { return quad_at(n, off, blockIdx.x); }

// v = p[s0 .. s0 + 3]; outside [lo, hi) zeros, and nothing is read there
__device__ __forceinline__ void quad_load(const Quad& q, const float* p, float v[4]) {
  if (q.full && ((uintptr_t)(p + q.s0) & 15) == 0) {
    const float4 a = *reinterpret_cast<const float4*>(p + q.s0);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q.has(k) ? p[q.s0 + k] : 0.0f;
  }
}

__device__ __forceinline__ void quad_store(const Quad& q, float* p, const float v[4]) {
  if (q.full && ((uintptr_t)(p + q.s0) & 15) == 0) {
    *reinterpret_cast<float4*>(p + q.s0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (q.has(k)) p[q.s0 + k] = v[k];
  }
}

// v = (p[s0 .. s0 + 3] != 0); outside [lo, hi) false, and nothing is read there
__device__ __forceinline__ void quad_load(const Quad& q, const unsigned char* p, bool v[4]) {
  if (q.full && ((uintptr_t)(p + q.s0) & 3) == 0) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p + q.s0);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ((w >> (8 * k)) & 0xFFu) != 0;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q.has(k) ? p[q.s0 + k] != 0 : false;
  }
}

// p[s0 + k] = 1 where flags[k] has `bit`, 0 elsewhere
__device__ __forceinline__ void quad_store(const Quad& q, unsigned char* p, const int flags[4], int bit) {
  if (q.full && ((uintptr_t)(p + q.s0) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p + q.s0) = (uint32_t)((flags[0] & bit) != 0) | ((uint32_t)((flags[1] & bit) != 0) << 8) |
                                             ((uint32_t)((flags[2] & bit) != 0) << 16) | ((uint32_t)((flags[3] & bit) != 0) << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (q.has(k)) p[q.s0 + k] = (flags[k] & bit) ? 1 : 0;
  }
}

// p[s0 + k] = the low byte of v[k] (0 .. 255)
__device__ __forceinline__ void quad_store_bytes(const Quad& q, unsigned char* p, const int v[4]) {
  if (q.full && ((uintptr_t)(p + q.s0) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(p + q.s0) = ((uint32_t)v[0] & 0xFFu) | (((uint32_t)v[1] & 0xFFu) << 8) |
                                             (((uint32_t)v[2] & 0xFFu) << 16) | (((uint32_t)v[3] & 0xFFu) << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (q.has(k)) p[q.s0 + k] = (unsigned char)v[k];
  }
}

// counts[j] += the number of pixels of the workgroup whose flags have bits[j], j < NC. Integer sums — ballot / popcount per wave
// (every lane gets the wave's sums; lane 0 hands them to LDS), the waves of the workgroup through LDS, one integer atomic add per
// workgroup and counter, none for a zero —, so the result does not depend on the order of arrival. Every thread of the workgroup
// calls it, once, with zero flags where it has no pixel.
template <int NC>
__device__ __forceinline__ void quad_count(const int flags[4], const int* bits, int* counts) {
  __shared__ int partial[NC][PQ_WAVES];
  int sum[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    sum[j] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[j] += __popcll(__ballot(flags[k] & bits[j]));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NC; ++j) partial[j][threadIdx.x >> 6] = sum[j];
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < PQ_WAVES; ++w) total += partial[threadIdx.x][w];
    if (total) atomicAdd(counts + threadIdx.x, total);
  }
}

}  // namespace atdn
