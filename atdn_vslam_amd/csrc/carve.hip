// Visibility votes and carving on the device: per voxel of the map's cloud, how many keyframes have it in view, how many confirm
// it and how many see straight through it — and the removal of the voxels a caller decides against. The rule — float64, every
// operation rounded on its own — is carve_vote of carve_host.h, which the kernel calls, so the kernel and the host form evaluate
// one function. The votes are integer sums: they commute, so the result does not depend on thread order, on launch geometry or
// on how the keyframes are split over calls.
//
// Launches on the caller's stream, nothing else (no host synchronisation, no memset; capturable):
//   carve_clear_kernel    (accumulate == 0 only) a thread per int32 of votes: zeros
//   carve_votes_kernel    a workgroup owns 256 points and blockIdx.y a chunk of CARVE_CHUNK list positions. A lane keeps its
//                         point's three coordinates in registers as doubles; the keyframe index and the pose row of a list
//                         position are the same in every lane (read through a wave-uniform index: scalar loads), only the depth
//                         reads are per lane. A lane sums its point's votes over the chunk in registers and adds the non-zero
//                         ones to votes with int32 atomic adds (agent scope) whose results nobody reads. No thread waits for
//                         another; the loop bounds are CARVE_CHUNK and (2 radius + 1)^2 with radius <= 8.
//   remove_clear_kernel   three threads: removed = 0
//   voxel_remove_kernel   a thread per key: a read-only probe from the key's home slot (voxel_home, the limit of insertion; an
//                         empty slot ends it); where the key is found n is exchanged for 0 — a repeated key gets 0 the second time
//                         and counts as not found — and S and C are stored as zeros. The key word stays: no probe chain breaks.
//                         The three counters go through LDS: at most three global atomics per workgroup.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "carve_host.h"
#include "flow_args.h"

namespace atdn {

constexpr int CARVE_THREADS = 256;
constexpr int CARVE_CHUNK = 4;                                    // list positions per workgroup (tests/carve_ref.py: CHUNK)
typedef unsigned long long carve_u64;
static_assert(sizeof(carve_u64) == 8, "64-bit atomics");

__device__ inline void carve_add(int* p, int v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CARVE_THREADS) void carve_clear_kernel(int* __restrict__ votes, long count) {
  const long i = (long)blockIdx.x * CARVE_THREADS + threadIdx.x;
  if (i < count) votes[i] = 0;
}

__global__ __launch_bounds__(CARVE_THREADS) void carve_votes_kernel(const float* __restrict__ points, int M,
                                                                    const float* __restrict__ depth,
                                                                    const float* __restrict__ poses,
                                                                    const int* __restrict__ indices, int N, int K, CarveParams c,
                                                                    int* __restrict__ votes) {
  const int i = (int)(blockIdx.x * CARVE_THREADS + threadIdx.x);  // < M + 256 <= 2^31 (checked by the entry point)
  const int j0 = (int)blockIdx.y * CARVE_CHUNK;
  const long n = (long)c.H * c.W;
  const bool live = i < M;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  if (live) {
    p0 = (double)points[3L * i];
    p1 = (double)points[3L * i + 1];
    p2 = (double)points[3L * i + 2];
  }
  int view = 0, sup = 0, fre = 0;
#pragma unroll
  for (int jj = 0; jj < CARVE_CHUNK; ++jj) {
    const int j = j0 + jj;                                        // the same in every lane, as is everything read through it
    if (j >= K) break;
    const int kf = __builtin_amdgcn_readfirstlane(indices ? indices[j] : j);
    if (kf < 0 || kf >= N) continue;
    if (live) {
      const int v = carve_vote(p0, p1, p2, poses + 12L * kf, depth + (long)kf * n, c);
      view += v & 1;
      sup += (v >> 1) & 1;
      fre += (v >> 2) & 1;
    }
  }
  if (live) {
    if (view) carve_add(votes + 3L * i, view);
    if (sup) carve_add(votes + 3L * i + 1, sup);
    if (fre) carve_add(votes + 3L * i + 2, fre);
  }
}

__global__ void remove_clear_kernel(int64_t* __restrict__ removed) {
  if (threadIdx.x < 3) removed[threadIdx.x] = 0;
}

__global__ __launch_bounds__(CARVE_THREADS) void voxel_remove_kernel(uint64_t* __restrict__ table, uint32_t cap_mask,
                                                                     int probe_limit, const int64_t* __restrict__ keys,
                                                                     const unsigned char* __restrict__ flags, long R,
                                                                     int64_t* __restrict__ removed) {
  __shared__ carve_u64 blk[3];
  if (threadIdx.x < 3) blk[threadIdx.x] = 0;
  __syncthreads();
  const long r = (long)blockIdx.x * CARVE_THREADS + threadIdx.x;
  uint64_t* slots = table + VOX_HEADER_WORDS;
  if (r < R && (!flags || flags[r])) {
    const uint64_t key = (uint64_t)keys[r];
    uint32_t s = voxel_home(key, cap_mask);
    carve_u64 held = 0;
    for (int i = 0; i < probe_limit; ++i) {
      carve_u64* e = (carve_u64*)(slots + 8 * (long)s);
      const carve_u64 cur = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == (carve_u64)VOX_EMPTY) break;
      if (cur == (carve_u64)key) {
        held = __hip_atomic_exchange(e + 1, (carve_u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (held) {
#pragma unroll
          for (int k = 2; k < VOX_SLOT_WORDS; ++k) __hip_atomic_store(e + k, (carve_u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        break;
      }
      s = (s + 1) & cap_mask;
    }
    if (held) {
      atomicAdd(&blk[0], (carve_u64)1);
      atomicAdd(&blk[1], held);
    } else {
      atomicAdd(&blk[2], (carve_u64)1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && blk[threadIdx.x])
    (void)__hip_atomic_fetch_add((carve_u64*)(removed + threadIdx.x), blk[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- argument rules, shared by the two entry points of each pair below (indices and flags may be null)

static void carve_check_votes(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K,
                              int H, int W, double fx, double fy, double cx, double cy, double near, double far, double rel,
                              double abs_tol, int radius, int accumulate, const int* votes) {
  ATDN_CHECK(depth && poses, "null argument");
  ATDN_CHECK(M >= 0 && M <= (1 << 30), "M must be in [0, 2^30]");
  ATDN_CHECK(M == 0 || (points && votes), "null argument");
  ATDN_CHECK(N >= 1 && K >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
  ATDN_CHECK(indices || K <= N, "without indices K keyframes are read: K <= N");
  ATDN_CHECK(K <= 65535 * CARVE_CHUNK, "too many keyframes in one call");
  check_pinhole(fx, fy, cx, cy);
  ATDN_CHECK(near > 0.0 && near <= far && std::isfinite(far), "0 < near <= far, far finite");
  ATDN_CHECK(std::isfinite(rel) && rel >= 0.0 && std::isfinite(abs_tol) && abs_tol >= 0.0, "rel and abs must be finite and >= 0");
  ATDN_CHECK(radius >= 0 && radius <= CARVE_MAX_RADIUS, "radius must be in [0, 8]");
  ATDN_CHECK(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
  ATDN_CHECK(((uintptr_t)points & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)poses & 3) == 0 &&
                 ((uintptr_t)indices & 3) == 0 && ((uintptr_t)votes & 3) == 0,
             "points, depth, poses, indices and votes must be 4-byte aligned");
  if (M == 0) return;
  const void* in[4] = {points, depth, poses, indices};
  const long in_bytes[4] = {(long)M * 12, (long)N * H * W * 4, (long)N * 48, (long)K * 4};
  const void* out[1] = {votes};
  const long out_bytes[1] = {(long)M * 12};
  check_disjoint(in, in_bytes, 4, out, out_bytes, 1);
}

static void carve_check_remove(const void* table, long capacity, const int64_t* keys, const uint8_t* flags, long R,
                               const int64_t* removed) {
  ATDN_CHECK(table && removed, "null argument");
  ATDN_CHECK(capacity >= 2 && capacity <= VOX_MAX_CAPACITY && (capacity & (capacity - 1)) == 0,
             "capacity must be a power of two in [2, 2^31]");
  ATDN_CHECK(R >= 0 && R <= (1L << 31), "R must be in [0, 2^31]");
  ATDN_CHECK(R == 0 || keys, "null argument");
  ATDN_CHECK(((uintptr_t)table & 7) == 0 && ((uintptr_t)keys & 7) == 0 && ((uintptr_t)removed & 7) == 0,
             "the table, keys and removed must be 8-byte aligned");
  const void* in[2] = {R ? keys : nullptr, R ? flags : nullptr};
  const long in_bytes[2] = {R * 8, R};
  const void* out[2] = {table, removed};
  const long out_bytes[2] = {voxel_table_words(capacity) * 8, 24};
  check_disjoint(in, in_bytes, 2, out, out_bytes, 2);
}

}  // namespace atdn

using namespace atdn;

int atdn_voxel_votes(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K, int H,
                     int W, double fx, double fy, double cx, double cy, double near, double far, double rel, double abs, int radius,
                     int accumulate, int* votes, void* stream) {
  ATDN_API_BEGIN
  carve_check_votes(points, M, depth, poses, indices, N, K, H, W, fx, fy, cx, cy, near, far, rel, abs, radius, accumulate, votes);
  if (M > 0) {
    const CarveParams c = carve_params(fx, fy, cx, cy, near, far, rel, abs, radius, H, W);
    if (!accumulate) {
      hipLaunchKernelGGL(carve_clear_kernel, dim3((unsigned)cdivl(3L * M, CARVE_THREADS)), dim3(CARVE_THREADS), 0,
                         (hipStream_t)stream, votes, 3L * M);
      ATDN_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(carve_votes_kernel, dim3((unsigned)cdivl(M, CARVE_THREADS), (unsigned)cdivl(K, CARVE_CHUNK)),
                       dim3(CARVE_THREADS), 0, (hipStream_t)stream, points, M, depth, poses, indices, N, K, c, votes);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}

int atdn_voxel_votes_host(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K,
                          int H, int W, double fx, double fy, double cx, double cy, double near, double far, double rel, double abs,
                          int radius, int accumulate, int* votes) {
  ATDN_API_BEGIN
  carve_check_votes(points, M, depth, poses, indices, N, K, H, W, fx, fy, cx, cy, near, far, rel, abs, radius, accumulate, votes);
  carve_votes_host(points, M, depth, poses, indices, N, K, carve_params(fx, fy, cx, cy, near, far, rel, abs, radius, H, W), accumulate,
                   votes);
  ATDN_API_END
}

int atdn_voxel_remove(void* table, long capacity, const int64_t* keys, const uint8_t* flags, long R, int64_t* removed,
                      void* stream) {
  ATDN_API_BEGIN
  carve_check_remove(table, capacity, keys, flags, R, removed);
  hipLaunchKernelGGL(remove_clear_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, removed);
  ATDN_HIP(hipGetLastError());
  if (R > 0) {
    hipLaunchKernelGGL(voxel_remove_kernel, dim3((unsigned)cdivl(R, CARVE_THREADS)), dim3(CARVE_THREADS), 0, (hipStream_t)stream,
                       (uint64_t*)table, (uint32_t)(capacity - 1), (int)voxel_probe_limit(capacity), keys, flags, R, removed);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}

int atdn_voxel_remove_host(void* table, long capacity, const int64_t* keys, const uint8_t* flags, long R, int64_t* removed) {
  ATDN_API_BEGIN
  carve_check_remove(table, capacity, keys, flags, R, removed);
  voxel_remove_host((uint64_t*)table, capacity, keys, flags, R, removed);
  ATDN_API_END
}
