// Voxel map on the device: a voxel-hashed accumulation of every keyframe's depth (and colour) into one point cloud — the
// library's scatter primitive. The rule — integers and float64, every operation rounded on its own — is voxel_point, voxel_home
// and voxel_emit of voxel_map_host.h, which these kernels call, so the kernels and the host form evaluate one set of functions.
// Every sum is an integer sum: the table's CONTENT (the set of keys and each key's sums) does not depend on thread order, launch
// geometry or how the keyframes are split over calls; only the slot a key lives in does, and the extraction is ordered by key
// by the caller. The table's layout is in voxel_map_host.h and include/atdn_hip.h.
//
// Launches on the caller's stream, nothing else (no host synchronisation; capturable):
//   voxel_clear_kernel      a thread per 64-bit word of the table
//   voxel_integrate_kernel  at most VOX_GRID workgroups of 256 threads; workgroup b owns the flat pixel indices
//                           256 (b + i gridDim.x) .. + 255 of [K,H,W] for i < iters (an argument): a wave reads 64 consecutive
//                           pixels of a row (4 bytes of depth, a mask byte, three colour bytes each). Equal keys are combined
//                           inside the wave before memory is touched (below); then the leaders, in parallel, find their slot —
//                           a plain read, a 64-bit compare-and-swap where the slot is empty, the next slot otherwise, at most
//                           `probe_limit` slots — and add n, S and C with 64-bit integer atomics whose results nobody reads. A
//                           failed compare-and-swap is never tried again: the slot's owner is permanent, the probe moves on.
//                           The five counters go through LDS: at most five global atomics per workgroup.
//   voxel_rehash_kernel     a thread per slot of the source table: the same find, the seven sums added
//   voxel_extract_kernel    a thread per slot: the wave's qualifying slots take consecutive output places from one returning
//                           atomic per wave on a scratch word of the header; places >= max_out are counted and not written.
//                           The workgroup that draws the last ticket (a second scratch word) writes `found` and zeroes both
// Wave aggregation: neighbouring pixels of a keyframe fall into the same voxel most of the time. Per 64 pixels: the lowest lane
// still to do is the leader, its key is read by lane, the lanes with that key are balloted, their q and colour bytes summed by a
// butterfly (five 32-bit values: 64 * 65536 and 64 * 255 fit), the leader keeps the sums, the lanes remember their leader. At
// most 64 rounds, none touches memory. Lanes learn whether their point was dropped from a ballot of the failed leaders.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "voxel_map_host.h"

namespace atdn {

constexpr int VOX_THREADS = 256;
constexpr long VOX_GRID = 2048;
typedef unsigned long long vox_u64;
static_assert(sizeof(vox_u64) == 8, "64-bit atomics");

__device__ inline void vox_add(uint64_t* p, uint64_t v) {
  (void)__hip_atomic_fetch_add((vox_u64*)p, (vox_u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the slot of `key` in `slots` (claimed when new: *fresh), or -1 after `limit` slots
__device__ inline long vox_find(uint64_t* slots, uint32_t cap_mask, int limit, uint64_t key, bool* fresh) {
  uint32_t s = voxel_home(key, cap_mask);
  *fresh = false;
  for (int i = 0; i < limit; ++i) {
    vox_u64* kp = (vox_u64*)(slots + 8 * (long)s);
    vox_u64 cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == VOX_EMPTY) {
      cur = atomicCAS(kp, (vox_u64)VOX_EMPTY, (vox_u64)key);
      if (cur == VOX_EMPTY) {
        *fresh = true;
        return (long)s;
      }
    }
    if (cur == key) return (long)s;
    s = (s + 1) & cap_mask;
  }
  return -1;
}

__device__ inline unsigned vox_wave_sum(unsigned v) {
#pragma unroll
  for (int s = 1; s < 64; s *= 2) v += (unsigned)__shfl_xor((int)v, s, 64);
  return v;
}

__global__ __launch_bounds__(VOX_THREADS) void voxel_clear_kernel(uint64_t* __restrict__ table, long words) {
  const long w = (long)blockIdx.x * VOX_THREADS + threadIdx.x;
  if (w < words) table[w] = (w >= VOX_HEADER_WORDS && ((w - VOX_HEADER_WORDS) & 7) == 0) ? VOX_EMPTY : 0;
}

__global__ __launch_bounds__(VOX_THREADS) void voxel_integrate_kernel(
    const float* __restrict__ depth, const float* __restrict__ poses, const unsigned char* __restrict__ images,
    const unsigned char* __restrict__ mask, const int* __restrict__ indices, int N, long total, int H, int W, int iters,
    VoxelParams c, int retry, uint64_t* __restrict__ table, uint32_t cap_mask, int probe_limit,
    unsigned char* __restrict__ pending) {
  __shared__ unsigned blk[5];
  if (threadIdx.x < 5) blk[threadIdx.x] = 0;
  __syncthreads();
  const long n = (long)H * W;
  const int lane = (int)(threadIdx.x & 63);
  uint64_t* slots = table + VOX_HEADER_WORDS;
  unsigned cand = 0, ins = 0, outs = 0, drop = 0, fresh_n = 0;
  for (int it = 0; it < iters; ++it) {
    const long p = ((long)it * gridDim.x + blockIdx.x) * VOX_THREADS + threadIdx.x;
    const bool in_range = p < total;
    bool valid = false;
    uint64_t key = 0;
    unsigned q[3] = {0, 0, 0}, crg = 0, cb = 0;
    if (in_range) {
      const int j = (int)(p / n);
      const long r = p - (long)j * n;
      const int y = (int)(r / W), x = (int)(r - (long)y * W);
      const int kf = indices ? indices[j] : j;
      if (kf >= 0 && kf < N && x % c.stride == 0 && y % c.stride == 0 && (!mask || mask[p])) {
        const int st = voxel_point(depth[(long)kf * n + r], poses + 12L * kf, x, y, c, &key, q);
        cand += st != VOX_PIXEL_SKIP;
        outs += st == VOX_PIXEL_OUTSIDE;
        valid = st == VOX_PIXEL_INSIDE;
        if (valid && images) {
          const unsigned char* im = images + (long)kf * 3 * n + r;
          crg = (unsigned)im[0] | ((unsigned)im[n] << 16);
          cb = (unsigned)im[2 * n];
        }
      }
    }
    // equal keys of the wave combine; no memory is touched and the trip count is at most 64
    vox_u64 todo = __ballot(valid);
    int my_leader = 0;
    unsigned an = 0, a0 = 0, a1 = 0, a2 = 0, arg = 0, ab = 0;
    for (int round = 0; round < 64; ++round) {
      if (!todo) break;                                           // the same in every lane
      const int L = __ffsll((long long)todo) - 1;
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, L);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), L);
      const uint64_t kl = ((uint64_t)hi << 32) | lo;
      const bool m = valid && key == kl;
      const vox_u64 mm = __ballot(m);
      const unsigned s0 = vox_wave_sum(m ? q[0] : 0u), s1 = vox_wave_sum(m ? q[1] : 0u), s2 = vox_wave_sum(m ? q[2] : 0u);
      unsigned srg = 0, sb = 0;
      if (images) {                                               // an argument: the same in every lane
        srg = vox_wave_sum(m ? crg : 0u);
        sb = vox_wave_sum(m ? cb : 0u);
      }
      if (lane == L) {
        an = (unsigned)__popcll(mm);
        a0 = s0; a1 = s1; a2 = s2; arg = srg; ab = sb;
      }
      if (m) my_leader = L;
      todo &= ~mm;
    }
    // the leaders, in parallel
    bool failed = false;
    if (an) {
      bool fresh;
      const long s = vox_find(slots, cap_mask, probe_limit, key, &fresh);
      if (s < 0) {
        failed = true;
      } else {
        fresh_n += fresh;
        uint64_t* e = slots + 8 * s;
        vox_add(e + 1, an);
        vox_add(e + 2, a0);
        vox_add(e + 3, a1);
        vox_add(e + 4, a2);
        if (images) {
          vox_add(e + 5, arg & 0xFFFFu);
          vox_add(e + 6, arg >> 16);
          vox_add(e + 7, ab);
        }
      }
    }
    const vox_u64 fails = __ballot(failed);
    const bool dropped = valid && ((fails >> my_leader) & 1);
    ins += valid && !dropped;
    drop += dropped;
    if (pending && in_range) pending[p] = dropped ? 1 : 0;
  }
  if (cand) atomicAdd(&blk[0], cand);
  if (ins) atomicAdd(&blk[1], ins);
  if (outs) atomicAdd(&blk[2], outs);
  if (drop) atomicAdd(&blk[3], drop);
  if (fresh_n) atomicAdd(&blk[4], fresh_n);
  __syncthreads();
  if (threadIdx.x < 5 && blk[threadIdx.x]) {
    const uint64_t v = blk[threadIdx.x];
    const int t = (int)threadIdx.x;
    // a retry pass re-integrates pixels that an earlier call counted as candidates and dropped
    if (!retry) {
      vox_add(table + t, v);
    } else if (t == VOX_INSERTED) {
      vox_add(table + VOX_INSERTED, v);
      vox_add(table + VOX_DROPPED, (uint64_t)0 - v);
    } else if (t == VOX_VOXELS) {
      vox_add(table + VOX_VOXELS, v);
    }
  }
}

__global__ __launch_bounds__(VOX_THREADS) void voxel_rehash_kernel(const uint64_t* __restrict__ src, long src_capacity,
                                                                   uint64_t* __restrict__ dst, uint32_t cap_mask,
                                                                   int probe_limit) {
  __shared__ unsigned fresh_blk;
  if (threadIdx.x == 0) fresh_blk = 0;
  __syncthreads();
  const long i = (long)blockIdx.x * VOX_THREADS + threadIdx.x;
  uint64_t* slots = dst + VOX_HEADER_WORDS;
  if (i < 4 && src[i]) vox_add(dst + i, src[i]);                  // candidates, inserted, outside, dropped
  if (i < src_capacity) {
    const uint64_t* e = src + VOX_HEADER_WORDS + 8 * i;
    const uint64_t key = e[0];
    if (key != VOX_EMPTY) {
      bool fresh;
      const long s = vox_find(slots, cap_mask, probe_limit, key, &fresh);
      if (s < 0) {
        vox_add(dst + VOX_INSERTED, (uint64_t)0 - e[1]);
        vox_add(dst + VOX_DROPPED, e[1]);
      } else {
        if (fresh) atomicAdd(&fresh_blk, 1u);
#pragma unroll
        for (int k = 1; k < VOX_SLOT_WORDS; ++k)
          if (e[k]) vox_add(slots + 8 * s + k, e[k]);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && fresh_blk) vox_add(dst + VOX_VOXELS, fresh_blk);
}

__global__ __launch_bounds__(VOX_THREADS) void voxel_extract_kernel(uint64_t* __restrict__ table, long capacity, int min_count,
                                                                    VoxelParams c, long max_out, float* __restrict__ points,
                                                                    unsigned char* __restrict__ colors, int* __restrict__ counts,
                                                                    int64_t* __restrict__ keys, int64_t* __restrict__ found) {
  const long s = (long)blockIdx.x * VOX_THREADS + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const uint64_t* e = table + VOX_HEADER_WORDS + 8 * s;
  uint64_t key = VOX_EMPTY, nn = 0;
  if (s < capacity) {
    key = e[0];
    nn = e[1];
  }
  const bool take = key != VOX_EMPTY && nn >= (uint64_t)min_count;
  const vox_u64 mm = __ballot(take);
  vox_u64* place = (vox_u64*)(table + VOX_EXTRACT_PLACE);
  vox_u64* ticket = (vox_u64*)(table + VOX_EXTRACT_TICKET);
  if (mm) {                                                       // the same in every lane
    const int first = __ffsll((long long)mm) - 1;
    vox_u64 base = 0;
    if (lane == first) base = atomicAdd(place, (vox_u64)__popcll(mm));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, first);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), first);
    const long at = (long)(((uint64_t)hi << 32) | lo) + __popcll(mm & (((vox_u64)1 << lane) - 1));
    if (take && at < max_out) {
      float pt[3];
      unsigned char rgb[3];
      voxel_emit(key, nn, e + 2, e + 5, c, pt, rgb);
#pragma unroll
      for (int a = 0; a < 3; ++a) points[3 * at + a] = pt[a];
      if (colors) {
#pragma unroll
        for (int a = 0; a < 3; ++a) colors[3 * at + a] = rgb[a];
      }
      counts[at] = (int)nn;
      keys[at] = (int64_t)key;
    }
  }
  // The workgroup that draws the last ticket reports the total and leaves both scratch words 0 for the next call. Nobody waits:
  // every workgroup's places were returned to it (the value was used above) before it draws its ticket.
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const vox_u64 drawn = atomicAdd(ticket, (vox_u64)1);
    if (drawn == (vox_u64)gridDim.x - 1) {
      __threadfence();
      *found = (int64_t)__hip_atomic_load(place, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(place, (vox_u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ticket, (vox_u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- argument rules, shared by the two entry points of each pair below (images, mask, indices, pending and colors may be null)

static void voxel_check_table(const void* table, long capacity) {
  ATDN_CHECK(table, "null argument");
  ATDN_CHECK(capacity >= 2 && capacity <= VOX_MAX_CAPACITY && (capacity & (capacity - 1)) == 0,
             "capacity must be a power of two in [2, 2^31]");
  ATDN_CHECK(((uintptr_t)table & 7) == 0, "the table must be 8-byte aligned");
}

static void voxel_check_grid(double voxel, double ox, double oy, double oz) {
  ATDN_CHECK(std::isfinite(voxel) && voxel > 0.0, "voxel must be finite and > 0");
  ATDN_CHECK(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), "the origin must be finite");
}

static void voxel_check_integrate(const float* depth, const float* poses, const unsigned char* images, const unsigned char* mask,
                           const int* indices, int N, int K, int H, int W, double fx, double fy, double cx, double cy, int stride,
                           double voxel, double ox, double oy, double oz, double min_z, double max_z, const void* table,
                           long capacity, const unsigned char* pending) {
  ATDN_CHECK(depth && poses, "null argument");
  voxel_check_table(table, capacity);
  ATDN_CHECK(N >= 1 && K >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
  ATDN_CHECK(indices || K <= N, "without indices K keyframes are read: K <= N");
  ATDN_CHECK((long)K * H * W < (1L << 40), "too many pixels in one call (K * H * W < 2^40)");
  check_pinhole(fx, fy, cx, cy);
  ATDN_CHECK(stride >= 1, "stride must be >= 1");
  voxel_check_grid(voxel, ox, oy, oz);
  ATDN_CHECK(!std::isnan(min_z) && !std::isnan(max_z), "min_z and max_z must not be NaN");
  const long n = (long)H * W;
  const void* in[5] = {depth, poses, images, mask, indices};
  const long in_bytes[5] = {(long)N * n * 4, (long)N * 48, (long)N * 3 * n, (long)K * n, (long)K * 4};
  const void* out[2] = {table, pending};
  const long out_bytes[2] = {voxel_table_words(capacity) * 8, (long)K * n};
  check_disjoint(in, in_bytes, 5, out, out_bytes, pending ? 2 : 1);
}

static void voxel_check_rehash(const void* src, long src_capacity, const void* dst, long dst_capacity) {
  voxel_check_table(src, src_capacity);
  voxel_check_table(dst, dst_capacity);
  ATDN_CHECK(dst_capacity >= src_capacity, "the destination must not be smaller than the source");
  ATDN_CHECK(disjoint(src, voxel_table_words(src_capacity) * 8, dst, voxel_table_words(dst_capacity) * 8), "the tables overlap");
}

static void voxel_check_extract(const void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz, long max_out,
                         const float* points, const unsigned char* colors, const int* counts, const int64_t* keys,
                         const int64_t* found) {
  voxel_check_table(table, capacity);
  ATDN_CHECK(points && counts && keys && found, "null argument");
  ATDN_CHECK(min_count >= 1, "min_count must be >= 1");
  ATDN_CHECK(max_out >= 1 && max_out <= VOX_MAX_CAPACITY, "max_out must be in [1, 2^31]");
  voxel_check_grid(voxel, ox, oy, oz);
  ATDN_CHECK(((uintptr_t)points & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)keys & 7) == 0 && ((uintptr_t)found & 7) == 0,
             "points and counts must be 4-byte aligned, keys and found 8-byte aligned");
  const void* in[1] = {table};
  const long in_bytes[1] = {voxel_table_words(capacity) * 8};
  const void* out[5] = {points, counts, keys, found, colors};
  const long out_bytes[5] = {max_out * 12, max_out * 4, max_out * 8, 8, max_out * 3};
  check_disjoint(in, in_bytes, 1, out, out_bytes, colors ? 5 : 4);
}

}  // namespace atdn

using namespace atdn;

long atdn_voxel_table_bytes(long capacity) {
  if (capacity < 2 || capacity > VOX_MAX_CAPACITY || (capacity & (capacity - 1)) != 0) return 0;
  return voxel_table_words(capacity) * 8;
}

int atdn_voxel_clear(void* table, long capacity, void* stream) {
  ATDN_API_BEGIN
  voxel_check_table(table, capacity);
  const long words = voxel_table_words(capacity);
  hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)cdivl(words, VOX_THREADS)), dim3(VOX_THREADS), 0, (hipStream_t)stream,
                     (uint64_t*)table, words);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_voxel_clear_host(void* table, long capacity) {
  ATDN_API_BEGIN
  voxel_check_table(table, capacity);
  voxel_clear_host((uint64_t*)table, capacity);
  ATDN_API_END
}

int atdn_voxel_integrate(const float* depth, const float* poses, const uint8_t* images, const uint8_t* mask, const int* indices, int N,
                         int K, int H, int W, double fx, double fy, double cx, double cy, int stride, double voxel, double ox,
                         double oy, double oz, double min_z, double max_z, int retry, void* table, long capacity, uint8_t* pending,
                         void* stream) {
  ATDN_API_BEGIN
  voxel_check_integrate(depth, poses, images, mask, indices, N, K, H, W, fx, fy, cx, cy, stride, voxel, ox, oy, oz, min_z, max_z,
                        table, capacity, pending);
  const long total = (long)K * H * W;
  const long chunks = cdivl(total, VOX_THREADS);
  const long grid = chunks < VOX_GRID ? chunks : VOX_GRID;
  const long iters = cdivl(chunks, grid);
  ATDN_CHECK(iters < (1L << 31), "too many pixels in one call");
  hipLaunchKernelGGL(voxel_integrate_kernel, dim3((unsigned)grid), dim3(VOX_THREADS), 0, (hipStream_t)stream, depth, poses, images,
                     mask, indices, N, total, H, W, (int)iters, voxel_params(fx, fy, cx, cy, stride, voxel, ox, oy, oz, min_z, max_z),
                     retry != 0, (uint64_t*)table, (uint32_t)(capacity - 1), (int)voxel_probe_limit(capacity), pending);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_voxel_integrate_host(const float* depth, const float* poses, const uint8_t* images, const uint8_t* mask, const int* indices,
                              int N, int K, int H, int W, double fx, double fy, double cx, double cy, int stride, double voxel,
                              double ox, double oy, double oz, double min_z, double max_z, int retry, void* table, long capacity,
                              uint8_t* pending) {
  ATDN_API_BEGIN
  voxel_check_integrate(depth, poses, images, mask, indices, N, K, H, W, fx, fy, cx, cy, stride, voxel, ox, oy, oz, min_z, max_z,
                        table, capacity, pending);
  voxel_integrate_host(depth, poses, images, mask, indices, N, K, H, W,
                       voxel_params(fx, fy, cx, cy, stride, voxel, ox, oy, oz, min_z, max_z), retry != 0, (uint64_t*)table, capacity,
                       pending);
  ATDN_API_END
}

int atdn_voxel_rehash(const void* src, long src_capacity, void* dst, long dst_capacity, void* stream) {
  ATDN_API_BEGIN
  voxel_check_rehash(src, src_capacity, dst, dst_capacity);
  hipLaunchKernelGGL(voxel_rehash_kernel, dim3((unsigned)cdivl(src_capacity, VOX_THREADS)), dim3(VOX_THREADS), 0,
                     (hipStream_t)stream, (const uint64_t*)src, src_capacity, (uint64_t*)dst, (uint32_t)(dst_capacity - 1),
                     (int)voxel_probe_limit(dst_capacity));
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_voxel_rehash_host(const void* src, long src_capacity, void* dst, long dst_capacity) {
  ATDN_API_BEGIN
  voxel_check_rehash(src, src_capacity, dst, dst_capacity);
  voxel_rehash_host((const uint64_t*)src, src_capacity, (uint64_t*)dst, dst_capacity);
  ATDN_API_END
}

int atdn_voxel_extract(void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz, long max_out,
                       float* points, uint8_t* colors, int* counts, int64_t* keys, int64_t* found, void* stream) {
  ATDN_API_BEGIN
  voxel_check_extract(table, capacity, min_count, voxel, ox, oy, oz, max_out, points, colors, counts, keys, found);
  hipLaunchKernelGGL(voxel_extract_kernel, dim3((unsigned)cdivl(capacity, VOX_THREADS)), dim3(VOX_THREADS), 0, (hipStream_t)stream,
                     (uint64_t*)table, capacity, min_count, voxel_params(1.0, 1.0, 0.0, 0.0, 1, voxel, ox, oy, oz, 0.0, 0.0),
                     max_out, points, colors, counts, keys, found);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_voxel_extract_host(void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz,
                            long max_out, float* points, uint8_t* colors, int* counts, int64_t* keys, int64_t* found) {
  ATDN_API_BEGIN
  voxel_check_extract(table, capacity, min_count, voxel, ox, oy, oz, max_out, points, colors, counts, keys, found);
  voxel_extract_host((const uint64_t*)table, capacity, min_count, voxel_params(1.0, 1.0, 0.0, 0.0, 1, voxel, ox, oy, oz, 0.0, 0.0),
                     max_out, points, colors, counts, keys, found);
  ATDN_API_END
}
