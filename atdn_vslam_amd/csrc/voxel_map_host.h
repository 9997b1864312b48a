// Voxel map: every keyframe's depth accumulated into one voxel-hashed point cloud — the rule in plain C++ (no HIP needed).
// voxel_point is the rule for one pixel (float64, every operation rounded on its own, fp contraction off), voxel_home the home
// slot of a key, voxel_emit the extraction of one voxel; voxel_*_host are the host forms behind atdn_voxel_*_host (voxel_map.hip),
// which serve CPU tensors. The kernels of voxel_map.hip call the same functions, so the two cannot drift apart; the independent
// statement the tests compare both with is tests/voxel_map_ref.py (NumPy). The rule is stated in full in include/atdn_hip.h.
//
// The table (atdn_voxel_table_bytes(capacity) = 64 + 64 * capacity bytes, 8-byte aligned, little-endian 64-bit words):
//   words 0..7   the header: candidates, inserted, outside, dropped, voxels (int64), two scratch words of the device extraction
//                (0 between calls), one reserved word (0)
//   words 8 + 8 s .. 8 + 8 s + 7   slot s < capacity: key (all ones = empty), n, S_x, S_y, S_z, C_red, C_green, C_blue (uint64)
// n < 2^31 points of q <= 65536 and colour bytes <= 255: S < 2^47 and C < 2^39, no 64-bit sum can overflow.
// home(key) = (((key * 0x9E3779B97F4A7C15 mod 2^64) >> 32) * capacity) >> 32, the top log2(capacity) bits of the product; linear
// probing, at most min(capacity, 1024) slots.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lm6.h"
#include "pixel_rule.h"

namespace atdn {

constexpr uint64_t VOX_EMPTY = ~(uint64_t)0;
constexpr int VOX_HEADER_WORDS = 8, VOX_SLOT_WORDS = 8;
constexpr long VOX_PROBE_LIMIT = 1024;
constexpr long VOX_MAX_CAPACITY = 1L << 31;
enum { VOX_CANDIDATES = 0, VOX_INSERTED = 1, VOX_OUTSIDE = 2, VOX_DROPPED = 3, VOX_VOXELS = 4, VOX_EXTRACT_PLACE = 5,
       VOX_EXTRACT_TICKET = 6 };
enum { VOX_PIXEL_SKIP = 0, VOX_PIXEL_OUTSIDE = 1, VOX_PIXEL_INSIDE = 2 };

struct VoxelParams {
  double fx, fy, cx, cy, voxel, o[3], min_z, max_z;
  int stride;
};

inline VoxelParams voxel_params(double fx, double fy, double cx, double cy, int stride, double voxel, double ox, double oy,
                                double oz, double min_z, double max_z) {
  return VoxelParams{fx, fy, cx, cy, voxel, {ox, oy, oz}, min_z, max_z, stride};
}

inline long voxel_table_words(long capacity) { return VOX_HEADER_WORDS + VOX_SLOT_WORDS * capacity; }
inline long voxel_probe_limit(long capacity) { return capacity < VOX_PROBE_LIMIT ? capacity : VOX_PROBE_LIMIT; }

ATDN_HD inline uint32_t voxel_home(uint64_t key, uint32_t cap_mask) {
  const uint64_t top = (key * 0x9E3779B97F4A7C15ull) >> 32;      // every bit of the key reaches the product's top bits
  return (uint32_t)((top * ((uint64_t)cap_mask + 1)) >> 32);
}

// One pixel that takes part: its depth, the 12 float32 of its keyframe's pose. VOX_PIXEL_SKIP: not a candidate;
// VOX_PIXEL_OUTSIDE: a candidate outside the key range; VOX_PIXEL_INSIDE: *key and q[3] are set.
ATDN_HD inline int voxel_point(float depth, const float* pose, int x, int y, const VoxelParams& c, uint64_t* key, unsigned q[3]) {
#pragma clang fp contract(off)
  const double z = (double)depth;
  if (!(c.min_z <= z && z <= c.max_z)) return VOX_PIXEL_SKIP;
  const double dx = (double)x - c.cx, dy = (double)y - c.cy;
  const double xn = dx / c.fx, yn = dy / c.fy;
  const double c0 = xn * z, c1 = yn * z;
  uint64_t k = 0;
  for (int a = 0; a < 3; ++a) {
    const double d = dot3((double)pose[4 * a], c0, (double)pose[4 * a + 1], c1, (double)pose[4 * a + 2], z);
    const double p = d + (double)pose[4 * a + 3];
    const double e = p - c.o[a];
    const double g = e / c.voxel;
    if (!(-1048576.0 <= g && g < 1048576.0)) return VOX_PIXEL_OUTSIDE;
    int ki = (int)g;                                             // |g| <= 2^20: the value of the rule's 64-bit truncation
    if ((double)ki > g) ki -= 1;
    const double f = g - (double)ki;
    const double fq = f * 65536.0;
    q[a] = (unsigned)(int)fq;                                    // 0 .. 65536
    k = (k << 21) | (uint64_t)(unsigned)(ki + 1048576);
  }
  *key = k;
  return VOX_PIXEL_INSIDE;
}

// The extraction of one voxel: the three coordinates and, from the colour sums, the three bytes.
ATDN_HD inline void voxel_emit(uint64_t key, uint64_t n, const uint64_t* S, const uint64_t* Cs, const VoxelParams& c, float point[3],
                               unsigned char rgb[3]) {
#pragma clang fp contract(off)
  for (int a = 0; a < 3; ++a) {
    const int64_t ki = (int64_t)((key >> (21 * (2 - a))) & 0x1FFFFF) - 1048576;
    const double m = (double)S[a] / (double)n;
    const double m5 = m + 0.5;
    const double fr = m5 / 65536.0;
    const double kk = (double)ki + fr;
    const double sc = kk * c.voxel;
    point[a] = (float)(c.o[a] + sc);
    rgb[a] = (unsigned char)((Cs[a] + n / 2) / n);
  }
}

// ---- host forms: the same table in host memory, one thread

inline void voxel_clear_host(uint64_t* table, long capacity) {
  for (int i = 0; i < VOX_HEADER_WORDS; ++i) table[i] = 0;
  uint64_t* slots = table + VOX_HEADER_WORDS;
  for (long s = 0; s < capacity; ++s) {
    slots[8 * s] = VOX_EMPTY;
    for (int i = 1; i < VOX_SLOT_WORDS; ++i) slots[8 * s + i] = 0;
  }
}

// the slot of `key` (claimed when new: *fresh), or -1 after the probe limit
inline long voxel_find_host(uint64_t* slots, long capacity, uint64_t key, bool* fresh) {
  const uint32_t mask = (uint32_t)(capacity - 1);
  uint32_t s = voxel_home(key, mask);
  const long limit = voxel_probe_limit(capacity);
  *fresh = false;
  for (long i = 0; i < limit; ++i) {
    if (slots[8 * (long)s] == key) return (long)s;
    if (slots[8 * (long)s] == VOX_EMPTY) {
      slots[8 * (long)s] = key;
      *fresh = true;
      return (long)s;
    }
    s = (s + 1) & mask;
  }
  return -1;
}

// depth [N,H,W], poses [N,12], images [N,3,H,W] or null, mask [K,H,W] or null, indices [K] or null (then keyframe j is j),
// pending [K,H,W] or null
inline void voxel_integrate_host(const float* depth, const float* poses, const unsigned char* images, const unsigned char* mask,
                                 const int* indices, int N, int K, int H, int W, const VoxelParams& c, int retry, uint64_t* table,
                                 long capacity, unsigned char* pending) {
  const long n = (long)H * W;
  int64_t* cnt = (int64_t*)table;
  uint64_t* slots = table + VOX_HEADER_WORDS;
  for (int j = 0; j < K; ++j) {
    const int kf = indices ? indices[j] : j;
    const bool frame_ok = kf >= 0 && kf < N;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const long r = (long)y * W + x;
        const long p = (long)j * n + r;
        if (pending) pending[p] = 0;
        if (!frame_ok || x % c.stride != 0 || y % c.stride != 0 || (mask && !mask[p])) continue;
        uint64_t key;
        unsigned q[3];
        const int st = voxel_point(depth[(long)kf * n + r], poses + 12L * kf, x, y, c, &key, q);
        if (st == VOX_PIXEL_SKIP) continue;
        if (!retry) cnt[VOX_CANDIDATES] += 1;
        if (st == VOX_PIXEL_OUTSIDE) {
          if (!retry) cnt[VOX_OUTSIDE] += 1;
          continue;
        }
        bool fresh;
        const long s = voxel_find_host(slots, capacity, key, &fresh);
        if (s < 0) {
          if (!retry) cnt[VOX_DROPPED] += 1;
          if (pending) pending[p] = 1;
          continue;
        }
        if (fresh) cnt[VOX_VOXELS] += 1;
        cnt[VOX_INSERTED] += 1;
        if (retry) cnt[VOX_DROPPED] -= 1;
        uint64_t* e = slots + 8 * s;
        e[1] += 1;
        for (int a = 0; a < 3; ++a) e[2 + a] += q[a];
        if (images)
          for (int a = 0; a < 3; ++a) e[5 + a] += images[((long)kf * 3 + a) * n + r];
      }
  }
}

inline void voxel_rehash_host(const uint64_t* src, long src_capacity, uint64_t* dst, long dst_capacity) {
  int64_t* cnt = (int64_t*)dst;
  const int64_t* scnt = (const int64_t*)src;
  for (int i = 0; i < 4; ++i) cnt[i] += scnt[i];
  const uint64_t* in = src + VOX_HEADER_WORDS;
  uint64_t* slots = dst + VOX_HEADER_WORDS;
  for (long i = 0; i < src_capacity; ++i) {
    const uint64_t* e = in + 8 * i;
    if (e[0] == VOX_EMPTY) continue;
    bool fresh;
    const long s = voxel_find_host(slots, dst_capacity, e[0], &fresh);
    if (s < 0) {
      cnt[VOX_INSERTED] -= (int64_t)e[1];
      cnt[VOX_DROPPED] += (int64_t)e[1];
      continue;
    }
    if (fresh) cnt[VOX_VOXELS] += 1;
    for (int k = 1; k < VOX_SLOT_WORDS; ++k) slots[8 * s + k] += e[k];
  }
}

// ascending key order; colors may be null
inline void voxel_extract_host(const uint64_t* table, long capacity, int min_count, const VoxelParams& c, long max_out, float* points,
                               unsigned char* colors, int* counts, int64_t* keys, int64_t* found) {
  const uint64_t* slots = table + VOX_HEADER_WORDS;
  std::vector<std::pair<uint64_t, long>> order;
  for (long s = 0; s < capacity; ++s)
    if (slots[8 * s] != VOX_EMPTY && slots[8 * s + 1] >= (uint64_t)min_count) order.emplace_back(slots[8 * s], s);
  std::sort(order.begin(), order.end());
  *found = (int64_t)order.size();
  for (long i = 0; i < (long)order.size() && i < max_out; ++i) {
    const uint64_t* e = slots + 8 * order[(size_t)i].second;
    float pt[3];
    unsigned char rgb[3];
    voxel_emit(e[0], e[1], e + 2, e + 5, c, pt, rgb);
    for (int a = 0; a < 3; ++a) points[3 * i + a] = pt[a];
    if (colors)
      for (int a = 0; a < 3; ++a) colors[3 * i + a] = rgb[a];
    counts[i] = (int)e[1];
    keys[i] = (int64_t)e[0];
  }
}

}  // namespace atdn
