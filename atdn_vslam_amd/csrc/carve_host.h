// Visibility votes and carving: does any keyframe see straight through a voxel, and how many confirm it — the rule in plain C++
// (no HIP needed). carve_vote is the rule for one point in one keyframe (float64, every operation rounded on its own, fp
// contraction off): a gather of one projection and a window of depth reads, three integer votes. carve_votes_host and
// voxel_remove_host are the host forms behind atdn_voxel_votes_host and atdn_voxel_remove_host (carve.hip), which serve CPU
// tensors. The kernels of carve.hip call carve_vote and voxel_home, so the two cannot drift apart; the independent statement the
// tests compare both with is tests/carve_ref.py (NumPy). The rule is stated in full in include/atdn_hip.h.
#pragma once
#include <cstdint>

#include "lm6.h"
#include "pixel_rule.h"
#include "voxel_map_host.h"

namespace atdn {

constexpr int CARVE_VIEW = 1, CARVE_SUPPORT = 2, CARVE_FREE = 4;
constexpr int CARVE_MAX_RADIUS = 8;

struct CarveParams {
  double fx, fy, cx, cy, near, far, rel, abs;
  int H, W, radius;
};

inline CarveParams carve_params(double fx, double fy, double cx, double cy, double near, double far, double rel, double abs_tol,
                                int radius, int H, int W) {
  return CarveParams{fx, fy, cx, cy, near, far, rel, abs_tol, H, W, radius};
}

// One point (its coordinates as doubles) in one keyframe: the 12 float32 of the pose, the keyframe's depth plane [H,W].
// Returns CARVE_VIEW | CARVE_SUPPORT | CARVE_FREE bits; 0 = not in view.
ATDN_HD inline int carve_vote(double p0, double p1, double p2, const float* pose, const float* plane, const CarveParams& c) {
#pragma clang fp contract(off)
  const double d0 = p0 - (double)pose[3], d1 = p1 - (double)pose[7], d2 = p2 - (double)pose[11];
  const double c0 = dot3((double)pose[0], d0, (double)pose[4], d1, (double)pose[8], d2);
  const double c1 = dot3((double)pose[1], d0, (double)pose[5], d1, (double)pose[9], d2);
  const double z = dot3((double)pose[2], d0, (double)pose[6], d1, (double)pose[10], d2);
  if (!(c.near <= z && z <= c.far)) return 0;
  const double xn = c0 / z, yn = c1 / z;
  const double u = xn * c.fx + c.cx, v = yn * c.fy + c.cy;
  const double a = u + 0.5, b = v + 0.5;
  const double r = (double)c.radius;
  if (!(a >= r && a < (double)(c.W - c.radius) && b >= r && b < (double)(c.H - c.radius))) return 0;
  const int x = (int)a, y = (int)b;                               // both >= radius; the window lies inside the image
  const double band = c.rel * z + c.abs;
  const double lo = z - band, hi = z + band;
  const double m = (double)plane[(long)y * c.W + x];
  if (!(c.near <= m && m <= c.far)) return CARVE_VIEW;            // an unmeasured centre: no support, and the window is not free
  if (!(m > hi)) return lo <= m ? (CARVE_VIEW | CARVE_SUPPORT) : CARVE_VIEW;
  bool free_ = true;
  for (int dy = -c.radius; dy <= c.radius; ++dy)
    for (int dx = -c.radius; dx <= c.radius; ++dx) {
      const double w = (double)plane[(long)(y + dy) * c.W + (x + dx)];
      free_ = free_ && (c.near <= w && w <= c.far && w > hi);
    }
  return free_ ? (CARVE_VIEW | CARVE_FREE) : CARVE_VIEW;
}

// ---- host forms: one thread

// points [M,3], depth [N,H,W], poses [N,12], indices [K] or null (then keyframe j is j), votes [M,3]
inline void carve_votes_host(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K,
                             const CarveParams& c, int accumulate, int* votes) {
  const long n = (long)c.H * c.W;
  for (int i = 0; i < M; ++i) {
    int sum[3] = {0, 0, 0};
    const double p0 = (double)points[3L * i], p1 = (double)points[3L * i + 1], p2 = (double)points[3L * i + 2];
    for (int j = 0; j < K; ++j) {
      const int kf = indices ? indices[j] : j;
      if (kf < 0 || kf >= N) continue;
      const int v = carve_vote(p0, p1, p2, poses + 12L * kf, depth + (long)kf * n, c);
      sum[0] += v & 1;
      sum[1] += (v >> 1) & 1;
      sum[2] += (v >> 2) & 1;
    }
    for (int a = 0; a < 3; ++a) votes[3L * i + a] = accumulate ? votes[3L * i + a] + sum[a] : sum[a];
  }
}

// The slot of `key` by a read-only probe (the home slot and the limit of insertion; an empty slot ends it), or -1.
inline long voxel_lookup_host(const uint64_t* slots, long capacity, uint64_t key) {
  const uint32_t mask = (uint32_t)(capacity - 1);
  uint32_t s = voxel_home(key, mask);
  const long limit = voxel_probe_limit(capacity);
  for (long i = 0; i < limit; ++i) {
    const uint64_t cur = slots[8 * (long)s];
    if (cur == VOX_EMPTY) return -1;
    if (cur == key) return (long)s;
    s = (s + 1) & mask;
  }
  return -1;
}

// keys [R], flags [R] or null (then every key); removed [3] = voxels emptied, points they held, flagged keys not found or empty
inline void voxel_remove_host(uint64_t* table, long capacity, const int64_t* keys, const unsigned char* flags, long R,
                              int64_t* removed) {
  uint64_t* slots = table + VOX_HEADER_WORDS;
  removed[0] = removed[1] = removed[2] = 0;
  for (long r = 0; r < R; ++r) {
    if (flags && !flags[r]) continue;
    const long s = voxel_lookup_host(slots, capacity, (uint64_t)keys[r]);
    if (s < 0 || slots[8 * s + 1] == 0) {
      removed[2] += 1;
      continue;
    }
    removed[0] += 1;
    removed[1] += (int64_t)slots[8 * s + 1];
    for (int k = 1; k < VOX_SLOT_WORDS; ++k) slots[8 * s + k] = 0;
  }
}

}  // namespace atdn
