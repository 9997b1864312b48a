// Map view: a point cloud rendered into cameras with a z-buffer — the rule in plain C++ (no HIP needed). view_point is the rule
// for one point in one camera (float64, every operation rounded on its own, fp contraction off): its pixel bounds and the high
// half of its word; view_word packs the word; view_resolve turns one pixel's word into its outputs; view_render_host is the host
// form behind atdn_view_render_host (map_view.hip), which serves CPU tensors. The kernels of map_view.hip call the same
// functions, so the two cannot drift apart; the independent statement the tests compare both with is tests/map_view_ref.py
// (NumPy). The rule is stated in full in include/atdn_hip.h.
//
// The word: (bits((float)z) << 32) | ((255 - min(n,255)) << 24) | red << 16 | green << 8 | blue; all ones = an empty pixel (no
// finite fp32 has the high half all ones). A pixel keeps the minimum word: the nearest point, then the better supported, then
// the smaller colour — a function of the set of points alone.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "lm6.h"
#include "pixel_rule.h"

namespace atdn {

constexpr uint64_t VIEW_EMPTY = ~(uint64_t)0;

struct ViewParams {
  double fx, fy, cx, cy, sx, sy, half_min, half_max, near, far;   // sx = ((0.5*splat)*size)*fx, sy with fy
  int H, W, min_count;
};

inline ViewParams view_params(double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near,
                              double far, int min_count, int H, int W) {
#pragma clang fp contract(off)
  const double s = (0.5 * splat) * size;
  return ViewParams{fx, fy, cx, cy, s * fx, s * fy, 0.5, 0.5 * (double)max_splat, near, far, H, W, min_count};
}

// ceil of a finite a with |a| < 2^31, spelled out: truncate, plus 1 if the integer converted back is below a
ATDN_HD inline int view_ceil(double a) {
  int i = (int)a;
  if ((double)i < a) i += 1;
  return i;
}

// The pixels lo..hi of an axis of `size` pixels that the half-open interval [centre - half, centre + half) covers; false if none
// (a NaN or an infinity among them). Every comparison is made in double before anything is converted.
ATDN_HD inline bool view_span(double centre, double half, int size, int* lo, int* hi) {
#pragma clang fp contract(off)
  const double a = centre - half, e = centre + half;
  const double last = (double)(size - 1);
  if (!(a <= last) || !(e > 0.0)) return false;
  *lo = a < 0.0 ? 0 : view_ceil(a);
  *hi = e > last ? size - 1 : view_ceil(e) - 1;
  return *lo <= *hi;
}

// One point in one camera: p[3], the 12 float32 of the pose. True iff VISIBLE; then box = {x0, x1, y0, y1} and *zbits are set.
ATDN_HD inline bool view_point(const float* p, const float* pose, const ViewParams& c, int box[4], uint32_t* zbits) {
#pragma clang fp contract(off)
  const double d0 = (double)p[0] - (double)pose[3], d1 = (double)p[1] - (double)pose[7], d2 = (double)p[2] - (double)pose[11];
  const double c0 = dot3((double)pose[0], d0, (double)pose[4], d1, (double)pose[8], d2);
  const double c1 = dot3((double)pose[1], d0, (double)pose[5], d1, (double)pose[9], d2);
  const double z = dot3((double)pose[2], d0, (double)pose[6], d1, (double)pose[10], d2);
  if (!(c.near <= z && z <= c.far)) return false;
  const double xn = c0 / z, yn = c1 / z;
  const double u = xn * c.fx + c.cx, v = yn * c.fy + c.cy;
  double hx = c.sx / z, hy = c.sy / z;
  hx = hx < c.half_min ? c.half_min : (hx > c.half_max ? c.half_max : hx);
  hy = hy < c.half_min ? c.half_min : (hy > c.half_max ? c.half_max : hy);
  if (!view_span(u, hx, c.W, &box[0], &box[1])) return false;
  if (!view_span(v, hy, c.H, &box[2], &box[3])) return false;
  const float zf = (float)z;
#if defined(__HIP_DEVICE_COMPILE__)
  *zbits = __float_as_uint(zf);
#else
  std::memcpy(zbits, &zf, 4);
#endif
  return true;
}

// rgb: the point's three colour bytes, or null
ATDN_HD inline uint64_t view_word(uint32_t zbits, int n, const unsigned char* rgb) {
  const uint32_t s = n < 255 ? (uint32_t)n : 255u;
  uint32_t lo = (255u - s) << 24;
  if (rgb) lo |= ((uint32_t)rgb[0] << 16) | ((uint32_t)rgb[1] << 8) | (uint32_t)rgb[2];
  return ((uint64_t)zbits << 32) | lo;
}

// One pixel: its word -> the bits of its depth, its support and its colour. False (and zeros) for an empty pixel.
ATDN_HD inline bool view_resolve(uint64_t word, uint32_t* depth_bits, unsigned char* support, unsigned char rgb[3]) {
  const bool covered = word != VIEW_EMPTY;
  const uint32_t lo = covered ? (uint32_t)word : 0xFF000000u;
  *depth_bits = covered ? (uint32_t)(word >> 32) : 0u;
  *support = (unsigned char)(255u - (lo >> 24));
  rgb[0] = (unsigned char)((lo >> 16) & 255u);
  rgb[1] = (unsigned char)((lo >> 8) & 255u);
  rgb[2] = (unsigned char)(lo & 255u);
  return covered;
}

// ---- host form: one thread, a z-buffer of its own

inline void view_render_host(const float* points, const unsigned char* colors, const int* counts, int M, const float* poses, int B,
                             const ViewParams& c, float* depth, unsigned char* colors_out, unsigned char* support,
                             int64_t* counts_out) {
  const long n = (long)c.H * c.W;
  std::vector<uint64_t> zbuf((size_t)n);
  for (int b = 0; b < B; ++b) {
    for (long i = 0; i < n; ++i) zbuf[(size_t)i] = VIEW_EMPTY;
    int64_t cand = 0, vis = 0, covered = 0;
    for (int i = 0; i < M; ++i) {
      if (counts[i] < c.min_count) continue;
      cand += 1;
      int box[4];
      uint32_t zbits;
      if (!view_point(points + 3L * i, poses + 12L * b, c, box, &zbits)) continue;
      vis += 1;
      const uint64_t word = view_word(zbits, counts[i], colors ? colors + 3L * i : nullptr);
      for (int y = box[2]; y <= box[3]; ++y)
        for (int x = box[0]; x <= box[1]; ++x) {
          uint64_t& w = zbuf[(size_t)((long)y * c.W + x)];
          if (word < w) w = word;
        }
    }
    for (long i = 0; i < n; ++i) {
      uint32_t bits;
      unsigned char s, rgb[3];
      covered += view_resolve(zbuf[(size_t)i], &bits, &s, rgb);
      std::memcpy(depth + (long)b * n + i, &bits, 4);
      support[(long)b * n + i] = s;
      if (colors_out)
        for (int a = 0; a < 3; ++a) colors_out[((long)b * 3 + a) * n + i] = rgb[a];
    }
    counts_out[3L * b] = cand;
    counts_out[3L * b + 1] = vis;
    counts_out[3L * b + 2] = covered;
  }
}

}  // namespace atdn
