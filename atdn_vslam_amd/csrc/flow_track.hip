// One step of a flow track on the device: the flow from an anchor frame to frame k (acc, with a liveness byte per pixel) composed
// with the flow k -> k+1 read bilinearly where each track stands, and — given the accumulated pose anchor <- frame k+1 and the
// calibration — the two-view depth of the composed correspondence written over the anchor's depth map where it is valid. The
// rule — float64, every operation rounded on its own — is flow_track_pixel of flow_track_host.h, which this kernel calls, so the
// kernel and the host form evaluate one function. One memset node and one launch on the caller's stream: asynchronous, capturable,
// no host synchronisation, no workspace; the pose is read from device memory. The counts are integer sums (ballot / popcount per
// wave, the waves of a workgroup through LDS, one integer atomic add per workgroup and counter), so they do not depend on the order
// of arrival: the same bits on every call.
//
// Decomposition. Per pixel the kernel streams 9 bytes of state in and 9 out (+ 4 in and 4 out of depth with a pose); the four taps
// of the flow (and the mask byte) are local gathers that stay in L2 (the two planes of a 376 x 1232 flow are 3.7 MB). The chain
// is ~30 float64 operations per pixel, the depth part the ~110 of two_view_pixel. A thread owns one aligned dword of the alive_out
// plane: four consecutive flat indices. The quads are cut on the ADDRESS of that plane, not on the index: with off = (address of
// alive_out[b, 0, 0]) & 3, quad q holds the indices 4q - off .. 4q - off + 3 of plane b, so H * W and the plane base of b >= 1 need
// not be multiples of four. Every other access of the quad — acc_in and acc_out (two float4 each), alive_in (a dword), depth (a
// float4 in, a float4 out) — is a vector access only where its own address is aligned at the quad (the same answer for every quad
// of a plane); the ragged quads at the head and the tail of a plane take scalar accesses of the indices inside the plane only.
// A thread reads the state of its own four pixels before it writes them and reads no other pixel's state, so acc_out == acc_in and
// alive_out == alive_in are safe; depth is read only to keep the values of the pixels that are not valid in a float4 store, and a
// quad without a valid pixel stores no depth at all.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "common.h"
#include "flow_track_host.h"

namespace atdn {

constexpr int FT_THREADS = 256;   // four waves
constexpr int FT_WAVES = FT_THREADS / 64;

// the four values p[s0 .. s0 + 3]; outside [lo, hi) zeros, and nothing is read there
__device__ __forceinline__ void ft_load4(const float* p, int s0, int lo, int hi, bool full, float v[4]) {
  if (full && ((uintptr_t)(p + s0) & 15) == 0) {
    const float4 a = *reinterpret_cast<const float4*>(p + s0);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = s0 + k;
      v[k] = (i >= lo && i < hi) ? p[i] : 0.0f;
    }
  }
}

__device__ __forceinline__ void ft_store4(float* p, int s0, int lo, int hi, bool full, const float v[4]) {
  if (full && ((uintptr_t)(p + s0) & 15) == 0) {
    *reinterpret_cast<float4*>(p + s0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = s0 + k;
      if (i >= lo && i < hi) p[i] = v[k];
    }
  }
}

// acc_in / acc_out and alive_in / alive_out may be the same buffers: no __restrict__ on them
template <bool DEPTH>
__global__ __launch_bounds__(FT_THREADS) void flow_track_kernel(const float* __restrict__ flow, const unsigned char* __restrict__ mask,
                                                                const float* acc_in, const unsigned char* alive_in, int H, int W,
                                                                float* acc_out, unsigned char* alive_out,
                                                                const float* __restrict__ pose, TwoViewCamera cam, float* depth,
                                                                int* __restrict__ counts) {
  __shared__ int partial[4][FT_WAVES];
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fx = flow + (long)b * 2 * n;
  const float* fy = fx + n;
  const unsigned char* m = mask ? mask + (long)b * n : nullptr;
  const float* ix = acc_in + (long)b * 2 * n;
  const float* iy = ix + n;
  float* ox = acc_out + (long)b * 2 * n;
  float* oy = ox + n;
  const unsigned char* li = alive_in + (long)b * n;
  unsigned char* lv = alive_out + (long)b * n;
  const int off = (int)((uintptr_t)lv & 3);
  const int q = blockIdx.x * FT_THREADS + threadIdx.x;
  const int s0 = 4 * q - off;                                  // first index of the quad: -3 .. n + 2 (n <= 2^24)
  const int lo = s0 > 0 ? s0 : 0, hi = s0 + 4 < n ? s0 + 4 : n;
  const bool full = hi - lo == 4;
  int flags[4] = {0, 0, 0, 0};
  if (lo < hi) {
    float ux[4], uy[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool live[4];
    ft_load4(ix, s0, lo, hi, full, ux);
    ft_load4(iy, s0, lo, hi, full, uy);
    if (full && ((uintptr_t)(li + s0) & 3) == 0) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(li + s0);
#pragma unroll
      for (int k = 0; k < 4; ++k) live[k] = ((w >> (8 * k)) & 0xFFu) != 0;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = s0 + k;
        live[k] = (i >= lo && i < hi) ? li[i] != 0 : false;
      }
    }
    float* d = nullptr;
    TwoViewPose P{};
    if (DEPTH) {
      d = depth + (long)b * n;
      ft_load4(d, s0, lo, hi, full, z);
      P = two_view_load_pose(pose + 12 * b);
    }
    float px[4], py[4];
    int y = lo / W, x = lo - y * W;                            // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = s0 + k;
      px[k] = ux[k];
      py[k] = uy[k];
      if (i >= lo && i < hi) {
        flags[k] = flow_track_pixel<DEPTH>(ux[k], uy[k], live[k], fx, fy, m, H, W, x, y, &P, &cam, &px[k], &py[k], &z[k]);
        if (++x == W) { x = 0; ++y; }
      }
    }
    ft_store4(ox, s0, lo, hi, full, px);
    ft_store4(oy, s0, lo, hi, full, py);
    if (full) {
      *reinterpret_cast<uint32_t*>(lv + s0) = (uint32_t)((flags[0] & FT_ALIVE) != 0) | ((uint32_t)((flags[1] & FT_ALIVE) != 0) << 8) |
                                              ((uint32_t)((flags[2] & FT_ALIVE) != 0) << 16) |
                                              ((uint32_t)((flags[3] & FT_ALIVE) != 0) << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = s0 + k;
        if (i >= lo && i < hi) lv[i] = (flags[k] & FT_ALIVE) ? 1 : 0;
      }
    }
    if (DEPTH && ((flags[0] | flags[1] | flags[2] | flags[3]) & TV_VALID)) ft_store4(d, s0, lo, hi, full, z);
  }
  // every lane of a wave gets the wave's four sums; lane 0 hands them to LDS
  int sum[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sum[0] += __popcll(__ballot(flags[k] & FT_ALIVE));
    if (DEPTH) {
      sum[1] += __popcll(__ballot(flags[k] & TV_INSIDE));
      sum[2] += __popcll(__ballot(flags[k] & TV_INLIER));
      sum[3] += __popcll(__ballot(flags[k] & TV_VALID));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) partial[j][threadIdx.x >> 6] = sum[j];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < FT_WAVES; ++w) total += partial[threadIdx.x][w];
    if (total) atomicAdd(counts + 4 * b + threadIdx.x, total);
  }
}

static bool disjoint(const void* a, long a_bytes, const void* b, long b_bytes) {
  const char* p = (const char*)a;
  const char* q = (const char*)b;
  return p + a_bytes <= q || q + b_bytes <= p;
}

// Argument rules shared by the device entry point below and the host one (capi.hip).
void flow_track_check_args(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in, int B,
                           int H, int W, const float* acc_out, const unsigned char* alive_out, const float* pose,
                           const TwoViewCamera& cam, const float* depth, const int* counts) {
  ATDN_CHECK(flow && acc_in && alive_in && acc_out && alive_out && counts, "null argument");
  ATDN_CHECK(B >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
  if (pose) {
    ATDN_CHECK(depth, "a pose needs a depth map");
    ATDN_CHECK(std::isfinite(cam.fx) && std::isfinite(cam.fy) && cam.fx > 0.0 && cam.fy > 0.0, "fx and fy must be finite and > 0");
    ATDN_CHECK(std::isfinite(cam.cx) && std::isfinite(cam.cy), "cx and cy must be finite");
    ATDN_CHECK(std::isfinite(cam.max_epipolar) && cam.max_epipolar >= 0.0, "max_epipolar must be finite and >= 0");
    ATDN_CHECK(std::isfinite(cam.min_sin2) && cam.min_sin2 >= 0.0, "min_sin2 must be finite and >= 0");
    ATDN_CHECK(std::isfinite(cam.max_depth) && cam.max_depth > 0.0, "max_depth must be finite and > 0");
  } else {
    ATDN_CHECK(!depth, "the chain-only form (no pose) takes no depth map");
  }
  const long n = (long)H * W;
  const void* in[5] = {flow, mask, acc_in, alive_in, pose};
  const long in_bytes[5] = {(long)B * 2 * n * 4, (long)B * n, (long)B * 2 * n * 4, (long)B * n, (long)B * 48};
  const void* out[4] = {acc_out, alive_out, depth, counts};
  const long out_bytes[4] = {(long)B * 2 * n * 4, (long)B * n, (long)B * n * 4, (long)B * 16};
  for (int o = 0; o < 4; ++o) {
    if (!out[o]) continue;
    for (int k = 0; k < 5; ++k) {
      if (!in[k]) continue;
      if ((o == 0 && k == 2 && acc_out == acc_in) || (o == 1 && k == 3 && alive_out == alive_in)) continue;   // in place
      ATDN_CHECK(disjoint(in[k], in_bytes[k], out[o], out_bytes[o]), "an output overlaps an input");
    }
    for (int k = o + 1; k < 4; ++k)
      if (out[k]) ATDN_CHECK(disjoint(out[k], out_bytes[k], out[o], out_bytes[o]), "two outputs overlap");
  }
}

}  // namespace atdn

using namespace atdn;

int atdn_flow_track_step(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in, int B,
                         int H, int W, float* acc_out, unsigned char* alive_out, const float* pose, double fx, double fy, double cx,
                         double cy, double max_epipolar, double min_sin2, double max_depth, float* depth, int* counts,
                         void* stream) {
  try {
    const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
    flow_track_check_args(flow, mask, acc_in, alive_in, B, H, W, acc_out, alive_out, pose, cam, depth, counts);
    const long n = (long)H * W;
    ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 16, (hipStream_t)stream));
    const long quads = (n + 3) / 4 + 1;                        // off <= 3 moves the last index into one more quad at most
    const dim3 grid((unsigned)cdivl(quads, FT_THREADS), (unsigned)B);
    if (pose)
      hipLaunchKernelGGL(flow_track_kernel<true>, grid, dim3(FT_THREADS), 0, (hipStream_t)stream, flow, mask, acc_in, alive_in, H,
                         W, acc_out, alive_out, pose, cam, depth, counts);
    else
      hipLaunchKernelGGL(flow_track_kernel<false>, grid, dim3(FT_THREADS), 0, (hipStream_t)stream, flow, mask, acc_in, alive_in, H,
                         W, acc_out, alive_out, pose, cam, depth, counts);
    ATDN_HIP(hipGetLastError());
    return 0;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return 1;
  } catch (...) {
    set_last_error("unknown error");
    return 1;
  }
}
