// Two-view geometry on the device: from a flow, a relative pose and the calibration, depth[b, 0, y, x] = the triangulated depth of
// pixel (x, y) in camera 1 (0 where there is none) and counts[b] = (correspondences inside image 2, epipolar inliers, valid
// depths). The rule — float64, every operation rounded on its own — is two_view_pixel of two_view_host.h, which this kernel calls,
// so the kernel and the host form evaluate one function. One memset node and one launch on the caller's stream: asynchronous,
// capturable, no host synchronisation, no workspace; the pose is read from device memory. The counts are integer sums (ballot /
// popcount per wave, the waves of a workgroup through LDS, one integer atomic add per workgroup and counter), so they do not
// depend on the order of arrival: the same bits on every call.
//
// Decomposition. The kernel streams 8 bytes of flow (+ 1 byte of mask) in and 4 bytes out per pixel; the ~110 float64 operations
// of a pixel include ten divisions. A thread owns four consecutive flat indices 4q .. 4q + 3 of a plane: two float4 loads of the
// flow, one dword of mask, one float4 store. Each of the three is a vector access only where its own address is aligned at the
// quad (the same answer for every quad of a plane, since a quad advances every address by a multiple of its vector size); a plane
// that is not — H * W not a multiple of four and b >= 1, or a buffer that starts off the grid — and the ragged last quad of a plane
// take scalar accesses, of the indices inside the plane only.
//
// atdn_depth_backproject below is the pinhole back-projection of a depth map (project_depth of the reference's utils/depth.py for
// a calibration without skew): 4 bytes in, 12 out per pixel, one pixel per thread, coalesced dwords.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "common.h"
#include "two_view_host.h"

namespace atdn {

constexpr int TV_THREADS = 256;   // four waves
constexpr int TV_WAVES = TV_THREADS / 64;

template <bool MASKED>
__global__ __launch_bounds__(TV_THREADS) void two_view_kernel(const float* __restrict__ flow, const float* __restrict__ pose,
                                                              const unsigned char* __restrict__ mask, int H, int W,
                                                              TwoViewCamera cam, float* __restrict__ depth,
                                                              int* __restrict__ counts) {
  __shared__ int partial[3][TV_WAVES];
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fu = flow + (long)b * 2 * n;
  const float* fv = fu + n;
  const unsigned char* m = MASKED ? mask + (long)b * n : nullptr;
  float* d = depth + (long)b * n;
  const int s0 = 4 * (blockIdx.x * TV_THREADS + threadIdx.x);   // first index of the quad: < n + 4 * TV_THREADS (n <= 2^24)
  const int hi = s0 + 4 < n ? s0 + 4 : n;                        // indices s0 .. hi - 1 are inside the plane
  const bool full = hi - s0 == 4;
  int flags[4] = {0, 0, 0, 0};
  if (s0 < hi) {
    float u[4], v[4], z[4];
    bool keep[4] = {true, true, true, true};
    const bool wide_in = (((uintptr_t)(fu + s0) | (uintptr_t)(fv + s0)) & 15) == 0;
    if (full && wide_in) {
      const float4 a = *reinterpret_cast<const float4*>(fu + s0);
      const float4 c = *reinterpret_cast<const float4*>(fv + s0);
      u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
      v[0] = c.x; v[1] = c.y; v[2] = c.z; v[3] = c.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = s0 + k < hi;
        u[k] = in ? fu[s0 + k] : 0.0f;
        v[k] = in ? fv[s0 + k] : 0.0f;
      }
    }
    if (MASKED) {
      if (full && ((uintptr_t)(m + s0) & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(m + s0);
#pragma unroll
        for (int k = 0; k < 4; ++k) keep[k] = ((w >> (8 * k)) & 0xFFu) != 0;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) keep[k] = s0 + k < hi ? m[s0 + k] != 0 : false;
      }
    }
    const TwoViewPose P = two_view_load_pose(pose + 12 * b);
    int y = s0 / W, x = s0 - y * W;                              // of index s0; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      z[k] = 0.0f;
      if (s0 + k < hi) {
        if (keep[k]) z[k] = two_view_pixel(u[k], v[k], P, cam, H, W, x, y, &flags[k]);
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (full && ((uintptr_t)(d + s0) & 15) == 0) {
      *reinterpret_cast<float4*>(d + s0) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (s0 + k < hi) d[s0 + k] = z[k];
    }
  }
  // every lane of a wave gets the wave's three sums; lane 0 hands them to LDS
  int sum[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sum[0] += __popcll(__ballot(flags[k] & TV_INSIDE));
    sum[1] += __popcll(__ballot(flags[k] & TV_INLIER));
    sum[2] += __popcll(__ballot(flags[k] & TV_VALID));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) partial[j][threadIdx.x >> 6] = sum[j];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < TV_WAVES; ++w) total += partial[threadIdx.x][w];
    if (total) atomicAdd(counts + 3 * b + threadIdx.x, total);
  }
}

__global__ __launch_bounds__(TV_THREADS) void depth_backproject_kernel(const float* __restrict__ depth, int H, int W, double fx,
                                                                       double fy, double cx, double cy,
                                                                       float* __restrict__ points) {
#pragma clang fp contract(off)
  const int n = H * W;
  const int i = blockIdx.x * TV_THREADS + threadIdx.x;
  if (i >= n) return;
  const int b = blockIdx.y;
  const int y = i / W, x = i - y * W;
  const double z = (double)depth[(long)b * n + i];
  const double dx = (double)x - cx, dy = (double)y - cy;
  const double zx = z * dx, zy = z * dy;
  float* p = points + (long)b * 3 * n + i;
  p[0] = (float)(zx / fx);
  p[n] = (float)(zy / fy);
  p[2 * (long)n] = (float)z;
}

static bool disjoint(const void* a, long a_bytes, const void* b, long b_bytes) {
  const char* p = (const char*)a;
  const char* q = (const char*)b;
  return p + a_bytes <= q || q + b_bytes <= p;
}

static void check_camera(int B, int H, int W, double fx, double fy, double cx, double cy) {
  ATDN_CHECK(B >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
  ATDN_CHECK(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0 && fy > 0.0, "fx and fy must be finite and > 0");
  ATDN_CHECK(std::isfinite(cx) && std::isfinite(cy), "cx and cy must be finite");
}

// Argument rules shared by the device entry point below and the host one (capi.hip).
void two_view_check_args(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W,
                         const TwoViewCamera& cam, const float* depth, const int* counts) {
  ATDN_CHECK(flow && pose && depth && counts, "null argument");
  check_camera(B, H, W, cam.fx, cam.fy, cam.cx, cam.cy);
  ATDN_CHECK(std::isfinite(cam.max_epipolar) && cam.max_epipolar >= 0.0, "max_epipolar must be finite and >= 0");
  ATDN_CHECK(std::isfinite(cam.min_sin2) && cam.min_sin2 >= 0.0, "min_sin2 must be finite and >= 0");
  ATDN_CHECK(std::isfinite(cam.max_depth) && cam.max_depth > 0.0, "max_depth must be finite and > 0");
  const long n = (long)H * W;
  const long d_bytes = (long)B * n * 4, c_bytes = (long)B * 12;
  const void* in[3] = {flow, pose, mask};
  const long in_bytes[3] = {(long)B * 2 * n * 4, (long)B * 48, (long)B * n};
  for (int k = 0; k < 3; ++k) {
    if (!in[k]) continue;
    ATDN_CHECK(disjoint(in[k], in_bytes[k], depth, d_bytes), "depth overlaps an input");
    ATDN_CHECK(disjoint(in[k], in_bytes[k], counts, c_bytes), "counts overlaps an input");
  }
  ATDN_CHECK(disjoint(depth, d_bytes, counts, c_bytes), "depth and counts overlap");
}

}  // namespace atdn

using namespace atdn;

int atdn_flow_two_view_depth(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth, float* depth,
                             int* counts, void* stream) {
  try {
    ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
    const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
    two_view_check_args(flow, pose, mask, B, H, W, cam, depth, counts);
    const long n = (long)H * W;
    ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 12, (hipStream_t)stream));
    const dim3 grid((unsigned)cdivl(cdivl(n, 4), TV_THREADS), (unsigned)B);
    if (mask)
      hipLaunchKernelGGL(two_view_kernel<true>, grid, dim3(TV_THREADS), 0, (hipStream_t)stream, flow, pose, mask, H, W, cam, depth,
                         counts);
    else
      hipLaunchKernelGGL(two_view_kernel<false>, grid, dim3(TV_THREADS), 0, (hipStream_t)stream, flow, pose, mask, H, W, cam, depth,
                         counts);
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

int atdn_depth_backproject(const float* depth, int B, int H, int W, double fx, double fy, double cx, double cy, float* points,
                           void* stream) {
  try {
    ATDN_CHECK(depth && points, "null argument");
    ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
    check_camera(B, H, W, fx, fy, cx, cy);
    const long n = (long)H * W;
    ATDN_CHECK(disjoint(depth, (long)B * n * 4, points, (long)B * 3 * n * 4), "depth and points overlap");
    hipLaunchKernelGGL(depth_backproject_kernel, dim3((unsigned)cdivl(n, TV_THREADS), (unsigned)B), dim3(TV_THREADS), 0,
                       (hipStream_t)stream, depth, H, W, fx, fy, cx, cy, points);
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
