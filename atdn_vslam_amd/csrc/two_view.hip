// Two-view geometry on the device: from a flow, a relative pose and the calibration, depth[b, 0, y, x] = the triangulated depth of
// pixel (x, y) in camera 1 (0 where there is none) and counts[b] = (correspondences inside image 2, epipolar inliers, valid
// depths). The rule — float64, every operation rounded on its own — is two_view_pixel of two_view_host.h, which this kernel calls,
// so the kernel and the host form evaluate one function. One memset node and one launch on the caller's stream: asynchronous,
// capturable, no host synchronisation, no workspace; the pose is read from device memory. The counts are integer sums (ballot /
// popcount per wave, the waves of a workgroup through LDS, one integer atomic add per workgroup and counter), so they do not
// depend on the order of arrival: the same bits on every call.
//
// Decomposition. The kernel streams 8 bytes of flow (+ 1 byte of mask) in and 4 bytes out per pixel; the ~110 float64 operations
// of a pixel include ten divisions. The frame is pixel_quads.h: a thread owns four consecutive flat indices 4q .. 4q + 3 of a plane
// (no anchor plane: off = 0): two float4 loads of the flow, one dword of mask, one float4 store, each of the three a vector access
// only where its own address is aligned at the quad.
//
// atdn_depth_backproject below is the pinhole back-projection of a depth map (project_depth of the reference's utils/depth.py for
// a calibration without skew): 4 bytes in, 12 out per pixel, one pixel per thread, coalesced dwords.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "pixel_quads.h"
#include "two_view_host.h"

namespace atdn {

template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void two_view_kernel(const float* __restrict__ flow, const float* __restrict__ pose,
                                                              const unsigned char* __restrict__ mask, int H, int W,
                                                              TwoViewCamera cam, float* __restrict__ depth,
                                                              int* __restrict__ counts) {
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fu = flow + (long)b * 2 * n;
  const float* fv = fu + n;
  float* d = depth + (long)b * n;
  const Quad q = quad_of(n, 0);
  int flags[4] = {0, 0, 0, 0};
  if (q.lo < q.hi) {
    float u[4], v[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool keep[4] = {true, true, true, true};
    quad_load(q, fu, u);
    quad_load(q, fv, v);
    if (MASKED) quad_load(q, mask + (long)b * n, keep);
    const TwoViewPose P = two_view_load_pose(pose + 12 * b);
    int y = q.lo / W, x = q.lo - y * W;                        // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (q.has(k)) {
        if (keep[k]) z[k] = two_view_pixel(u[k], v[k], P, cam, H, W, x, y, &flags[k]);
        if (++x == W) { x = 0; ++y; }
      }
    }
    quad_store(q, d, z);
  }
  const int bits[3] = {TV_INSIDE, TV_INLIER, TV_VALID};
  quad_count<3>(flags, bits, counts + 3 * b);
}

__global__ __launch_bounds__(PQ_THREADS) void depth_backproject_kernel(const float* __restrict__ depth, int H, int W, double fx,
                                                                       double fy, double cx, double cy,
                                                                       float* __restrict__ points) {
#pragma clang fp contract(off)
  const int n = H * W;
  const int i = blockIdx.x * PQ_THREADS + threadIdx.x;
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

// Argument rules shared by the two entry points of atdn_flow_two_view_depth below.
static void two_view_check_args(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W,
                         const TwoViewCamera& cam, const float* depth, const int* counts) {
  ATDN_CHECK(flow && pose && depth && counts, "null argument");
  check_plane_batch(B, H, W, false);
  check_two_view_camera(cam);
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
  ATDN_API_BEGIN
  ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
  const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
  two_view_check_args(flow, pose, mask, B, H, W, cam, depth, counts);
  ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 12, (hipStream_t)stream));
  const dim3 grid(quad_blocks((long)H * W, false), (unsigned)B);
  if (mask)
    hipLaunchKernelGGL(two_view_kernel<true>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, flow, pose, mask, H, W, cam, depth,
                       counts);
  else
    hipLaunchKernelGGL(two_view_kernel<false>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, flow, pose, mask, H, W, cam, depth,
                       counts);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_flow_two_view_depth_host(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W, double fx,
                                  double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth,
                                  float* depth, int* counts) {
  ATDN_API_BEGIN
  const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
  two_view_check_args(flow, pose, mask, B, H, W, cam, depth, counts);
  two_view_depth_host(flow, pose, mask, B, H, W, cam, depth, counts);
  ATDN_API_END
}

int atdn_depth_backproject(const float* depth, int B, int H, int W, double fx, double fy, double cx, double cy, float* points,
                           void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(depth && points, "null argument");
  check_plane_batch(B, H, W);
  check_pinhole(fx, fy, cx, cy);
  const long n = (long)H * W;
  ATDN_CHECK(disjoint(depth, (long)B * n * 4, points, (long)B * 3 * n * 4), "depth and points overlap");
  hipLaunchKernelGGL(depth_backproject_kernel, dim3((unsigned)cdivl(n, PQ_THREADS), (unsigned)B), dim3(PQ_THREADS), 0,
                     (hipStream_t)stream, depth, H, W, fx, fy, cx, cy, points);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}
