// Multi-view keyframe depth on the device: per anchor pixel the inverse depth that best explains its correspondences in the
// listed views of a flow bank (what depth.FlowTrack keeps of its last steps), with its information and its number of inliers.
// The rule — float64, every operation rounded on its own — is multiview_pixel of multiview_depth_host.h, which this kernel
// calls, so the kernel and the host form evaluate one function. One memset node and one launch on the caller's stream:
// asynchronous, capturable, no host synchronisation, no workspace; slots and poses are read from device memory. No atomics on
// the data; the counts are integer sums (pixel_quads.h), the same bits on every call.
//
// Decomposition. Per pixel S * 9 bytes in, 9 out (+ 4 of the initial depth) and (iters + 2) evaluations of S views with four
// float64 divisions each: arithmetic on the float64 pipe, not traffic. ONE pixel per thread, not the four of pixel_quads.h: the
// flows and liveness of the views of a pixel are read once and held over all evaluations, 2 * 16 registers plus a bit mask per
// pixel — four pixels would hold 128 registers before the first float64 temporary. Consecutive lanes own consecutive pixels, so
// a wave reads 256 contiguous bytes per flow plane and view and no access needs an alignment: every plane base and every H * W
// take the same path. The first S threads of the workgroup convert one pose each (pnp_internal_pose, the host's function) into
// LDS, 12 float64 per view, and every thread reads them as broadcasts at constant offsets of the unrolled view loop. The counts
// go through quad_count with one flag per thread (see DESIGN.md for the register figures).
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "multiview_depth_host.h"
#include "pixel_quads.h"

namespace atdn {

__global__ __launch_bounds__(PQ_THREADS) void multiview_depth_kernel(const float* __restrict__ acc_bank,
                                                                     const unsigned char* __restrict__ alive_bank,
                                                                     const float* __restrict__ poses, const int* __restrict__ slots,
                                                                     const float* __restrict__ depth_init, int N, int S, int H, int W,
                                                                     MultiviewParams c, float* __restrict__ depth,
                                                                     float* __restrict__ info, unsigned char* __restrict__ views,
                                                                     int* __restrict__ counts) {
  __shared__ double pose[MV_MAX_VIEWS * MV_POSE];
  __shared__ int slot[MV_MAX_VIEWS];
  const long n = (long)H * W;
  const int b = blockIdx.y;
  if ((int)threadIdx.x < S) multiview_view(poses, slots + (long)b * S, N, (int)threadIdx.x, slot, pose);
  __syncthreads();
  const long p = (long)blockIdx.x * PQ_THREADS + threadIdx.x;
  int flags[4] = {0, 0, 0, 0};
  if (p < n) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const long o = (long)b * n + p;
    float z, ri;
    int vw;
    flags[0] = multiview_pixel(acc_bank, alive_bank, slot, pose, S, n, p, x, y, H, W, depth_init ? depth_init[o] : 0.0f, c, &z, &ri, &vw);
    depth[o] = z;
    info[o] = ri;
    views[o] = (unsigned char)vw;
  }
  const int bits[3] = {MV_CAND, MV_SOLVED, MV_VALID};
  quad_count<3>(flags, bits, counts + 3 * b);
}

// Argument rules shared by the two entry points below (depth_init may be null), and the parameters of the call.
static MultiviewParams multiview_check_args(const float* acc_bank, const unsigned char* alive_bank, const float* poses,
                                            const int* slots, const float* depth_init, int N, int B, int S, int H, int W, double fx,
                                            double fy, double cx, double cy, double scale_px, double inlier_px, double min_z,
                                            int min_views, double max_rel_sigma, double max_depth, int iters, const float* depth,
                                            const float* info, const unsigned char* views, const int* counts) {
  ATDN_CHECK(acc_bank && alive_bank && poses && slots, "null argument");
  const void* out[4] = {depth, info, views, counts};
  check_plane_solver(B, H, W, true, fx, fy, cx, cy, scale_px, inlier_px, out, 4);
  ATDN_CHECK(N >= 1, "the bank is empty (N >= 1)");
  ATDN_CHECK(S >= 1 && S <= MV_MAX_VIEWS, "S must be in [1, ATDN_MULTIVIEW_MAX_VIEWS]");
  ATDN_CHECK(min_views >= 1 && min_views <= S, "min_views must be in [1, S]");
  ATDN_CHECK(iters >= 0 && iters <= 16, "iters must be in [0, 16]");
  ATDN_CHECK(std::isfinite(min_z) && min_z > 0.0, "min_z must be finite and > 0");
  ATDN_CHECK(std::isfinite(max_rel_sigma) && max_rel_sigma > 0.0, "max_rel_sigma must be finite and > 0");
  ATDN_CHECK(std::isfinite(max_depth) && max_depth > 0.0, "max_depth must be finite and > 0");
  const long n = (long)H * W;
  const void* in[5] = {acc_bank, alive_bank, poses, slots, depth_init};
  const long in_bytes[5] = {(long)N * 2 * n * 4, (long)N * n, (long)N * 48, (long)B * S * 4, (long)B * n * 4};
  const long out_bytes[4] = {(long)B * n * 4, (long)B * n * 4, (long)B * n, (long)B * 12};
  check_disjoint(in, in_bytes, 5, out, out_bytes, 4);
  return multiview_params(fx, fy, cx, cy, scale_px, inlier_px, min_z, min_views, max_rel_sigma, max_depth, iters, H, W);
}

}  // namespace atdn

using namespace atdn;

int atdn_multiview_depth(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                         const float* depth_init, int N, int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                         double scale_px, double inlier_px, double min_z, int min_views, double max_rel_sigma, double max_depth,
                         int iters, float* depth, float* info, unsigned char* views, int* counts, void* stream) {
  ATDN_API_BEGIN
  const MultiviewParams c = multiview_check_args(acc_bank, alive_bank, poses, slots, depth_init, N, B, S, H, W, fx, fy, cx, cy,
                                                 scale_px, inlier_px, min_z, min_views, max_rel_sigma, max_depth, iters, depth, info,
                                                 views, counts);
  ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 12, (hipStream_t)stream));
  hipLaunchKernelGGL(multiview_depth_kernel, dim3((unsigned)cdivl((long)H * W, PQ_THREADS), (unsigned)B), dim3(PQ_THREADS), 0,
                     (hipStream_t)stream, acc_bank, alive_bank, poses, slots, depth_init, N, S, H, W, c, depth, info, views, counts);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_multiview_depth_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                              const float* depth_init, int N, int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                              double scale_px, double inlier_px, double min_z, int min_views, double max_rel_sigma, double max_depth,
                              int iters, float* depth, float* info, unsigned char* views, int* counts) {
  ATDN_API_BEGIN
  const MultiviewParams c = multiview_check_args(acc_bank, alive_bank, poses, slots, depth_init, N, B, S, H, W, fx, fy, cx, cy,
                                                 scale_px, inlier_px, min_z, min_views, max_rel_sigma, max_depth, iters, depth, info,
                                                 views, counts);
  multiview_depth_host(acc_bank, alive_bank, poses, slots, depth_init, N, B, S, H, W, c, depth, info, views, counts);
  ATDN_API_END
}
