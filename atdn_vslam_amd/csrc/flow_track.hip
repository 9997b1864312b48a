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
// is ~30 float64 operations per pixel, the depth part the ~110 of two_view_pixel. The frame is pixel_quads.h: a thread owns four
// consecutive flat indices, and the alive_out plane anchors the quads, so its store is a dword for every whole quad. Every other
// access of the quad — acc_in and acc_out (two float4 each), alive_in (a dword), depth (a float4 in, a float4 out) — is a vector
// access only where its own address is aligned at the quad.
// A thread reads the state of its own four pixels before it writes them and reads no other pixel's state, so acc_out == acc_in and
// alive_out == alive_in are safe; depth is read only to keep the values of the pixels that are not valid in a float4 store, and a
// quad without a valid pixel stores no depth at all.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "flow_track_host.h"
#include "pixel_quads.h"

namespace atdn {

// acc_in / acc_out and alive_in / alive_out may be the same buffers: no __restrict__ on them
template <bool DEPTH>
__global__ __launch_bounds__(PQ_THREADS) void flow_track_kernel(const float* __restrict__ flow, const unsigned char* __restrict__ mask,
                                                                const float* acc_in, const unsigned char* alive_in, int H, int W,
                                                                float* acc_out, unsigned char* alive_out,
                                                                const float* __restrict__ pose, TwoViewCamera cam, float* depth,
                                                                int* __restrict__ counts) {
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
  const Quad q = quad_of(n, (int)((uintptr_t)lv & 3));
  int flags[4] = {0, 0, 0, 0};
  if (q.lo < q.hi) {
    float ux[4], uy[4], px[4], py[4], z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool live[4];
    quad_load(q, ix, ux);
    quad_load(q, iy, uy);
    quad_load(q, li, live);
    float* d = nullptr;
    TwoViewPose P{};
    if (DEPTH) {
      d = depth + (long)b * n;
      quad_load(q, d, z);
      P = two_view_load_pose(pose + 12 * b);
    }
    int y = q.lo / W, x = q.lo - y * W;                        // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = ux[k];
      py[k] = uy[k];
      if (q.has(k)) {
        flags[k] = flow_track_pixel<DEPTH>(ux[k], uy[k], live[k], fx, fy, m, H, W, x, y, &P, &cam, &px[k], &py[k], &z[k]);
        if (++x == W) { x = 0; ++y; }
      }
    }
    quad_store(q, ox, px);
    quad_store(q, oy, py);
    quad_store(q, lv, flags, FT_ALIVE);
    if (DEPTH && ((flags[0] | flags[1] | flags[2] | flags[3]) & TV_VALID)) quad_store(q, d, z);
  }
  const int bits[4] = {FT_ALIVE, TV_INSIDE, TV_INLIER, TV_VALID};
  quad_count<DEPTH ? 4 : 1>(flags, bits, counts + 4 * b);      // without a pose no TV_* bit is ever set: those counts stay zero
}

// Argument rules shared by the two entry points below.
static void flow_track_check_args(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in, int B,
                           int H, int W, const float* acc_out, const unsigned char* alive_out, const float* pose,
                           const TwoViewCamera& cam, const float* depth, const int* counts) {
  ATDN_CHECK(flow && acc_in && alive_in && acc_out && alive_out && counts, "null argument");
  check_plane_batch(B, H, W);
  if (pose) {
    ATDN_CHECK(depth, "a pose needs a depth map");
    check_two_view_camera(cam);
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
  ATDN_API_BEGIN
  const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
  flow_track_check_args(flow, mask, acc_in, alive_in, B, H, W, acc_out, alive_out, pose, cam, depth, counts);
  ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 16, (hipStream_t)stream));
  const dim3 grid(quad_blocks((long)H * W, true), (unsigned)B);
  if (pose)
    hipLaunchKernelGGL(flow_track_kernel<true>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, flow, mask, acc_in, alive_in, H, W,
                       acc_out, alive_out, pose, cam, depth, counts);
  else
    hipLaunchKernelGGL(flow_track_kernel<false>, grid, dim3(PQ_THREADS), 0, (hipStream_t)stream, flow, mask, acc_in, alive_in, H, W,
                       acc_out, alive_out, pose, cam, depth, counts);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_flow_track_step_host(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in,
                              int B, int H, int W, float* acc_out, unsigned char* alive_out, const float* pose, double fx,
                              double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth, float* depth,
                              int* counts) {
  ATDN_API_BEGIN
  const TwoViewCamera cam{fx, fy, cx, cy, max_epipolar, min_sin2, max_depth};
  flow_track_check_args(flow, mask, acc_in, alive_in, B, H, W, acc_out, alive_out, pose, cam, depth, counts);
  flow_track_step_host(flow, mask, acc_in, alive_in, B, H, W, acc_out, alive_out, pose, cam, depth, counts);
  ATDN_API_END
}
