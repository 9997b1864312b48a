// Forward-backward consistency of a pair of flows on the device: mask[b, y, x] = 1 where following flow_fw from (x, y) and then
// flow_bw (bilinear) from where it lands returns to the start, and count[b] = the number of ones. The rule — float64, every
// operation rounded on its own — is flow_consistent_pixel of flow_consistency_host.h, which this kernel calls, so the kernel and
// the host form evaluate one function. One memset node and one launch on the caller's stream: asynchronous, capturable, no host
// synchronisation, no workspace. The count is an integer sum (ballot / popcount per wave, the waves of a workgroup through LDS,
// one integer atomic add per workgroup), so it does not depend on the order of arrival: the same bits on every call.
//
// Decomposition. The kernel streams 16 bytes in and 1 byte out per pixel; the four taps of flow_bw are local gathers that stay in
// L2 (the two planes of a 376 x 1232 pair are 3.7 MB), and the ~40 float64 operations per pixel are far off the critical path. The
// frame is pixel_quads.h: a thread owns four consecutive flat indices, two float4 loads of flow_fw, one dword store. The mask plane
// anchors the quads, so the store is a dword for every whole quad; a plane whose flow_fw rows are not 16-byte aligned at the
// quad boundaries takes scalar loads.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "flow_consistency_host.h"
#include "pixel_quads.h"

namespace atdn {

__global__ __launch_bounds__(PQ_THREADS) void flow_consistency_kernel(const float* __restrict__ flow_fw,
                                                                      const float* __restrict__ flow_bw, int H, int W,
                                                                      double alpha1, double alpha2,
                                                                      unsigned char* __restrict__ mask, int* __restrict__ count) {
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fx = flow_fw + (long)b * 2 * n;
  const float* fy = fx + n;
  const float* bx = flow_bw + (long)b * 2 * n;
  const float* by = bx + n;
  unsigned char* m = mask + (long)b * n;
  const Quad q = quad_of(n, (int)((uintptr_t)m & 3));
  int ok[4] = {0, 0, 0, 0};
  if (q.lo < q.hi) {
    float vx[4], vy[4];
    quad_load(q, fx, vx);
    quad_load(q, fy, vy);
    int y = q.lo / W, x = q.lo - y * W;                        // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (q.has(k)) {
        ok[k] = flow_consistent_pixel(vx[k], vy[k], bx, by, H, W, x, y, alpha1, alpha2);
        if (++x == W) { x = 0; ++y; }
      }
    }
    quad_store(q, m, ok, 1);
  }
  const int one[1] = {1};
  quad_count<1>(ok, one, count + b);
}

// Argument rules shared by the two entry points below.
static void flow_consistency_check_args(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                                 const unsigned char* mask, const int* count) {
  ATDN_CHECK(flow_fw && flow_bw && mask && count, "null argument");
  check_plane_batch(B, H, W, false);
  ATDN_CHECK(std::isfinite(alpha1) && std::isfinite(alpha2) && alpha1 >= 0.0 && alpha2 >= 0.0, "alpha1 and alpha2 must be finite and >= 0");
  const long n = (long)H * W;
  const long in_bytes = (long)B * 2 * n * 4, m_bytes = (long)B * n, c_bytes = (long)B * 4;
  for (const float* in : {flow_fw, flow_bw}) {
    ATDN_CHECK(disjoint(in, in_bytes, mask, m_bytes), "mask overlaps an input");
    ATDN_CHECK(disjoint(in, in_bytes, count, c_bytes), "count overlaps an input");
  }
  ATDN_CHECK(disjoint(mask, m_bytes, count, c_bytes), "mask and count overlap");
}

}  // namespace atdn

using namespace atdn;

int atdn_flow_consistency(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                          unsigned char* mask, int* count, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
  flow_consistency_check_args(flow_fw, flow_bw, B, H, W, alpha1, alpha2, mask, count);
  ATDN_HIP(hipMemsetAsync(count, 0, (size_t)B * 4, (hipStream_t)stream));
  hipLaunchKernelGGL(flow_consistency_kernel, dim3(quad_blocks((long)H * W, true), (unsigned)B), dim3(PQ_THREADS), 0,
                     (hipStream_t)stream, flow_fw, flow_bw, H, W, alpha1, alpha2, mask, count);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_flow_consistency_host(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                               unsigned char* mask, int* count) {
  ATDN_API_BEGIN
  flow_consistency_check_args(flow_fw, flow_bw, B, H, W, alpha1, alpha2, mask, count);
  flow_consistency_host(flow_fw, flow_bw, B, H, W, alpha1, alpha2, mask, count);
  ATDN_API_END
}
