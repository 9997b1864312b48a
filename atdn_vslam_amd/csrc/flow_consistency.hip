// Forward-backward consistency of a pair of flows on the device: mask[b, y, x] = 1 where following flow_fw from (x, y) and then
// flow_bw (bilinear) from where it lands returns to the start, and count[b] = the number of ones. The rule — float64, every
// operation rounded on its own — is flow_consistent_pixel of flow_consistency_host.h, which this kernel calls, so the kernel and
// the host form evaluate one function. One memset node and one launch on the caller's stream: asynchronous, capturable, no host
// synchronisation, no workspace. The count is an integer sum (ballot / popcount per wave, the waves of a workgroup through LDS,
// one integer atomic add per workgroup), so it does not depend on the order of arrival: the same bits on every call.
//
// Decomposition. The kernel streams 16 bytes in and 1 byte out per pixel; the four taps of flow_bw are local gathers that stay in
// L2 (the two planes of a 376 x 1232 pair are 3.7 MB), and the ~40 float64 operations per pixel are far off the critical path. A
// thread owns one aligned dword of the mask: four consecutive flat indices, two float4 loads of flow_fw, one dword store. The
// quads are cut on the ADDRESS of the mask plane, not on the index: with off = (address of mask[b, 0, 0]) & 3, quad q holds the
// indices 4q - off .. 4q - off + 3 of plane b, so H * W and the plane base of b >= 1 need not be multiples of four. The ragged
// quads at the head and the tail of a plane take byte stores and scalar loads; so does a whole plane whose flow_fw rows are not
// 16-byte aligned at the quad boundaries (scalar loads only — the dword stores stay).
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "common.h"
#include "flow_consistency_host.h"

namespace atdn {

constexpr int FC_THREADS = 256;   // four waves
constexpr int FC_WAVES = FC_THREADS / 64;

__global__ __launch_bounds__(FC_THREADS) void flow_consistency_kernel(const float* __restrict__ flow_fw,
                                                                      const float* __restrict__ flow_bw, int H, int W,
                                                                      double alpha1, double alpha2,
                                                                      unsigned char* __restrict__ mask, int* __restrict__ count) {
  __shared__ int partial[FC_WAVES];
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fx = flow_fw + (long)b * 2 * n;
  const float* fy = fx + n;
  const float* bx = flow_bw + (long)b * 2 * n;
  const float* by = bx + n;
  unsigned char* m = mask + (long)b * n;
  const int off = (int)((uintptr_t)m & 3);
  const int q = blockIdx.x * FC_THREADS + threadIdx.x;
  const int s0 = 4 * q - off;                                  // first index of the quad: -3 .. n + 2 (n <= 2^24)
  const int lo = s0 > 0 ? s0 : 0, hi = s0 + 4 < n ? s0 + 4 : n;
  const bool full = hi - lo == 4;
  // the same answer for every quad of a plane: s0 advances by four floats
  const bool wide = (((uintptr_t)fx + 4 * (long)s0) & 15) == 0 && (((uintptr_t)fy + 4 * (long)s0) & 15) == 0;
  bool r[4] = {false, false, false, false};
  if (lo < hi) {
    float vx[4], vy[4];
    if (full && wide) {
      const float4 a = *reinterpret_cast<const float4*>(fx + s0);
      const float4 c = *reinterpret_cast<const float4*>(fy + s0);
      vx[0] = a.x; vx[1] = a.y; vx[2] = a.z; vx[3] = a.w;
      vy[0] = c.x; vy[1] = c.y; vy[2] = c.z; vy[3] = c.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = s0 + k;
        const bool in = i >= lo && i < hi;
        vx[k] = in ? fx[i] : 0.0f;
        vy[k] = in ? fy[i] : 0.0f;
      }
    }
    int y = lo / W, x = lo - y * W;                            // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = s0 + k;
      if (i >= lo && i < hi) {
        r[k] = flow_consistent_pixel(vx[k], vy[k], bx, by, H, W, x, y, alpha1, alpha2);
        if (++x == W) { x = 0; ++y; }
      }
    }
    if (full) {
      *reinterpret_cast<uint32_t*>(m + s0) = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = s0 + k;
        if (i >= lo && i < hi) m[i] = r[k] ? 1 : 0;
      }
    }
  }
  // every lane of a wave gets the wave's number of ones; lane 0 hands it to LDS
  int ones = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) ones += __popcll(__ballot(r[k]));
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = ones;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < FC_WAVES; ++w) total += partial[w];
    if (total) atomicAdd(count + b, total);
  }
}

// Argument rules shared by the device entry point below and the host one (capi.hip).
void flow_consistency_check_args(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                                 const unsigned char* mask, const int* count) {
  ATDN_CHECK(flow_fw && flow_bw && mask && count, "null argument");
  ATDN_CHECK(B >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
  ATDN_CHECK(std::isfinite(alpha1) && std::isfinite(alpha2) && alpha1 >= 0.0 && alpha2 >= 0.0, "alpha1 and alpha2 must be finite and >= 0");
  const long n = (long)H * W;
  const char* m0 = (const char*)mask;
  const char* c0 = (const char*)count;
  const long in_bytes = (long)B * 2 * n * 4, m_bytes = (long)B * n, c_bytes = (long)B * 4;
  for (const char* in : {(const char*)flow_fw, (const char*)flow_bw}) {
    ATDN_CHECK(in + in_bytes <= m0 || m0 + m_bytes <= in, "mask overlaps an input");
    ATDN_CHECK(in + in_bytes <= c0 || c0 + c_bytes <= in, "count overlaps an input");
  }
  ATDN_CHECK(m0 + m_bytes <= c0 || c0 + c_bytes <= m0, "mask and count overlap");
}

}  // namespace atdn

using namespace atdn;

int atdn_flow_consistency(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                          unsigned char* mask, int* count, void* stream) {
  try {
    ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
    flow_consistency_check_args(flow_fw, flow_bw, B, H, W, alpha1, alpha2, mask, count);
    const long n = (long)H * W, c_bytes = (long)B * 4;
    ATDN_HIP(hipMemsetAsync(count, 0, (size_t)c_bytes, (hipStream_t)stream));
    const long quads = (n + 3) / 4 + 1;                        // off <= 3 moves the last index into one more quad at most
    hipLaunchKernelGGL(flow_consistency_kernel, dim3((unsigned)cdivl(quads, FC_THREADS), (unsigned)B), dim3(FC_THREADS), 0,
                       (hipStream_t)stream, flow_fw, flow_bw, H, W, alpha1, alpha2, mask, count);
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
