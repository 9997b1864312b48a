// Flow bank kernels: the fp16 training set of CLVO kept in HBM (atdn_vslam_amd/flowbank.py).
//
// * atdn_flow_pack_f16: fp32 flow_up of the flow network -> fp16 bank slots, `tensor.half()` of a column window
//   (what the reference's flow files hold, FlowKittiDataset3 reads them, datasets.py:176-189).
// * atdn_flow_gather_clips: bank slots -> the fp32 [B,T,2,H,W] batch of atdn_clvo_trainer_forward_backward, with the
//   reverse-flow augmentation of FlowKittiDataset3.__getitem__ (datasets.py:220-224) folded in.
//
// Both are memory-bound copies: every lane moves 16 bytes of fp16 (8 values) per access, the fp32 side as 2 x 16 bytes.
// Conversions are plain casts (round to nearest even, NaN stays NaN, overflow to +-inf: what torch's cast does) and the
// decode + negation are exact, so both match their torch expressions bit for bit.
#include "../../include/atdn_hip.h"

#include <vector>

#include "common.h"

namespace atdn {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// rows of W columns of an fp32 [rows, Wsrc] array starting at column x0 -> fp16 [rows, W]; W % 8 == 0.
// ALIGNED: the source window starts 16-byte aligned in every row (x0 % 4 == 0, Wsrc % 4 == 0, aligned base).
template <bool ALIGNED>
__global__ __launch_bounds__(256) void flow_pack_f16_kernel(const float* __restrict__ src, long rows, int Wsrc, int x0, int W,
                                                            _Float16* __restrict__ dst) {
  const int vpr = W >> 3;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * vpr) return;
  const long row = i / vpr;
  const int c = (int)(i - row * vpr) << 3;
  const float* s = src + row * Wsrc + x0 + c;
  float v[8];
  if (ALIGNED) {
    const float4 a = *reinterpret_cast<const float4*>(s);
    const float4 b = *reinterpret_cast<const float4*>(s + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = s[k];
  }
  half8 h;
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = (_Float16)v[k];
  *reinterpret_cast<half8*>(dst + row * W + c) = h;
}

// one launch covers up to GATHER_MAX frames of the output; entry f of the table is the bank slot of output frame f0 + f,
// with bit 31 set when that frame is negated. The table travels by value in the kernel arguments.
constexpr int GATHER_MAX = 512;
struct GatherTable {
  unsigned slot[GATHER_MAX];
};

__global__ __launch_bounds__(256) void flow_gather_kernel(const _Float16* __restrict__ bank, long per, const GatherTable tab,
                                                          float* __restrict__ out) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;   // 8-value vector within the frame
  if (v * 8 >= per) return;
  const unsigned e = tab.slot[blockIdx.y];
  const long slot = (long)(e & 0x7FFFFFFFu);
  const half8 h = *reinterpret_cast<const half8*>(bank + slot * per + v * 8);
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = (float)h[k];
  if (e >> 31) {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = -f[k];
  }
  float4* d = reinterpret_cast<float4*>(out + (long)blockIdx.y * per + v * 8);
  d[0] = make_float4(f[0], f[1], f[2], f[3]);
  d[1] = make_float4(f[4], f[5], f[6], f[7]);
}

}  // namespace atdn

using namespace atdn;

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int atdn_flow_pack_f16(const float* flow_up, int B, int H, int Wsrc, int x0, int W, uint16_t* dst, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(flow_up && dst && B >= 1 && H >= 1 && W >= 8, "bad argument");
  ATDN_CHECK(W % 8 == 0, "the bank width must be a multiple of 8");
  ATDN_CHECK(x0 >= 0 && (long)x0 + W <= Wsrc, "column window [x0, x0+W) outside the source rows");
  ATDN_CHECK(aligned16(dst), "the destination slot must be 16-byte aligned");
  const long rows = (long)B * 2 * H;
  const long n = rows * (W / 8);
  ATDN_CHECK(n <= (long)0x7FFFFFFF * 256, "flow too large");
  const bool al = x0 % 4 == 0 && Wsrc % 4 == 0 && aligned16(flow_up);
  const dim3 grid((unsigned)cdivl(n, 256));
  _Float16* d = reinterpret_cast<_Float16*>(dst);
  if (al) hipLaunchKernelGGL((flow_pack_f16_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, flow_up, rows, Wsrc, x0, W, d);
  else hipLaunchKernelGGL((flow_pack_f16_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, flow_up, rows, Wsrc, x0, W, d);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_flow_gather_clips(const uint16_t* bank, int n_flows, int H, int W, const int* start, const int* reverse, int B, int T,
                           float* out, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(bank && start && reverse && out && n_flows >= 1 && H >= 1 && W >= 1 && B >= 1 && T >= 1, "bad argument");
  const long per = 2L * H * W;
  ATDN_CHECK(per % 8 == 0, "H * W must be a multiple of 4 (16-byte frames)");
  ATDN_CHECK(aligned16(bank) && aligned16(out), "bank and output must be 16-byte aligned");
  ATDN_CHECK(T <= n_flows, "clip longer than the bank");
  // every index is checked on the host before anything is launched: no slot outside the bank can reach the device
  std::vector<unsigned> slots((size_t)B * T);
  for (int b = 0; b < B; ++b) {
    if (start[b] < 0 || start[b] > n_flows - T) {
      char msg[160];
      snprintf(msg, sizeof msg, "clip %d: start %d outside [0, %d] (bank of %d flows, clips of %d)", b, start[b], n_flows - T,
               n_flows, T);
      throw Error(msg);
    }
    const bool rev = reverse[b] != 0;
    for (int t = 0; t < T; ++t)
      slots[(size_t)b * T + t] = (unsigned)(rev ? start[b] + T - 1 - t : start[b] + t) | (rev ? 0x80000000u : 0u);
  }
  const unsigned gx = (unsigned)cdivl(per / 8, 256);
  const long frames = (long)B * T;
  for (long f0 = 0; f0 < frames; f0 += GATHER_MAX) {
    const int nf = (int)std::min<long>(GATHER_MAX, frames - f0);
    GatherTable tab;
    for (int f = 0; f < GATHER_MAX; ++f) tab.slot[f] = f < nf ? slots[f0 + f] : 0u;
    hipLaunchKernelGGL(flow_gather_kernel, dim3(gx, (unsigned)nf), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const _Float16*>(bank),
                       per, tab, out + f0 * per);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}
