// See conv16.h: conv16_kernel, stem16_kernel and tconv16_s2_kernel with their launchers. Forward passes, eval-mode tails and data
// gradients of every 16-channel convolution of the CLVO encoder, for the inference head (clvo.hip) and the trainer (clvo_train.hip).
#include "conv16.h"

#include "common.h"
#include "mish.h"

namespace atdn {
namespace {
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int c16_pitch(int S) { return S == 1 ? 16 : S == 2 ? 20 : 24; }   // floats per patch pixel: conflict-free b128 reads

// Eval-mode tail of a CLVO block fused into the store (inference head, clvo.hip): TAIL 0 = none (z = acc + bias: the
// training forward, whose BatchNorm needs batch statistics first), 1 = BN(Mish(.)) with the folded affine, 2 = the
// ResidualConv tail BN2(Mish(BN1(Mish(.)) + skip)). Per-channel constants live in registers (channel = lane & 15).
struct C16Consts { float sc, sh, sc2, sh2; };
template <int TAIL>
__device__ __forceinline__ C16Consts c16_consts(const Conv16Tail& t, int n) {
  C16Consts c{1.f, 0.f, 1.f, 0.f};
  if constexpr (TAIL >= 1) { c.sc = t.sc[n]; c.sh = t.sh[n]; }
  if constexpr (TAIL == 2) { c.sc2 = t.sc2[n]; c.sh2 = t.sh2[n]; }
  return c;
}
// mish(x) = x tanh(softplus(x)) = x t / (t + 2) with t = e^x (e^x + 2): one v_exp_f32 and one v_rcp_f32 instead of the
// expf / log1pf / tanhf chain of mishf_ (for x > 20 the ratio is 1 in fp32; for x -> -inf it tends to e^x with full relative
// accuracy). The inference head spent a third of its time in these tails: encoder 0.80 -> 0.50 ms per 16 pairs; features agree
// with the libm form to 1.4e-7 relative (checksum of 16 x 512 features), golden poses within their 1e-5 (round 4). Training
// (TAIL 0 + separate BatchNorm / Mish kernels) keeps mishf_.
__device__ __forceinline__ float mish_tail_(float x) {
  const float n = __builtin_amdgcn_exp2f(fminf(x, 20.f) * 1.4426950408889634f);
  const float t = n * (n + 2.f);
  return x * (t * __builtin_amdgcn_rcpf(t + 2.f));
}
template <int TAIL>
__device__ __forceinline__ float c16_tail(float v, const C16Consts& c, const float* skip, long o) {
  if constexpr (TAIL == 0) return v;
  const float y = mish_tail_(v) * c.sc + c.sh;
  if constexpr (TAIL == 1) return y;
  return mish_tail_(y + skip[o]) * c.sc2 + c.sh2;
}

// Training forward (TAIL 0) with `st.part` set: the sums of Mish(z) and Mish(z)^2 per (statistics group, channel) that the
// BatchNorm behind the convolution needs (layers/conv.py:38: bn(activation(conv(x)))) are taken from the values on their way
// to memory — the separate pass that re-read z for them was 9 % of a training iteration. A lane keeps the sums of its four
// channels while the block's tiles stay in one group (group = image / st.group_imgs: the images of one time step) and the
// block writes ONE partial row per group it met: part[group][block][2][16] (zeroed by the launcher; bn_finalize adds the rows
// in double, in a fixed order: no atomics).
struct C16StatAcc {
  float s1[4], s2[4];
  int grp;
};
__device__ __forceinline__ void c16_stat_flush(C16StatAcc& a, const Conv16Stats& st, float (*sred)[2][16]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { a.s1[e] += __shfl_xor(a.s1[e], m); a.s2[e] += __shfl_xor(a.s2[e], m); }
    if (n == 0) { sred[wave][0][4 * g + e] = a.s1[e]; sred[wave][1][4 * g + e] = a.s2[e]; }
    a.s1[e] = 0.f; a.s2[e] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int which = threadIdx.x >> 4, ch = threadIdx.x & 15;
    const float t = (sred[0][which][ch] + sred[1][which][ch]) + (sred[2][which][ch] + sred[3][which][ch]);
    st.part[(((long)a.grp * gridDim.x + blockIdx.x) * 2 + which) * 16 + ch] = t;
  }
  __syncthreads();
}

// K operand order: MFMA (tap, j) holds channel 4g + j in k-slot g = lane >> 4, so a lane's float4 (channels 4g..4g+3 of
// its pixel) feeds the four MFMAs of a tap component by component.
template <int K, int S, int TH, int TW, int TAIL = 0>
__global__ __launch_bounds__(256) void conv16_kernel(const float* __restrict__ x, int nimg, int H, int W,
                                                     const float* __restrict__ w, int transposed,
                                                     const float* __restrict__ bias, int pad, int Ho, int Wo,
                                                     float* __restrict__ z, int tiles_x, int tiles_img, int ntiles,
                                                     int accumulate, const Conv16Tail tail, const Conv16Stats stat) {
  constexpr int PH = (TH - 1) * S + K, PW = (TW - 1) * S + K, PP = c16_pitch(S);
  __shared__ __attribute__((aligned(16))) float patch[PH * PW * PP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // weights into operand registers once per (persistent) block: breg[tap][j] = w(n = lane & 15, c = 4*(lane >> 4) + j, tap)
  const int n = lane & 15, g = lane >> 4;
  float breg[K * K][4];
#pragma unroll
  for (int tap = 0; tap < K * K; ++tap)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * g + j;
      breg[tap][j] = transposed ? w[((long)c * 16 + n) * K * K + (K * K - 1 - tap)] : w[((long)n * 16 + c) * K * K + tap];
    }
  // Round 5: the weights are the ROW operand and the patch the COLUMN operand, so D comes out as (row = output channel 4g + e,
  // column = pixel lane & 15): a lane holds four consecutive channels of ONE pixel and stores 16 bytes, a wave one contiguous KiB
  // (the other way round every store instruction wrote four 64-byte pieces, 4 bytes per lane). Same products, same sums.
  float bv[4];
  C16Consts cc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { bv[e] = bias ? bias[4 * g + e] : 0.f; cc[e] = c16_consts<TAIL>(tail, 4 * g + e); }
  constexpr int TILES = TH * TW / 16, TPR = TW / 16;   // 16-pixel MFMA tiles of the block tile; per row
  static_assert(TILES % 2 == 0, "two tiles per wave and trip");
  // the patch of the next block tile is fetched into registers while this one is computed
  constexpr int NV = PH * PW * 4, NF = (NV + 255) / 256;
  float4 pre[NF];
  auto fetch = [&](int bt) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int iy0 = (tloc / tiles_x) * TH * S - pad, ix0 = (tloc % tiles_x) * TW * S - pad;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f;
      const int q = i & 3, px = (i >> 2) % PW, py = (i >> 2) / PW;
      const int iy = iy0 + py, ix = ix0 + px;
      pre[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < NV && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        pre[f] = *reinterpret_cast<const float4*>(x + (((long)img * H + iy) * W + ix) * 16 + 4 * q);
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  __shared__ float sred[4][2][16];
  C16StatAcc sa{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, -1};
  const bool stats = TAIL == 0 && stat.part != nullptr;
  for (int bt = blockIdx.x; bt < ntiles; bt += gridDim.x) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int oy0 = (tloc / tiles_x) * TH, ox0 = (tloc % tiles_x) * TW;
    if (stats) {   // (uniform over the block: every thread walks the same tiles)
      const int grp = img / stat.group_imgs;
      if (grp != sa.grp) {
        if (sa.grp >= 0) c16_stat_flush(sa, stat, sred);
        sa.grp = grp;
      }
    }
    __syncthreads();   // everyone is done with the previous patch
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f;
      if (i < NV) *reinterpret_cast<float4*>(patch + ((i >> 2) / PW * PW + (i >> 2) % PW) * PP + 4 * (i & 3)) = pre[f];
    }
    __syncthreads();
    if (bt + (int)gridDim.x < ntiles) fetch(bt + gridDim.x);
    for (int t = 2 * wave; t < TILES; t += 8) {   // two independent accumulation chains per wave
      const int ty0 = t / TPR, tx0 = (t % TPR) * 16, ty1 = (t + 1) / TPR, tx1 = ((t + 1) % TPR) * 16;
      f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      // in the patch operand lane & 15 is the pixel of the row
      const float* b0 = patch + ((ty0 * S) * PW + (tx0 + n) * S) * PP + 4 * g;
      const float* b1 = patch + ((ty1 * S) * PW + (tx1 + n) * S) * PP + 4 * g;
#pragma unroll
      for (int tap = 0; tap < K * K; ++tap) {
        const int off = ((tap / K) * PW + (tap % K)) * PP;
        const float4 a0 = *reinterpret_cast<const float4*>(b0 + off);
        const float4 a1 = *reinterpret_cast<const float4*>(b1 + off);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][0], a0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][0], a1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][1], a0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][1], a1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][2], a0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][2], a1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][3], a0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][3], a1.w, acc1, 0, 0, 0);
      }
      // D: row (output channel) = 4*g + e, column (pixel) = lane & 15
      auto put = [&](const f32x4_t& acc, int oy, int ox) __attribute__((always_inline)) {
        if (oy >= Ho || ox >= Wo) return;
        const long o = (((long)img * Ho + oy) * Wo + ox) * 16 + 4 * g;
        float4* pz = reinterpret_cast<float4*>(z + o);
        float v[4];
        if constexpr (TAIL == 0) {
          float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
          if (accumulate) old = *pz;
          const float od[4] = {old.x, old.y, old.z, old.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = acc[e] + bv[e] + od[e];
          if (stats) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float m = mish_fast(v[e]); sa.s1[e] += m; sa.s2[e] += m * m; }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = c16_tail<TAIL>(acc[e] + bv[e], cc[e], tail.skip, o + e);
        }
        *pz = make_float4(v[0], v[1], v[2], v[3]);
      };
      put(acc0, oy0 + ty0, ox0 + tx0 + n);
      put(acc1, oy0 + ty1, ox0 + tx1 + n);
    }
  }
  if (stats && sa.grp >= 0) c16_stat_flush(sa, stat, sred);
}

template <int K, int S, int TH, int TW, int TAIL = 0>
void conv16_launch(const float* x, int nimg, int H, int W, const float* w, bool transposed, const float* bias, int pad,
                   float* z, bool accumulate, hipStream_t st, const Conv16Tail& tail = Conv16Tail{}, Conv16Stats* stat = nullptr) {
  const int Ho = (H + 2 * pad - K) / S + 1, Wo = (W + 2 * pad - K) / S + 1;
  const int tx = cdiv(Wo, TW), ty = cdiv(Ho, TH);
  const int ntiles = nimg * tx * ty;
  const int grid = ntiles < 256 * 3 ? ntiles : 256 * 3;   // persistent blocks: the weights are loaded into registers once
  Conv16Stats sv;
  if (stat && stat->part) {
    ATDN_CHECK(TAIL == 0 && !accumulate && stat->group_imgs >= 1 && nimg % stat->group_imgs == 0, "conv16 statistics: plain training forward only");
    const int groups = nimg / stat->group_imgs;
    ATDN_CHECK((long)groups * grid * 32 <= stat->capacity, "conv16 statistics: partial buffer too small");
    ATDN_HIP(hipMemsetAsync(stat->part, 0, (size_t)groups * grid * 32 * sizeof(float), st));   // blocks write the groups they meet
    stat->rows = grid;
    sv = *stat;
  }
  hipLaunchKernelGGL((conv16_kernel<K, S, TH, TW, TAIL>), dim3(grid), dim3(256), 0, st, x, nimg, H, W, w, transposed ? 1 : 0, bias,
                     pad, Ho, Wo, z, tx, tx * ty, ntiles, accumulate ? 1 : 0, tail, sv);
  ATDN_HIP(hipGetLastError());
}
}  // namespace

// Stem of the CLVO encoder: 7x7, stride 2, pad 3, 2 -> 16 channels on NHWC4 input (channels 2, 3 unused). A patch row in
// LDS holds (column, channel) pairs back to back, so the 14 (kx, c) products of one kernel row of one output pixel are 14
// consecutive floats starting at 4*px: four MFMAs per kernel row (k-slot g of MFMA j = pair index 4g + j, the last two
// pairs carry zero weights) fed by one ds_read_b128.
namespace {
constexpr int ST_TH = 8, ST_TW = 64, ST_PH = (ST_TH - 1) * 2 + 7, ST_PWC = (ST_TW - 1) * 2 + 8, ST_ROWP = ST_PWC * 2;
template <int TAIL>
__global__ __launch_bounds__(256) void stem16_kernel(const float* __restrict__ x, int nimg, int H, int W,
                                                     const float* __restrict__ w /*[16][2][7][7]*/,
                                                     const float* __restrict__ bias, int Ho, int Wo, float* __restrict__ z,
                                                     int tiles_x, int tiles_img, int ntiles, const Conv16Tail tail,
                                                     const Conv16Stats stat) {
  __shared__ __attribute__((aligned(16))) float patch[ST_PH * ST_ROWP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
  float breg[7][4];
#pragma unroll
  for (int ky = 0; ky < 7; ++ky)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = 4 * g + j, kx = f >> 1, c = f & 1;
      breg[ky][j] = kx < 7 ? w[(((long)n * 2 + c) * 7 + ky) * 7 + kx] : 0.f;
    }
  float bv[4];   // (weights as the row operand: a lane ends up with channels 4g..4g+3 of one pixel, see conv16_kernel)
  C16Consts cc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { bv[e] = bias ? bias[4 * g + e] : 0.f; cc[e] = c16_consts<TAIL>(tail, 4 * g + e); }
  constexpr int NV = ST_PH * ST_PWC, NF = (NV + 255) / 256;
  float2 pre[NF];
  auto fetch = [&](int bt) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int iy0 = (tloc / tiles_x) * ST_TH * 2 - 3, ix0 = (tloc % tiles_x) * ST_TW * 2 - 3;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f, px = i % ST_PWC, py = i / ST_PWC;
      const int iy = iy0 + py, ix = ix0 + px;
      pre[f] = make_float2(0.f, 0.f);
      if (i < NV && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        pre[f] = *reinterpret_cast<const float2*>(x + (((long)img * H + iy) * W + ix) * 4);
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  constexpr int TILES = ST_TH * ST_TW / 16, TPR = ST_TW / 16;
  __shared__ float sred[4][2][16];
  C16StatAcc sa{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, -1};
  const bool stats = TAIL == 0 && stat.part != nullptr;
  for (int bt = blockIdx.x; bt < ntiles; bt += gridDim.x) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int oy0 = (tloc / tiles_x) * ST_TH, ox0 = (tloc % tiles_x) * ST_TW;
    if (stats) {
      const int grp = img / stat.group_imgs;
      if (grp != sa.grp) {
        if (sa.grp >= 0) c16_stat_flush(sa, stat, sred);
        sa.grp = grp;
      }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f;
      if (i < NV) *reinterpret_cast<float2*>(patch + (i / ST_PWC) * ST_ROWP + (i % ST_PWC) * 2) = pre[f];
    }
    __syncthreads();
    if (bt + (int)gridDim.x < ntiles) fetch(bt + gridDim.x);
    for (int t = 2 * wave; t < TILES; t += 8) {
      const int ty0 = t / TPR, tx0 = (t % TPR) * 16, ty1 = (t + 1) / TPR, tx1 = ((t + 1) % TPR) * 16;
      f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const float* b0 = patch + (ty0 * 2) * ST_ROWP + 4 * (tx0 + n) + 4 * g;   // lane & 15 = pixel of the patch operand
      const float* b1 = patch + (ty1 * 2) * ST_ROWP + 4 * (tx1 + n) + 4 * g;
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const float4 a0 = *reinterpret_cast<const float4*>(b0 + ky * ST_ROWP);
        const float4 a1 = *reinterpret_cast<const float4*>(b1 + ky * ST_ROWP);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][0], a0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][0], a1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][1], a0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][1], a1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][2], a0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][2], a1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][3], a0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[ky][3], a1.w, acc1, 0, 0, 0);
      }
      auto put = [&](const f32x4_t& acc, int oy, int ox) __attribute__((always_inline)) {
        if (oy >= Ho || ox >= Wo) return;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c16_tail<TAIL>(acc[e] + bv[e], cc[e], nullptr, 0);
        *reinterpret_cast<float4*>(z + (((long)img * Ho + oy) * Wo + ox) * 16 + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
        if (stats) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float m = mish_fast(v[e]); sa.s1[e] += m; sa.s2[e] += m * m; }
        }
      };
      put(acc0, oy0 + ty0, ox0 + tx0 + n);
      put(acc1, oy0 + ty1, ox0 + tx1 + n);
    }
  }
  if (stats && sa.grp >= 0) c16_stat_flush(sa, stat, sred);
}
}  // namespace

void launch_stem16(const float* x4, int nimg, int H, int W, const float* w, const float* bias, float* z, hipStream_t st,
                   const Conv16Tail* tail, Conv16Stats* stat) {
  const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
  const int tx = cdiv(Wo, ST_TW), ty = cdiv(Ho, ST_TH), ntiles = nimg * tx * ty;
  const int grid = ntiles < 256 * 4 ? ntiles : 256 * 4;
  if (tail) {
    ATDN_CHECK(tail->sc && tail->sh && !tail->skip, "stem tail is BN(Mish(.))");
    ATDN_CHECK(!stat || !stat->part, "stem statistics: training forward only");
    hipLaunchKernelGGL(stem16_kernel<1>, dim3(grid), dim3(256), 0, st, x4, nimg, H, W, w, bias, Ho, Wo, z, tx, tx * ty, ntiles, *tail,
                       Conv16Stats{});
  } else {
    Conv16Stats sv;
    if (stat && stat->part) {
      ATDN_CHECK(stat->group_imgs >= 1 && nimg % stat->group_imgs == 0, "stem statistics: whole groups of images");
      const int groups = nimg / stat->group_imgs;
      ATDN_CHECK((long)groups * grid * 32 <= stat->capacity, "stem statistics: partial buffer too small");
      ATDN_HIP(hipMemsetAsync(stat->part, 0, (size_t)groups * grid * 32 * sizeof(float), st));
      stat->rows = grid;
      sv = *stat;
    }
    hipLaunchKernelGGL(stem16_kernel<0>, dim3(grid), dim3(256), 0, st, x4, nimg, H, W, w, bias, Ho, Wo, z, tx, tx * ty, ntiles,
                       Conv16Tail{}, sv);
  }
  ATDN_HIP(hipGetLastError());
}

// Data gradient of a stride-2 16 -> 16 convolution without the zero-stuffed map: dx[y][x][c] = sum over the taps whose
// source (y + PAD - ky)/2, (x + PAD - kx)/2 is integral. Output pixels of one row and one column parity share their tap
// list (1, 2, 2 or 4 taps for 3x3), and 16 of them read 16 consecutive dz columns, so each parity class is a small
// stride-1 convolution on the dz patch. Wave w owns rows 2w and 2w+1 of the 8 x 64 tile (every class once).
namespace {
template <int K, int PAD>
__global__ __launch_bounds__(256) void tconv16_s2_kernel(const float* __restrict__ dz, int nimg, int Ho, int Wo,
                                                         const float* __restrict__ w, int H, int W, int accumulate,
                                                         float* __restrict__ dx, int tiles_x, int tiles_img, int ntiles) {
  constexpr int TH = 8, TW = 64, PH = TH / 2 + 2, PW = TW / 2 + 2;
  __shared__ __attribute__((aligned(16))) float patch[PH * PW * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = lane & 15, g = lane >> 4;
  float breg[K * K][4];   // contraction over n: slot g of MFMA j = output channel 4g + j; row = input channel idx
#pragma unroll
  for (int tap = 0; tap < K * K; ++tap)
#pragma unroll
    for (int j = 0; j < 4; ++j) breg[tap][j] = w[((long)(4 * g + j) * 16 + idx) * K * K + tap];
  constexpr int NV = PH * PW * 4, NF = (NV + 255) / 256;
  float4 pre[NF];
  auto fetch = [&](int bt) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int oyb = (tloc / tiles_x) * (TH / 2) - 1, oxb = (tloc % tiles_x) * (TW / 2) - 1;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pc = (i >> 2) % PW, pr = (i >> 2) / PW;
      const int oy = oyb + pr, ox = oxb + pc;
      pre[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < NV && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo)
        pre[f] = *reinterpret_cast<const float4*>(dz + (((long)img * Ho + oy) * Wo + ox) * 16 + 4 * q);
    }
  };
  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int bt = blockIdx.x; bt < ntiles; bt += gridDim.x) {
    const int img = bt / tiles_img, tloc = bt - img * tiles_img;
    const int y0 = (tloc / tiles_x) * TH, x0 = (tloc % tiles_x) * TW;
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int i = tid + 256 * f;
      if (i < NV) *reinterpret_cast<float4*>(patch + (i >> 2) * 16 + 4 * (i & 3)) = pre[f];
    }
    __syncthreads();
    if (bt + (int)gridDim.x < ntiles) fetch(bt + gridDim.x);
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const int ly = 2 * wave + py, y = y0 + ly;
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          if ((py + PAD - ky) & 1) continue;
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            if ((px + PAD - kx) & 1) continue;
            // (ly + PAD - ky)/2 and (px + PAD - kx)/2 are exact; the patch starts one dz row / column before the tile
            const float* b = patch + ((((ly + PAD - ky) >> 1) + 1) * PW + idx + ((px + PAD - kx) >> 1) + 1) * 16 + 4 * g;
            const float4 a0 = *reinterpret_cast<const float4*>(b);
            const float4 a1 = *reinterpret_cast<const float4*>(b + 16 * 16);
            const int tap = ky * K + kx;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][0], a0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][0], a1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][1], a0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][1], a1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][2], a0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][2], a1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][3], a0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(breg[tap][3], a1.w, acc1, 0, 0, 0);
          }
        }
        if (y < H) {   // (weights as the row operand: the lane holds channels 4g..4g+3 of pixel idx, see conv16_kernel)
          const int xa = x0 + 2 * idx + px, xb = xa + 32;
          float4* pa = reinterpret_cast<float4*>(dx + (((long)img * H + y) * W + xa) * 16 + 4 * g);
          auto put = [&](float4* q, const f32x4_t& acc) __attribute__((always_inline)) {
            float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
            if (accumulate) old = *q;
            *q = make_float4(acc[0] + old.x, acc[1] + old.y, acc[2] + old.z, acc[3] + old.w);
          };
          if (xa < W) put(pa, acc0);
          if (xb < W) put(pa + 32 * 4, acc1);
        }
      }
    }
  }
}
}  // namespace

void launch_tconv16_s2(const float* dz, int nimg, int Ho, int Wo, const float* w, int K, int pad, int H, int W, bool accumulate,
                       float* dx, hipStream_t st) {
  const int tx = cdiv(W, 64), ty = cdiv(H, 8), ntiles = nimg * tx * ty;
  const int grid = ntiles < 256 * 4 ? ntiles : 256 * 4;
  if (K == 3 && pad == 1)
    hipLaunchKernelGGL((tconv16_s2_kernel<3, 1>), dim3(grid), dim3(256), 0, st, dz, nimg, Ho, Wo, w, H, W, accumulate ? 1 : 0, dx,
                       tx, tx * ty, ntiles);
  else if (K == 1 && pad == 0)
    hipLaunchKernelGGL((tconv16_s2_kernel<1, 0>), dim3(grid), dim3(256), 0, st, dz, nimg, Ho, Wo, w, H, W, accumulate ? 1 : 0, dx,
                       tx, tx * ty, ntiles);
  else throw Error("tconv16_s2: no kernel for this shape");
  ATDN_HIP(hipGetLastError());
}

void launch_conv16(const float* x, int nimg, int H, int W, const float* w, bool transposed, const float* bias, int K, int S,
                   int pad, float* z, hipStream_t st, bool accumulate, Conv16Stats* stat) {
  const Conv16Tail nt{};
  if (K == 3 && S == 1) conv16_launch<3, 1, 8, 64>(x, nimg, H, W, w, transposed, bias, pad, z, accumulate, st, nt, stat);
  else if (K == 3 && S == 2) conv16_launch<3, 2, 4, 32>(x, nimg, H, W, w, transposed, bias, pad, z, accumulate, st, nt, stat);
  else if (K == 3 && S == 3) conv16_launch<3, 3, 2, 32>(x, nimg, H, W, w, transposed, bias, pad, z, accumulate, st, nt, stat);
  else if (K == 1 && S == 2) conv16_launch<1, 2, 4, 32>(x, nimg, H, W, w, transposed, bias, pad, z, accumulate, st, nt, stat);
  else if (K == 1 && S == 1) conv16_launch<1, 1, 8, 64>(x, nimg, H, W, w, transposed, bias, pad, z, accumulate, st, nt, stat);
  else throw Error("conv16: no kernel for this shape");
}

void launch_conv16_eval(const float* x, int nimg, int H, int W, const float* w, const float* bias, int K, int S, int pad,
                        const Conv16Tail& tail, float* z, hipStream_t st) {
  ATDN_CHECK(tail.sc && tail.sh, "eval tail needs the folded BatchNorm affine");
  const bool res = tail.skip != nullptr;
  ATDN_CHECK(!res || (tail.sc2 && tail.sh2), "residual tail needs the second affine");
  if (K == 3 && S == 1 && !res) conv16_launch<3, 1, 8, 64, 1>(x, nimg, H, W, w, false, bias, pad, z, false, st, tail);
  else if (K == 3 && S == 2 && res) conv16_launch<3, 2, 4, 32, 2>(x, nimg, H, W, w, false, bias, pad, z, false, st, tail);
  else if (K == 3 && S == 3 && !res) conv16_launch<3, 3, 2, 32, 1>(x, nimg, H, W, w, false, bias, pad, z, false, st, tail);
  else throw Error("conv16_eval: no kernel for this shape");
}

}  // namespace atdn
