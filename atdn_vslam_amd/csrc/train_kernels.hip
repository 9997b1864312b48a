// See train_kernels.h. Everything here is HBM- or latency-bound bookkeeping around the convolutions; kernels are
// written for coalesced 16-byte accesses (NHWC16 maps: one float4 per thread) and deterministic reductions
// (per-block partials + a second pass, no floating-point atomics).
#include "train_kernels.h"

#include <cstdint>
#include "clvo_composite.h"
#include "common.h"
#include "mish.h"
#include <algorithm>
#include <cmath>

namespace atdn {

namespace {
__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }
constexpr int kRedThreads = 256;
constexpr long kPixPerBlock = 16384;  // pixels one reduction block walks over
}  // namespace

// ------------------------------------------------------------------------------------------------ BatchNorm (train)
int bn_partial_blocks(long P) { return (int)cdivl(P, kPixPerBlock); }

// v1, v2 per element via F; block (blockIdx.x, group blockIdx.y) walks kPixPerBlock pixels, thread = one float4
template <class F>
__global__ __launch_bounds__(kRedThreads) void reduce2_kernel(long P, int nblk, float* __restrict__ part, F f) {
  const int g = blockIdx.y, blk = blockIdx.x;
  const int quad = threadIdx.x & 3, lane_pix = threadIdx.x >> 2;
  const long p0 = (long)blk * kPixPerBlock, p1 = min(p0 + kPixPerBlock, P);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int kStep = kRedThreads / 4;
  long p = p0 + lane_pix;
  for (; p + 3 * kStep < p1; p += 4 * kStep) {   // four independent loads in flight per thread
    typename F::Elem e0 = f.load((long)g * P + p, quad), e1 = f.load((long)g * P + p + kStep, quad),
                     e2 = f.load((long)g * P + p + 2 * kStep, quad), e3 = f.load((long)g * P + p + 3 * kStep, quad);
    f.acc(e0, g, quad, s1, s2); f.acc(e1, g, quad, s1, s2); f.acc(e2, g, quad, s1, s2); f.acc(e3, g, quad, s1, s2);
  }
  for (; p < p1; p += kStep) f.acc(f.load((long)g * P + p, quad), g, quad, s1, s2);
  __shared__ float red[2][kRedThreads][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[0][threadIdx.x][e] = s1[e]; red[1][threadIdx.x][e] = s2[e]; }
  __syncthreads();
  if (threadIdx.x < 32) {  // 2 quantities x 16 channels
    const int which = threadIdx.x >> 4, ch = threadIdx.x & 15;
    float acc = 0.f;
    for (int t = (ch >> 2); t < kRedThreads; t += 4) acc += red[which][t][ch & 3];
    part[(((long)g * nblk + blk) * 2 + which) * 16 + ch] = acc;
  }
}

// 256 threads = 16 slices x 16 channels: a slice sums every 16th partial in double, thread ch < 16 adds the slices in order
__device__ __forceinline__ void sum_partials2(const float* __restrict__ part_g, int nblk, double (*r)[16][16], double& s1,
                                              double& s2) {
  const int ch = threadIdx.x & 15, sl = threadIdx.x >> 4;
  double a = 0.0, b = 0.0;
  for (int k = sl; k < nblk; k += 16) {
    a += (double)part_g[((long)k * 2 + 0) * 16 + ch];
    b += (double)part_g[((long)k * 2 + 1) * 16 + ch];
  }
  __syncthreads();   // r is reused between groups
  r[0][sl][ch] = a; r[1][sl][ch] = b;
  __syncthreads();
  s1 = 0.0; s2 = 0.0;
  if (threadIdx.x < 16)
    for (int k = 0; k < 16; ++k) { s1 += r[0][k][ch]; s2 += r[1][k][ch]; }
}

// One block per group sums its partial rows (round 5: up to 1,024 of them when a convolution kernel took the statistics — the
// groups one after the other in ONE block cost 70 us per layer); a second, 16-thread launch walks the running statistics through
// the groups IN ORDER, as G successive forward() calls would. (Not a last-block-finishes counter: a device-scope release on this
// chip writes back an XCD's whole L2, kernels.hip.)
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int nblk, double invP, double unbias,
                                                          float* __restrict__ mean, float* __restrict__ rstd,
                                                          float* __restrict__ var_g) {
  __shared__ double r[2][16][16];
  const int ch = threadIdx.x & 15, g = blockIdx.x;
  double s1, s2;
  sum_partials2(part + (long)g * nblk * 32, nblk, r, s1, s2);
  if (threadIdx.x < 16) {
    const double mu = s1 * invP;
    double var = s2 * invP - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[g * 16 + ch] = (float)mu;
    rstd[g * 16 + ch] = (float)(1.0 / sqrt(var + 1e-5));
    var_g[g * 16 + ch] = (float)(var * unbias);
  }
}
__global__ void bn_running_kernel(const float* __restrict__ mean, const float* __restrict__ var_g, int G, float* __restrict__ rm,
                                  float* __restrict__ rv) {
  const int ch = threadIdx.x;
  float m_run = rm[ch], v_run = rv[ch];
  for (int g = 0; g < G; ++g) {
    m_run = 0.9f * m_run + 0.1f * mean[g * 16 + ch];                 // torch: running = (1-momentum)*running + momentum*batch
    v_run = 0.9f * v_run + 0.1f * var_g[g * 16 + ch];
  }
  rm[ch] = m_run; rv[ch] = v_run;
}
void launch_bn_finalize(const float* part, int G, int rows, long P, float* running_mean, float* running_var, float* mean,
                        float* rstd, float* var_scratch, hipStream_t st) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(G), dim3(256), 0, st, part, rows, 1.0 / (double)P,
                     P > 1 ? (double)P / (double)(P - 1) : 1.0, mean, rstd, var_scratch);
  ATDN_HIP(hipGetLastError());
  hipLaunchKernelGGL(bn_running_kernel, dim3(1), dim3(16), 0, st, mean, var_scratch, G, running_mean, running_var);
  ATDN_HIP(hipGetLastError());
}

// (round 5: one group per blockIdx.y and a strip of pixels per block, four float4 — eight with the residual — in flight per thread and
// the channel constants in registers; the one-float4-per-thread form with its 64-bit division per thread ran at 2.6 TB/s on the
// largest map)
constexpr long kApplyPix = 4096;   // pixels per block
__global__ __launch_bounds__(256) void bn_apply_kernel(const float4* __restrict__ z, long P, int mish, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float4* __restrict__ add,
                                                       float4* __restrict__ y, float* __restrict__ next_part) {
  const int g = blockIdx.y;
  const int quad = threadIdx.x & 3, lane_pix = threadIdx.x >> 2;
  const long p0 = (long)blockIdx.x * kApplyPix, p1 = min(p0 + kApplyPix, P);
  float mu[4], rs[4], ga[4], be[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ch = quad * 4 + e;
    mu[e] = mean[g * 16 + ch]; rs[e] = rstd[g * 16 + ch]; ga[e] = gamma[ch]; be[e] = beta[ch];
  }
  float n1[4] = {0.f, 0.f, 0.f, 0.f}, n2[4] = {0.f, 0.f, 0.f, 0.f};   // next_part: sums of Mish(y), Mish(y)^2
  auto one = [&](const float4 v, const float4 r) {
    const float a[4] = {v.x, v.y, v.z, v.w}, rr[4] = {r.x, r.y, r.z, r.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = mish ? mish_fast(a[e]) : a[e];
      o[e] = (x - mu[e]) * rs[e] * ga[e] + be[e];
      o[e] += rr[e];   // (zeros without a residual: x + 0 = x)
      if (next_part) { const float m = mish_fast(o[e]); n1[e] += m; n2[e] += m * m; }
    }
    return make_float4(o[0], o[1], o[2], o[3]);
  };
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int kStep = 256 / 4;
  long p = p0 + lane_pix;
  for (; p + 3 * kStep < p1; p += 4 * kStep) {
    const long i0 = ((long)g * P + p) * 4 + quad, i1 = i0 + 4L * kStep, i2 = i0 + 8L * kStep, i3 = i0 + 12L * kStep;
    const float4 v0 = z[i0], v1 = z[i1], v2 = z[i2], v3 = z[i3];
    float4 r0 = zero, r1 = zero, r2 = zero, r3 = zero;
    if (add) { r0 = add[i0]; r1 = add[i1]; r2 = add[i2]; r3 = add[i3]; }
    y[i0] = one(v0, r0); y[i1] = one(v1, r1); y[i2] = one(v2, r2); y[i3] = one(v3, r3);
  }
  for (; p < p1; p += kStep) {
    const long i = ((long)g * P + p) * 4 + quad;
    y[i] = one(z[i], add ? add[i] : zero);
  }
  if (next_part) {   // the block's partial row, reduced like reduce2_kernel's
    __shared__ float red[2][256][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][threadIdx.x][e] = n1[e]; red[1][threadIdx.x][e] = n2[e]; }
    __syncthreads();
    if (threadIdx.x < 32) {
      const int which = threadIdx.x >> 4, ch = threadIdx.x & 15;
      float acc = 0.f;
      for (int t = (ch >> 2); t < 256; t += 4) acc += red[which][t][ch & 3];
      next_part[(((long)g * gridDim.x + blockIdx.x) * 2 + which) * 16 + ch] = acc;
    }
  }
}
int bn_apply_partial_rows(long P) { return (int)cdivl(P, kApplyPix); }
void launch_bn_apply(const float* z, int G, long P, bool mish, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* add, float* y, hipStream_t st, float* next_part) {
  hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)cdivl(P, kApplyPix), G), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(z), P, mish ? 1 : 0, mean, rstd, gamma, beta,
                     reinterpret_cast<const float4*>(add), reinterpret_cast<float4*>(y), next_part);
  ATDN_HIP(hipGetLastError());
}

struct StatsBwd {
  const float4* dy; const float4* z; int mish; const float* mean; const float* rstd;
  struct Elem { float4 d, v; };
  __device__ __forceinline__ Elem load(long pix, int quad) const { return {dy[pix * 4 + quad], z[pix * 4 + quad]}; }
  __device__ __forceinline__ void acc(const Elem& el, int g, int quad, float* s1, float* s2) const {
    const float4 d = el.d, v = el.v;
    const float dd[4] = {d.x, d.y, d.z, d.w}, a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = quad * 4 + e;
      const float x = mish ? mish_fast(a[e]) : a[e];
      const float xh = (x - mean[g * 16 + ch]) * rstd[g * 16 + ch];
      s1[e] += dd[e];
      s2[e] += dd[e] * xh;
    }
  }
};
void launch_bn_bwd_stats(const float* dy, const float* z, int G, long P, bool mish, const float* mean, const float* rstd,
                         float* part, hipStream_t st) {
  const int nblk = bn_partial_blocks(P);
  hipLaunchKernelGGL((reduce2_kernel<StatsBwd>), dim3(nblk, G), dim3(kRedThreads), 0, st, P, nblk, part,
                     StatsBwd{reinterpret_cast<const float4*>(dy), reinterpret_cast<const float4*>(z), mish ? 1 : 0, mean, rstd});
  ATDN_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int G, int nblk,
                                                              float* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  __shared__ double r[2][16][16];
  const int ch = threadIdx.x & 15;
  const bool lead = threadIdx.x < 16;
  double tg = 0.0, tb = 0.0;
  for (int g = 0; g < G; ++g) {
    double s1, s2;
    sum_partials2(part + (long)g * nblk * 32, nblk, r, s1, s2);
    if (lead) {
      sums[(g * 2 + 0) * 16 + ch] = (float)s1;
      sums[(g * 2 + 1) * 16 + ch] = (float)s2;
      tb += s1;
      tg += s2;
    }
  }
  if (lead) { dgamma[ch] += (float)tg; dbeta[ch] += (float)tb; }
}
void launch_bn_bwd_finalize(const float* part, int G, long P, float* sums, float* dgamma, float* dbeta, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(1), dim3(256), 0, st, part, G, bn_partial_blocks(P), sums, dgamma, dbeta);
  ATDN_HIP(hipGetLastError());
}

// dz and the per-block sums of dz (bias gradient of the convolution that produced z)
__global__ __launch_bounds__(kRedThreads) void bn_bwd_apply_kernel(const float4* __restrict__ dy, const float4* __restrict__ z,
                                                                   long P, int nblk, int mish, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ sums, float invP,
                                                                   float4* __restrict__ dz, float* __restrict__ part_db) {
  const int g = blockIdx.y, blk = blockIdx.x;
  const int quad = threadIdx.x & 3, lane_pix = threadIdx.x >> 2;
  const long p0 = (long)blk * kPixPerBlock, p1 = min(p0 + kPixPerBlock, P);
  float mu[4], rs[4], ga[4], m1[4], m2[4], sdb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ch = quad * 4 + e;
    mu[e] = mean[g * 16 + ch]; rs[e] = rstd[g * 16 + ch]; ga[e] = gamma[ch];
    m1[e] = sums[(g * 2 + 0) * 16 + ch] * invP;
    m2[e] = sums[(g * 2 + 1) * 16 + ch] * invP;
  }
  auto one = [&](long i, const float4 d, const float4 v) {
    const float dd[4] = {d.x, d.y, d.z, d.w}, a[4] = {v.x, v.y, v.z, v.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      MishVal mv = {a[e], 1.0f};
      if (mish) mv = mish_both(a[e]);
      const float xh = (mv.y - mu[e]) * rs[e];
      const float da = ga[e] * rs[e] * (dd[e] - m1[e] - xh * m2[e]);
      o[e] = da * mv.dy;
      sdb[e] += o[e];
    }
    dz[i] = make_float4(o[0], o[1], o[2], o[3]);
  };
  constexpr int kStep = kRedThreads / 4;
  long p = p0 + lane_pix;
  for (; p + 3 * kStep < p1; p += 4 * kStep) {   // eight independent loads in flight per thread
    const long i0 = ((long)g * P + p) * 4 + quad, i1 = i0 + 4L * kStep, i2 = i0 + 8L * kStep, i3 = i0 + 12L * kStep;
    const float4 d0 = dy[i0], v0 = z[i0], d1 = dy[i1], v1 = z[i1], d2 = dy[i2], v2 = z[i2], d3 = dy[i3], v3 = z[i3];
    one(i0, d0, v0); one(i1, d1, v1); one(i2, d2, v2); one(i3, d3, v3);
  }
  for (; p < p1; p += kStep) { const long i = ((long)g * P + p) * 4 + quad; one(i, dy[i], z[i]); }
  __shared__ float red[kRedThreads][4];
#pragma unroll
  for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = sdb[e];
  __syncthreads();
  if (threadIdx.x < 16) {
    const int ch = threadIdx.x;
    float acc = 0.f;
    for (int t = (ch >> 2); t < kRedThreads; t += 4) acc += red[t][ch & 3];
    part_db[((long)g * nblk + blk) * 16 + ch] = acc;
  }
}
void launch_bn_bwd_apply(const float* dy, const float* z, int G, long P, bool mish, const float* mean, const float* rstd,
                         const float* gamma, const float* sums, float* dz, float* part_db, hipStream_t st) {
  const int nblk = bn_partial_blocks(P);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nblk, G), dim3(kRedThreads), 0, st, reinterpret_cast<const float4*>(dy),
                     reinterpret_cast<const float4*>(z), P, nblk, mish ? 1 : 0, mean, rstd, gamma, sums, 1.0f / (float)P,
                     reinterpret_cast<float4*>(dz), part_db);
  ATDN_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void sum_partials16_kernel(const float* __restrict__ part, long rows, float* __restrict__ out) {
  __shared__ double r[16][16];
  const int ch = threadIdx.x & 15, sl = threadIdx.x >> 4;
  double s = 0.0;
  for (long k = sl; k < rows; k += 16) s += (double)part[k * 16 + ch];
  r[sl][ch] = s;
  __syncthreads();
  if (threadIdx.x < 16) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += r[k][ch];
    out[ch] += (float)t;
  }
}
void launch_sum_partials16(const float* part, long rows, float* out, hipStream_t st) {
  hipLaunchKernelGGL(sum_partials16_kernel, dim3(1), dim3(256), 0, st, part, rows, out);
  ATDN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ transposed conv
__global__ void zero_stuff_kernel(const float4* __restrict__ dz, int Ho, int Wo, int stride, int Hs, int Ws,
                                  float4* __restrict__ D, long total4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int quad = (int)(i & 3);
  long pix = i >> 2;
  const int x = (int)(pix % Ws); pix /= Ws;
  const int y = (int)(pix % Hs);
  const long img = pix / Hs;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (y % stride == 0 && x % stride == 0) {
    const int oy = y / stride, ox = x / stride;
    if (oy < Ho && ox < Wo) v = dz[((img * Ho + oy) * Wo + ox) * 4 + quad];
  }
  D[i] = v;
}
void launch_zero_stuff(const float* dz, int nimg, int Ho, int Wo, int stride, int Hs, int Ws, float* D, hipStream_t st) {
  const long total4 = (long)nimg * Hs * Ws * 4;
  hipLaunchKernelGGL(zero_stuff_kernel, dim3((unsigned)cdivl(total4, 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(dz), Ho, Wo, stride, Hs, Ws, reinterpret_cast<float4*>(D), total4);
  ATDN_HIP(hipGetLastError());
}

__global__ void add_inplace_kernel(float4* __restrict__ a, const float4* __restrict__ b, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  float4 x = a[i];
  const float4 y = b[i];
  x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
  a[i] = x;
}
void launch_add_inplace(float* a, const float* b, long n, hipStream_t st) {
  ATDN_CHECK(n % 4 == 0, "add_inplace: length must be a multiple of 4");
  hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)cdivl(n / 4, 256)), dim3(256), 0, st, reinterpret_cast<float4*>(a),
                     reinterpret_cast<const float4*>(b), n / 4);
  ATDN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ weight gradients
namespace {
constexpr int WG_TW = 32;        // output columns staged per step
constexpr int WG_BLOCKS = 1024;  // persistent blocks; partials are [output][block]
constexpr int WG_MFMA_BLOCKS = 768, WG_SLOTS = WG_MFMA_BLOCKS * 4;   // MFMA variant: one partial per wave
constexpr int wg_nf4(int S, int KW) { return (3 * S + KW + 3) / 4; }   // float4 loads covering 4 output columns of one tap row
constexpr int wg_pwpad(int S, int KW) {
  int need = (WG_TW - 4) * S + wg_nf4(S, KW) * 4;
  int p = ((WG_TW - 1) * S + KW + 3) / 4 * 4;
  if (p < need) p = need;
  if ((p / 4) % 2 == 0) p += 4;   // odd multiple of 4 dwords: the 16 channel rows of a ds_read_b128 group hit 16 distinct bank quads
  return p;
}
}  // namespace
long wgrad_scratch_floats(int, int, int Cin, int KH, int KW) { return (long)WG_SLOTS * KH * KW * 16 * Cin; }

// Thread (n, c, g): output channel n, input channel c, and the kernel rows ky = g, g + GROUPS, ... with ALL kx of those
// rows (GROUPS = 256 / (16*CIN)). The staged input patch is channel-major in LDS, xs[py][c][px], so the 3*S + KW
// consecutive px a thread needs for 4 adjacent output columns are NF4 aligned ds_read_b128; the gradient tile is
// ds[r][n][col] (one b128 per 4 columns): 0.2 LDS loads per FMA instead of 1.1 with a pixel-major patch.
template <int S, int KH, int KW, int CIN, int R>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ x, int Cpix, int nimg, int H, int W,
                                                         const float* __restrict__ dz, int Ho, int Wo, int pad,
                                                         float* __restrict__ scratch) {
  constexpr int PAIRS = 16 * CIN, GROUPS = 256 / PAIRS, NKY = (KH + GROUPS - 1) / GROUPS;
  constexpr int PH = (R - 1) * S + KH, PWP = wg_pwpad(S, KW), NF4 = wg_nf4(S, KW);
  __shared__ __attribute__((aligned(16))) float xs[PH * CIN * PWP];
  __shared__ __attribute__((aligned(16))) float ds[R * 16 * WG_TW];
  const int pair = threadIdx.x % PAIRS, g = threadIdx.x / PAIRS;
  const bool worker = g < GROUPS;
  const int c = pair % CIN, n = pair / CIN;
  float acc[NKY][KW];
#pragma unroll
  for (int i = 0; i < NKY; ++i)
#pragma unroll
    for (int k = 0; k < KW; ++k) acc[i][k] = 0.f;
  const int rblocks = cdiv_dev(Ho, R), cblocks = cdiv_dev(Wo, WG_TW);
  const long items = (long)nimg * rblocks * cblocks;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int cb0 = (int)(it % cblocks);
    const int rb = (int)((it / cblocks) % rblocks);
    const int img = (int)(it / ((long)cblocks * rblocks));
    const int oy0 = rb * R, ox0 = cb0 * WG_TW;
    const int iy0 = oy0 * S - pad, ix0 = ox0 * S - pad;
    __syncthreads();
    for (int i = threadIdx.x; i < PH * PWP; i += 256) {   // one patch pixel per thread: CIN channels, scattered by row
      const int px = i % PWP, py = i / PWP;
      const int iy = iy0 + py, ix = ix0 + px;
      const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const float* src = x + (((long)img * H + (ok ? iy : 0)) * W + (ok ? ix : 0)) * Cpix;
#pragma unroll
      for (int ch = 0; ch < CIN; ++ch) xs[(py * CIN + ch) * PWP + px] = ok ? src[ch] : 0.f;
    }
    for (int i = threadIdx.x; i < R * WG_TW; i += 256) {
      const int col = i % WG_TW, r = i / WG_TW;
      const int oy = oy0 + r, ox = ox0 + col;
      const bool ok = oy < Ho && ox < Wo;
      const float4* src = reinterpret_cast<const float4*>(dz + (((long)img * Ho + (ok ? oy : 0)) * Wo + (ok ? ox : 0)) * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = src[q];
        ds[(r * 16 + 4 * q + 0) * WG_TW + col] = ok ? v.x : 0.f;
        ds[(r * 16 + 4 * q + 1) * WG_TW + col] = ok ? v.y : 0.f;
        ds[(r * 16 + 4 * q + 2) * WG_TW + col] = ok ? v.z : 0.f;
        ds[(r * 16 + 4 * q + 3) * WG_TW + col] = ok ? v.w : 0.f;
      }
    }
    __syncthreads();
    if (worker) {
#pragma unroll 1
      for (int r = 0; r < R; ++r)
#pragma unroll 2
        for (int cb = 0; cb < WG_TW / 4; ++cb) {
          const float4 d4 = *reinterpret_cast<const float4*>(ds + (r * 16 + n) * WG_TW + cb * 4);
          const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int i = 0; i < NKY; ++i) {
            const int ky = g + i * GROUPS;
            if (ky < KH) {
              const float4* xp = reinterpret_cast<const float4*>(xs + ((r * S + ky) * CIN + c) * PWP + cb * 4 * S);
              float xr[NF4 * 4];
#pragma unroll
              for (int q = 0; q < NF4; ++q) {
                const float4 v = xp[q];
                xr[4 * q] = v.x; xr[4 * q + 1] = v.y; xr[4 * q + 2] = v.z; xr[4 * q + 3] = v.w;
              }
#pragma unroll
              for (int kx = 0; kx < KW; ++kx)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][kx] += d[j] * xr[j * S + kx];
            }
          }
        }
    }
  }
  if (worker) {
#pragma unroll
    for (int i = 0; i < NKY; ++i) {
      const int ky = g + i * GROUPS;
      if (ky < KH) {
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) {
          const int o = ((ky * KW + kx) * 16 + n) * CIN + c;
          scratch[(long)o * gridDim.x + blockIdx.x] = acc[i][kx];
        }
      }
    }
  }
}

// CIN = 16 on the matrix cores: dW[n][c](tap) = sum_px dz[px][n] * x[px*S + tap][c] is a 16 x 16 x (pixels) product per tap,
// v_mfma_f32_16x16x4_f32 with A = dz^T and B = x, both read from the channel-major LDS images with b128 loads (k-slot g of
// MFMA j holds pixel 4g + j of a 16-pixel group). Each wave owns whole 16-pixel groups and keeps the K*K accumulator tiles;
// its partial goes to scratch slot 4*block + wave, summed by conv_wgrad_reduce_kernel in a fixed order. The next item's
// pixels are fetched into registers while the current one is multiplied.
typedef float wg_f32x4 __attribute__((ext_vector_type(4)));
template <int S, int K, int R>
__global__ __launch_bounds__(256) void conv_wgrad16_mfma_kernel(const float* __restrict__ x, int nimg, int H, int W,
                                                                const float* __restrict__ dz, int Ho, int Wo, int pad,
                                                                float* __restrict__ scratch, int nslots) {
  constexpr int PH = (R - 1) * S + K, PWP = wg_pwpad(S, K), NF4 = wg_nf4(S, K), DSP = WG_TW + 4;
  constexpr int NX = PH * PWP * 4, NXF = (NX + 255) / 256, ND = R * WG_TW * 4, NDF = (ND + 255) / 256;
  __shared__ __attribute__((aligned(16))) float xs[PH * 16 * PWP];
  __shared__ __attribute__((aligned(16))) float ds[R * 16 * DSP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = lane & 15, g = lane >> 4;
  wg_f32x4 acc[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) acc[t] = wg_f32x4{0.f, 0.f, 0.f, 0.f};
  const int rblocks = cdiv_dev(Ho, R), cblocks = cdiv_dev(Wo, WG_TW);
  const long items = (long)nimg * rblocks * cblocks;
  float4 fx[NXF], fd[NDF];
  auto fetch = [&](long it) {
    const int cb0 = (int)(it % cblocks), rb = (int)((it / cblocks) % rblocks), img = (int)(it / ((long)cblocks * rblocks));
    const int oy0 = rb * R, ox0 = cb0 * WG_TW, iy0 = oy0 * S - pad, ix0 = ox0 * S - pad;
#pragma unroll
    for (int f = 0; f < NXF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, px = pix % PWP, py = pix / PWP;
      const int iy = iy0 + py, ix = ix0 + px;
      fx[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < NX && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        fx[f] = *reinterpret_cast<const float4*>(x + (((long)img * H + iy) * W + ix) * 16 + 4 * q);
    }
#pragma unroll
    for (int f = 0; f < NDF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, col = pix % WG_TW, r = pix / WG_TW;
      const int oy = oy0 + r, ox = ox0 + col;
      fd[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < ND && oy < Ho && ox < Wo) fd[f] = *reinterpret_cast<const float4*>(dz + (((long)img * Ho + oy) * Wo + ox) * 16 + 4 * q);
    }
  };
  if ((long)blockIdx.x < items) fetch(blockIdx.x);
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NXF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, px = pix % PWP, py = pix / PWP;
      if (i < NX) {
        float* d = xs + (py * 16 + 4 * q) * PWP + px;
        d[0] = fx[f].x; d[PWP] = fx[f].y; d[2 * PWP] = fx[f].z; d[3 * PWP] = fx[f].w;
      }
    }
#pragma unroll
    for (int f = 0; f < NDF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, col = pix % WG_TW, r = pix / WG_TW;
      if (i < ND) {
        float* d = ds + (r * 16 + 4 * q) * DSP + col;
        d[0] = fd[f].x; d[DSP] = fd[f].y; d[2 * DSP] = fd[f].z; d[3 * DSP] = fd[f].w;
      }
    }
    __syncthreads();
    if (it + gridDim.x < items) fetch(it + gridDim.x);
#pragma unroll 1
    for (int grp = wave; grp < R * (WG_TW / 16); grp += 4) {
      const int r = grp / (WG_TW / 16), c0 = (grp % (WG_TW / 16)) * 16;
      const float4 d4 = *reinterpret_cast<const float4*>(ds + (r * 16 + idx) * DSP + c0 + 4 * g);
      const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const float4* xp = reinterpret_cast<const float4*>(xs + ((r * S + ky) * 16 + idx) * PWP + (c0 + 4 * g) * S);
        float xr[NF4 * 4];
#pragma unroll
        for (int q = 0; q < NF4; ++q) {
          const float4 v = xp[q];
          xr[4 * q] = v.x; xr[4 * q + 1] = v.y; xr[4 * q + 2] = v.z; xr[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[ky * K + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[j], xr[j * S + kx], acc[ky * K + kx], 0, 0, 0);
      }
    }
  }
  // D: row = output channel n = 4g + e, column = input channel c = lane & 15
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = (t * 16 + 4 * g + e) * 16 + idx;
      scratch[(long)o * nslots + blockIdx.x * 4 + wave] = acc[t][e];
    }
}

// Weight gradient of the stem on the auxiliary input (xn0, xn1, 1): 7x7, stride 2, pad 3, NHWC4. Two column sets per kernel
// row: set 1 = (kx, c in {0,1}) pairs, which are 16 consecutive floats of an interleaved patch row starting at 4*px; set 2 =
// the constant channel (a validity mask after zero padding), 8 consecutive floats starting at 2*px. Same pixel-to-k-slot
// assignment and scratch layout as conv_wgrad16_mfma_kernel.
constexpr int SW_R = 4, SW_PH = (SW_R - 1) * 2 + 7, SW_PWC = (WG_TW - 1) * 2 + 8, SW_XP = 144, SW_MP = 80, SW_DSP = WG_TW + 4;
__global__ __launch_bounds__(256) void stem_wgrad_mfma_kernel(const float* __restrict__ x4, int nimg, int H, int W,
                                                              const float* __restrict__ dz, int Ho, int Wo,
                                                              float* __restrict__ scratch, int nslots) {
  __shared__ __attribute__((aligned(16))) float xs[SW_PH * SW_XP];
  __shared__ __attribute__((aligned(16))) float ms[SW_PH * SW_MP];
  __shared__ __attribute__((aligned(16))) float ds[SW_R * 16 * SW_DSP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, idx = lane & 15, g = lane >> 4;
  wg_f32x4 acc1[7], acc2[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) { acc1[t] = wg_f32x4{0.f, 0.f, 0.f, 0.f}; acc2[t] = wg_f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int i = tid; i < SW_PH * SW_XP; i += 256) xs[i] = 0.f;   // padding columns stay zero
  for (int i = tid; i < SW_PH * SW_MP; i += 256) ms[i] = 0.f;
  const int rblocks = cdiv_dev(Ho, SW_R), cblocks = cdiv_dev(Wo, WG_TW);
  const long items = (long)nimg * rblocks * cblocks;
  constexpr int NX = SW_PH * SW_PWC, NXF = (NX + 255) / 256, ND = SW_R * WG_TW * 4, NDF = (ND + 255) / 256;
  float4 fx[NXF], fd[NDF];
  auto fetch = [&](long it) {
    const int cb0 = (int)(it % cblocks), rb = (int)((it / cblocks) % rblocks), img = (int)(it / ((long)cblocks * rblocks));
    const int oy0 = rb * SW_R, ox0 = cb0 * WG_TW, iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
#pragma unroll
    for (int f = 0; f < NXF; ++f) {
      const int i = tid + 256 * f, px = i % SW_PWC, py = i / SW_PWC;
      const int iy = iy0 + py, ix = ix0 + px;
      fx[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < NX && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
        fx[f] = *reinterpret_cast<const float4*>(x4 + (((long)img * H + iy) * W + ix) * 4);
    }
#pragma unroll
    for (int f = 0; f < NDF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, col = pix % WG_TW, r = pix / WG_TW;
      const int oy = oy0 + r, ox = ox0 + col;
      fd[f] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (i < ND && oy < Ho && ox < Wo) fd[f] = *reinterpret_cast<const float4*>(dz + (((long)img * Ho + oy) * Wo + ox) * 16 + 4 * q);
    }
  };
  if ((long)blockIdx.x < items) fetch(blockIdx.x);
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NXF; ++f) {
      const int i = tid + 256 * f, px = i % SW_PWC, py = i / SW_PWC;
      if (i < NX) {
        *reinterpret_cast<float2*>(xs + py * SW_XP + 2 * px) = make_float2(fx[f].x, fx[f].y);
        ms[py * SW_MP + px] = fx[f].z;
      }
    }
#pragma unroll
    for (int f = 0; f < NDF; ++f) {
      const int i = tid + 256 * f, q = i & 3, pix = i >> 2, col = pix % WG_TW, r = pix / WG_TW;
      if (i < ND) {
        float* d = ds + (r * 16 + 4 * q) * SW_DSP + col;
        d[0] = fd[f].x; d[SW_DSP] = fd[f].y; d[2 * SW_DSP] = fd[f].z; d[3 * SW_DSP] = fd[f].w;
      }
    }
    __syncthreads();
    if (it + gridDim.x < items) fetch(it + gridDim.x);
#pragma unroll 1
    for (int grp = wave; grp < SW_R * (WG_TW / 16); grp += 4) {
      const int r = grp / (WG_TW / 16), c0 = (grp % (WG_TW / 16)) * 16;
      const float4 d4 = *reinterpret_cast<const float4*>(ds + (r * 16 + idx) * SW_DSP + c0 + 4 * g);
      const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const float* xr = xs + (r * 2 + ky) * SW_XP + 4 * (c0 + 4 * g) + idx;   // pixel 4g + j: + 4j
        const float* mr = ms + (r * 2 + ky) * SW_MP + 2 * (c0 + 4 * g) + idx;   //              + 2j
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc1[ky] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[j], xr[4 * j], acc1[ky], 0, 0, 0);
          acc2[ky] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[j], mr[2 * j], acc2[ky], 0, 0, 0);
        }
      }
    }
  }
  // D: row n = 4g + e; set 1 column idx = 2*kx + c, set 2 column idx = kx
#pragma unroll
  for (int ky = 0; ky < 7; ++ky)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = 4 * g + e, slot = blockIdx.x * 4 + wave;
      if ((idx >> 1) < 7) scratch[(long)(((ky * 7 + (idx >> 1)) * 16 + n) * 3 + (idx & 1)) * nslots + slot] = acc1[ky][e];
      if (idx < 7) scratch[(long)(((ky * 7 + idx) * 16 + n) * 3 + 2) * nslots + slot] = acc2[ky][e];
    }
}

// one wave per output: sum its partials, add into dW (OIHW)
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ scratch, int nblk, int Cin, int KH,
                                                                int KW, float* __restrict__ dW) {
  const int total = KH * KW * 16 * Cin;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= total) return;
  float s = 0.f;
  for (int b = lane; b < nblk; b += 64) s += scratch[(long)o * nblk + b];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) {
    const int c = o % Cin, n = (o / Cin) & 15, tap = o / (Cin * 16);
    dW[((long)n * Cin + c) * KH * KW + tap] += s;
  }
}

template <int S, int KH, int KW, int CIN, int R>
static void wgrad_launch(const float* x, int Cpix, int nimg, int H, int W, const float* dz, int Ho, int Wo, int pad,
                         float* scratch, float* dW, hipStream_t st) {
  const long items = (long)nimg * cdiv(Ho, R) * cdiv(Wo, WG_TW);
  const int nblk = (int)std::min<long>(items, WG_BLOCKS);
  hipLaunchKernelGGL((conv_wgrad_kernel<S, KH, KW, CIN, R>), dim3(nblk), dim3(256), 0, st, x, Cpix, nimg, H, W, dz, Ho, Wo, pad,
                     scratch);
  ATDN_HIP(hipGetLastError());
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(cdiv(KH * KW * 16 * CIN, 4)), dim3(256), 0, st, scratch, nblk, CIN, KH, KW, dW);
  ATDN_HIP(hipGetLastError());
}

template <int S, int K, int R>
static void wgrad16_mfma_launch(const float* x, int nimg, int H, int W, const float* dz, int Ho, int Wo, int pad, float* scratch,
                                float* dW, hipStream_t st) {
  const long items = (long)nimg * cdiv(Ho, R) * cdiv(Wo, WG_TW);
  const int nblk = (int)std::min<long>(items, WG_MFMA_BLOCKS);
  hipLaunchKernelGGL((conv_wgrad16_mfma_kernel<S, K, R>), dim3(nblk), dim3(256), 0, st, x, nimg, H, W, dz, Ho, Wo, pad, scratch,
                     nblk * 4);
  ATDN_HIP(hipGetLastError());
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(cdiv(K * K * 16 * 16, 4)), dim3(256), 0, st, scratch, nblk * 4, 16, K, K, dW);
  ATDN_HIP(hipGetLastError());
}

void launch_conv_wgrad(const float* x, int Cpix, int Cin, int nimg, int H, int W, const float* dz, int Ho, int Wo, int KH,
                       int KW, int stride, int pad, float* scratch, float* dW, hipStream_t st) {
  ATDN_CHECK(Cpix >= Cin && Cpix % 4 == 0, "conv_wgrad: channel layout");
  if (Cin == 16 && Cpix == 16) {
    if (KH == 3 && KW == 3 && stride == 1) return wgrad16_mfma_launch<1, 3, 8>(x, nimg, H, W, dz, Ho, Wo, pad, scratch, dW, st);
    if (KH == 3 && KW == 3 && stride == 2) return wgrad16_mfma_launch<2, 3, 4>(x, nimg, H, W, dz, Ho, Wo, pad, scratch, dW, st);
    if (KH == 1 && KW == 1 && stride == 2) return wgrad16_mfma_launch<2, 1, 4>(x, nimg, H, W, dz, Ho, Wo, pad, scratch, dW, st);
  }
  if (Cin == 3 && Cpix == 4 && KH == 7 && KW == 7 && stride == 2 && pad == 3) {
    const long items = (long)nimg * cdiv(Ho, SW_R) * cdiv(Wo, WG_TW);
    const int nblk = (int)std::min<long>(items, WG_MFMA_BLOCKS);
    hipLaunchKernelGGL(stem_wgrad_mfma_kernel, dim3(nblk), dim3(256), 0, st, x, nimg, H, W, dz, Ho, Wo, scratch, nblk * 4);
    ATDN_HIP(hipGetLastError());
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(cdiv(49 * 16 * 3, 4)), dim3(256), 0, st, scratch, nblk * 4, 3, 7, 7, dW);
    ATDN_HIP(hipGetLastError());
    return;
  }
  // the last conv (3x3, stride 3) is the one shape without an MFMA kernel
  if (Cin == 16 && KH == 3 && KW == 3 && stride == 3) wgrad_launch<3, 3, 3, 16, 2>(x, Cpix, nimg, H, W, dz, Ho, Wo, pad, scratch, dW, st);
  else throw Error("conv_wgrad: no kernel for this convolution shape");
}

// The stem sees x0[c] = xn[c]*w[c] + b[c] (depthwise 1x1 on the normalised flow, zero padding applied AFTER it).
// With A = weight gradient of the stem conv taken on the auxiliary input (xn0, xn1, 1): A[n][c][tap], c = 0..2,
//   dW1[n][c][tap] += w[c]*A[n][c][tap] + b[c]*A[n][2][tap]
//   dw[c] += sum_{n,tap} W1[n][c][tap]*A[n][c][tap],   db[c] += sum_{n,tap} W1[n][c][tap]*A[n][2][tap]
// which is what back-propagating through the transposed stem convolution would give, without computing dx0.
__global__ __launch_bounds__(256) void stem_combine_kernel(const float* __restrict__ A, const float* __restrict__ W1,
                                                           const float* __restrict__ w, const float* __restrict__ b, int taps,
                                                           float* __restrict__ dW1, float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[256][4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < 16 * 2 * taps; i += 256) {
    const int tap = i % taps, c = (i / taps) & 1, n = i / (2 * taps);
    const float a = A[((long)n * 3 + c) * taps + tap], ones = A[((long)n * 3 + 2) * taps + tap];
    const float wv = W1[i];
    dW1[i] += w[c] * a + b[c] * ones;
    s[c] += wv * a;
    s[2 + c] += wv * ones;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[threadIdx.x][e] = s[e];
  __syncthreads();
  if (threadIdx.x < 4) {
    float acc = 0.f;
    for (int t = 0; t < 256; ++t) acc += red[t][threadIdx.x];
    if (threadIdx.x < 2) dw[threadIdx.x] += acc; else db[threadIdx.x - 2] += acc;
  }
}
void launch_stem_combine(const float* A, const float* W1, const float* w, const float* b, int taps, float* dW1, float* dw,
                         float* db, hipStream_t st) {
  hipLaunchKernelGGL(stem_combine_kernel, dim3(1), dim3(256), 0, st, A, W1, w, b, taps, dW1, dw, db);
  ATDN_HIP(hipGetLastError());
}

// (xn0, xn1, 1, 0) per pixel: the auxiliary stem input for the weight gradients
__global__ void prep_flow_aux_kernel(const float* __restrict__ flow, int B, long HW, float sx, float sy, float4* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HW) return;
  const long img = i / HW, p = i - img * HW;
  const float* s = flow + img * 2 * HW + p;
  out[i] = make_float4(s[0] / sx, s[HW] / sy, 1.f, 0.f);
}
void launch_prep_flow_aux(const float* flow, int nimg, int H, int W, float* out4, hipStream_t st) {
  const long n = (long)nimg * H * W;
  hipLaunchKernelGGL(prep_flow_aux_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, st, flow, nimg, (long)H * W, 58.1837f,
                     17.7647f, reinterpret_cast<float4*>(out4));
  ATDN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ small dense algebra
// 64x64 output tile, 16x16 threads x 4x4 values, K step 16; op(A) is M x K, op(B) is K x N
__global__ __launch_bounds__(256) void gemm_kernel(int transA, int transB, int M, int N, int K, const float* __restrict__ A,
                                                   int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
                                                   int ldc, float beta, const float* __restrict__ bias) {
  __shared__ float As[16][64 + 1], Bs[16][64 + 1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  float acc[4][4] = {};
  for (int k0 = 0; k0 < K; k0 += 16) {
    for (int i = threadIdx.x; i < 16 * 64; i += 256) {
      const int kk = i & 15, mm = i >> 4;   // consecutive threads walk K for the non-transposed A (rows contiguous)
      const int m = m0 + mm, k = k0 + kk;
      float v = 0.f;
      if (m < M && k < K) v = transA ? A[(long)k * lda + m] : A[(long)m * lda + k];
      As[kk][mm] = v;
    }
    for (int i = threadIdx.x; i < 16 * 64; i += 256) {
      const int nn = i & 63, kk = i >> 6;
      const int n = n0 + nn, k = k0 + kk;
      float v = 0.f;
      if (n < N && k < K) v = transB ? B[(long)n * ldb + k] : B[(long)k * ldb + n];
      Bs[kk][nn] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      float a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = As[kk][ty * 4 + i]; b[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
      if (m < M && n < N) {
        float v = acc[i][j] + (bias ? bias[n] : 0.f);
        if (beta != 0.f) v += beta * C[(long)m * ldc + n];
        C[(long)m * ldc + n] = v;
      }
    }
}
// A not transposed and K a multiple of 8: v_mfma_f32_32x32x2_f32, one 32x32 tile of C per block, K split over the four
// waves and summed through LDS in a fixed order. The recurrent products of the LSTMs (M = batch, K up to 2048) would
// otherwise run on a handful of blocks. K order inside a step of 8: MFMA j holds k = kb + 4h + j in slot h = lane >> 5, so
// every lane feeds four MFMAs from one float4 of its row.
typedef float f32x16_t __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void gemm_rows_kernel(int transB, int M, int N, int K, const float* __restrict__ A, int lda,
                                                        const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
                                                        float beta, const float* __restrict__ bias) {
  __shared__ float red[4][32][33];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
  const int steps = K / 8, per = (steps + 3) / 4;
  const int s0 = wave * per, s1 = min(steps, s0 + per);
  const bool mok = m0 + r < M, nok = n0 + r < N;
  const float* arow = A + (long)(mok ? m0 + r : 0) * lda + 4 * h;
  const float* brow = transB ? B + (long)(nok ? n0 + r : 0) * ldb + 4 * h : B + (long)(4 * h) * ldb + (nok ? n0 + r : 0);
  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int sidx = s0; sidx < s1; ++sidx) {
    const int kb = sidx * 8;
    float4 a = *reinterpret_cast<const float4*>(arow + kb);
    float4 b;
    if (transB) b = *reinterpret_cast<const float4*>(brow + kb);
    else { const float* q = brow + (long)kb * ldb; b = make_float4(q[0], q[ldb], q[2L * ldb], q[3L * ldb]); }
    if (!mok) a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!nok) b = make_float4(0.f, 0.f, 0.f, 0.f);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][(i >> 2) * 8 + h * 4 + (i & 3)][r] = acc[i];   // D: row, column = lane & 31
  __syncthreads();
  for (int i = threadIdx.x; i < 32 * 32; i += 256) {
    const int mm = i >> 5, nn = i & 31, m = m0 + mm, n = n0 + nn;
    if (m < M && n < N) {
      float v = ((red[0][mm][nn] + red[1][mm][nn]) + red[2][mm][nn]) + red[3][mm][nn];
      if (bias) v += bias[n];
      if (beta != 0.f) v += beta * C[(long)m * ldc + n];
      C[(long)m * ldc + n] = v;
    }
  }
}

void launch_gemm(bool transA, bool transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                 int ldc, float beta, const float* bias, hipStream_t st) {
  const bool aligned = (lda % 4 == 0) && ((uintptr_t)A % 16 == 0) && (!transB || ((ldb % 4 == 0) && ((uintptr_t)B % 16 == 0)));
  if (!transA && K % 8 == 0 && K >= 64 && aligned) {
    hipLaunchKernelGGL(gemm_rows_kernel, dim3(cdiv(N, 32), cdiv(M, 32)), dim3(256), 0, st, transB ? 1 : 0, M, N, K, A, lda, B,
                       ldb, C, ldc, beta, bias);
    ATDN_HIP(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(gemm_kernel, dim3(cdiv(N, 64), cdiv(M, 64)), dim3(256), 0, st, transA ? 1 : 0, transB ? 1 : 0, M, N, K, A,
                     lda, B, ldb, C, ldc, beta, bias);
  ATDN_HIP(hipGetLastError());
}

__global__ void colsum_kernel(const float* __restrict__ X, int rows, int cols, int ld, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += X[(long)r * ld + c];
  out[c] += s;
}
void launch_colsum(const float* X, int rows, int cols, int ld, float* out, hipStream_t st) {
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 256)), dim3(256), 0, st, X, rows, cols, ld, out);
  ATDN_HIP(hipGetLastError());
}

__global__ void mish_fwd_kernel(const float* __restrict__ z, float* __restrict__ a, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = mish_fast(z[i]);
}
void launch_mish_fwd(const float* z, float* a, long n, hipStream_t st) {
  hipLaunchKernelGGL(mish_fwd_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, st, z, a, n);
  ATDN_HIP(hipGetLastError());
}
__global__ void mish_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z, float* __restrict__ dz, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dz[i] = dy[i] * mish_grad(z[i]);
}
void launch_mish_bwd(const float* dy, const float* z, float* dz, long n, hipStream_t st) {
  hipLaunchKernelGGL(mish_bwd_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, st, dy, z, dz, n);
  ATDN_HIP(hipGetLastError());
}

__global__ void permute_p16_kernel(const float* __restrict__ src, int P, int to_chw, float* __restrict__ dst, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long img = i / (16L * P);
  const int r = (int)(i - img * 16L * P);
  if (to_chw) {  // dst index r = c*P + p
    const int c = r / P, p = r - c * P;
    dst[i] = src[img * 16L * P + (long)p * 16 + c];
  } else {       // dst index r = p*16 + c
    const int p = r >> 4, c = r & 15;
    dst[i] = src[img * 16L * P + (long)c * P + p];
  }
}
void launch_nhwc_to_chw(const float* src, int nimg, int P, float* dst, hipStream_t st) {
  const long total = (long)nimg * 16 * P;
  hipLaunchKernelGGL(permute_p16_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, st, src, P, 1, dst, total);
  ATDN_HIP(hipGetLastError());
}
void launch_chw_to_nhwc(const float* src, int nimg, int P, float* dst, hipStream_t st) {
  const long total = (long)nimg * 16 * P;
  hipLaunchKernelGGL(permute_p16_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, st, src, P, 0, dst, total);
  ATDN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ LSTM cell
__global__ void lstm_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ c_in, int B, float* __restrict__ act,
                                float* __restrict__ c_out, float* __restrict__ tanhc, float* __restrict__ h_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 512) return;
  const int b = i >> 9, j = i & 511;
  const float* p = pre + (long)b * 2048;
  const float ig = sigmoidf_(p[j]), fg = sigmoidf_(p[512 + j]), gg = tanhf(p[1024 + j]), og = sigmoidf_(p[1536 + j]);
  float* a = act + (long)b * 2048;
  a[j] = ig; a[512 + j] = fg; a[1024 + j] = gg; a[1536 + j] = og;
  const float c = fg * c_in[i] + ig * gg;
  const float tc = tanhf(c);
  c_out[i] = c;
  tanhc[i] = tc;
  h_out[i] = og * tc;
}
void launch_lstm_fwd(const float* pre, const float* c_in, int B, float* act, float* c_out, float* tanhc, float* h_out,
                     hipStream_t st) {
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(cdiv(B * 512, 256)), dim3(256), 0, st, pre, c_in, B, act, c_out, tanhc, h_out);
  ATDN_HIP(hipGetLastError());
}
__global__ void lstm_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ dc_out, const float* __restrict__ act,
                                const float* __restrict__ c_in, const float* __restrict__ tanhc, int B,
                                float* __restrict__ dpre, float* __restrict__ dc_in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * 512) return;
  const int b = i >> 9, j = i & 511;
  const float* a = act + (long)b * 2048;
  const float ig = a[j], fg = a[512 + j], gg = a[1024 + j], og = a[1536 + j];
  const float tc = tanhc[i];
  const float dhv = dh[i];
  const float dc = (dc_out ? dc_out[i] : 0.f) + dhv * og * (1.f - tc * tc);
  float* d = dpre + (long)b * 2048;
  d[j] = dc * gg * ig * (1.f - ig);
  d[512 + j] = dc * c_in[i] * fg * (1.f - fg);
  d[1024 + j] = dc * ig * (1.f - gg * gg);
  d[1536 + j] = dhv * tc * og * (1.f - og);
  dc_in[i] = dc * fg;
}
void launch_lstm_bwd(const float* dh, const float* dc_out, const float* act, const float* c_in, const float* tanhc, int B,
                     float* dpre, float* dc_in, hipStream_t st) {
  hipLaunchKernelGGL(lstm_bwd_kernel, dim3(cdiv(B * 512, 256)), dim3(256), 0, st, dh, dc_out, act, c_in, tanhc, B, dpre, dc_in);
  ATDN_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ loss, optimiser
// rows r = t*B + b (step-major, as the trainer stores its activations); targets are [B][T][3] like the reference's
__global__ void clvo_loss_kernel(const float* __restrict__ pr, const float* __restrict__ pt, const float* __restrict__ tr_,
                                 const float* __restrict__ tt, int B, int T, float* __restrict__ loss, float* __restrict__ d_rot,
                                 float* __restrict__ d_tr) {
  __shared__ double red[256];
  double s = 0.0;
  const float invB = 1.0f / (float)B;
  for (int i = threadIdx.x; i < B * T * 3; i += blockDim.x) {
    const int e = i % 3, r = i / 3;
    const int t = r / B, b = r - t * B;
    const long ti = ((long)b * T + t) * 3 + e;
    const float dr = pr[i] - tr_[ti], dt = pt[i] - tt[ti];
    s += (double)(1.0f * dt * dt) + (double)(100.0f * dr * dr);
    d_rot[i] = 2.0f * 100.0f * dr * invB;
    d_tr[i] = 2.0f * 1.0f * dt * invB;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int t = 0; t < blockDim.x; ++t) a += red[t];
    loss[0] = (float)(a / (double)B);
  }
}
void launch_clvo_loss(const float* pred_rot, const float* pred_tr, const float* true_rot, const float* true_tr, int B, int T,
                      float* loss, float* d_rot, float* d_tr, hipStream_t st) {
  hipLaunchKernelGGL(clvo_loss_kernel, dim3(1), dim3(256), 0, st, pred_rot, pred_tr, true_rot, true_tr, B, T, loss, d_rot, d_tr);
  ATDN_HIP(hipGetLastError());
}

// CLVO_Loss(alpha, w) with the composite term (loss.py:25-101; arithmetic and clamps: clvo_composite.h). One workgroup walks the
// batch in passes of `cpp` clips whose transforms fit in LDS. Per pass: one thread per step builds P_t of the predictions and of
// the targets; one thread per window chains the w transforms, converts back to Euler + translation, adds the window loss and
// (with_grad) leaves dl/dC in LDS; one thread per step then writes that step's gradient: alpha x the relative-pose gradient of
// clvo_loss_kernel, plus (1-alpha)/B x the windows covering the step, summed in ascending window order by that one thread (no
// atomics: two launches on the same inputs give the same bits). Predictions and gradients are step-major (r = t*B + b) when
// step_major, else [B][T][3] like the targets. loss3 = {L, mean_b L_rel, mean_b L_com}.
__global__ void __launch_bounds__(256) clvo_loss_composite_kernel(const float* __restrict__ pr, const float* __restrict__ pt,
                                                                  const float* __restrict__ tr_,
                                                                  const float* __restrict__ tt, int B, int T, int w, float alpha,
                                                                  int with_grad, int step_major, int cpp, float* __restrict__ loss3,
                                                                  float* __restrict__ d_rot, float* __restrict__ d_tr) {
  using composite::Affine;
  extern __shared__ double composite_lds[];
  __shared__ double red[2][256];
  Affine* Pp = reinterpret_cast<Affine*>(composite_lds);   // [cpp][T] predictions
  Affine* Pt = Pp + (long)cpp * T;                         // [cpp][T] targets
  Affine* Gw = Pt + (long)cpp * T;                         // [cpp][T-w+1] dl/dC per window
  const int NW = T - w + 1;
  const float invB = 1.0f / (float)B;
  const double com_scale = (1.0 - (double)alpha) / (double)B;
  double s_rel = 0.0, s_com = 0.0;
  for (int c0 = 0; c0 < B; c0 += cpp) {
    const int nc = min(cpp, B - c0);
    for (int idx = threadIdx.x; idx < nc * T; idx += blockDim.x) {
      const int c = idx / T, t = idx - c * T, b = c0 + c;
      const long ti = ((long)b * T + t) * 3, pi = step_major ? ((long)t * B + b) * 3 : ti;
      Pp[idx] = composite::from_pose(pr + pi, pt + pi);
      Pt[idx] = composite::from_pose(tr_ + ti, tt + ti);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nc * NW; idx += blockDim.x) {
      const int c = idx / NW, j = idx - c * NW;
      const Affine cp = composite::chain(Pp + (long)c * T, j, w), ct = composite::chain(Pt + (long)c * T, j, w);
      s_com += composite::window_loss(cp, ct, with_grad ? Gw + idx : nullptr);
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nc * T; idx += blockDim.x) {
      const int c = idx / T, t = idx - c * T, b = c0 + c;
      const long ti = ((long)b * T + t) * 3, pi = step_major ? ((long)t * B + b) * 3 : ti;
      double gr[3] = {0.0, 0.0, 0.0}, gt[3] = {0.0, 0.0, 0.0};
      if (with_grad) composite::step_gradient(Pp + (long)c * T, Gw + (long)c * NW, T, w, t, pr + pi, gr, gt);
      for (int e = 0; e < 3; ++e) {
        const float dr = pr[pi + e] - tr_[ti + e], dt = pt[pi + e] - tt[ti + e];
        s_rel += (double)(1.0f * dt * dt) + (double)(100.0f * dr * dr);
        const float rel_r = alpha * (2.0f * 100.0f * dr * invB), rel_t = alpha * (2.0f * 1.0f * dt * invB);   // (as clvo_loss_kernel)
        d_rot[pi + e] = with_grad ? (float)((double)rel_r + com_scale * gr[e]) : rel_r;
        d_tr[pi + e] = with_grad ? (float)((double)rel_t + com_scale * gt[e]) : rel_t;
      }
    }
    __syncthreads();   // the next pass overwrites the transforms
  }
  red[0][threadIdx.x] = s_rel;
  red[1][threadIdx.x] = s_com;
  __syncthreads();
  if (threadIdx.x == 0) {
    double rel = 0.0, com = 0.0;
    for (int t = 0; t < blockDim.x; ++t) { rel += red[0][t]; com += red[1][t]; }
    rel /= (double)B;
    com /= (double)B;
    loss3[0] = (float)((double)alpha * rel + (1.0 - (double)alpha) * com);
    loss3[1] = (float)rel;
    loss3[2] = (float)com;
  }
}
void launch_clvo_loss_composite(const float* pred_rot, const float* pred_tr, const float* true_rot, const float* true_tr, int B, int T,
                                float alpha, int w, bool with_grad, bool step_major, float* loss3, float* d_rot, float* d_tr,
                                hipStream_t st) {
  constexpr int kLdsSteps = 160;   // transforms resident per pass: 3 x 160 x 96 B = 45 KiB of LDS
  ATDN_CHECK(B >= 1 && T >= 1, "clvo loss: empty batch or sequence");
  ATDN_CHECK(w >= 1 && w <= T, "clvo loss: the composite window needs 1 <= w <= sequence length");
  ATDN_CHECK(T <= kLdsSteps, "clvo loss: sequence length above 160");
  const int cpp = std::min(B, kLdsSteps / T);
  const size_t lds = (size_t)3 * cpp * T * sizeof(composite::Affine);
  hipLaunchKernelGGL(clvo_loss_composite_kernel, dim3(1), dim3(256), lds, st, pred_rot, pred_tr, true_rot, true_tr, B, T, w, alpha,
                     with_grad ? 1 : 0, step_major ? 1 : 0, cpp, loss3, d_rot, d_tr);
  ATDN_HIP(hipGetLastError());
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             long n, float lr, float wd, float eps, float b1, float b2, float bc1, float sqrt_bc2) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gr = g[i];
  float pv = p[i] * (1.f - lr * wd);
  const float mv = b1 * m[i] + (1.f - b1) * gr;
  const float vv = b2 * v[i] + (1.f - b2) * gr * gr;
  m[i] = mv;
  v[i] = vv;
  const float denom = sqrtf(vv) / sqrt_bc2 + eps;
  pv -= (lr / bc1) * (mv / denom);
  p[i] = pv;
}
void launch_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float wd, float eps, float beta1, float beta2,
                  int t, hipStream_t st) {
  const double bc1 = 1.0 - std::pow((double)beta1, (double)t), bc2 = 1.0 - std::pow((double)beta2, (double)t);
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, st, p, g, m, v, n, lr, wd, eps, beta1, beta2,
                     (float)bc1, (float)std::sqrt(bc2));
  ATDN_HIP(hipGetLastError());
}

}  // namespace atdn
