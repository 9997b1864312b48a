// Mish for the CLVO encoder's training and statistics kernels (train_kernels.hip, conv16.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace atdn {

// Mish and its derivative from ONE exponential: with n = e^x, tanh(softplus(x)) = t/(t+2), t = n(n+2).
// (The library formula x*tanh(log1p(exp(x))) costs ~40 instructions per element and made the BatchNorm passes
// ALU-bound at 0.9 TB/s; the two forms agree to a few ulp.)
struct MishVal { float y, dy; };
__device__ __forceinline__ MishVal mish_both(float x) {
  if (x > 20.0f) return {x, 1.0f};
  // (round 5: v_rcp_f32 — 1 ulp — instead of the two IEEE divisions, ~10 instructions each: the statistics taken inside the
  // convolution kernels pay for every vector instruction of their epilogue)
  const float n = __expf(x);
  const float t = n * (n + 2.0f);
  const float th = t * __builtin_amdgcn_rcpf(t + 2.0f);
  const float sg = n * __builtin_amdgcn_rcpf(1.0f + n);
  return {x * th, th + x * (1.0f - th * th) * sg};
}
__device__ __forceinline__ float mish_fast(float x) { return mish_both(x).y; }
__device__ __forceinline__ float mish_grad(float x) { return mish_both(x).dy; }

}  // namespace atdn
