// The conv16 family: the 16-channel convolutions of the CLVO encoder (odometry/network.py:63-73) on v_mfma_f32_16x16x4_f32.
// Inference (clvo.hip, eval-mode tails fused into the store) and training (clvo_train.hip: forward with BatchNorm statistics,
// data gradients) run the same kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace atdn {
// ---- 16 -> 16 channel convolution on NHWC16 maps with v_mfma_f32_16x16x4_f32 (exact fp32): the thin convolutions of
// the CLVO encoder fill a 32x32 MFMA tile to a quarter (N = 16, K rows padded 48 -> 64); here N is exactly one
// 16-column tile, K = KH*KW*16 needs no padding, the whole weight tensor sits in operand registers for the lifetime
// of the block and the input is read from an LDS halo patch with one ds_read_b128 per tap and 16-pixel tile.
// w: OIHW [16][16][K][K]; transposed = use w[c][n][K-1-ky][K-1-kx] instead (data gradient of a convolution).
// z[img][oy][ox][n] = bias[n] + sum x[img][oy*S - pad + ky][ox*S - pad + kx][c] * w(n, c, ky, kx)
// the 7x7 stride-2 pad-3 stem (2 -> 16 channels) on NHWC4 input, same MFMA; w: OIHW [16][2][7][7]
// eval-mode tail fused into the store (inference head): BN(Mish(.)) with the folded affine sc/sh, and with `skip`
// ([nimg][Ho][Wo][16]) the ResidualConv tail BN2(Mish(BN1(Mish(.)) + skip))
struct Conv16Tail {
  const float* sc = nullptr; const float* sh = nullptr;
  const float* skip = nullptr; const float* sc2 = nullptr; const float* sh2 = nullptr;
};
// Training forward only: BatchNorm statistics of Mish(z) taken in the producing kernel (see c16_stat_flush in conv16.hip).
// `part` [groups][rows][2][16] with `capacity` floats; the launcher zeroes what it uses and sets `rows` (partial rows per group) for
// launch_bn_finalize (train_kernels.h). group_imgs = images per statistics group (the images of one time step).
struct Conv16Stats {
  float* part = nullptr; int group_imgs = 1; long capacity = 0; int rows = 0;
};
void launch_stem16(const float* x4, int nimg, int H, int W, const float* w, const float* bias, float* z, hipStream_t st,
                   const Conv16Tail* tail = nullptr, Conv16Stats* stat = nullptr);
// data gradient of a stride-2 16 -> 16 convolution (w OIHW, K = 3 pad 1 or K = 1 pad 0): dx [nimg][H][W][16] from
// dz [nimg][Ho][Wo][16]; accumulate: dx += instead of dx =
void launch_tconv16_s2(const float* dz, int nimg, int Ho, int Wo, const float* w, int K, int pad, int H, int W, bool accumulate,
                       float* dx, hipStream_t st);
void launch_conv16(const float* x, int nimg, int H, int W, const float* w, bool transposed, const float* bias, int K, int S,
                   int pad, float* z, hipStream_t st, bool accumulate = false,   // accumulate: z += instead of z =
                   Conv16Stats* stat = nullptr);
// the same convolution with an eval-mode tail: K = 3 with S = 1 or 3 (Conv blocks), K = 3, S = 2 with tail.skip (ResidualConv)
void launch_conv16_eval(const float* x, int nimg, int H, int W, const float* w, const float* bias, int K, int S, int pad,
                        const Conv16Tail& tail, float* z, hipStream_t st);
}  // namespace atdn
