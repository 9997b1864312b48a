// Kernels of the CLVO training step other than the 16-channel convolutions' forward and data-gradient passes (conv16.h):
// train-mode BatchNorm + Mish forward and backward on NHWC16 maps with per-call statistics groups, zero-stuffing for the
// stride-3 transposed convolution, weight gradients of the thin convolutions, small dense GEMMs, LSTM cell forward/backward,
// loss and AdamW. Used by clvo_train.hip.
// Reference semantics: torch.nn.BatchNorm2d (training), nn.Mish, nn.LSTMCell, odometry/loss.py, torch.optim.AdamW.
#pragma once
#include <hip/hip_runtime.h>

namespace atdn {

// ---- train-mode BatchNorm over NHWC16 maps; G statistic groups of P pixels each (a group = one forward() call)
constexpr int BN_C = 16;
int bn_partial_blocks(long P);  // blocks per group the backward reduction kernels use
// Forward statistics are taken by the kernel that writes the layer's input: part[G][rows][2][16] holds per-group partial sums
// and sums of squares of mish(z), `rows` of them per group (Conv16Stats::rows, or bn_apply_partial_rows(P) after
// launch_bn_apply(..., next_part)).
// mean/rstd [G][16]; running stats updated sequentially over the G calls (momentum 0.1, unbiased variance)
// (var_scratch: [G][16] floats, the groups' unbiased variances between the two launches)
void launch_bn_finalize(const float* part, int G, int rows, long P, float* running_mean, float* running_var, float* mean,
                        float* rstd, float* var_scratch, hipStream_t st);
// y = (act(z) - mean) * rstd * gamma + beta (+ add), act = mish or identity.
// next_part (optional, [G][bn_apply_partial_rows(P)][2][16]): sums of Mish(y), Mish(y)^2 — the statistics of a BatchNorm that
// follows y directly (ResidualConv.out_block: bn(mish(x + skip)), layers/conv.py:78-80,88)
int bn_apply_partial_rows(long P);
void launch_bn_apply(const float* z, int G, long P, bool mish, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* add, float* y, hipStream_t st, float* next_part = nullptr);
// backward: part[G][nblk][2][16] = sum dy, sum dy*xhat
void launch_bn_bwd_stats(const float* dy, const float* z, int G, long P, bool mish, const float* mean, const float* rstd,
                         float* part, hipStream_t st);
// sums[G][2][16] from the partials; dgamma += sum_g sum dy*xhat, dbeta += sum_g sum dy
void launch_bn_bwd_finalize(const float* part, int G, long P, float* sums, float* dgamma, float* dbeta, hipStream_t st);
// dz = gamma*rstd*(dy - sum_dy/P - xhat*sum_dyx/P) * act'(z); part_db[G][nblk][16] = per-block sums of dz
void launch_bn_bwd_apply(const float* dy, const float* z, int G, long P, bool mish, const float* mean, const float* rstd,
                         const float* gamma, const float* sums, float* dz, float* part_db, hipStream_t st);
// out[16] += sum over G*nblk partial rows of 16
void launch_sum_partials16(const float* part, long rows, float* out, hipStream_t st);

// ---- transposed convolution support
// D[img][Hs][Ws][16] = dz[img][y/s][x/s][:] where y, x are multiples of s inside the Ho x Wo map, else 0
void launch_zero_stuff(const float* dz, int nimg, int Ho, int Wo, int stride, int Hs, int Ws, float* D, hipStream_t st);
void launch_add_inplace(float* a, const float* b, long n, hipStream_t st);

// ---- weight gradient of a thin convolution: x [nimg][H][W][Cpix] (Cin real channels), dz [nimg][Ho][Wo][16]
// dW[n][c][ky][kx] += sum dz[.,oy,ox,n] * x[., oy*s - pad + ky, ox*s - pad + kx, c]   (OIHW, N = 16)
// scratch: at least wgrad_scratch_floats(...) floats
long wgrad_scratch_floats(int nimg, int Ho, int Cin, int KH, int KW);
void launch_conv_wgrad(const float* x, int Cpix, int Cin, int nimg, int H, int W, const float* dz, int Ho, int Wo, int KH,
                       int KW, int stride, int pad, float* scratch, float* dW, hipStream_t st);
// depthwise 1x1 in front of the encoder: x0[c] = xn[c]*w[c] + b[c] with xn = flow/std. Its gradients and the stem
// conv's weight gradient all follow from A = conv_wgrad of the stem taken on the auxiliary input (xn0, xn1, 1)
// (launch_prep_flow_aux, Cin = 3): see stem_combine_kernel. No data gradient of the stem conv is ever formed.
void launch_prep_flow_aux(const float* flow, int nimg, int H, int W, float* out4, hipStream_t st);
void launch_stem_combine(const float* A /*[16][3][taps]*/, const float* W1 /*[16][2][taps]*/, const float* w, const float* b,
                         int taps, float* dW1, float* dw, float* db, hipStream_t st);

// ---- dense algebra on small matrices (row-major): C[M][N] = beta*C + op(A)*op(B) (+ bias[N] broadcast over rows)
void launch_gemm(bool transA, bool transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                 int ldc, float beta, const float* bias, hipStream_t st);
void launch_colsum(const float* X, int rows, int cols, int ld, float* out /* += */, hipStream_t st);
void launch_mish_fwd(const float* z, float* a, long n, hipStream_t st);
void launch_mish_bwd(const float* dy, const float* z, float* dz, long n, hipStream_t st);
// [nimg][P][16] <-> [nimg][16][P]
void launch_nhwc_to_chw(const float* src, int nimg, int P, float* dst, hipStream_t st);
void launch_chw_to_nhwc(const float* src, int nimg, int P, float* dst, hipStream_t st);

// ---- LSTM cell (torch gate order i, f, g, o; hidden 512). pre[B][2048] = x W_ih^T + h W_hh^T + b_ih + b_hh
// act[B][2048] (sigmoid/tanh applied), c_out = f*c_in + i*g, tanhc = tanh(c_out), h_out = o*tanhc
void launch_lstm_fwd(const float* pre, const float* c_in, int B, float* act, float* c_out, float* tanhc, float* h_out,
                     hipStream_t st);
// dpre[B][2048], dc_in[B][512] from dh[B][512] (all consumers summed), dc_out[B][512] (from the next step; may be null)
void launch_lstm_bwd(const float* dh, const float* dc_out, const float* act, const float* c_in, const float* tanhc, int B,
                     float* dpre, float* dc_in, hipStream_t st);

// ---- loss (odometry/loss.py, alpha = 1): L = mean_b sum_t (delta*|dt|^2 + khi*|dr|^2); also the gradients
void launch_clvo_loss(const float* pred_rot, const float* pred_tr, const float* true_rot, const float* true_tr, int B, int T,
                      float* loss /*[1]*/, float* d_rot, float* d_tr, hipStream_t st);
// ---- loss with the composite term (CLVO_Loss(alpha, w); clvo_composite.h): L = mean_b(alpha*L_rel + (1-alpha)*L_com), L_com the
// same weighted error on the product of every window of w consecutive transforms, converted back to Euler + translation.
// with_grad false: the composite term leaves the gradients alone, as in the reference's detached graph (d = alpha x the above);
// true: its hand-derived gradient is added. step_major: predictions and gradients are rows r = t*B + b (the trainer's layout),
// else [B][T][3] like the targets. loss3 = {L, mean_b L_rel, mean_b L_com} (device). One launch, deterministic; 1 <= w <= T <= 160.
void launch_clvo_loss_composite(const float* pred_rot, const float* pred_tr, const float* true_rot, const float* true_tr, int B, int T,
                                float alpha, int w, bool with_grad, bool step_major, float* loss3 /*[3]*/, float* d_rot, float* d_tr,
                                hipStream_t st);

// ---- AdamW (torch.optim.AdamW, amsgrad off) on a flat range; t = 1-based step
void launch_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float wd, float eps, float beta1,
                  float beta2, int t, hipStream_t st);

}  // namespace atdn
