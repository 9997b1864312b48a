/* libatdn_hip — C ABI of the MI355X-native ATDN vSLAM visual-odometry inference path.
 *
 * The reference has no FFI layer: its boundary is two Python nn.Module call contracts. Each entry point
 * below names the reference interface it stands in for. All tensor arguments are raw DEVICE pointers to
 * dense fp32 buffers (tensor.data_ptr()) unless marked host; `stream` is a hipStream_t
 * (torch.cuda.current_stream().cuda_stream), 0/NULL = the default stream.
 *
 * Every function returns 0 on success and non-zero on error; atdn_last_error() then holds the message
 * (thread-local). Handles are not re-entrant: one handle per (device, thread), like the reference modules.
 */
#ifndef ATDN_HIP_H
#define ATDN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct atdn_gma atdn_gma;   /* RAFTGMA flow network handle */
typedef struct atdn_clvo atdn_clvo; /* ATDNVO pose head handle */
typedef struct atdn_vae atdn_vae;   /* MappingVAE encoder handle (relocalisation embedding) */
typedef struct atdn_clvo_trainer atdn_clvo_trainer; /* ATDNVO training-iteration handle */

int atdn_version(void);
const char* atdn_last_error(void);

/* ---------------------------------------------------------------------------------------------------
 * GMA optical flow  —  replaces torch.nn.DataParallel(RAFTGMA(GMA_Parameters()))
 *   construction + checkpoint: atdn_vslam/slam_framework/neural_slam.py:51-53
 *   forward:                   whl:GMA/core/network.py:72-129 (called at neural_slam.py:202,395)
 * ------------------------------------------------------------------------------------------------- */

/* H, W: frame size after the caller's resize/pad (multiples of 8, each at least 128; 376x1232 in NeuralSLAM,
 * neural_slam.py:54,198-199). Below 128 level 3 of the correlation pyramid (H/64 x W/64 cells) is one cell high or wide, and
 * the reference's bilinear_sampler divides by H/64 - 1 = 0 there (utils/utils.py:63-64): its flow is NaN, so there is nothing
 * to reproduce and atdn_gma_create refuses the size. max_batch: largest number of frame pairs per forward.
 * precision: ATDN_PRECISION_F32 = every GEMM on the exact-fp32 matrix core (v_mfma_f32_32x32x2_f32);
 *            ATDN_PRECISION_SPLIT_F16 = every channel-wide GEMM as three f16 MFMAs on split operands
 *            (x = hi + lo, fp32 accumulate): fp32-grade results at 5.3x the matrix rate (the default);
 *            ATDN_PRECISION_F16 = the fast mode: the same kernels and tensors, but only the hi x hi MFMA of every
 *            product (plain f16 operands, fp32 accumulate) — what the reference itself runs on a GPU under
 *            `mixed_precision` autocast (utils/gma_parameters.py:11); flow within ~1e-2 px of the fp32 CPU path;
 *            ATDN_PRECISION_SPLIT_F16_TWO_PASS = split-f16 arithmetic on the f16 mode's op sequence: the two-pass stem
 *            (statistics, then recompute + normalise) and separate normalisation passes in the feature network instead of
 *            normalise-on-load. Kept for verification: it is the only way to hold that precision-independent plumbing, which
 *            otherwise only the f16 mode runs, to the fp32-grade yardstick; slower than ATDN_PRECISION_SPLIT_F16. */
#define ATDN_PRECISION_F32 0
#define ATDN_PRECISION_SPLIT_F16 1
#define ATDN_PRECISION_F16 2
#define ATDN_PRECISION_SPLIT_F16_TWO_PASS 3
int atdn_gma_create(atdn_gma** out, int H, int W, int max_batch, int precision);

/* Low-latency form for the reference's per-frame call pattern — NeuralSLAM.__call__ runs the flow network on ONE pair per
 * frame (neural_slam.py:202; evaluate_odometry.py:63-66 likewise): launches that would leave most of the chip idle at one to
 * four pairs are cut finer (attention x V along its key axis, with fp32 partial sums). Same results within rounding (another
 * summation order: 8e-5 px at KITTI size after 12 iterations), NOT bit-identical to the default path, whose clip / continued / pair modes are bit-identical to
 * each other. Call between atdn_gma_create and atdn_gma_finalize; `on` = 0 / 1. */
int atdn_gma_set_low_latency(atdn_gma* h, int on);

/* One state-dict entry (load_state_dict, neural_slam.py:52). `key` as in the checkpoint, with or without the
 * DataParallel "module." prefix; `data` is a HOST fp32 buffer of the given shape. Non-float buffers
 * (num_batches_tracked, rel_ind) need not be passed. */
int atdn_gma_load(atdn_gma* h, const char* key, const float* data, const int64_t* shape, int rank);

/* Packs weights for the MFMA kernels (BatchNorm folded), uploads them, allocates the HBM workspace. */
int atdn_gma_finalize(atdn_gma* h);

/* flow_low, flow_up = flow_net(image1, image2, iters=iters, flow_init=flow_init, test_mode=True)
 *   im1, im2   [B,3,H,W]   RGB 0..255
 *   flow_init  [B,2,H/8,W/8] or NULL          (network.py:103-104)
 *   flow_low   [B,2,H/8,W/8], flow_up [B,2,H,W]; channel 0 = x flow, 1 = y flow */
int atdn_gma_forward(atdn_gma* h, const float* im1, const float* im2, int B, int iters, const float* flow_init,
                     float* flow_low, float* flow_up, void* stream);

/* flow_predictions = flow_net(image1, image2, iters=iters, flow_init=flow_init, test_mode=False)   (network.py:106-129:
 * the training-time return of RAFTGMA.forward — the convex upsampling of EVERY iteration's flow with that iteration's mask)
 *   flow_predictions  [iters,B,2,H,W]; slice iters-1 equals atdn_gma_forward's flow_up
 * The mask head runs once per iteration in this call (atdn_gma_forward needs only the last one's); launched kernel by kernel,
 * not as a graph. Inference only: no gradients are produced. */
int atdn_gma_forward_predictions(atdn_gma* h, const float* im1, const float* im2, int B, int iters, const float* flow_init,
                                 float* flow_predictions, void* stream);

/* The same for B consecutive pairs of one clip, as NeuralSLAM walks a sequence (neural_slam.py:196-217: frame t is
 * image2 of pair t-1 and image1 of pair t): frames [B+1,3,H,W]; pair b = (frames[b], frames[b+1]). The feature
 * network runs once per frame instead of twice. Split-f16 handles only. */
int atdn_gma_forward_sequence(atdn_gma* h, const float* frames, int B, int iters, const float* flow_init,
                              float* flow_low, float* flow_up, void* stream);
/* The same for the NEXT clip of one sequence on this handle: frames[0] must be the frame that was frames[B] of the
 * previous atdn_gma_forward_sequence(_continued) call; its features are reused (device-side copy) and the feature
 * network runs on frames[1..B] only, so every frame of a long sequence passes through it exactly once. Results equal
 * the non-continued call's (and atdn_gma_forward's) bit for bit: no kernel's summation order depends on how many images
 * share a launch. */
int atdn_gma_forward_sequence_continued(atdn_gma* h, const float* frames, int B, int iters, const float* flow_init,
                                        float* flow_low, float* flow_up, void* stream);

/* Copies an internal activation to a HOST buffer for parity tests ("fmap", "pyr0".."pyr3", "attn", "net",
 * "x", "corrfeat", "cor1" (relu(convc1(lookup)) of the last iteration), "mask", "coords1", "flow4", "qk", "img4"). Returns the number of floats copied, -1 on error.
 * "sf_clamped" returns ONE float: how many values the split-f16 storage format had to clamp (|x| > 65504, or NaN)
 * on this device since the last such read, and resets the count — non-zero means the activations of this checkpoint
 * left the format's range and results are not fp32-grade (use ATDN_PRECISION_F32). */
long atdn_gma_debug_read(atdn_gma* h, const char* name, float* host, long capacity, void* stream);

/* Per-stage device time (ms, summed over `reps` eager forwards of batch B), measured with HIP events on
 * `stream`. ms_out has ATDN_GMA_STAGES entries: fnet, corr, pool, cnet, attention (row softmax), lookup, motion_encoder
 * (without convc1), aggregate (the attention x V kernel alone), gru_zr (fused z|r convolution, horizontal 1x5 pass),
 * gru_q (horizontal pass), flow_head, mask, gru_ctx (once-per-pair context part of the GRU convolutions; split-f16
 * pipeline only), attn_logits (q,k projection + first QK^T sweep), agg_vt (the v^T projection in front of attention x V; zero since
 * attention x V reads the motion features as stored and to_v lives in the ConvGRU weights),
 * convc1 (the 1x1 convolution behind the lookup; zero when it is fused into the lookup), gru_zr_v / gru_q_v (the vertical
 * 5x1 passes).
 * Stages that hold launches of ONE kernel (aggregate, gru_zr, gru_zr_v, gru_q, gru_q_v, lookup, corr) divide into
 * per-launch times. */
#define ATDN_GMA_STAGES 18
int atdn_gma_profile(atdn_gma* h, int B, int iters, int reps, float* ms_out, void* stream);
/* The same for one of the three call forms: mode 0 = atdn_gma_forward (pair mode, 2B feature-network passes; what
 * atdn_gma_profile times), 1 = atdn_gma_forward_sequence (B + 1 passes), 2 = atdn_gma_forward_sequence_continued (B passes:
 * a continued clip of a long sequence, the form bench.py times). Split-f16 / f16 handles only for modes 1 and 2. */
int atdn_gma_profile_mode(atdn_gma* h, int B, int iters, int reps, int mode, float* ms_out, void* stream);

/* Range report (how far a checkpoint's activations are from the 65504 limit of the split-f16 format, BEFORE it clamps).
 * atdn_gma_set_range_probe switches the probe of an ATDN_PRECISION_F32 handle on / off (`on` = 1 / 0; any other precision is
 * an error that says why: only the exact-fp32 path writes every intermediate tensor as plain fp32 and never clamps). While it
 * is on, atdn_gma_forward (and atdn_gma_forward_predictions) launch kernel by kernel instead of replaying a graph, and after
 * every producing launch a reduction kernel takes (max |x|, finite values with |x| > 65504, non-finite values) of the valid part
 * of the tensor just written; the call returns after the stream has been synchronised and the table read back. Switched off
 * again (the default) the handle launches exactly what it did before, and gives the same bits.
 *   atdn_gma_range_rows   number of rows of the last probed forward (0 before one), -1 on error
 *   atdn_gma_range_row    row `index` in execution order: `name` (the reference's module path, e.g. "fnet.layer2.0.conv1.raw",
 *                         "corr.0", "gru.h2"; NUL-terminated into a HOST buffer of name_capacity bytes, 64 suffice),
 *                         `iteration` (0-based refinement iteration, -1 for tensors written outside the loop: one row per tensor
 *                         there, one row per tensor and iteration inside it), `limited` (1: the default split-f16 path keeps
 *                         this tensor, or values that are this tensor's one to one, in the range-limited format; 0: it holds it
 *                         in plain fp32 or never has it in memory — "att.logits", "corr.0".."corr.3"), `max_abs` (largest finite
 *                         magnitude), `over` (finite values with |x| > 65504; 65504 itself is not counted), `nonfinite` (infinities
 *                         and NaNs; they do not enter max_abs). All outputs are HOST pointers. */
int atdn_gma_set_range_probe(atdn_gma* h, int on);
long atdn_gma_range_rows(atdn_gma* h);
int atdn_gma_range_row(atdn_gma* h, long index, char* name, int name_capacity, int* iteration, int* limited, float* max_abs,
                       int64_t* over, int64_t* nonfinite);
/* The reduction kernel on a caller's DEVICE tensor: `rows` rows of `cols` fp32 values, row pitch `ld` floats (ld >= cols unless
 * rows <= 1), starting at any 4-byte boundary; 64-bit element indexing. A pure read.
 *   atdn_range_probe         allocates and zeroes a slot, launches, synchronises `stream`, writes the three results (HOST pointers)
 *   atdn_range_probe_launch  the launch alone, adding into `slot`: 24 bytes of DEVICE memory { uint32 max_bits; uint32 unused;
 *                            uint64 over; uint64 nonfinite } that the caller zeroed (maximum and sums accumulate over launches) */
int atdn_range_probe(const float* x, int64_t rows, int64_t cols, int64_t ld, float* max_abs, int64_t* over, int64_t* nonfinite,
                     void* stream);
int atdn_range_probe_launch(const float* x, int64_t rows, int64_t cols, int64_t ld, void* slot, void* stream);

size_t atdn_gma_workspace_bytes(atdn_gma* h);
void atdn_gma_destroy(atdn_gma* h);

/* Diagnostic: bytes of device memory the library's buffer owners hold at this moment, over every handle and device of the
 * process (workspaces, weight arenas, on-demand scratch, the per-call scratch of the unit entries while they run). A handle's
 * create / finalize / calls raise it, its destroy takes it back to the value from before the create: a leak test compares the
 * two exactly. Not counted: the three process-lifetime blocks the library never frees (a 256-byte line of zeros, the split-f16
 * saturation counter, the cached resize tables). Thread-safe. */
int64_t atdn_device_bytes_live(void);

/* ---------------------------------------------------------------------------------------------------
 * CLVO pose head  —  replaces ATDNVO()  (atdn_vslam/odometry/network.py:20-162)
 *   construction: evaluate_odometry.py:124, neural_slam.py:57-59 ; forward: network.py:122-146
 * The module's hidden LSTM attributes become an explicit state tensor so the stateless CNN encoder can be
 * sharded over frame pairs while the recurrence runs as one ordered scan.
 * ------------------------------------------------------------------------------------------------- */

/* H, W: flow size (must reduce to a 16x4x13 map: H in [353,448], W in [1217,1312]); else an error like the
 * reference's Linear(832) shape error. */
int atdn_clvo_create(atdn_clvo** out, int H, int W, int max_batch);
int atdn_clvo_load(atdn_clvo* h, const char* key, const float* data, const int64_t* shape, int rank);
int atdn_clvo_finalize(atdn_clvo* h);

/* features = encoder_CNN(normalize_flow(flows))   (network.py:131-134): flow [B,2,H,W] -> feat [B,512] */
int atdn_clvo_encode(atdn_clvo* h, const float* flow, int B, float* feat, void* stream);

/* T ordered recurrent steps (network.py:137-146) for Bs independent sequences:
 *   feat [T,Bs,512]; state [4,Bs,512] = lstm1_h, lstm1_c, lstm2_h, lstm2_c (in/out; zeros == reset_lstm());
 *   rot, tr [T,Bs,3] (Euler yxz radians, translation). */
int atdn_clvo_step(atdn_clvo* h, const float* feat, int T, int Bs, float* state, float* rot, float* tr, void* stream);
/* Which route the last atdn_clvo_step of this handle took (host bookkeeping only): 0 no step yet, 1 per-step kernel launched
 * eagerly, 2 per-step kernel replayed from a captured graph, 3 persistent scan (one launch per sequence), 4 persistent scan that
 * gave up, the sequence repeated on the per-step kernel. A null handle reports 0. */
int atdn_clvo_last_scan_path(atdn_clvo* h);
void atdn_clvo_destroy(atdn_clvo* h);

/* ---------------------------------------------------------------------------------------------------
 * CLVO training iteration  —  replaces the body of train() in train_odometry.py:21-49 for one batch:
 *   model.train(); T x model(fl[:, j]) with the LSTM state carried; CLVO_Loss(alpha, w); loss.backward();
 *   optimizer.step() (AdamW, train_odometry.py:99); model.reset_lstm().
 * The loss is CLVO_Loss(alpha = 1) (relative-pose term only) until atdn_clvo_trainer_set_loss chooses the composite term:
 *   L = mean_b(alpha * L_rel + (1 - alpha) * L_com), L_com summed over every window of w consecutive steps: the w predicted
 *   transforms chained, likewise the true ones, both products converted back to Euler yxz + translation (matrix2euler), and the
 *   same 1 * |d tr|^2 + 100 * |d euler|^2 taken (no angle wrapping).
 *   mode 0 ("reference"): the composite term enters the loss value only; the gradients are alpha x those of alpha = 1 (the
 *     reference builds its matrices and Euler vectors with torch.tensor(...), which cuts the graph).
 *   mode 1 ("gradient"): the composite term contributes its true gradient, (1 - alpha)/batch * dL_com/d(pred_rot, pred_tr).
 *   The radicand 1 - C12^2 of matrix2euler is clamped at 0 for the value and at FLT_EPSILON in the derivative (the reference
 *   returns NaN there). With alpha == 1 the composite term is not evaluated at all, whatever w and mode say.
 * BatchNorm layers use per-call batch statistics and update their running averages (momentum 0.1), as torch does.
 * Gradients sit in ONE flat device buffer (`atdn_clvo_trainer_gradients`): data-parallel training all-reduces that
 * buffer (RCCL, averaged over ranks) between forward_backward and adamw_step — see atdn_vslam_amd/training.py.
 * State-dict keys as in ATDNVO().state_dict().
 * ------------------------------------------------------------------------------------------------- */
int atdn_clvo_trainer_create(atdn_clvo_trainer** out, int H, int W, int batch, int sequence_length);
int atdn_clvo_trainer_load(atdn_clvo_trainer* h, const char* key, const float* data, const int64_t* shape, int rank);
int atdn_clvo_trainer_finalize(atdn_clvo_trainer* h);
/* flows [batch, T, 2, H, W], true_rot / true_tr [batch, T, 3] (device). Returns the loss; pred_rot / pred_tr
 * [batch, T, 3] (device) are optional. Overwrites the gradient buffer, advances the BatchNorm running statistics. */
int atdn_clvo_trainer_forward_backward(atdn_clvo_trainer* h, const float* flows, const float* true_rot, const float* true_tr,
                                       float* pred_rot, float* pred_tr, float* loss_out, void* stream);
int atdn_clvo_trainer_gradients(atdn_clvo_trainer* h, float** device_ptr, long* count);
/* Selects the loss of the forward_backward calls that follow (see above). Fails for w < 1, w > sequence_length, mode not 0 / 1. */
int atdn_clvo_trainer_set_loss(atdn_clvo_trainer* h, float alpha, int w, int mode);
/* {L, mean_b L_rel, mean_b L_com} of the last forward_backward (host); fails unless that call ran with alpha != 1. */
int atdn_clvo_trainer_loss_terms(atdn_clvo_trainer* h, float* terms3_host);
/* The loss on its own: pred_rot, pred_tr, true_rot, true_tr and the gradients d_rot, d_tr are [B, T, 3] device fp32;
 * loss3_host receives {L, mean_b L_rel, mean_b L_com}. One kernel launch, deterministic (no atomics); synchronises the stream.
 * Fails for w < 1, w > T, T > 160 or a mode other than 0 / 1. */
int atdn_clvo_loss(const float* pred_rot, const float* pred_tr, const float* true_rot, const float* true_tr, int B, int T, float alpha,
                   int w, int mode, float* loss3_host, float* d_rot, float* d_tr, void* stream);
/* torch.optim.AdamW (betas 0.9 / 0.999) on every parameter forward() uses; step is 1-based */
int atdn_clvo_trainer_adamw_step(atdn_clvo_trainer* h, float lr, float weight_decay, float eps, int step, void* stream);
/* copy a named tensor to the host: kind 0 parameter, 1 gradient, 2 BatchNorm running statistic; returns the count or -1 */
long atdn_clvo_trainer_read(atdn_clvo_trainer* h, const char* key, int kind, float* host, long capacity, void* stream);
void atdn_clvo_trainer_destroy(atdn_clvo_trainer* h);

/* ---------------------------------------------------------------------------------------------------
 * MappingVAE encoder  —  replaces the embedding half of atdn_vslam/localization/network.py `MappingVAE.forward`
 * (57-70, non-variational: mu = mean_lin(encoder(get_rgb_norm()(image)))), which NeuralSLAM's relocalisation
 * evaluates for every keyframe and query (slam_framework/neural_slam.py:88-103,158-164,355-383). State-dict keys
 * as in MappingVAE().state_dict() (encoder.*, mean_lin.*); decoder.* keys are accepted and ignored by the host
 * mirror (the decoder only feeds the VAE's training loss, which stays on stock PyTorch).
 * ------------------------------------------------------------------------------------------------- */
int atdn_vae_create(atdn_vae** out, int H, int W, int max_batch);
int atdn_vae_load(atdn_vae* h, const char* key, const float* data, const int64_t* shape, int rank);
int atdn_vae_finalize(atdn_vae* h);
/* size of the embedding map: six stride-2 blocks, 376x1232 -> 6x20 */
int atdn_vae_embedding_shape(const atdn_vae* h, int* out_h, int* out_w);
/* images [B,3,H,W] float32 with values 0..255 (device) -> mu [B][out_h*out_w][128] channels-last (device) */
int atdn_vae_encode(atdn_vae* h, const float* images, int B, float* mu, void* stream);
/* The encoder's layer plan for H x W frames (host only, no handle, no GPU): stages[3k .. 3k+2] = height, width and floats per
 * pixel of what stage k writes (k = 0: the 7x7 stem, 1..6: the stride-2 residual blocks; 3 channels travel as 4, pad lane 0),
 * floats[0..3] = floats per image of the four scratch buffers of a handle: the normalised frames, the stem / block outputs,
 * the first convolution of a block (at the block's input size), the skip convolution. A stride-2 layer writes
 * ceil(h/2) x ceil(w/2) pixels, so odd sizes need more than H*W*4. floats [4], stages [21]; 1 <= H, W and H*W <= 2^24. */
int atdn_vae_scratch_floats(int H, int W, long* floats, int* stages);
/* Tests only: runs the encoder up to stage k and copies that stage's output, as the next layer reads it, to out (DEVICE,
 * `capacity` floats >= B * stages[3k] * stages[3k+1] * stages[3k+2]): channels-last [B][h][w][floats per pixel]. */
int atdn_vae_debug_stage(atdn_vae* h, const float* images, int B, int stage, float* out, long capacity, void* stream);
void atdn_vae_destroy(atdn_vae* h);

/* ---------------------------------------------------------------------------------------------------
 * Pose algebra (host, no GPU)  —  replaces atdn_vslam/utils/transforms.py
 * ------------------------------------------------------------------------------------------------- */

/* transform(rot, tr) (transforms.py:97-119, euler2matrix "yxz" :79-81): HOST rot[3], tr[3] -> row-major 4x4 */
int atdn_pose_transform_f32(const float* rot, const float* tr, float* mat16);
/* rel2abs (transforms.py:147-170): HOST rot[T,3], tr[T,3] -> poses [T+1,4,4] float64, identity first */
int atdn_pose_rel2abs(const float* rot, const float* tr, int T, double* poses);
/* NeuralSLAM's running pose (neural_slam.py:204-207): pose(4x4 fp32, in/out) = pose @ transform(rot, tr) */
int atdn_pose_accumulate_f32(float* pose16, const float* rot, const float* tr);

/* ---------------------------------------------------------------------------------------------------
 * Frame front-end  —  replaces, per camera frame, `im.to(device)`, `TF.resize(im, (376, 1232))` and
 * `InputPadder.pad` (neural_slam.py:197-199,219-221; whl:GMA/core/utils/utils.py:8-20)
 * ------------------------------------------------------------------------------------------------- */

/* torchvision's tensor resize is bilinear, align_corners = False; it antialiases from torchvision 0.17 on
 * (F.interpolate(..., antialias=True)) and does not before that. The reference pins no version
 * (/root/reference/pyproject.toml:14-16), so both are served; ANTIALIAS is the default everywhere. */
#define ATDN_RESIZE_BILINEAR 0
#define ATDN_RESIZE_ANTIALIAS 1

/* src [planes,Hin,Win] (planes = any product of leading dims, e.g. B*3) -> dst [planes,Hout,Wout]; antialiased.
 * Weight tables are cached per (device, geometry, mode); no intermediate buffer: safe on any number of streams.
 * RATIO LIMIT (ANTIALIAS only): a weight table holds 8 taps per output pixel, which serves every down-scaling ratio up to and
 * including 4x per axis (at 4x each pixel has exactly 8 taps). A geometry in which some output pixel needs more (129 -> 32
 * already does) is refused with an error by these calls and by atdn_ingest_create, and dst is left untouched. Up-scaling
 * and ATDN_RESIZE_BILINEAR (two taps) have no limit. */
int atdn_resize_frames(const float* src, int planes, int Hin, int Win, int Hout, int Wout, float* dst, void* stream);
int atdn_resize_frames_mode(const float* src, int planes, int Hin, int Win, int Hout, int Wout, int antialias, float* dst,
                            void* stream);
/* the same from uint8 pixels already on the device (the conversion to fp32 is fused into the resize) */
int atdn_resize_frames_u8(const uint8_t* src, int planes, int Hin, int Win, int Hout, int Wout, int antialias, float* dst,
                          void* stream);

/* F.pad(x, [left, right, top, bottom], mode="replicate") as InputPadder.pad applies it (utils.py:19-20):
 * src [planes,H,W] -> dst [planes,H+top+bottom,W+left+right] */
int atdn_pad_frames(const float* src, int planes, int H, int W, int left, int right, int top, int bottom, float* dst,
                    void* stream);

/* uint8 camera frames in HOST memory -> fp32 frames at the network size on the device, in one call:
 * asynchronous H2D copy (pinned host memory; pageable memory works but serialises) on the handle's own copy stream
 * into one of two device staging slots, then resize + uint8->fp32 on `stream`. Consecutive calls alternate slots, so
 * the copy of the next clip overlaps the flow network of the current one.
 * LIFETIME: the copy is asynchronous. `host_frames` must stay valid (and unmodified) until the copy has completed:
 * that is guaranteed once the SECOND-NEXT call of atdn_ingest_frames_u8 on the same handle has returned (a call waits
 * on the host for the copy that last used its staging slot), or once `stream` has been synchronised after this call.
 * A caller that keeps the host buffers of its last two calls alive is safe (pipeline.FrameIngest does).
 *   host_frames [n_frames,3,Hin,Win] uint8 (HOST) -> dst [n_frames,3,Hout,Wout] fp32 (DEVICE), n_frames <= max_frames */
typedef struct atdn_ingest atdn_ingest;
int atdn_ingest_create(atdn_ingest** out, int Hin, int Win, int Hout, int Wout, int max_frames, int antialias);
int atdn_ingest_frames_u8(atdn_ingest* h, const uint8_t* host_frames, int n_frames, float* dst, void* stream);
void atdn_ingest_destroy(atdn_ingest* h);

/* ---------------------------------------------------------------------------------------------------
 * Flow bank  —  replaces the reference's fp16 flow files and FlowKittiDataset3 (flowbank.py)
 *   files:   dataset/flows2/<seq>/%06d.pt, fp16 [1,2,376,1232+] (read at odometry/datasets.py:176-189)
 *   samples: FlowKittiDataset3.__getitem__ (odometry/datasets.py:196-226), batched by the DataLoader of
 *            train_odometry.py:78-85
 * fp16 buffers are raw device pointers to IEEE binary16 values (torch.float16 data_ptr()).
 * ------------------------------------------------------------------------------------------------- */

/* `flow_up[..., x0:x0+W].half()` into a bank slot: the fp16 flow file the reference stores, written on the device.
 *   flow_up [B,2,H,Wsrc] fp32 -> dst [B,2,H,W] fp16 (16-byte aligned; W % 8 == 0; 0 <= x0, x0 + W <= Wsrc).
 * Round to nearest even; a NaN stays a NaN and values beyond +-65504 become +-inf, as tensor.half() does. */
int atdn_flow_pack_f16(const float* flow_up, int B, int H, int Wsrc, int x0, int W, uint16_t* dst, void* stream);

/* One training batch out of the bank, the reverse-flow augmentation folded in (odometry/datasets.py:220-224):
 *   out[b,t] = reverse[b] ? -bank[start[b]+T-1-t] : bank[start[b]+t]
 * bank [n_flows,2,H,W] fp16 -> out [B,T,2,H,W] fp32 (what atdn_clvo_trainer_forward_backward reads). `start` and `reverse`
 * are HOST arrays of B ints; every start must satisfy 0 <= start[b] <= n_flows - T, or the call fails before launching
 * anything. H * W % 4 == 0; bank and out 16-byte aligned. Bit-identical to the torch expression (exact decode and negation). */
int atdn_flow_gather_clips(const uint16_t* bank, int n_flows, int H, int W, const int* start, const int* reverse, int B, int T,
                           float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Warm start  —  replaces forward_interpolate of the flow package (whl:GMA/core/utils/utils.py:28-56; its evaluate.py feeds
 * the result to the next pair as flow_init, network.py:103-104)
 * ------------------------------------------------------------------------------------------------- */

/* forward_interpolate(flow_low[b]) for every b (utils.py:28-56, which leaves the device and calls scipy's
 * griddata(method='nearest') twice): the flow pushed forward along itself.
 *   flow_low, out [B,2,h,w] fp32 DEVICE, not overlapping; channel 0 = dx, 1 = dy; batches are independent.
 * Source i = y*w + x sits at (x + dx_i, y + dy_i), formed in float64, and is valid when 0 < x1 < w and 0 < y1 < h (all strict;
 * NaN / infinite flows are invalid). out at grid point (qx, qy) = (dx_j, dy_j) of the valid source j nearest to it:
 * (qx - x1)^2 + (qy - y1)^2 in float64, every operation rounded separately, equal distances to the lowest j (scipy leaves ties
 * unspecified). Outputs are bit copies of inputs. With NO valid source out is all zeros — the wheel's function raises there
 * (griddata on an empty point set). One launch on `stream`: asynchronous, capturable, no atomics, no workspace, the same bits on
 * every call. B <= 65535, h * w <= 2^24. */
int atdn_flow_forward_interpolate(const float* flow_low, int B, int h, int w, float* out, void* stream);
/* The same function (utils.py:28-56) on HOST buffers in plain C++, float64, by the same rules and with the same results:
 * serves CPU tensors, needs no GPU. */
int atdn_flow_forward_interpolate_host(const float* flow_low, int B, int h, int w, float* out);

/* ---------------------------------------------------------------------------------------------------
 * Flow consistency  —  no counterpart in the reference or the flow package: the forward-backward check of UnFlow (Meister et
 * al., AAAI 2018, eq. 2) and ARFlow, which relocalisation uses to tell "same place" from "different place" (keyframe_map.py,
 * verify=True) and which is the usual occlusion mask of a flow pair
 * ------------------------------------------------------------------------------------------------- */

/* mask[b,0,y,x] = 1 where following flow_fw from (x, y) and then flow_bw from where it lands returns to the start, else 0;
 * count[b] = the number of ones of mask[b].
 *   flow_fw, flow_bw [B,2,H,W] fp32 DEVICE, channel 0 = x; mask [B,1,H,W] uint8 DEVICE, count [B] int32 DEVICE; mask and count
 *   overlap neither each other nor the inputs. alpha1, alpha2 finite and >= 0 (UnFlow: 0.01, 0.5). B <= 65535, H * W <= 2^24.
 * The rule, for pixel (x, y), everything in float64 and every operation rounded on its own (no fused multiply-add), in exactly
 * this order:
 *   x1 = x + fw_x, y1 = y + fw_y                                 (exact in float64)
 *   inside = 0 <= x1 <= W-1 && 0 <= y1 <= H-1                    (closed intervals; a NaN fails)
 *   not inside: mask = 0, and flow_bw is not read for this pixel
 *   x0 = floor(x1), ax = x1 - x0; y0 = floor(y1), ay = y1 - y0
 *   taps t00, t10, t01, t11 of flow_bw at (x0, y0), (min(x0+1, W-1), y0), (x0, min(y0+1, H-1)), (min(x0+1, W-1), min(y0+1, H-1));
 *   all four are always read, zero-weight ones too (0 * NaN and 0 * inf are NaN and reach the result)
 *   per channel: top = t00*(1-ax) + t10*ax, bot = t01*(1-ax) + t11*ax, b = top*(1-ay) + bot*ay
 *   sx = fw_x + b_x, sy = fw_y + b_y, diff = sx*sx + sy*sy
 *   mag = (fw_x*fw_x + fw_y*fw_y) + (b_x*b_x + b_y*b_y), thr = alpha1*mag + alpha2
 *   mask = inside && diff <= thr && diff <= DBL_MAX              (plain comparisons: any NaN gives 0)
 * The last clause keeps a pixel with an INFINITE flow_bw tap of non-zero weight at 0 (there diff = thr = +inf, and inf <= inf
 * holds); finite fp32 inputs always give a finite diff, so it changes nothing for them. A NaN or an infinity in flow_fw at a
 * pixel or in one of its four taps therefore gives 0 at that pixel, and touches no other pixel than those that read it.
 * A memset of `count` and one launch on `stream`: asynchronous, capturable, no host synchronisation, no workspace. The count
 * is an integer sum (wave ballots, LDS, one integer atomic add per workgroup; no float atomics): the same bits on every call. */
int atdn_flow_consistency(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                          unsigned char* mask, int* count, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/flow_consistency_host.h, the per-pixel function the kernel
 * calls too): serves CPU tensors, needs no GPU, the same bits. */
int atdn_flow_consistency_host(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                               unsigned char* mask, int* count);

/* ---------------------------------------------------------------------------------------------------
 * Two-view geometry  —  what a flow and a relative pose determine at every pixel once the camera calibration is known: how far
 * the correspondence lies from its epipolar line (the share of pixels that agree scores the pose against its own flow, without
 * ground truth) and, by triangulation, the depth of the pixel. The reference has no producer of depth; atdn_depth_backproject
 * is the device form of project_depth of its utils/depth.py:23-46 for a calibration without skew
 * ------------------------------------------------------------------------------------------------- */

/* depth[b,0,y,x] = the triangulated depth of pixel (x, y) of image 1 in camera 1, 0 where there is none; counts[b] = (number of
 * correspondences inside image 2, number of epipolar inliers among them, number of valid depths among those).
 *   flow [B,2,H,W] fp32 DEVICE, frame 1 -> frame 2, channel 0 = x. pose [B,12] fp32 DEVICE: the rows of [R|t] with
 *   X1 = R X2 + t, i.e. r_ij = pose[b][4*i + j], t_i = pose[b][4*i + 3] — the first three rows of transform(rot, tr) of the pose
 *   head, the matrix a running pose is multiplied by (atdn_pose_transform_f32). mask [B,H,W] uint8 DEVICE or NULL: pixels whose
 *   byte is 0 are skipped (the mask of atdn_flow_consistency fits). depth [B,1,H,W] fp32 DEVICE, counts [B,3] int32 DEVICE; depth
 *   and counts overlap neither each other nor an input. fx, fy finite and > 0; cx, cy finite; max_epipolar (pixels) and min_sin2
 *   finite and >= 0; max_depth finite and > 0. B <= 65535, H * W <= 2^24. Anything else fails before a launch.
 * The rule, for pixel (x, y) with flow (u, v), everything in float64 and every operation rounded on its own (no fused
 * multiply-add), in exactly this order:
 *   mask given and mask[y,x] == 0: depth 0, counted nowhere
 *   x2 = x + u, y2 = y + v                                        (exact in float64)
 *   inside = 0 <= x2 <= W-1 && 0 <= y2 <= H-1                     (closed intervals; a NaN fails); not inside: depth 0, counted nowhere
 *   a0 = (x - cx)/fx, a1 = (y - cy)/fy                            (the ray of the pixel; a2 = 1)
 *   q0 = (x2 - cx)/fx, q1 = (y2 - cy)/fy                          (the ray of the correspondence in camera 2; q2 = 1)
 *   b_i = (r_i0*q0 + r_i1*q1) + r_i2                  i = 0,1,2   (b = R q)
 *   n0 = t1 - t2*a1, n1 = t2*a0 - t0, n2 = t0*a1 - t1*a0          (n = t x a)
 *   res = (n0*b0 + n1*b1) + n2*b2
 *   m0 = (r00*n0 + r10*n1) + r20*n2, m1 = (r01*n0 + r11*n1) + r21*n2, l0 = m0/fx, l1 = m1/fy
 *   epi2 = (res*res) / (l0*l0 + l1*l1)                            (squared pixel distance of (x2, y2) from its epipolar line in image 2)
 *   inlier = epi2 <= max_epipolar*max_epipolar                    (plain comparison: 0/0 from t = 0 is NaN and fails)
 *   aa = (a0*a0 + a1*a1) + 1, bb = (b0*b0 + b1*b1) + b2*b2, ab = (a0*b0 + a1*b1) + b2
 *   at = (a0*t0 + a1*t1) + t2, bt = (b0*t0 + b1*t1) + b2*t2
 *   p = aa*bb, det = p - ab*ab, sin2 = det/p                      (sin^2 of the angle between the two rays)
 *   z1 = (bb*at - ab*bt)/det, z2 = (ab*at - aa*bt)/det            (least-squares solution of z1*a - z2*b = t)
 *   valid = inlier && sin2 >= min_sin2 && z1 >= FLT_MIN && z2 > 0 && z1 <= max_depth
 *   depth = valid ? (float)z1 : 0
 * No square root and no transcendental: + - * / and comparisons, all correctly rounded, so the device, the host form and any
 * IEEE float64 restatement agree bit for bit. `z1 >= FLT_MIN` (2^-126) stands where `z1 > 0` would: a smaller positive z1 rounds
 * to a float32 zero or subnormal, and a pixel counted valid would carry the value that means "no depth"; with it every valid
 * depth is a normal positive float32 and counts[b][2] is the number of non-zero depths. Parallel rays (det = 0: no parallax, or a
 * pixel at the epipole) give z1 = +-inf or NaN and are never valid, whatever min_sin2 is; t = 0 gives no inliers. A NaN or an
 * infinity in the flow of a pixel gives depth 0 there and touches no other pixel; one in the pose fails every comparison it reaches.
 * A memset of `counts` and one launch on `stream`: asynchronous, capturable, no host synchronisation, no workspace. The counts
 * are integer sums (wave ballots, LDS, one integer atomic add per workgroup and counter; no float atomics): the same bits on
 * every call. */
int atdn_flow_two_view_depth(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth, float* depth,
                             int* counts, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/two_view_host.h, the per-pixel function the kernel calls too):
 * serves CPU tensors, needs no GPU, the same bits. */
int atdn_flow_two_view_depth_host(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W, double fx,
                                  double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth,
                                  float* depth, int* counts);

/* points[b] = [3,H,W] fp32: the pinhole back-projection of depth[b] (project_depth of utils/depth.py:23-46 with
 * calib = [[fx,0,cx],[0,fy,cy],[0,0,1]]): for z = depth[b,0,y,x],
 *   X = (z*(x - cx))/fx, Y = (z*(y - cy))/fy, Z = z
 * each formed in float64 (every operation rounded on its own) and rounded to fp32 once — the reference inverts the fp32 matrix and
 * multiplies in fp32. depth [B,1,H,W], points [B,3,H,W] fp32 DEVICE, not overlapping; fx, fy finite and > 0, cx, cy finite;
 * B <= 65535, H * W <= 2^24. One launch on `stream`: asynchronous, capturable. */
int atdn_depth_backproject(const float* depth, int B, int H, int W, double fx, double fy, double cx, double cy, float* points,
                           void* stream);

/* One step of a flow track: the correspondence of every pixel of an ANCHOR frame carried one frame further, and its depth over
 * the whole baseline. acc is the flow from the anchor to frame k on the anchor's grid, alive says which pixels still have a track;
 * the step composes acc with the flow k -> k+1, read bilinearly where each track stands — p(k+1) = p(k) + flow_k(p(k)) — and, given
 * the accumulated pose anchor <- frame k+1, triangulates the composed correspondence by the rule of atdn_flow_two_view_depth and
 * writes the depth over the anchor's depth map where it is valid (the latest valid triangulation wins).
 *   flow [B,2,H,W] fp32 DEVICE, frame k -> k+1 on frame k's grid, channel 0 = x. mask [B,H,W] uint8 DEVICE or NULL, on frame k's
 *   grid: 0 = do not trust the flow here (the mask of atdn_flow_consistency of that pair fits). acc_in, acc_out [B,2,H,W] fp32
 *   DEVICE: the flow anchor -> frame k, and anchor -> frame k+1, on the anchor's grid. alive_in, alive_out [B,H,W] uint8 DEVICE:
 *   any non-zero byte in = alive; out is exactly 0 or 1. pose [B,12] fp32 DEVICE or NULL: anchor <- frame k+1 in the convention of
 *   atdn_flow_two_view_depth (X_anchor = R X + t). depth [B,1,H,W] fp32 DEVICE, in/out. counts [B,4] int32 DEVICE = (alive_out,
 *   inside, inliers, valid), the last three those of the two-view rule.
 *   acc_out == acc_in and alive_out == alive_in (the same pointer) are allowed: a pixel's own state is read before it is written
 *   and no other pixel's is read. Every other overlap of an output with an input or another output is refused.
 *   pose == NULL is the chain-only form: depth must be NULL, counts[b][1..3] = 0, and fx .. max_depth are ignored. With a pose:
 *   depth not NULL; fx, fy finite and > 0; cx, cy finite; max_epipolar and min_sin2 finite and >= 0; max_depth finite and > 0.
 *   B <= 65535, H * W <= 2^24, B, H, W >= 1. Anything else fails before a launch.
 * The rule, for pixel (x, y) of image b, everything in float64 and every operation rounded on its own (no fused multiply-add), in
 * exactly this order ("dead" = alive_out 0, acc_out = acc_in bit for bit, depth untouched, counted nowhere):
 *   alive_in == 0: dead
 *   x1 = x + acc_x, y1 = y + acc_y                                (exact in float64)
 *   inside = 0 <= x1 <= W-1 && 0 <= y1 <= H-1                     (closed intervals; a NaN fails); not inside: dead
 *   x0 = floor(x1), ax = x1 - x0; y0 = floor(y1), ay = y1 - y0
 *   taps t00, t10, t01, t11 of flow at (x0, y0), (min(x0+1, W-1), y0), (x0, min(y0+1, H-1)), (min(x0+1, W-1), min(y0+1, H-1));
 *   all four are always read, zero-weight ones too (0 * NaN and 0 * inf are NaN and reach the result)
 *   per channel: top = t00*(1-ax) + t10*ax, bot = t01*(1-ax) + t11*ax, s = top*(1-ay) + bot*ay
 *   n_x = acc_x + s_x, n_y = acc_y + s_y; finite = |n_x| <= DBL_MAX && |n_y| <= DBL_MAX
 *   trusted = mask == NULL || mask[floor(y1 + 0.5)][floor(x1 + 0.5)] != 0       (always inside the image, given `inside`)
 *   alive_out = inside && finite && trusted; otherwise dead
 *   acc_out = ((float)n_x, (float)n_y), one rounding each; a value that rounds to a float32 infinity makes the pixel dead
 *   alive and pose != NULL: the rule of atdn_flow_two_view_depth for pixel (x, y) with the flow acc_out (the fp32 values), this
 *   pose and no mask -> inside2, inlier, valid, z1; valid: depth = (float)z1; otherwise depth untouched
 *   counts = (number of alive_out, of inside2, of inlier, of valid)
 * So: a dead track never comes back. A NaN or an infinity in acc_in at a pixel, or in one of its four taps, makes that pixel dead
 * and touches no other pixel; one in the pose fails every comparison it reaches, so the chain is unaffected and no depth is
 * written. The depth at a pixel is the triangulation of the LAST step at which it was valid: the caller zeroes depth (and acc,
 * and sets alive) at the start of a track. Only + - * /, floor, comparisons and one double -> float conversion, all correctly
 * rounded: the device, the host form and any IEEE float64 restatement agree bit for bit.
 * A memset of `counts` and one launch on `stream`: asynchronous, capturable, no host synchronisation, no workspace. The counts
 * are integer sums (wave ballots, LDS, one integer atomic add per workgroup and counter; no float atomics): the same bits on
 * every call. */
int atdn_flow_track_step(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in, int B,
                         int H, int W, float* acc_out, unsigned char* alive_out, const float* pose, double fx, double fy, double cx,
                         double cy, double max_epipolar, double min_sin2, double max_depth, float* depth, int* counts, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/flow_track_host.h, the per-pixel function the kernel calls too):
 * serves CPU tensors, needs no GPU, the same bits. */
int atdn_flow_track_step_host(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in,
                              int B, int H, int W, float* acc_out, unsigned char* alive_out, const float* pose, double fx,
                              double fy, double cx, double cy, double max_epipolar, double min_sin2, double max_depth, float* depth,
                              int* counts);

/* Keyframe depth fusion: the geometric-consistency filter of multi-view stereo (COLMAP / MVSNet fusion) over a bank of depth maps
 * with poses. For target i = targets[b], every pixel with a depth is projected into the sources sources[b][.], their depth is
 * read there and projected back; the pixel is kept where at least min_views sources agree, optionally averaged with their
 * estimates. Gather only (no atomics on the data), deterministic. All targets of a call read the same, unfused bank.
 *   bank [N,H,W] fp32 DEVICE, 0 = no depth. poses [N,12] fp32 DEVICE: the rows of [R|t], world <- camera (r_ij = poses[k][4*i + j],
 *   t_i = poses[k][4*i + 3]), as a keyframe map holds them. targets [B] int32 DEVICE, sources [B,S] int32 DEVICE (may be NULL only
 *   when S == 0). fused [B,1,H,W] fp32, views [B,H,W] uint8, counts [B,3] int32 = (has, seen, kept), all DEVICE. No other pointer
 *   may be NULL; every output is disjoint from every input and from the other outputs (fusing into the bank in place is an
 *   "overlap" error). 1 <= N, 1 <= B <= 65535, 0 <= S <= 255, 1 <= min_views <= 255, H * W <= 2^24; fx, fy finite and > 0; cx, cy
 *   finite; max_reproj (pixels), max_rel_depth and min_z finite and > 0; average 0 or not 0. Anything else fails before a launch.
 * The rule, everything in float64 and every operation rounded on its own (no fused multiply-add), in exactly this order. The
 * sources of target i are walked in list order; a slot with j < 0, j >= N or j == i is skipped and reads nothing; a target outside
 * [0, N) gives all-zero outputs. Per (target i, source j), once, from the float32 rows, every dot product (p0 + p1) + p2:
 *   R = R_j^T R_i:  R_kl = (rj_0k*ri_0l + rj_1k*ri_1l) + rj_2k*ri_2l
 *   d_m = ti_m - tj_m,  t_k = (rj_0k*d_0 + rj_1k*d_1) + rj_2k*d_2                               (X_j = R X_i + t)
 * Pixel (x, y) with z = bank[i][y][x]:
 *   has = z > 0; not has: fused 0, views 0, counted nowhere
 *   a0 = (x - cx)/fx, a1 = (y - cy)/fy, X = (z*a0, z*a1, z)
 * Per source:
 *   Xs_k = ((R_k0*X0 + R_k1*X1) + R_k2*X2) + t_k
 *   front = Xs_2 >= min_z                                         not front: the source is not ok and reads nothing
 *   u = fx*(Xs_0/Xs_2) + cx, v = fy*(Xs_1/Xs_2) + cy
 *   inside = 0 <= u <= W-1 && 0 <= v <= H-1                       (closed intervals; a NaN fails); not inside: not ok, nothing read
 *   ds = bank[j] at (u, v), bilinear exactly as the flow of atdn_flow_track_step is read: x0 = floor(u), ax = u - x0, y0 = floor(v),
 *   ay = v - y0, taps t00, t10, t01, t11 at (x0, y0), (min(x0+1, W-1), y0), (x0, min(y0+1, H-1)), (min(x0+1, W-1), min(y0+1, H-1)),
 *   all four always read; top = t00*(1-ax) + t10*ax, bot = t01*(1-ax) + t11*ax, ds = top*(1-ay) + bot*ay
 *   ok = front && inside && all four taps > 0                     (a hole is not interpolated across)
 *   q0 = (u - cx)/fx, q1 = (v - cy)/fy, Y = (ds*q0 - t0, ds*q1 - t1, ds - t2)
 *   Yt_k = (R_0k*Y0 + R_1k*Y1) + R_2k*Y2                          (the source's surface point in the target camera)
 *   back = ok && Yt_2 >= min_z
 *   xr = fx*(Yt_0/Yt_2) + cx, yr = fy*(Yt_1/Yt_2) + cy
 *   e2 = (xr - x)*(xr - x) + (yr - y)*(yr - y),  rd = |Yt_2 - z| / z
 *   consistent = back && e2 <= max_reproj*max_reproj && rd <= max_rel_depth
 *   consistent: n += 1, zsum += Yt_2                              (n starts at 0, zsum at z)
 * Result:
 *   views = n (written for every pixel); kept = has && n >= min_views
 *   fused = kept ? (float)(average ? zsum/(n + 1) : z) : 0
 *   counts = (number of has, of seen, of kept), seen = has and ok for at least one source
 * Only + - * /, floor, |.|, comparisons and one double -> float conversion, all correctly rounded: the device, the host form and any
 * IEEE float64 restatement agree bit for bit. Any NaN fails every comparison it reaches.
 * A memset of `counts` and one launch on `stream`: asynchronous, capturable, no host synchronisation, no workspace. The counts
 * are integer sums (wave ballots, LDS, one integer atomic add per workgroup and counter; no float atomics): the same bits on
 * every call. */
int atdn_depth_fuse(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S, int H, int W,
                    double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth, int min_views, double min_z,
                    int average, float* fused, unsigned char* views, int* counts, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/depth_fusion_host.h, the functions the kernel calls too): serves
 * CPU tensors, needs no GPU, the same bits and the same argument rules. */
int atdn_depth_fuse_host(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S, int H,
                         int W, double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth, int min_views,
                         double min_z, int average, float* fused, unsigned char* views, int* counts);

/* Multi-view keyframe depth: per anchor pixel, the inverse depth that best explains its correspondences in up to
 * ATDN_MULTIVIEW_MAX_VIEWS later frames with known poses — the depth half of bundle adjustment, the batch form of a depth filter —
 * by Levenberg-Marquardt on the reprojection error under the Geman-McClure loss, with the information of the result.
 * atdn_flow_track_step keeps one triangulation per pixel (the last valid one); this uses every correspondence of the interval.
 *   acc_bank [N,2,H,W] fp32 DEVICE: slot k is the flow from the anchor frame to some later frame on the anchor's grid, channel 0 =
 *   x (the acc_out of atdn_flow_track_step). alive_bank [N,H,W] uint8 DEVICE, any non-zero byte = alive. poses [N,12] fp32 DEVICE,
 *   anchor <- that frame in the convention of atdn_flow_two_view_depth (X_anchor = R X + t; r_ij = poses[k][4*i + j], t_i =
 *   poses[k][4*i + 3]). slots [B,S] int32 DEVICE: the views of problem b, walked in list order; a slot with k < 0 or k >= N is
 *   skipped and reads nothing. depth_init [B,1,H,W] fp32 DEVICE or NULL: a depth to start from, 0 = none at that pixel.
 *   depth [B,1,H,W] fp32 (0 = none), info [B,1,H,W] fp32, views [B,H,W] uint8, counts [B,3] int32 = (candidates, solved, valid),
 *   all DEVICE. 1 <= N, 1 <= B <= 65535, 1 <= S <= ATDN_MULTIVIEW_MAX_VIEWS, 1 <= min_views <= S, 0 <= iters <= 16, H * W <= 2^24;
 *   fx, fy finite and > 0; cx, cy finite; scale_px, inlier_px (pixels), min_z, max_rel_sigma and max_depth finite and > 0. Only
 *   depth_init may be NULL; every output is disjoint from every input and from every other output. Anything else fails before a
 *   launch.
 * The rule, everything in float64 and every operation rounded on its own (no fused multiply-add), only + - * / and comparisons,
 * in exactly this order. Constants: c2 = scale_px*scale_px, thr = inlier_px*inlier_px, e = (double)(H + W),
 * rho_behind = (0.5*(e*e)) / (1 + (e*e)/c2) (those of atdn_pnp_terms), min_rel_info = 1 / (max_rel_sigma*max_rel_sigma).
 * Per (problem, listed view), once, from the float32 row, the internal pose of atdn_pnp_terms:
 *   Rc = R^T,  tc_i = -((r_0i*t_0 + r_1i*t_1) + r_2i*t_2)                                       (X = Rc X_anchor + tc)
 * Pixel (x, y): a0 = (x - cx)/fx, a1 = (y - cy)/fy. Per listed view, in list order:
 *   (u, v) = acc_bank[k][:, y, x];  x2 = x + u, y2 = y + v
 *   obs = alive byte != 0 && 0 <= x2 <= W-1 && 0 <= y2 <= H-1     (closed intervals; a NaN fails)
 *   m_i = (rc_i0*a0 + rc_i1*a1) + rc_i2                           (the pixel's ray in that view; its point is m + rho*tc)
 *   kx = fx*(tc_0*m_2 - m_0*tc_2),  ky = fy*(tc_1*m_2 - m_1*tc_2)
 *   xt = x2 - cx,  yt = y2 - cy
 * Linear start over the obs views, each sum starting at +0.0:
 *   Ax = fx*tc_0 - xt*tc_2,  Bx = xt*m_2 - fx*m_0;  Ay, By likewise with fy, yt and index 1
 *   num = num + (Ax*Bx + Ay*By),  den = den + (Ax*Ax + Ay*Ay);  n_obs counts the obs views
 * cand = n_obs >= min_views; not cand: depth 0, info 0, views 0, counted nowhere.
 * The evaluation E(rho) over the obs views in list order; g, h, cost start at +0.0 and n_in at 0:
 *   P_i = m_i + rho*tc_i
 *   front = P_2 >= min_z*rho                                      not front: cost = cost + rho_behind, nothing else from this view
 *   iz = 1/P_2,  px = (fx*P_0)*iz,  py = (fy*P_1)*iz
 *   rx = (px + cx) - x2,  ry = (py + cy) - y2,  e2 = rx*rx + ry*ry
 *   s = 1 + e2/c2,  w = 1/(s*s),  r = (0.5*e2)/s
 *   Jx = (kx*iz)*iz,  Jy = (ky*iz)*iz
 *   g = g + ((w*Jx)*rx + (w*Jy)*ry),  h = h + ((w*Jx)*Jx + (w*Jy)*Jy),  cost = cost + r,  n_in += (e2 <= thr)
 * Start: rho_lin = num/den, lin_ok = 0 < rho_lin <= DBL_MAX. With depth_init and 0 < z0 <= FLT_MAX at the pixel: rho_0 = 1/z0, and
 * both E(rho_lin) (if lin_ok) and E(rho_0) are formed; the start is the one of smaller cost, the linear one on a tie or when only
 * it exists. Neither exists: not solved, depth 0, info 0, views 0.
 * Steps k = 1 .. iters, lambda = 1e-3 at the start:
 *   rho' = rho - g/(h + lambda*h)
 *   accepted iff 0 < rho' <= DBL_MAX && cost(rho') < cost(rho)    (a NaN fails)
 *   accepted: rho, g, h, cost, n_in are the trial's, lambda = max(lambda/3, 1e-9); rejected: lambda = min(4*lambda, 1e6)
 *   (the decision rule and the constants of atdn_pnp_solve)
 * Result:
 *   z = 1/rho,  ri = (h*rho)*rho                                  (the inverse variance of the RELATIVE depth for unit pixel noise:
 *                                                                  sigma_z / z = noise_px / sqrt(ri))
 *   valid = solved && n_in >= min_views && ri >= min_rel_info && z >= FLT_MIN && z <= max_depth
 *   depth = valid ? (float)z : 0,  info = valid ? (float)min(ri, FLT_MAX) : 0,  views = solved ? n_in : 0
 *   counts = (number of cand, of solved, of valid)
 * So: with every tc = 0 (no baseline) den = 0 and no pixel is solved from the linear start. A NaN or an infinity in a view's flow
 * removes that view at that pixel only. A NaN or an infinity in a pose fails every comparison it reaches: the linear start of
 * every pixel that observes that view fails, and in an evaluation the view counts as behind. All operations are correctly
 * rounded: the device, the host form and any IEEE float64 restatement agree bit for bit.
 * A memset of `counts` and one launch on `stream`: asynchronous, capturable, no host synchronisation, no workspace. The counts
 * are integer sums (wave ballots, LDS, one integer atomic add per workgroup and counter; no float atomics): the same bits on
 * every call. */
#define ATDN_MULTIVIEW_MAX_VIEWS 16
int atdn_multiview_depth(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                         const float* depth_init, int N, int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                         double scale_px, double inlier_px, double min_z, int min_views, double max_rel_sigma, double max_depth,
                         int iters, float* depth, float* info, unsigned char* views, int* counts, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/multiview_depth_host.h, the per-pixel function the kernel calls
 * too): serves CPU tensors, needs no GPU, the same bits and the same argument rules. */
int atdn_multiview_depth_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                              const float* depth_init, int N, int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                              double scale_px, double inlier_px, double min_z, int min_views, double max_rel_sigma, double max_depth,
                              int iters, float* depth, float* info, unsigned char* views, int* counts);

/* Windowed dense bundle adjustment over the same banks: the joint Levenberg-Marquardt refinement of the poses of the listed views
 * and of the inverse depths of the anchor's candidate pixels, the depths eliminated by the Schur complement. The anchor's own pose
 * is the frame of reference and is not refined; there are no priors. atdn_bundle_terms is one evaluation (all sums of the reduced
 * normal equations at the given poses and depth, for scoring), atdn_bundle_adjust the solver.
 *   acc_bank, alive_bank, poses, slots: as for atdn_multiview_depth. depth_init [B,1,H,W] fp32 DEVICE, mandatory. mask [B,H,W]
 *   uint8 DEVICE or NULL (non-zero = allowed). stride >= 1, 0 <= iters <= 16, the other limits those of atdn_multiview_depth.
 *   poses_out [B,S,12] fp32 (the public convention; an empty slot is all zeros), depth [B,1,H,W] fp32 (the refined depth at the
 *   candidates, 0 elsewhere, fully written), cost [B,2] fp64 (initial, final), counts [B,4] int32 = (candidates; observations in
 *   front of their camera at the final state; those within inlier_px; accepted steps); sums [B, NS] fp64 and counts [B,3] for
 *   atdn_bundle_terms. workspace: atdn_bundle_workspace_bytes(B, S, H, W, stride) bytes DEVICE, 8-byte aligned, an output like the
 *   others; nothing in it is read before this call has written it. Only mask may be NULL; anything else fails before a launch.
 * The rule, everything in float64 and every operation rounded on its own, only + - * / and comparisons, in exactly this order.
 * Constants c2, thr, rho_behind and the internal pose (Rc, tc) of a listed view: those of atdn_multiview_depth.
 * Positions: Hs = ceil(H/stride), Ws = ceil(W/stride); position q = ys*Ws + xs is pixel (x, y) = (xs*stride, ys*stride).
 * Candidates, fixed for the whole solve: the mask allows the pixel, 0 < depth_init <= FLT_MAX, and obs (atdn_multiview_depth) holds
 * in at least min_views listed views. rho = 1/depth_init at the start. a0 = (x - cx)/fx, a1 = (y - cy)/fy.
 * One obs view of a candidate at (Rc, tc, rho):
 *   m_i = (rc_i0*a0 + rc_i1*a1) + rc_i2,  P_i = m_i + rho*tc_i
 *   front = P_2 >= min_z*rho                   not front: the view costs rho_behind and every term below is +0.0
 *   iz = 1/P_2,  px = (fx*P_0)*iz,  py = (fy*P_1)*iz,  rx = (px + cx) - x2,  ry = (py + cy) - y2,  e2 = rx*rx + ry*ry
 *   s = 1 + e2/c2,  w = 1/(s*s),  cost = (0.5*e2)/s
 *   ax = fx*iz, ay = fy*iz, bx = -(px*iz), by = -(py*iz)                      (A = [[ax, 0, bx], [0, ay, by]])
 *   Jx = (bx*m_1, ax*m_2 - bx*m_0, -(ax*m_1), rho*ax, 0, rho*bx)               (-A [m]x and rho A)
 *   Jy = (by*m_1 - ay*m_2, -(by*m_0), ay*m_0, 0, rho*ay, rho*by)
 *   jrx = ax*tc_0 + bx*tc_2,  jry = ay*tc_1 + by*tc_2                         (A tc)
 *   H_ij = (w*Jx_i)*Jx_j + (w*Jy_i)*Jy_j (i <= j),  g_i = (w*Jx_i)*rx + (w*Jy_i)*ry,  E_i = (w*Jx_i)*jrx + (w*Jy_i)*jry
 *   c_s = (w*jrx)*jrx + (w*jry)*jry,  b_s = (w*jrx)*rx + (w*jry)*ry;  inlier = e2 <= thr
 * Per candidate c, b and cost are the sums of c_s, b_s and the views' costs over its obs views in list order, from +0.0; E is the
 * concatenation of the E of the views (+0.0 for the others), n = 6 S values; ic = 1/c, bc = b*ic.
 * Sums over candidates, NS = n(n+1)/2 + n + 27 S + 1 values in this layout: T0 (upper triangle row by row), entry (i, j) takes
 * (E_i*ic)*E_j; v0, entry i takes E_i*bc; per view the 21 H_ij row by row and the 6 g_i; the cost. A candidate whose c is not > 0
 * gives its cost only. Order: the positions are cut into chunks of 512 consecutive q; every sum of a chunk starts at +0.0 and
 * takes the chunk's candidates in ascending q; the chunk sums are added in chunk order from +0.0. atdn_bundle_terms returns these
 * sums and counts = (candidates, front observations, inliers).
 * Gauge (scale is unobservable): g = the last non-empty listed view, j = the index of its largest |tc_j| at the start, the lowest
 * on a tie; unknown 6 g + 3 + j is held, and so are the six unknowns of every empty slot. If that |tc_j| is 0 (or no view is
 * listed) no step is taken: the outputs are the inputs and no step is accepted.
 * Step from the accepted sums with damping lambda, opl = 1 + lambda; H and g are zero between different views:
 *   S_ij = H_ij - T0_ij/opl (i < j),  S_ii = (H_ii + lambda*H_ii) - T0_ii/opl,  rhs_i = -(g_i - v0_i/opl)
 *   a held unknown: its row and column +0.0, its diagonal 1, its rhs +0.0
 *   S = L D L^T without pivoting, column j = 0 .. n-1: d_j = S_jj - sum_k L_jk*(L_jk*d_k) and, for i > j,
 *   L_ij = (S_ij - sum_k L_ik*(L_jk*d_k)) / d_j, each sum subtracted term by term in ascending k < j; forward, diagonal and backward
 *   solve as in atdn_pnp_solve with 6 replaced by n. A pivot not > 0 or a step that is not finite: no step, the trial is the
 *   accepted state again (and is rejected, its cost being no smaller).
 *   trial poses: Rc' = C(dw) Rc, tc' = tc + dt per non-empty view (C: the Cayley matrix of atdn_pnp_solve; tc is NOT rotated)
 *   trial depth per candidate, from c, b, E at the ACCEPTED state: e = sum over its obs views in list order, from +0.0, of
 *   ((((E_0*d_0 + E_1*d_1) + E_2*d_2) + E_3*d_3) + E_4*d_4) + E_5*d_5 with that view's six step entries;
 *   rho' = rho - (b + e)/(c*opl); rho' not in (0, DBL_MAX] or c not > 0: rho' = rho.
 * Decision and lambda: those of atdn_pnp_solve — evaluation 0 is accepted with lambda = 1e-3, a later one iff its cost is smaller;
 * T0 and v0 do not depend on lambda, so a rejected step needs no new sums. After `iters` steps: poses_out = the inputs' rows if
 * no step was accepted, otherwise the accepted poses in the public convention rounded to float32; depth = (float)(1/rho).
 * 2 (iters + 1) launches on `stream`: asynchronous, capturable, no host synchronisation, no atomics, no memset: the same bits on
 * every call. */
long atdn_bundle_workspace_bytes(int B, int S, int H, int W, int stride);   /* 0: arguments out of range */
int atdn_bundle_terms(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                      const float* depth, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                      double cx, double cy, int stride, double scale_px, double inlier_px, double min_z, int min_views, double* sums,
                      int* counts, void* workspace, void* stream);
int atdn_bundle_adjust(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                       const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                       double cx, double cy, int stride, int iters, double scale_px, double inlier_px, double min_z, int min_views,
                       float* poses_out, float* depth, double* cost, int* counts, void* workspace, void* stream);
/* The same functions on HOST buffers in plain C++ float64 (csrc/bundle_host.h, whose functions the kernels call too): serve CPU
 * tensors, need no GPU and no workspace, the same bits and the same argument rules. */
int atdn_bundle_terms_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                           const float* depth, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                           double cx, double cy, int stride, double scale_px, double inlier_px, double min_z, int min_views,
                           double* sums, int* counts);
int atdn_bundle_adjust_host(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                            const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W, double fx,
                            double fy, double cx, double cy, int stride, int iters, double scale_px, double inlier_px, double min_z,
                            int min_views, float* poses_out, float* depth, double* cost, int* counts);

/* ---------------------------------------------------------------------------------------------------
 * Pose from depth and flow (robust PnP)  —  a depth map of image 1 gives a 3-D point per pixel, the flow image 1 -> image 2 gives
 * that point's pixel in image 2: the pose that explains the correspondences, by Levenberg-Marquardt on the reprojection error
 * under the Geman-McClure loss, batched over problems, all on the device. atdn_pnp_terms is one evaluation (the normal
 * equations, the cost and the share of reprojection inliers of a given pose: the depth-aware sibling of the epipolar score),
 * atdn_pnp_solve the solver. The reference has nothing like it.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of the workspace of atdn_pnp_terms / atdn_pnp_solve for B planes of H x W (0 for sizes they refuse): one solver state per
 * problem and, per chunk of 1024 pixels, 28 float64 sums and four int32. No call reads what an earlier call left there. */
long atdn_pnp_workspace_bytes(int B, int H, int W);

/* sums[b] = the 28 reprojection terms of pose[b] summed over the plane, counts[b] = (candidates, used, inliers).
 *   depth [B,H,W] fp32 DEVICE: the depth of every pixel of image 1 in camera 1, 0 = none. flow [B,2,H,W] fp32 DEVICE, image 1 ->
 *   image 2, channel 0 = x. mask [B,H,W] uint8 DEVICE or NULL: pixels whose byte is 0 are skipped. pose [B,12] fp32 DEVICE: the
 *   rows of [R|t] with X1 = R X2 + t, as for atdn_flow_two_view_depth. sums [B,28] float64 DEVICE, counts [B,3] int32 DEVICE,
 *   workspace: atdn_pnp_workspace_bytes(B, H, W) bytes DEVICE, 8-byte aligned like sums; no output (the workspace is one)
 *   overlaps an input or another output. fx, fy finite and > 0; cx, cy finite; scale_px, inlier_px (pixels) and min_z finite and
 *   > 0. B <= 65535, H * W <= 2^24, B, H, W >= 1. Anything else fails before a launch.
 * The rule: everything in float64, every operation rounded on its own (no fused multiply-add), only + - * / and comparisons, in
 * exactly this order.
 * Internal pose (X2 = Rc X1 + tc): Rc = R^T (a copy), tc_i = -((r_0i*t_0 + r_1i*t_1) + r_2i*t_2).
 * Constants: c2 = scale_px*scale_px, thr = inlier_px*inlier_px, e = (double)(H + W), rho_behind = (0.5*(e*e)) / (1 + (e*e)/c2).
 * Pixel (x, y) with z = depth, (u, v) = flow:
 *   x2 = x + u, y2 = y + v                                        (exact in float64)
 *   cand = mask byte != 0 && 0 < z <= FLT_MAX && 0 <= x2 <= W-1 && 0 <= y2 <= H-1      (closed; a NaN fails)
 *   X1 = (z*(x - cx))/fx, Y1 = (z*(y - cy))/fy
 *   X = ((rc_00*X1 + rc_01*Y1) + rc_02*z) + tc_0, Y and Z likewise with rows 1 and 2 of Rc
 *   used = cand && Z >= min_z
 *   iz = 1/Z, px = (fx*X)*iz, py = (fy*Y)*iz
 *   rx = (px + cx) - x2, ry = (py + cy) - y2, e2 = rx*rx + ry*ry
 *   s = 1 + e2/c2, w = 1/(s*s), rho = (0.5*e2)/s                  (Geman-McClure: redescending, no square root)
 *   inlier = used && e2 <= thr
 *   a = fx*iz, b = -(px*iz), k = fy*iz, d = -(py*iz)
 *   Jx = (b*Y, a*Z - b*X, -(a*Y), a, 0, b), Jy = (d*Y - k*Z, -(d*X), k*X, 0, k, d)
 *     (the Jacobian of (rx, ry) with respect to (w0, w1, w2, v0, v1, v2) for X2 <- X2 + w x X2 + v)
 *   terms 0..20: H_ij = (w*Jx_i)*Jx_j + (w*Jy_i)*Jy_j for i <= j, row by row (00, 01, .., 05, 11, .., 55); the products with the
 *     structural zeros of Jx and Jy are formed like any other
 *   terms 21..26: g_i = (w*Jx_i)*rx + (w*Jy_i)*ry;  term 27: rho
 *   cand && !used (the point is behind camera 2, or a NaN pose): term 27 = rho_behind, the others +0.0 — without it a step that
 *     pushes points behind the camera would lower the cost
 *   !cand: +0.0 in all 28 terms
 * Sums (their order is part of the rule; + is the float64 addition):
 *   a plane is cut into chunks of 1024 consecutive flat indices i = y*W + x; indices >= H*W contribute +0.0 to every term;
 *   inside a chunk, thread j = 0..255 owns the indices 4j .. 4j+3 and forms v[j] = ((t0 + t1) + t2) + t3; then for stride = 1, 2,
 *   4, .., 128: v[i] = v[i] + v[i + stride] for every i that is a multiple of 2*stride; the chunk sum is v[0];
 *   the plane sum is the chunk sums added in chunk order, starting from chunk 0's.
 * The three counts are integer sums over the plane. No atomics and no memset: every workgroup writes its own slot of the
 * workspace and a second launch adds the slots in order, so the same inputs give the same bits on every call. Two launches on
 * `stream`: asynchronous, capturable, no host synchronisation. */
int atdn_pnp_terms(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                   double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, double* sums,
                   int* counts, void* workspace, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/pnp_host.h, the functions the kernels call too): serves CPU
 * tensors, needs no GPU and no workspace, the same bits. */
int atdn_pnp_terms_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                        double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, double* sums,
                        int* counts);

/* pose_out[b] = the pose after `iters` Levenberg-Marquardt steps from pose_init[b] on the terms above; cost[b] and
 * counts[b] = (candidates, used, inliers, accepted steps) at it. Arguments as for atdn_pnp_terms; pose_init, pose_out [B,12]
 * fp32 DEVICE, cost [B] float64 DEVICE (8-byte aligned), counts [B,4] int32 DEVICE, 0 <= iters <= 64.
 * State per problem: the accepted pose, the trial pose, the accepted terms, lambda, the accepted counts, the number of accepted
 * steps. Evaluation 0 is at the internal form of pose_init and always becomes the accepted point, with lambda = 1e-3. After
 * evaluation k >= 1 (at the trial pose): accepted iff cost_trial < cost_accepted (a NaN fails); on accept the pose, terms and
 * counts are the trial's and lambda = max(lambda/3, 1e-9); on reject lambda = min(4*lambda, 1e6). Then, unless k = iters:
 *   A = H of the accepted terms with A_ii = H_ii + lambda*H_ii
 *   LDL^T without pivoting, for j = 0..5:  d_j = A_jj - sum_{k<j} L_jk*(L_jk*d_k)   (subtracted one by one, k ascending)
 *                                           L_ij = (A_ij - sum_{k<j} L_ik*(L_jk*d_k)) / d_j  for i > j, likewise
 *   y_i = -g_i - sum_{k<i} L_ik*y_k (k ascending);  y_i = y_i/d_i;  delta_i = y_i - sum_{k>i} L_ki*delta_k (i = 5..0, k ascending)
 *   some d_j > 0 fails, or some |delta_i| <= DBL_MAX fails: the trial is the accepted pose again
 *   retraction (rational, exactly orthonormal in exact arithmetic): h = 0.5*delta_w, n2 = (h0*h0 + h1*h1) + h2*h2, f = 2/(1 + n2),
 *     M_ii = h_i*h_i - n2, M_ij = K_ij + h_i*h_j with K = [h]x = ((0, -h2, h1), (h2, 0, -h0), (-h1, h0, 0)),
 *     E_ii = 1 + f*M_ii, E_ij = f*M_ij;  Rc'_ij = (E_i0*Rc_0j + E_i1*Rc_1j) + E_i2*Rc_2j,
 *     tc'_i = ((E_i0*tc_0 + E_i1*tc_1) + E_i2*tc_2) + delta_v_i
 * `iters` steps are iters + 1 evaluations, two launches each (the terms; the order-fixed sum with the decision and the step, one
 * workgroup per problem); no host synchronisation, capturable. Output: R = Rc^T, t_i = -((rc_0i*tc_0 + rc_1i*tc_1) + rc_2i*tc_2)
 * of the accepted pose, each rounded to fp32 once; when no step was accepted pose_out holds the bits of pose_init — a plane
 * without depth returns exactly what it was given, cost +0.0 and zero counts. */
int atdn_pnp_solve(const float* depth, const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W,
                   double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, int iters,
                   float* pose_out, double* cost, int* counts, void* workspace, void* stream);
int atdn_pnp_solve_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose_init, int B, int H,
                        int W, double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, int iters,
                        float* pose_out, double* cost, int* counts);

/* ---------------------------------------------------------------------------------------------------
 * Pose from flow alone (epipolar refinement)  —  the flow image 1 -> image 2 gives every pixel a correspondence, a relative pose
 * gives it an epipolar line: the pose that puts the correspondences on their lines, by Levenberg-Marquardt on the signed pixel
 * distance under the Geman-McClure loss, over the FIVE degrees of freedom two views show — the rotation and the direction of the
 * translation; the length of t is kept to the last bit of its own rounding —, batched over problems, all on the device.
 * atdn_epipolar_terms is one evaluation, atdn_epipolar_solve the solver. It needs no depth (atdn_pnp_solve does) and it is a
 * REFINEMENT from a pose that is already near, e.g. the pose head's: the cost does not see the sign of t nor the twisted pair
 * (R, t) <-> (rotation by pi about t, t), and nothing here chooses among them or searches globally. The reference has nothing
 * like it.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of the workspace of atdn_epipolar_terms / atdn_epipolar_solve for B planes of H x W (0 for sizes they refuse): as
 * atdn_pnp_workspace_bytes. No call reads what an earlier call left there. */
long atdn_epipolar_workspace_bytes(int B, int H, int W);

/* sums[b] = the 28 epipolar terms of pose[b] summed over the plane, counts[b] = (candidates, used, inliers).
 *   flow [B,2,H,W] fp32 DEVICE, image 1 -> image 2, channel 0 = x. mask [B,H,W] uint8 DEVICE or NULL: pixels whose byte is 0 are
 *   skipped. pose [B,12] fp32 DEVICE: the rows of [R|t] with X1 = R X2 + t, as for atdn_flow_two_view_depth. sums [B,28] float64
 *   DEVICE, counts [B,3] int32 DEVICE, workspace: atdn_epipolar_workspace_bytes(B, H, W) bytes DEVICE, 8-byte aligned like sums;
 *   no output (the workspace is one) overlaps an input or another output. fx, fy finite and > 0; cx, cy finite; scale_px,
 *   inlier_px (pixels) finite and > 0. B <= 65535, H * W <= 2^24, B, H, W >= 1. Anything else fails before a launch.
 * The rule: everything in float64, every operation rounded on its own (no fused multiply-add), only + - * / and comparisons — no
 * square root —, in exactly this order. r_ij, t_i: the pose as float64. c2 = scale_px*scale_px, thr = inlier_px*inlier_px.
 * Pixel (x, y) with (u, v) = flow:
 *   x2, y2, inside, a0, a1, q0, q1, b_i, n_i, res, m0, m1, l0, l1, ll = l0*l0 + l1*l1, epi2 = (res*res)/ll
 *                                                                 exactly as in atdn_flow_two_view_depth (one shared function)
 *   cand = mask byte != 0 && inside;  used = cand && ll > 0 && epi2 <= DBL_MAX  (a NaN fails);  inlier = used && epi2 <= thr
 *   s = 1 + epi2/c2, w = 1/(s*s), rho = (0.5*epi2)/s              (Geman-McClure)
 *   The step (dw, dth) acts as R <- C(dw) R, t <- C(dth) t with C the Cayley matrix below: the translation is rotated, never
 *   added to. With x*y - z*w meaning two rounded products and their rounded difference:
 *   Jres = (b x n, t x k) with k = a x b, a2 = 1:
 *     Jres_0 = b1*n2 - b2*n1, Jres_1 = b2*n0 - b0*n2, Jres_2 = b0*n1 - b1*n0
 *     k0 = a1*b2 - b1, k1 = b0 - a0*b2, k2 = a0*b1 - a1*b0
 *     Jres_3 = t1*k2 - t2*k1, Jres_4 = t2*k0 - t0*k2, Jres_5 = t0*k1 - t1*k0
 *   at = (a0*t0 + a1*t1) + t2;  e0 = l0/fx, e1 = l1/fy
 *   dm_j (j = 0, 1; the derivative of m_j; r_.j is column j of R):  R^T [n]x  and  R^T [a]x [t]x = (r_.j . t) a^T - at (r_.j)^T:
 *     dm_j0 = r_1j*n2 - r_2j*n1, dm_j1 = r_2j*n0 - r_0j*n2, dm_j2 = r_0j*n1 - r_1j*n0
 *     rt_j = (r_0j*t0 + r_1j*t1) + r_2j*t2
 *     dm_j3 = rt_j*a0 - at*r_0j, dm_j4 = rt_j*a1 - at*r_1j, dm_j5 = rt_j - at*r_2j
 *   kk = res/(2*ll), ww = w/ll
 *   dll_i = 2*(e0*dm_0i + e1*dm_1i),  j_i = Jres_i - kk*dll_i    (the derivative of res/sqrt(ll), times sqrt(ll): no root)
 *   terms 0..20: H_ij = (ww*j_i)*j_j for i <= j, row by row (00, 01, .., 05, 11, .., 55)
 *   terms 21..26: g_i = (ww*j_i)*res;  term 27: rho
 *   !used: +0.0 in all 28 terms
 * Sums and counts: exactly as for atdn_pnp_terms (chunks of 1024 flat indices, four per thread, the binary tree, the chunks in
 * order; no atomics, no memset). Two launches on `stream`: asynchronous, capturable, no host synchronisation.
 * counts[2]/counts[0] is the share of the flow's correspondences within inlier_px of their epipolar line; with no mask and
 * inlier_px = max_epipolar, counts[0] and counts[2] equal counts[0] and counts[1] of atdn_flow_two_view_depth at the same pose. */
int atdn_epipolar_terms(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx, double fy,
                        double cx, double cy, double scale_px, double inlier_px, double* sums, int* counts, void* workspace,
                        void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/epipolar_host.h, the functions the kernels call too): serves CPU
 * tensors, needs no GPU and no workspace, the same bits. */
int atdn_epipolar_terms_host(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double scale_px, double inlier_px, double* sums, int* counts);

/* pose_out[b] = the pose after `iters` Levenberg-Marquardt steps from pose_init[b] on the terms above; cost[b] and
 * counts[b] = (candidates, used, inliers, accepted steps) at it. Arguments as for atdn_epipolar_terms; pose_init, pose_out
 * [B,12] fp32 DEVICE, cost [B] float64 DEVICE (8-byte aligned), counts [B,4] int32 DEVICE, 0 <= iters <= 64.
 * The state, the decision rule and the lambda constants are those of atdn_pnp_solve, on the pose (R, t) in float64; evaluation 0
 * is at pose_init. Then, unless k = iters, from the accepted terms and the accepted t:
 *   A = H;  tt = (t0*t0 + t1*t1) + t2*t2;  gamma = ((H_33 + H_44) + H_55)/tt;  A_(3+i)(3+j) = A_(3+i)(3+j) + (gamma*t_i)*t_j
 *     (the gauge term: dth along t does not move t, the data give that direction no curvature, this gives it the block's mean)
 *   A_ii = A_ii + lambda*A_ii;  LDL^T, the two triangular solves and the failure rule of atdn_pnp_solve, delta = (dw, dth)
 *   C(d): h = 0.5*d, n2 = (h0*h0 + h1*h1) + h2*h2, f = 2/(1 + n2), C_ii = 1 + f*(h_i*h_i - n2), C_ij = f*(K_ij + h_i*h_j), K = [h]x
 *   R'_ij = (C(dw)_i0*r_0j + C(dw)_i1*r_1j) + C(dw)_i2*r_2j,  t'_i = (C(dth)_i0*t0 + C(dth)_i1*t1) + C(dth)_i2*t2
 * t = 0, a NaN in the pose or a plane without candidates need no special case: no pixel is used, the sums are +0.0, gamma or a
 * pivot fails, the trial is the accepted pose again and no step is ever accepted.
 * Output: the accepted R and t, each rounded to fp32 once; when no step was accepted pose_out holds the bits of pose_init.
 * `iters` steps are iters + 1 evaluations, two launches each; no host synchronisation, capturable. Under a redescending loss
 * the valley between rotation and translation direction of a forward motion is flat: small images with many outliers converge
 * linearly and may want more steps than the default of the Python layer. */
int atdn_epipolar_solve(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W, double fx,
                        double fy, double cx, double cy, double scale_px, double inlier_px, int iters, float* pose_out, double* cost,
                        int* counts, void* workspace, void* stream);
int atdn_epipolar_solve_host(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double scale_px, double inlier_px, int iters, float* pose_out,
                             double* cost, int* counts);

/* ---------------------------------------------------------------------------------------------------
 * Ground plane of a depth map (camera height and metric scale)  —  a camera of known height over a road sees a plane n . X = h.
 * With q = n / h, the ray a = ((x - cx)/fx, (y - cy)/fy, 1) and the depth z of a pixel, e = z*(q . a) - 1 is the RELATIVE depth
 * residual: linear in q, dimensionless, meaningful when the scale of the depth is wrong. The fitted height of a depth whose
 * scale is off by s is s * h_true: camera_height / h is the correction. n . X = h*(1 + e): a pixel stands -h*e above the road.
 * atdn_ground_terms is one evaluation, atdn_ground_solve a start vote and a Levenberg-Marquardt solve, atdn_ground_classify the
 * per-pixel map. No square root and no transcendental anywhere: the outputs are q and sums; normal = q / |q| and h = 1 / |q| are
 * formed by the caller. The reference has nothing like it.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of the workspace of atdn_ground_terms / atdn_ground_solve for B planes of H x W, whatever the rows (0 for sizes they
 * refuse): one solver state per problem; per chunk of 1024 pixels 10 float64 sums and four int32; per vote workgroup (at most 32
 * a plane) 320 int32. No call reads what an earlier call left there. */
long atdn_ground_workspace_bytes(int B, int H, int W);

/* sums[b] = the 10 terms of q[b] summed over the rows [y0, y1) of plane b, counts[b] = (candidates, used, inliers).
 *   depth [B,H,W] fp32 DEVICE. mask [B,H,W] uint8 DEVICE or NULL: pixels whose byte is 0 are skipped. q [B,3] float64 DEVICE.
 *   sums [B,10] float64 DEVICE, counts [B,3] int32 DEVICE, workspace: atdn_ground_workspace_bytes(B, H, W) bytes DEVICE; q, sums
 *   and workspace 8-byte aligned; no output (the workspace is one) overlaps an input or another output. 0 <= y0 < y1 <= H.
 *   fx, fy finite and > 0; cx, cy finite; scale_rel, inlier_rel (relative depth), min_z and max_depth finite and > 0.
 *   B <= 65535, H * W <= 2^24, B, H, W >= 1. Anything else fails before a launch.
 * The rule: everything in float64, every operation rounded on its own (no fused multiply-add), only + - * /, comparisons and
 * integer operations, in exactly this order. Constants: c2 = scale_rel*scale_rel, thr = inlier_rel*inlier_rel.
 * Pixel (x, y) of a row y0 <= y < y1, z = (double)depth:
 *   cand = mask byte != 0;  used = cand && min_z <= z <= max_depth           (a NaN or an infinity fails)
 *   ax = (x - cx)/fx, ay = (y - cy)/fy
 *   e = z*((q0*ax + q1*ay) + q2*1) - 1,  e2 = e*e
 *   s = 1 + e2/c2, w = 1/(s*s), rho = (0.5*e2)/s                             (Geman-McClure)
 *   inlier = used && e2 <= thr
 *   J = (z*ax, z*ay, z)                                                      (the derivative of e with respect to q)
 *   terms 0..5: H_ij = (w*J_i)*J_j for i <= j, row by row (00, 01, 02, 11, 12, 22); terms 6..8: g_i = (w*J_i)*e; term 9: rho
 *   !used: +0.0 in all 10 terms
 * Sums: the band is the plane of the (y1 - y0)*W flat indices i = (y - y0)*W + x, summed exactly as a plane of atdn_pnp_terms
 * (chunks of 1024 flat indices, four per thread, the binary tree over 256 threads, the chunks in order) over 10 terms instead of
 * 28. The three counts are integer sums. Two launches on `stream`: asynchronous, capturable, no host synchronisation. */
int atdn_ground_terms(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1, double fx,
                      double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z, double max_depth,
                      double* sums, int* counts, void* workspace, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/ground_host.h, the functions the kernels call too): serves CPU
 * tensors, needs no GPU and no workspace, the same bits. */
int atdn_ground_terms_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                           double fx, double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z,
                           double max_depth, double* sums, int* counts);

/* q[b] = the plane after the start vote (or from q_init[b]) and `iters` Levenberg-Marquardt steps on the terms above; sums[b] the
 * 10 terms and counts[b] = (candidates, used, inliers, accepted steps, votes of the mode, mode bin) at it. Arguments as for
 * atdn_ground_terms; q_init [B,3] float64 DEVICE or NULL (the vote); (nx, ny, nz) the prior normal, finite and not zero (any
 * length); min_votes >= 1; 0 <= iters <= 64; q [B,3] float64, sums [B,10] float64, counts [B,6] int32 DEVICE.
 * Start vote (q_init NULL): nothing lies below the road, so under the prior normal the ground pixels share one height and
 * everything else spreads over smaller ones. For every used pixel
 *   hgt = z*((nx*ax + ny*ay) + nz*1);  k = (int64)(bits(hgt) >> 47) - 1019*32;  the pixel votes for bin k iff 0 <= k < 320
 *   (the exponent and the top 5 mantissa bits of the float64: 2^-4 <= hgt < 2^6 in 320 bins of 1.6 .. 3.1 % relative width)
 *   smoothed_k = c_{k-1} + c_k + c_{k+1} (c_-1 = c_320 = 0); the mode is the k of the largest smoothed_k — among equal ones that
 *   of the largest c_k (a single populated bin k has smoothed_{k-1} = smoothed_k = smoothed_{k+1}: the mode is k), among those
 *   the lowest k —, votes = smoothed_k
 *   votes < min_votes: there is no plane — q = 0, sums = +0.0 and all six counts 0
 *   otherwise the start is q = (nx, ny, nz) / centre, each component one division, centre = the float64 of the bits
 *   ((k + 1019*32) << 47) | (1 << 46)
 * With q_init the start is q_init, votes = 0 and bin = -1.
 * Decision and lambda: those of atdn_pnp_solve — evaluation 0 is accepted with lambda = 1e-3, a later one iff its cost (term 9)
 * is smaller (a NaN fails); lambda = max(lambda/3, 1e-9) on accept, min(4*lambda, 1e6) on reject. Then, unless k = iters:
 *   A = H of the accepted terms with A_ii = H_ii + lambda*H_ii; LDL^T without pivoting and the two triangular solves of
 *   atdn_pnp_solve with 6 replaced by 3, right-hand side -g; some d_j > 0 fails, or some |delta_i| <= DBL_MAX fails: the trial
 *   is the accepted q again; otherwise trial_i = q_i + delta_i.
 * Two launches for the vote and two per evaluation (the terms; one wave per problem for the order-fixed sum, the decision and
 * the step); the histogram is counted in LDS per workgroup and the workgroups' histograms are added by the second launch:
 * integer sums, no global atomics, no memset, no host synchronisation, capturable. */
int atdn_ground_solve(const float* depth, const unsigned char* mask, const double* q_init, int B, int H, int W, int y0, int y1,
                      double fx, double fy, double cx, double cy, double nx, double ny, double nz, double scale_rel,
                      double inlier_rel, double min_z, double max_depth, int min_votes, int iters, double* q, double* sums,
                      int* counts, void* workspace, void* stream);
int atdn_ground_solve_host(const float* depth, const unsigned char* mask, const double* q_init, int B, int H, int W, int y0, int y1,
                           double fx, double fy, double cx, double cy, double nx, double ny, double nz, double scale_rel,
                           double inlier_rel, double min_z, double max_depth, int min_votes, int iters, double* q, double* sums,
                           int* counts);

/* residual [B,H,W] fp32 = e of every used pixel of the rows [y0, y1) at q[b], rounded to fp32 once (+0.0 elsewhere), on_ground
 * [B,H,W] uint8 = 1 where e2 <= inlier_rel*inlier_rel there, 0 elsewhere. Arguments as for atdn_ground_terms. One launch. */
int atdn_ground_classify(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                         double fx, double fy, double cx, double cy, double inlier_rel, double min_z, double max_depth,
                         float* residual, unsigned char* on_ground, void* stream);
int atdn_ground_classify_host(const float* depth, const unsigned char* mask, const double* q, int B, int H, int W, int y0, int y1,
                              double fx, double fy, double cx, double cy, double inlier_rel, double min_z, double max_depth,
                              float* residual, unsigned char* on_ground);

/* ---------------------------------------------------------------------------------------------------
 * Pose-graph optimisation (loop closure)  —  the poses of the keyframes are the nodes, a measured relative pose between two of
 * them is an edge: consecutive keyframes by odometry, revisits by relocalisation and PnP. Levenberg-Marquardt over the graph
 * with a conjugate-gradient solve preconditioned by the block-tridiagonal part of the system (a keyframe graph is a chain plus
 * a few loops), batched over graphs, all on the device in ONE launch. atdn_pose_graph_terms is one evaluation,
 * atdn_pose_graph_solve the solver. The reference has nothing like it.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of the workspace of atdn_pose_graph_terms / atdn_pose_graph_solve for B graphs of N nodes and E edges (0 for sizes they
 * refuse): per graph 190 float64 per node, 122 per edge and (5 E + 3 N + 1) int32 rounded up to 8 bytes. No call reads what an
 * earlier call left there. */
long atdn_pose_graph_workspace_bytes(int B, int N, int E);

/* cost[b] = the cost of graph b at poses[b], edge_chi2[b][e] = c_e of every edge, counts[b] = (valid edges, absent edges).
 *   poses [B,N,12] fp32 DEVICE: the rows of [R|t] of every node, world <- camera. edge_index [B,2,E] int32 DEVICE: the i's of
 *   the E edges, then their j's. edge_pose [B,E,12] fp32 DEVICE: the rows of the measurement Z_e = [Rz|tz] of T_i^-1 T_j.
 *   edge_weight [B,E,2] float64 DEVICE = (w_rot, w_tr), 1/sigma^2 in rad^-2 and m^-2, 8-byte aligned. edge_robust [B,E] uint8
 *   DEVICE or NULL: a non-zero byte puts the edge under the Geman-McClure loss of scale robust_scale (NULL: none).
 *   cost [B] float64, edge_chi2 [B,E] float64 (both 8-byte aligned), counts [B,2] int32, workspace of
 *   atdn_pose_graph_workspace_bytes(B, N, E) bytes (8-byte aligned), all DEVICE; no output (the workspace is one) overlaps an
 *   input or another output. 1 <= B <= 1024, 2 <= N <= 2048, 1 <= E <= 8192, robust_scale finite and > 0. Anything else fails
 *   before a launch. The B graphs are independent.
 * The rule: everything in float64, every operation rounded on its own (no fused multiply-add), only + - * / and comparisons, in
 * exactly this order. dot3(a, b) = (a0*b0 + a1*b1) + a2*b2. Poses and measurements are converted to float64 exactly.
 * Edge e = (i, j) is ABSENT if i or j is outside [0, N), i == j, or a weight fails 0 <= w <= DBL_MAX: it contributes nothing,
 * reads no pose and has edge_chi2 = +0.0. An edge that is not absent is valid; a valid edge with w_rot == 0 and w_tr == 0 is
 * IDLE: it is counted, has edge_chi2 = c_e (+0.0) and takes part in nothing else, so that it gives the same bits as the list
 * without it. The other valid edges are ACTIVE.
 * Residual of an edge at (R_i, t_i), (R_j, t_j):
 *   M_ab = dot3(column a of R_i, column b of R_j);  Re_ab = dot3(column a of Rz, column b of M)          (Re = Rz^T R_i^T R_j)
 *   d = t_j - t_i;  tm_a = dot3(column a of R_i, d);  u = tm - tz;  te_a = dot3(column a of Rz, u)
 *   a = (0.5*(Re_21 - Re_12), 0.5*(Re_02 - Re_20), 0.5*(Re_10 - Re_01))       (indices from 0: the chordal rotation error, sin of
 *     the angle times the axis, no trigonometry; monotone in the angle below 90 degrees, far above any drift a loop closure sees)
 *   c_e = w_rot*dot3(a, a) + w_tr*dot3(te, te)
 *   not robust: cost term c_e, omega = 1.  robust, q = robust_scale*robust_scale: s = q + c_e, cost term (q*c_e)/s,
 *   omega = (q/s)*(q/s)
 * Cost: node n's share is the sum of the cost terms of the active edges whose i is n, in ascending edge number (+0.0 without
 * one); the cost is the ordered sum of the shares over the nodes (below). Summing by node rather than by edge number is what
 * makes an idle edge invisible.
 * Ordered sum over the nodes n = 0 .. N-1: chunks of 256 consecutive nodes, +0.0 beyond N; in a chunk for stride = 1, 2, .., 128:
 * v[i] = v[i] + v[i + stride] for every i that is a multiple of 2*stride; the chunk sums are added in chunk order (the tree of
 * atdn_pnp_terms).
 * One launch on `stream`: asynchronous, capturable, no host synchronisation, no atomics, no memset. */
int atdn_pose_graph_terms(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                          const unsigned char* edge_robust, int B, int N, int E, double robust_scale, double* cost,
                          double* edge_chi2, int* counts, void* workspace, void* stream);
/* The same function on HOST buffers in plain C++ float64 (csrc/pose_graph_host.h, the functions the kernel calls too): serves
 * CPU tensors, needs no GPU and no workspace, the same bits. */
int atdn_pose_graph_terms_host(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                               const unsigned char* edge_robust, int B, int N, int E, double robust_scale, double* cost,
                               double* edge_chi2, int* counts);

/* poses_out[b] = the poses of graph b after `iters` Levenberg-Marquardt steps (iters + 1 cost evaluations). Arguments as for
 * atdn_pose_graph_terms, and: fixed [B,N] uint8 DEVICE or NULL (a non-zero byte holds the node; NULL: none is held — the
 * caller should hold at least one, the gauge), 0 <= iters <= 32, 1 <= cg_iters <= 128, cg_tol finite and > 0, poses_out
 * [B,N,12] fp32, cost [B,2] float64 = (the cost at poses, the last accepted cost), edge_chi2 [B,E] float64 = c_e at poses_out
 * (what atdn_pose_graph_terms returns for poses_out), counts [B,4] int32 = (valid edges, absent edges, accepted steps, CG
 * iterations in total).
 * A node is FREE if it is not held and has at least one active edge; every other node is left out of the system and its pose
 * comes back with the input bits. A step moves node n by x_n = (dw, dt): R <- R C(dw), t <- R dt + t (C: the Cayley map below).
 * Jacobians of (a, te) of an edge with respect to that step (6 x 6, rows (a, te), columns (dw, dt); tr = (Re_00 + Re_11) + Re_22):
 *   node j: rows 0..2: 0.5*(tr - Re_aa) on the diagonal, -0.5*Re_ba off it, then zeros; rows 3..5: zeros, then Re
 *   node i: rows 0..2: -0.5*dot3(row a of G, row b of Rz) with G_aa = tr - Re_aa, G_ab = -Re_ab, then zeros;
 *           rows 3..5: P_ab = dot3(column a of Rz, column b of [tm]x) with [tm]x = ((0, -tm2, tm1), (tm2, 0, -tm0), (-tm1, tm0, 0)),
 *           then -Rz^T
 * With w = omega*(w_rot, w_rot, w_rot, w_tr, w_tr, w_tr), an edge's blocks are (X^T W Y)_ab = the sum over k = 0..5, in that
 * order, of (w_k*X_ka)*Y_kb — the products with the structural zeros formed like any other —: A_ii = Ji^T W Ji and
 * A_jj = Jj^T W Jj (a <= b computed, the rest mirrored), A_ij = Ji^T W Jj; its gradients g_a = the sum over k of (w_k*J_ka)*r_k
 * with r = (a, te).
 * A free node's diagonal block D_n and gradient g_n are the sums of A_ii / g_i (where it is the edge's i) or A_jj / g_j (where it
 * is the j) over its active edges in ascending edge number. The damped system: A = D_n with (D_n)_aa + lambda*(D_n)_aa on the
 * diagonal, and for every active edge between two free nodes A_ij at (i, j) and its transpose at (j, i). (A p)_n = the rows of
 * the damped D_n times p_n (b ascending), then + the edge blocks times the other node's p, edge by edge in ascending edge number
 * (each a sum over b ascending). U_n, the block (n, n+1) of the preconditioner, exists where n and n+1 are both free: the sum
 * over the active edges that join them, in ascending edge number, of A_ij (i == n) or its transpose (zeros without such an edge).
 * Block LDL^T, n ascending over the free nodes: S_n = damped D_n, minus, where n-1 is free, for a >= b the sum over c ascending
 * of (U_{n-1})_ca*(W_{n-1})_cb; S_n = L diag(d) L^T by the 6 x 6 recurrence of atdn_pnp_solve on its lower triangle; a pivot that
 * is not > 0 fails the step; where n+1 is free, W_n = S_n^-1 U_n column by column (forward, divide, backward as there).
 * z = M^-1 r: forwards y_n = r_n - (sum over c ascending of (W_{n-1})_ca*(y_{n-1})_c) where n-1 is free; backwards
 * z_n = S_n^-1 y_n - (sum over c ascending of (W_n)_ac*(z_{n+1})_c) where n+1 is free. Vectors are +0.0 at nodes that are not free.
 * Dot products: a node's six products summed in index order, then the ordered sum over the nodes.
 * PCG for A x = -g: x = 0, r = -g, z = M^-1 r, p = z, rz = r.z, thr = (cg_tol*cg_tol)*rz; no iteration unless rz > 0 (a zero
 * right-hand side gives a zero step). At most cg_iters times: pAp = p.(A p); stop unless pAp > 0; alpha = rz/pAp;
 * x = x + alpha*p; r = r - alpha*(A p) (one iteration counted); z = M^-1 r; rz' = r.z; stop unless rz' > thr; beta = rz'/rz;
 * p = z + beta*p; rz = rz'.
 * Retraction of a free node (the Cayley map of atdn_pnp_solve): h = 0.5*dw, n2 = (h0*h0 + h1*h1) + h2*h2, f = 2/(1 + n2),
 *   M_ii = h_i*h_i - n2, M_ij = K_ij + h_i*h_j with K = [h]x, C_ii = 1 + f*M_ii, C_ij = f*M_ij;
 *   R'_ab = dot3(row a of R, column b of C), t'_a = dot3(row a of R, dt) + t_a.
 * Outer loop: the first evaluation is at poses and is the accepted point, lambda = 1e-3. Each of the `iters` steps: linearise at
 * the accepted point (unless the last step was rejected: the linearisation stands), factor, PCG, retract, evaluate the cost
 * at the trial; accepted iff cost_trial < cost_accepted (a NaN fails); on accept lambda = max(lambda/3, 1e-9), on reject
 * lambda = min(4*lambda, 1e6) (the decision rule and the constants of atdn_pnp_solve). A failed pivot or a step with some
 * |x| <= DBL_MAX failing is a rejection without an evaluation.
 * Output: each value of an accepted free node's pose rounded to fp32 once; with no accepted step every pose holds the input bits.
 * The Geman-McClure loss works when the drift at a loop is within robust_scale: far beyond it every robust edge saturates
 * (omega -> 0) and nothing moves — a property of the loss. Solve with a large scale first, then a smaller one.
 * One launch of one workgroup per graph on `stream`: asynchronous, capturable, no host synchronisation, no atomics, no memset;
 * every loop bound is an argument. */
int atdn_pose_graph_solve(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                          const unsigned char* edge_robust, const unsigned char* fixed, int B, int N, int E, double robust_scale,
                          int iters, int cg_iters, double cg_tol, float* poses_out, double* cost, double* edge_chi2, int* counts,
                          void* workspace, void* stream);
int atdn_pose_graph_solve_host(const float* poses, const int* edge_index, const float* edge_pose, const double* edge_weight,
                               const unsigned char* edge_robust, const unsigned char* fixed, int B, int N, int E,
                               double robust_scale, int iters, int cg_iters, double cg_tol, float* poses_out, double* cost,
                               double* edge_chi2, int* counts);

/* ---------------------------------------------------------------------------------------------------
 * Voxel map  —  every keyframe's depth (and colour) accumulated into ONE voxel-hashed point cloud: the scatter primitive of the
 * library. A pixel's point falls into a cubic voxel; per voxel the table keeps the number of points, the sum of their sub-voxel
 * positions and of their colour bytes, all as exact integers. Integer sums commute: every bit of the result is independent of
 * thread order, launch geometry and of how the keyframes are split over calls. The reference has nothing like it.
 *
 * The rule. Integer arithmetic or float64 with every operation rounded on its own (no fused multiply-add); only + - * /,
 * comparisons and the two conversions named below.
 *   depth [N,H,W] fp32; poses [N,12] fp32, rows of [R|t], world <- camera; (fx, fy, cx, cy) float64; images [N,3,H,W] uint8 or
 *   NULL (channels 0, 1, 2 are red, green, blue as stored); mask [K,H,W] uint8 or NULL (a zero byte excludes the pixel);
 *   stride >= 1: only pixels with x % stride == 0 && y % stride == 0 take part; voxel > 0, origin o, min_z, max_z.
 * Per pixel (k, y, x) that takes part:
 *   z = (double)depth; the pixel is a CANDIDATE iff min_z <= z && z <= max_z (a NaN fails)
 *   xn = ((double)x - cx)/fx, yn = ((double)y - cy)/fy, c = (xn*z, yn*z, z)
 *   p_a = dot3(row a of R, c) + t_a, dot3 = (r_a0*c_0 + r_a1*c_1) + r_a2*c_2;  g_a = (p_a - o_a)/voxel
 *   the candidate is OUTSIDE unless -2^20 <= g_a && g_a < 2^20 for all three axes (a NaN or an infinity from a pose lands
 *   here): counted, not inserted
 *   k_a = floor(g_a): truncated to an integer, minus 1 if the integer converted back exceeds g_a
 *   f_a = g_a - (double)k_a, q_a = (integer)(f_a*65536), truncated: 0 .. 65535, and 65536 for the negative g_a so small that
 *   g_a + 1 rounds to 1
 *   key = ((k_x + 2^20) << 42) | ((k_y + 2^20) << 21) | (k_z + 2^20)
 * Per voxel, exact integers: n = the number of inserted points, S_a = the sum of q_a, C_c = the sum of colour byte c (with images).
 * Extraction with min_count >= 1: the voxels with n >= min_count, and of each
 *   points_a = (float)(o_a + ((double)k_a + ((double)S_a/(double)n + 0.5)/65536)*voxel)
 *   colors_c = (C_c + n/2)/n in integer division;  counts = n;  keys = key
 * Counters (int64): candidates, inserted, outside, dropped, voxels; always candidates == inserted + outside + dropped.
 *
 * The table: atdn_voxel_table_bytes(capacity) = 64 + 64*capacity bytes, 8-byte aligned, capacity a power of two in [2, 2^31],
 * little-endian 64-bit words. Words 0..7: the header — candidates, inserted, outside, dropped, voxels, two scratch words of the device extraction (0 between
 * calls), one reserved (0). Words
 * 8 + 8 s .. 8 + 8 s + 7: slot s — key (all ones = empty), n, S_x, S_y, S_z, C_red, C_green, C_blue. While the table holds fewer
 * than 2^31 points S < 2^47 and C < 2^39: no sum can overflow. Open addressing with linear probing from
 * home(key) = (((key * 0x9E3779B97F4A7C15 mod 2^64) >> 32) * capacity) >> 32 (the top log2(capacity) bits of the product: every
 * bit of the key reaches them), over at most min(capacity, 1024) slots; a point that
 * finds neither its key nor an empty slot there is counted as DROPPED. Which slot a key lives in depends on the order of
 * arrival; the set of keys and every sum do not. On the device insertion is a 64-bit compare-and-swap on the key word and the
 * sums are 64-bit integer atomic adds whose results nobody reads; no thread waits for another, there is no lock and no retry,
 * every loop bound is an argument or a constant. DEVICE entry points take device memory and are launches on `stream`
 * (asynchronous, capturable, no host synchronisation); the _host twins take host memory, run on the calling thread and give the
 * same bits.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of a table of `capacity` slots (0 for a capacity the entry points refuse). */
long atdn_voxel_table_bytes(long capacity);

/* An empty table: every key all ones, every sum and counter 0. One launch. */
int atdn_voxel_clear(void* table, long capacity, void* stream);
int atdn_voxel_clear_host(void* table, long capacity);

/* Adds the pixels of K keyframes to the table. depth, poses, images are banks of N keyframes; list position j < K reads keyframe
 * indices[j] (int32 [K], DEVICE; an index outside [0, N) contributes nothing; repeats are integrated again), or keyframe j when
 * indices is NULL (then K <= N). mask and pending are [K,H,W] by list position. pending (or NULL) is written in full: 1 at
 * exactly the pixels this call dropped, 0 elsewhere — grow the table (atdn_voxel_rehash) and call again with mask = pending and
 * retry = 1: a retry call counts no candidates, and every point it inserts moves from `dropped` to `inserted`, so a grown table
 * ends with the bits of one that was large from the start. No output may overlap an input or another output. One launch. */
int atdn_voxel_integrate(const float* depth, const float* poses, const uint8_t* images, const uint8_t* mask, const int* indices, int N,
                         int K, int H, int W, double fx, double fy, double cx, double cy, int stride, double voxel, double ox,
                         double oy, double oz, double min_z, double max_z, int retry, void* table, long capacity, uint8_t* pending,
                         void* stream);
int atdn_voxel_integrate_host(const float* depth, const float* poses, const uint8_t* images, const uint8_t* mask, const int* indices,
                              int N, int K, int H, int W, double fx, double fy, double cx, double cy, int stride, double voxel,
                              double ox, double oy, double oz, double min_z, double max_z, int retry, void* table, long capacity,
                              uint8_t* pending);

/* Re-inserts every occupied slot of src into dst (dst_capacity >= src_capacity, the tables disjoint), sums included, and adds
 * src's candidates, inserted, outside and dropped to dst's: into a cleared dst, the table as if it had been that large from the
 * start. An entry that finds no slot (dst was not empty) moves its n from inserted to dropped. One launch. */
int atdn_voxel_rehash(const void* src, long src_capacity, void* dst, long dst_capacity, void* stream);
int atdn_voxel_rehash_host(const void* src, long src_capacity, void* dst, long dst_capacity);

/* The voxels with n >= min_count, compacted: points [max_out,3] fp32, colors [max_out,3] uint8 (or NULL), counts [max_out]
 * int32, keys [max_out] int64, found [1] int64 = the number of qualifying voxels, which may exceed max_out: nothing is written
 * past max_out entries. The device writes in table order (which entries are kept when found > max_out is then arbitrary); the
 * host form writes in ascending key order. voxel and origin are those of the integration. One launch, no memset: the device
 * form counts in the header's two scratch words and leaves them 0, so two extractions of ONE table must not run concurrently. */
int atdn_voxel_extract(void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz, long max_out,
                       float* points, uint8_t* colors, int* counts, int64_t* keys, int64_t* found, void* stream);
int atdn_voxel_extract_host(void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz,
                            long max_out, float* points, uint8_t* colors, int* counts, int64_t* keys, int64_t* found);

/* ---------------------------------------------------------------------------------------------------
 * Map view  —  a point cloud (what atdn_voxel_extract writes, or a cloud read back from map.ply) rendered into B cameras with a
 * z-buffer: the inverse of atdn_voxel_integrate and the library's second scatter primitive. Every point is a flat square splat
 * that carries one 64-bit word; a pixel keeps the MINIMUM word of the splats that cover it. min commutes: every bit of the
 * result is a function of the SET of points alone, independent of thread order and launch geometry. The reference has nothing
 * like it.
 *
 * The rule. Float64 with every operation rounded on its own (no fused multiply-add); only + - * /, comparisons and the
 * conversions named below.
 *   points [M,3] fp32; colors [M,3] uint8 or NULL (red, green, blue); counts [M] int32; poses [B,12] fp32, rows of [R|t],
 *   world <- camera; (fx, fy, cx, cy) float64; H, W; size > 0 the edge of a voxel; splat > 0 the footprint in voxel edges;
 *   max_splat >= 1 the cap of a footprint's side in pixels; 0 < near <= far, far finite and representable in fp32; min_count >= 1.
 * Per camera b and point i with counts[i] >= min_count (a CANDIDATE; n = counts[i]):
 *   d_a = (double)p_a - (double)t_a;  c_a = dot3(r_0a, d_0, r_1a, d_1, r_2a, d_2), dot3 = (x0*y0 + x1*y1) + x2*y2 (column a
 *   of R: c = R^T d);  z = c_2
 *   in range iff near <= z && z <= far (a NaN fails)
 *   u = (c_0/z)*fx + cx,  v = (c_1/z)*fy + cy
 *   hx = (((0.5*splat)*size)*fx)/z, then 0.5 where hx < 0.5 and 0.5*max_splat where hx > 0.5*max_splat; hy with fy
 *   the footprint is the half-open square [u-hx, u+hx) x [v-hy, v+hy): with a = u-hx and e = u+hx it covers the columns
 *     x0 = 0 where a < 0, else ceil(a), which needs a <= W-1;   x1 = W-1 where e > W-1, else ceil(e)-1, which needs e > 0
 *   ceil(a) = a truncated to an integer, plus 1 if the integer converted back is below a. Both needs are compared in double
 *   before any conversion, so a NaN or an infinity that fails one converts nothing. Rows y0, y1 likewise from v, hy and H.
 *   the point is VISIBLE iff it is in range, both needs hold on both axes, and x0 <= x1 && y0 <= y1
 *   word = (bits((float)z) << 32) | ((255 - min(n,255)) << 24) | (red << 16) | (green << 8) | blue   (colour bytes 0 without
 *   colours), the same on every pixel (y0..y1) x (x0..x1)
 * Per pixel: the minimum word over the visible points that cover it; all ones = empty. Positive fp32 bit patterns order like the
 * numbers, so the minimum is the nearest point; among equal fp32 depths the larger min(n,255), then the smaller packed colour.
 * Outputs, 0 everywhere at an empty pixel:
 *   depth [B,H,W] fp32 = the word's high half reinterpreted;  colors_out [B,3,H,W] uint8 or NULL;  support [B,H,W] uint8 =
 *   min(n,255) of the winner;  counts_out [B,3] int64 = candidates, visible points, covered pixels of camera b.
 * A NaN or an infinity in a pose or a point writes nothing: that (camera, point) is simply not visible.
 * ------------------------------------------------------------------------------------------------- */

/* Bytes of the device form's workspace, 8*B*H*W: one word per pixel. 0 for sizes the entry point refuses (a dimension < 1,
 * B > 65535 or B*H*W >= 2^31). */
long atdn_view_workspace_bytes(int B, int H, int W);

/* Renders M >= 0 points into B cameras (M == 0: points, colors and counts may be NULL; empty images). All pointers DEVICE;
 * points, counts, poses and depth 4-byte aligned, counts_out and workspace 8-byte aligned; no output may overlap an input or
 * another output (the workspace counts as an output). Three launches on `stream` (asynchronous, capturable, no host
 * synchronisation, no memset): a clear of the workspace and counts_out, the splat — plain 64-bit read, then an unsigned 64-bit
 * atomic min whose result nobody reads, only where the new word is smaller — and the resolve. No thread waits for another, there
 * is no lock and no retry, every loop bound is an argument or a constant. The _host twin takes host memory, runs on the calling
 * thread and gives the same bits. */
int atdn_view_render(const float* points, const uint8_t* colors, const int* counts, int M, const float* poses, int B, int H, int W,
                     double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near, double far,
                     int min_count, float* depth, uint8_t* colors_out, uint8_t* support, int64_t* counts_out, void* workspace,
                     void* stream);
int atdn_view_render_host(const float* points, const uint8_t* colors, const int* counts, int M, const float* poses, int B, int H,
                          int W, double fx, double fy, double cx, double cy, double size, double splat, int max_splat, double near,
                          double far, int min_count, float* depth, uint8_t* colors_out, uint8_t* support, int64_t* counts_out);

/* ---------------------------------------------------------------------------------------------------
 * Visibility votes and carving  —  per point of the map's cloud: how many keyframes have it in view, how many measured a depth
 * that confirms it, how many see straight through it; and the removal of voxels from the table. The only way a voxel leaves
 * the voxel map. A gather (point x keyframe: one projection, a window of depth reads, three integer votes), no render and no
 * scatter. Integer sums commute: every bit of the votes is independent of thread order, launch geometry and of how the
 * keyframes are split over calls. The reference has nothing like it.
 *
 * The rule. Float64 with every operation rounded on its own (no fused multiply-add); only + - * /, comparisons and the
 * conversions named below.
 *   points [M,3] fp32 (what atdn_voxel_extract writes, or a cloud read from map.ply); depth [N,H,W] fp32; poses [N,12] fp32, rows
 *   of [R|t], world <- camera; indices [K] int32 or NULL as in atdn_voxel_integrate (an index outside [0, N) contributes
 *   nothing, a repeat votes again, NULL means keyframe j at list position j and K <= N); (fx, fy, cx, cy) float64;
 *   0 < near <= far, far finite; rel >= 0 and abs >= 0, finite; radius in 0..8; accumulate in {0, 1}.
 * Per point i and list position j (keyframe k):
 *   d_a = (double)p_a - (double)t_a;  c_a = dot3(r_0a, d_0, r_1a, d_1, r_2a, d_2), dot3 = (x0*y0 + x1*y1) + x2*y2 (column a
 *   of R: c = R^T d, as in the map view);  z = c_2
 *   IN RANGE iff near <= z && z <= far (a NaN fails)
 *   u = (c_0/z)*fx + cx,  v = (c_1/z)*fy + cy,  a = u + 0.5,  b = v + 0.5
 *   IN VIEW iff in range and a >= radius && a < W - radius && b >= radius && b < H - radius, every comparison made in double
 *   before any conversion (a NaN or an infinity converts nothing); then x and y are a and b truncated (both non-negative), and
 *   the whole (2 radius + 1)^2 window around (x, y) lies inside the image
 *   band = rel*z + abs,  lo = z - band,  hi = z + band
 *   a depth m is MEASURED iff near <= m && m <= far, evaluated on (double)depth: 0, NaN, +-inf and negative values fail
 *   SUPPORT iff the centre depth is measured and lo <= m && m <= hi
 *   FREE iff every pixel of the window is measured and has m > hi (the centre belongs to the window: FREE and SUPPORT exclude
 *   each other; requiring the whole window keeps slanted surfaces and silhouettes from carving themselves)
 *   everything else is occluded or unknown and casts no vote
 * votes [M,3] int32 = per point the number of list positions IN VIEW, with SUPPORT, FREE: written with accumulate == 0, added
 * to what is there with accumulate == 1.
 *
 * Removal. keys [R] int64, flags [R] uint8 or NULL (NULL: every key; else the keys with a non-zero flag). Each flagged key is
 * looked up by a read-only probe: the home slot and the min(capacity, 1024) limit of insertion, ended by an empty slot. Where
 * the key is found with n > 0, n, S and C become 0 and the key word stays: the emptied voxel keeps its slot, so no probe chain
 * breaks; atdn_voxel_extract skips it (n >= min_count >= 1 fails before any division), atdn_voxel_rehash carries it along
 * unchanged, a later atdn_voxel_integrate refills it like any voxel. The header's five counters are not touched: `inserted`
 * keeps meaning points ever inserted, `voxels` occupied slots. removed [3] int64 = voxels emptied, points they held, flagged
 * keys not found or already empty (a repeated key counts once as emptied, then as already empty).
 * ------------------------------------------------------------------------------------------------- */

/* Votes of M >= 0 points (M == 0: nothing is launched, points and votes may be NULL). All pointers DEVICE and 4-byte aligned;
 * votes may not overlap an input. One launch with accumulate == 1, two with 0 (a clear of votes first), on `stream`
 * (asynchronous, capturable, no host synchronisation, no memset): int32 atomic adds whose results nobody reads, only where a
 * vote is non-zero. No thread waits for another, there is no lock and no retry, every loop bound is an argument or a constant.
 * The _host twin takes host memory, runs on the calling thread and gives the same bits. */
int atdn_voxel_votes(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K, int H,
                     int W, double fx, double fy, double cx, double cy, double near, double far, double rel, double abs, int radius,
                     int accumulate, int* votes, void* stream);
int atdn_voxel_votes_host(const float* points, int M, const float* depth, const float* poses, const int* indices, int N, int K,
                          int H, int W, double fx, double fy, double cx, double cy, double near, double far, double rel, double abs,
                          int radius, int accumulate, int* votes);

/* Empties the voxels of the flagged keys (R >= 0; R == 0: removed = 0 and nothing else). table, keys and removed 8-byte aligned;
 * neither the table nor removed may overlap keys, flags or each other. Two launches on `stream` (a clear of removed, then a
 * thread per key: a 64-bit exchange on n, plain zero stores on S and C), no memset, no host synchronisation. Must not run
 * concurrently with another call on the same table. */
int atdn_voxel_remove(void* table, long capacity, const int64_t* keys, const uint8_t* flags, long R, int64_t* removed,
                      void* stream);
int atdn_voxel_remove_host(void* table, long capacity, const int64_t* keys, const uint8_t* flags, long R, int64_t* removed);

/* ---------------------------------------------------------------------------------------------------
 * Keyframe map  —  replaces the keyframe list of NeuralSLAM's relocalisation (keyframe_map.py)
 *   embeddings: Frame.embedding, one MappingVAE call per keyframe (slam_framework/neural_slam.py:88-103,158-164)
 *   search:     the per-keyframe torch.norm loop, torch.stack and argmin (neural_slam.py:374-383)
 *   images:     torch.load(rgb_file).to(device).float() of the chosen keyframe (neural_slam.py:386-390)
 * ------------------------------------------------------------------------------------------------- */

/* dist[q][k] = torch.norm(bank[k] - queries[q], p=2) (neural_slam.py:379) for every keyframe and query in one launch, then
 * idx[q][0..topk) = the topk nearest keyframes of query q, ascending, equal distances by the lower index (idx[q][0] is
 * torch.argmin of the reference's list, neural_slam.py:382).
 *   bank [K][D] fp32 (a row is what atdn_vae_encode writes for one image: D = out_h * out_w * 128), queries [Q][D],
 *   dist [Q][K] fp32, idx [Q][topk] int32; all DEVICE. D % 4 == 0, bank and queries 16-byte aligned, K >= 1, any Q >= 1
 *   (16 queries share one pass over the bank), 1 <= topk <= min(K, 16); anything else fails before a launch.
 * The difference is formed first and squared (no |a|^2 + |b|^2 - 2ab expansion): a row equal to the query gives exactly 0.
 * The summation order is fixed (keyframe_map.hip), so dist[q][k] depends on row k and query q alone: the same bits whatever
 * Q, K, the row's slot or the other queries are. Relative error of a distance <= 2.3e-6 for D <= 16384. */
int atdn_map_search(const float* bank, int K, int D, const float* queries, int Q, int topk, float* dist, int* idx, void* stream);

/* out[j] = float(bank[index_host[j]]): uint8 keyframe images of the image bank as the fp32 batch the VAE encoder and the
 * flow network read. bank [K][plane_bytes] uint8 (plane_bytes = 3 * H * W, a multiple of 16; DEVICE, 16-byte aligned),
 * out [n][plane_bytes] fp32 (DEVICE, 16-byte aligned). `index_host` is a HOST array of n ints, each checked against
 * [0, K) before anything is launched; repeated and unordered indices are fine. Exact. */
int atdn_map_gather_images_u8(const uint8_t* bank, int K, long plane_bytes, const int* index_host, int n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------
 * Individual kernels, exported for unit parity tests and roofline micro-benchmarks
 * ------------------------------------------------------------------------------------------------- */

/* CorrBlock.__call__ (whl:GMA/core/corr.py:32-53): pyramid level l is [B*H8*W8][H_l*W_l] with
 * H_l = H8 >> l, W_l = W8 >> l; coords [B*H8*W8][2] (x,y); out [B*H8*W8][ldo], channel l*81 + i*9 + j. */
int atdn_corr_lookup(const float* pyr0, const float* pyr1, const float* pyr2, const float* pyr3, int B, int H8,
                     int W8, const float* coords, float* out, int ldo, void* stream);

/* CorrBlock.__init__ (corr.py:16-30,55-63): fmap1, fmap2 channels-last [B][H8*W8][C] (C % 32 == 0) ->
 * pyr0..pyr3 as above. */
int atdn_corr_pyramid(const float* fmap1, const float* fmap2, int B, int H8, int W8, int C, float* pyr0, float* pyr1,
                      float* pyr2, float* pyr3, void* stream);

/* The same two operations through the kernels of the DEFAULT (split-f16) path — what atdn_gma_forward launches and
 * bench.py times: corr_bricks_kernel for all four levels (corr.py:16-30,55-63; levels 1-3 from 2x2-pooled target features,
 * avg_pool2d commutes with the dot product), the brick-major pyramid, and lookup_conv_kernel (corr.py:32-53 +
 * utils/utils.py:59-73 bilinear_sampler; fused with convc1 of update.py:76-78). fmap1, fmap2 fp32 channels-last
 * [B][H8*W8][C], C = 256 (corr_bricks_kernel) or 160 (corr_bricks_kernel_k160, the chunk count the network's folded feature head
 * runs; here all 160 channels are caller features), volume = <f1, f2> / sqrt(C); coords [B*H8*W8][2] (x, y) or NULL when no
 * lookup is wanted. Every output is optional
 * (NULL skips it): pyr0..pyr3 = the levels un-bricked to the reference's row-major [B*H8*W8][H_l*W_l]; samples
 * [B*H8*W8][324], channel l*81 + i*9 + j (the FUSED = false instantiation of the sampling code); cor1 [B*H8*W8][256] =
 * relu(convc1(samples)) from the fused instantiation, with convc1's HOST weight [256][324] (torch layout [256,324,1,1])
 * and HOST bias [256]. Synchronises the stream before returning. */
int atdn_corr_lookup_bricks(const float* fmap1, const float* fmap2, int B, int H8, int W8, int C, const float* coords,
                            float* pyr0, float* pyr1, float* pyr2, float* pyr3, float* samples,
                            const float* convc1_weight_host, const float* convc1_bias_host, float* cor1, void* stream);
/* ... with the arithmetic named: fast = 0 is the call above (three f16 MFMAs per product), fast = 1 the plain-f16 builds of
 * the same kernels (precision "f16": the hi x hi product alone) — corr_bricks_kernel<true> / corr_bricks_kernel_k160<true> and
 * lookup_conv_kernel<true, true>. `samples` comes from the sampling-only instantiation in either mode. */
int atdn_corr_lookup_bricks_mode(const float* fmap1, const float* fmap2, int B, int H8, int W8, int C, const float* coords,
                                 float* pyr0, float* pyr1, float* pyr2, float* pyr3, float* samples,
                                 const float* convc1_weight_host, const float* convc1_bias_host, float* cor1, int fast,
                                 void* stream);

/* Generic NHWC convolution through the implicit-GEMM MFMA engine: src [nimg][H][W][Cin] (Cin % 32 == 0 or
 * Cin in {4,16}), HOST weight in torch layout [Cout][Cin][KH][KW] (+ HOST bias or NULL), dst
 * [nimg][Ho][Wo][Cout]; relu != 0 applies ReLU. */
int atdn_conv2d_nhwc(const float* src, int nimg, int H, int W, int Cin, const float* weight_host,
                     const float* bias_host, int Cout, int KH, int KW, int stride, int padH, int padW, int relu,
                     float* dst, void* stream);

/* The same convolution through the split-f16 engine (three f16 MFMAs per product, fp32-grade result):
 * src fp32 NHWC (converted internally to the sf format), Cin % 32 == 0, fp32 NHWC output. */
int atdn_conv2d_nhwc_sf(const float* src, int nimg, int H, int W, int Cin, const float* weight_host,
                        const float* bias_host, int Cout, int KH, int KW, int stride, int padH, int padW, float* dst,
                        void* stream);
/* ... with the epilogue named: sf_store = 0 writes fp32 (what atdn_conv2d_nhwc_sf does), sf_store = 1 writes the split-f16
 * format through the channel-vector store the product's layers use (Cout % 32 == 0) and decodes it to fp32 `dst`.
 * Tests of the 1x5 / 5x1 halo-patch kernels add one of two bits, which change the tiling and never the result: bit 1 (values 2, 3:
 * the epilogue of 0, 1) runs them on the rectangular 8 x 16-pixel x 128-channel tiles, bit 2 (values 4, 5) on the 128-pixel run
 * tiles where the shape allows them (run length >= 43), both whatever the grid size; without them the product's dispatch rules
 * choose, which take small grids to smaller tiles. Other kernel shapes ignore the bits.
 * Bit 3 (value 8, combined with any of the above: 8..13) runs the dispatch as a precision-"f16" forward does: the FAST builds of
 * the same kernels, which issue the hi x hi MFMA alone, i.e. wscale * sum f16(x) * f16(w / wscale) + bias in fp32. The bit is
 * an argument of this call's dispatch: no state outlives the call. Valid values: 0..15 with (sf_store & 6) != 6. */
int atdn_conv2d_nhwc_sf_epi(const float* src, int nimg, int H, int W, int Cin, const float* weight_host,
                            const float* bias_host, int Cout, int KH, int KW, int stride, int padH, int padW, int sf_store,
                            float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ATDN_HIP_H */
