// Pose from flow alone on the device: the epipolar terms of a pose (atdn_epipolar_terms) and a Levenberg-Marquardt solve over
// them (atdn_epipolar_solve), batched over problems. The rule — float64, every operation rounded on its own — is epipolar_pixel,
// epipolar_lm_step and epipolar_output of epipolar_host.h (over plane_lm.h and the 6 x 6 algebra of lm6.h), which these kernels
// call, so the kernels and the host form evaluate one function, and the ORDER of every sum is part of the rule
// (include/atdn_hip.h): the same bits on every call and on both paths.
//
// Two launches per evaluation, nothing else on the stream (no memset, no atomics, no host synchronisation; capturable), the
// shape of pnp.hip:
//   epipolar_terms_kernel     (chunks, B) workgroups of pixel_quads.h with off = 0. A thread streams 9 bytes per pixel (two planes
//                             of flow, mask), keeps the 28 sums of its four pixels in 56 VGPRs and hands them to the fixed tree
//                             of plane_sum.h, which stores the workgroup's sums in ITS slot of the workspace.
//   epipolar_finalise_kernel  one wave per problem: the ordered sum of plane_sum.h; thread 0 then either writes the sums out
//                             (atdn_epipolar_terms) or takes the Levenberg-Marquardt decision and the next step (gauge term,
//                             6 x 6 LDL^T, two Cayley matrices, in registers) on the problem's state in the workspace.
// The pose of evaluation 0 is read from the caller's float32 pose by both kernels; later ones from the state.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "epipolar_host.h"
#include "flow_args.h"
#include "plane_sum.h"

namespace atdn {

// pose32 != nullptr: the public float32 poses [B,12]; otherwise the trial pose of the problem's state
template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void epipolar_terms_kernel(const float* __restrict__ flow,
                                                                    const unsigned char* __restrict__ mask,
                                                                    const float* __restrict__ pose32,
                                                                    const PlaneLmState* __restrict__ state, int H, int W,
                                                                    EpipolarParams cam, double* __restrict__ csums,
                                                                    int* __restrict__ ccounts) {
#pragma clang fp contract(off)
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fu = flow + (long)b * 2 * n;
  const float* fv = fu + n;
  const Quad q = quad_of(n, 0);
  double p[12];
  if (pose32) {
    epipolar_load_pose(pose32 + 12 * b, p);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = state[b].trial[i];
  }
  const TwoViewPose P = epipolar_pose(p);
  double acc[PLANE_TERMS];
#pragma unroll
  for (int e = 0; e < PLANE_TERMS; ++e) acc[e] = 0.0;
  float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool keep[4] = {true, true, true, true};
  if (q.lo < q.hi) {
    quad_load(q, fu, u);
    quad_load(q, fv, v);
    if (MASKED) quad_load(q, mask + (long)b * n, keep);
  }
  int y = q.lo / W, x = q.lo - y * W;                          // of index lo; the quad may cross the end of a row
  int cnt[3] = {0, 0, 0};
  // One pixel at a time, as in pnp_terms_kernel: four pixels in flight would take every register of the file.
#pragma nounroll
  for (int k = 0; k < 4; ++k) {
    const float uk = k == 0 ? u[0] : k == 1 ? u[1] : k == 2 ? u[2] : u[3];
    const float vk = k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
    const bool kk = k == 0 ? keep[0] : k == 1 ? keep[1] : k == 2 ? keep[2] : keep[3];
    double t[PLANE_TERMS];
    int flags = 0;
    if (q.has(k)) {
      flags = epipolar_pixel(uk, vk, kk, P, cam, H, W, x, y, t);
      if (++x == W) { x = 0; ++y; }
    } else {
#pragma unroll
      for (int e = 0; e < PLANE_TERMS; ++e) t[e] = 0.0;
    }
#pragma unroll
    for (int e = 0; e < PLANE_TERMS; ++e) acc[e] = k == 0 ? t[e] : acc[e] + t[e];   // ((t0 + t1) + t2) + t3
#pragma unroll
    for (int j = 0; j < 3; ++j) cnt[j] += __popcll(__ballot(flags & (1 << j)));   // the wave's count, in every lane
  }
  plane_chunk_reduce(acc, cnt, b, csums, ccounts);
}

// k < 0: atdn_epipolar_terms (the plane sums go to sums_out / counts_out). k >= 0: evaluation k of a solve of `iters` steps.
__global__ __launch_bounds__(PLANE_FIN_THREADS) void epipolar_finalise_kernel(const double* __restrict__ csums,
                                                                               const int* __restrict__ ccounts, int chunks, int k,
                                                                               int iters, PlaneLmState* __restrict__ state,
                                                                               const float* __restrict__ pose_init,
                                                                               double* __restrict__ sums_out,
                                                                               int* __restrict__ counts_out,
                                                                               float* __restrict__ pose_out,
                                                                               double* __restrict__ cost_out) {
#pragma clang fp contract(off)
  __shared__ double S[PLANE_TERMS];
  __shared__ int Cn[3];
  const int b = blockIdx.x;
  const int t = threadIdx.x;
  plane_ordered_sum(csums, ccounts, chunks, b, S, Cn);
  if (k < 0) {
    if (t < PLANE_TERMS) sums_out[(long)b * PLANE_TERMS + t] = S[t];
    if (t < 3) counts_out[3 * b + t] = Cn[t];
    return;
  }
  if (t != 0) return;
  PlaneLmState& s = state[b];
  if (k == 0) epipolar_load_pose(pose_init + 12 * b, s.trial);
  plane_lm_update(s, S, Cn, k);
  if (k < iters)
    epipolar_lm_step(s);
  else
    epipolar_output(s, pose_init + 12 * b, pose_out + 12 * b, cost_out + b, counts_out + 4 * b);
}

static void epipolar_launch_terms(const float* flow, const unsigned char* mask, const float* pose32, const PlaneWorkspace& ws, int B,
                                  int H, int W, const EpipolarParams& cam, hipStream_t stream) {
  const dim3 grid((unsigned)plane_chunks(H, W), (unsigned)B);
  if (mask)
    hipLaunchKernelGGL(epipolar_terms_kernel<true>, grid, dim3(PQ_THREADS), 0, stream, flow, mask, pose32, ws.state, H, W, cam,
                       ws.sums, ws.counts);
  else
    hipLaunchKernelGGL(epipolar_terms_kernel<false>, grid, dim3(PQ_THREADS), 0, stream, flow, mask, pose32, ws.state, H, W, cam,
                       ws.sums, ws.counts);
  ATDN_HIP(hipGetLastError());
}

// Argument rules shared by the device entry points below and the host ones (capi.hip). out[i] of out_bytes[i]: the outputs
// (a workspace among them), none of which may overlap an input or another output.
void epipolar_check_args(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx, double fy,
                         double cx, double cy, double scale_px, double inlier_px, bool grid_limit, const void* const* out,
                         const long* out_bytes, int n_out) {
  ATDN_CHECK(flow && pose, "null argument");
  check_plane_solver(B, H, W, grid_limit, fx, fy, cx, cy, scale_px, inlier_px, out, n_out);
  const long n = (long)H * W;
  const void* in[3] = {flow, mask, pose};
  const long in_bytes[3] = {(long)B * 2 * n * 4, (long)B * n, (long)B * 48};
  check_disjoint(in, in_bytes, 3, out, out_bytes, n_out);
}

}  // namespace atdn

using namespace atdn;

long atdn_epipolar_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long)H * W > (1L << 24)) return 0;
  return (long)plane_workspace_size(B, H, W);
}

int atdn_epipolar_terms(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx, double fy,
                        double cx, double cy, double scale_px, double inlier_px, double* sums, int* counts, void* workspace,
                        void* stream) {
  ATDN_API_BEGIN
  check_plane_batch(B, H, W);
  const void* out[3] = {sums, counts, workspace};
  const long out_bytes[3] = {(long)B * PLANE_TERMS * 8, (long)B * 12, (long)plane_workspace_size(B, H, W)};
  epipolar_check_args(flow, mask, pose, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, true, out, out_bytes, 3);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "workspace and sums must be 8-byte aligned");
  const EpipolarParams cam = epipolar_params(fx, fy, cx, cy, scale_px, inlier_px);
  const PlaneWorkspace ws = plane_carve(workspace, B, H, W);
  epipolar_launch_terms(flow, mask, pose, ws, B, H, W, cam, (hipStream_t)stream);
  hipLaunchKernelGGL(epipolar_finalise_kernel, dim3((unsigned)B), dim3(PLANE_FIN_THREADS), 0, (hipStream_t)stream, ws.sums,
                     ws.counts, (int)plane_chunks(H, W), -1, 0, ws.state, pose, sums, counts, (float*)nullptr, (double*)nullptr);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_epipolar_solve(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W, double fx,
                        double fy, double cx, double cy, double scale_px, double inlier_px, int iters, float* pose_out, double* cost,
                        int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  check_plane_batch(B, H, W);
  const void* out[4] = {pose_out, cost, counts, workspace};
  const long out_bytes[4] = {(long)B * 48, (long)B * 8, (long)B * 16, (long)plane_workspace_size(B, H, W)};
  epipolar_check_args(flow, mask, pose_init, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, true, out, out_bytes, 4);
  ATDN_CHECK(iters >= 0 && iters <= 64, "iters must be in [0, 64]");
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)cost & 7) == 0, "workspace and cost must be 8-byte aligned");
  const EpipolarParams cam = epipolar_params(fx, fy, cx, cy, scale_px, inlier_px);
  const PlaneWorkspace ws = plane_carve(workspace, B, H, W);
  for (int k = 0; k <= iters; ++k) {
    epipolar_launch_terms(flow, mask, k == 0 ? pose_init : nullptr, ws, B, H, W, cam, (hipStream_t)stream);
    hipLaunchKernelGGL(epipolar_finalise_kernel, dim3((unsigned)B), dim3(PLANE_FIN_THREADS), 0, (hipStream_t)stream, ws.sums,
                       ws.counts, (int)plane_chunks(H, W), k, iters, ws.state, pose_init, (double*)nullptr, counts, pose_out, cost);
    ATDN_HIP(hipGetLastError());
  }
  ATDN_API_END
}
