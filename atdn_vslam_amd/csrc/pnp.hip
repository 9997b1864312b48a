// Pose from depth and flow on the device: the reprojection terms of a pose (atdn_pnp_terms) and a Levenberg-Marquardt solve over
// them (atdn_pnp_solve), batched over problems. The rule — float64, every operation rounded on its own — is pnp_pixel,
// plane_lm_update (plane_lm.h), pnp_lm_step and pnp_output of pnp_host.h (over the 6 x 6 algebra of lm6.h), which these kernels call, so the
// kernels and the host form evaluate one function, and the ORDER of every sum is part of the rule (include/atdn_hip.h): the same
// bits on every call and on both paths.
//
// Two launches per evaluation, nothing else on the stream (no memset, no atomics, no host synchronisation; capturable):
//   pnp_terms_kernel     (chunks, B) workgroups of pixel_quads.h with off = 0: workgroup c of plane b owns the flat indices
//                        1024 c .. 1024 c + 1023, a thread four consecutive ones. It streams 13 bytes per pixel (depth, two planes
//                        of flow, mask), keeps the 28 sums of its pixels in 56 VGPRs, reduces them by the fixed binary tree — wave
//                        shuffles for the strides 1 .. 32, LDS for (w0 + w1) + (w2 + w3) — and stores them in ITS slot of the
//                        workspace (store-and-sum: cdna_hip_programming.md, Guideline 12).
//   plane_finalise_kernel<PnpSolver> (plane_sum.h)  one wave per problem: thread e < 28 adds the chunk sums of term e in chunk order (coalesced: the 28
//                        terms of a chunk are contiguous), threads 32 .. 34 the integer counts; thread 0 then either writes the
//                        sums out (atdn_pnp_terms) or takes the Levenberg-Marquardt decision and the next step (the 6 x 6 LDL^T
//                        of lm6.h, fully unrolled, in registers) on the problem's PlaneLmState in the workspace.
// The pose of evaluation 0 is read from the caller's float32 pose by both kernels; later ones from the state.
// The tree, the ordered sum, the workspace, the finalise kernel and the launches of a call (plane_run) are written once, in
// plane_sum.h, for this file and epipolar.hip. The host twins of the two entry points stand below them.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "flow_args.h"
#include "plane_sum.h"
#include "pnp_host.h"

namespace atdn {

// pose32 != nullptr: the public float32 poses [B,12]; otherwise the trial pose of the problem's state
template <bool MASKED>
__global__ __launch_bounds__(PQ_THREADS) void pnp_terms_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                               const unsigned char* __restrict__ mask,
                                                               const float* __restrict__ pose32,
                                                               const PlaneLmState* __restrict__ state, int H, int W, PnpParams cam,
                                                               double* __restrict__ csums, int* __restrict__ ccounts) {
#pragma clang fp contract(off)
  const int n = H * W;
  const int b = blockIdx.y;
  const float* fu = flow + (long)b * 2 * n;
  const float* fv = fu + n;
  const Quad q = quad_of(n, 0);
  double P[12];
  if (pose32) {
    pnp_internal_pose(pose32 + 12 * b, P);
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = state[b].trial[i];
  }
  double acc[PLANE_TERMS];
#pragma unroll
  for (int e = 0; e < PLANE_TERMS; ++e) acc[e] = 0.0;
  float z[4] = {0.0f, 0.0f, 0.0f, 0.0f}, u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool keep[4] = {true, true, true, true};
  if (q.lo < q.hi) {
    quad_load(q, depth + (long)b * n, z);
    quad_load(q, fu, u);
    quad_load(q, fv, v);
    if (MASKED) quad_load(q, mask + (long)b * n, keep);
  }
  int y = q.lo / W, x = q.lo - y * W;                          // of index lo; the quad may cross the end of a row
  int cnt[3] = {0, 0, 0};
  // One pixel at a time (not unrolled: four pixels in flight would take every register of the file and leave one workgroup per
  // CU); the four values of the quad are picked by selects so that the arrays stay in registers.
#pragma nounroll
  for (int k = 0; k < 4; ++k) {
    const float zk = k == 0 ? z[0] : k == 1 ? z[1] : k == 2 ? z[2] : z[3];
    const float uk = k == 0 ? u[0] : k == 1 ? u[1] : k == 2 ? u[2] : u[3];
    const float vk = k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
    const bool kk = k == 0 ? keep[0] : k == 1 ? keep[1] : k == 2 ? keep[2] : keep[3];
    double t[PLANE_TERMS];
    int flags = 0;
    if (q.has(k)) {
      flags = pnp_pixel(zk, uk, vk, kk, P, cam, H, W, x, y, t);
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

static void pnp_launch_terms(const float* depth, const float* flow, const unsigned char* mask, const float* pose32,
                             const PlaneWorkspace& ws, int B, int H, int W, const PnpParams& cam, hipStream_t stream) {
  const dim3 grid((unsigned)plane_chunks(H, W), (unsigned)B);
  if (mask)
    hipLaunchKernelGGL(pnp_terms_kernel<true>, grid, dim3(PQ_THREADS), 0, stream, depth, flow, mask, pose32, ws.state, H, W, cam,
                       ws.sums, ws.counts);
  else
    hipLaunchKernelGGL(pnp_terms_kernel<false>, grid, dim3(PQ_THREADS), 0, stream, depth, flow, mask, pose32, ws.state, H, W, cam,
                       ws.sums, ws.counts);
  ATDN_HIP(hipGetLastError());
}

struct PnpCall {
  const float* depth;
  const float* flow;
  const unsigned char* mask;
  const float* pose;
  int B, H, W;
  double fx, fy, cx, cy, scale_px, inlier_px, min_z;
};

// Argument rules of an entry pair. out[i] of out_bytes[i]: the outputs, none of which may be null or overlap an input or another
// output. The device form (`device`) limits B to gridDim.y before anything else, and its workspace is one more output.
static void pnp_check_args(const PnpCall& c, bool device, const void* const* out, const long* out_bytes, int n_out) {
  if (device) check_plane_batch(c.B, c.H, c.W);
  ATDN_CHECK(c.depth && c.flow && c.pose, "null argument");
  check_plane_solver(c.B, c.H, c.W, device, c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, out, n_out);
  ATDN_CHECK(std::isfinite(c.min_z) && c.min_z > 0.0, "min_z must be finite and > 0");
  const long n = (long)c.H * c.W;
  const void* in[4] = {c.depth, c.flow, c.mask, c.pose};
  const long in_bytes[4] = {(long)c.B * n * 4, (long)c.B * 2 * n * 4, (long)c.B * n, (long)c.B * 48};
  check_disjoint(in, in_bytes, 4, out, out_bytes, n_out);
}

// Both forms of atdn_pnp_terms: the checks and the camera
static PnpParams pnp_terms_args(const PnpCall& c, double* sums, int* counts, bool device, void* workspace) {
  const void* out[3] = {sums, counts, workspace};
  const long out_bytes[3] = {(long)c.B * PLANE_TERMS * 8, (long)c.B * 12, (long)plane_workspace_size(c.B, c.H, c.W)};
  pnp_check_args(c, device, out, out_bytes, device ? 3 : 2);
  return pnp_params(c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, c.min_z, c.H, c.W);
}

// Both forms of atdn_pnp_solve
static PnpParams pnp_solve_args(const PnpCall& c, int iters, float* pose_out, double* cost, int* counts, bool device,
                                void* workspace) {
  const void* out[4] = {pose_out, cost, counts, workspace};
  const long out_bytes[4] = {(long)c.B * 48, (long)c.B * 8, (long)c.B * 16, (long)plane_workspace_size(c.B, c.H, c.W)};
  pnp_check_args(c, device, out, out_bytes, device ? 4 : 3);
  ATDN_CHECK(iters >= 0 && iters <= 64, "iters must be in [0, 64]");
  return pnp_params(c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, c.min_z, c.H, c.W);
}

// the launches of a call: plane_run (plane_sum.h) over pnp_launch_terms
static void pnp_run(const PnpCall& c, const PnpParams& cam, int iters, double* sums, int* counts, float* pose_out, double* cost,
                    void* workspace, void* stream) {
  plane_run<PnpSolver>([&](const float* pose32, const PlaneWorkspace& ws) {
    pnp_launch_terms(c.depth, c.flow, c.mask, pose32, ws, c.B, c.H, c.W, cam, (hipStream_t)stream);
  }, workspace, c.B, c.H, c.W, iters, c.pose, sums, counts, pose_out, cost, (hipStream_t)stream);
}

}  // namespace atdn

using namespace atdn;

long atdn_pnp_workspace_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long)H * W > (1L << 24)) return 0;
  return (long)plane_workspace_size(B, H, W);
}

int atdn_pnp_terms(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                   double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, double* sums,
                   int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const PnpCall c{depth, flow, mask, pose, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, min_z};
  const PnpParams cam = pnp_terms_args(c, sums, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "workspace and sums must be 8-byte aligned");
  pnp_run(c, cam, -1, sums, counts, nullptr, nullptr, workspace, stream);
  ATDN_API_END
}

int atdn_pnp_terms_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                        double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, double* sums,
                        int* counts) {
  ATDN_API_BEGIN
  const PnpCall c{depth, flow, mask, pose, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, min_z};
  const PnpParams cam = pnp_terms_args(c, sums, counts, false, nullptr);
  pnp_terms_host(depth, flow, mask, pose, B, H, W, cam, sums, counts);
  ATDN_API_END
}

int atdn_pnp_solve(const float* depth, const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W,
                   double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, int iters,
                   float* pose_out, double* cost, int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const PnpCall c{depth, flow, mask, pose_init, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, min_z};
  const PnpParams cam = pnp_solve_args(c, iters, pose_out, cost, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)cost & 7) == 0, "workspace and cost must be 8-byte aligned");
  pnp_run(c, cam, iters, nullptr, counts, pose_out, cost, workspace, stream);
  ATDN_API_END
}

int atdn_pnp_solve_host(const float* depth, const float* flow, const unsigned char* mask, const float* pose_init, int B, int H,
                        int W, double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, int iters,
                        float* pose_out, double* cost, int* counts) {
  ATDN_API_BEGIN
  const PnpCall c{depth, flow, mask, pose_init, B, H, W, fx, fy, cx, cy, scale_px, inlier_px, min_z};
  const PnpParams cam = pnp_solve_args(c, iters, pose_out, cost, counts, false, nullptr);
  pnp_solve_host(depth, flow, mask, pose_init, B, H, W, cam, iters, pose_out, cost, counts);
  ATDN_API_END
}
