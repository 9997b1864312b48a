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
//   plane_finalise_kernel<EpipolarSolver> (plane_sum.h)  one wave per problem: the ordered sum of plane_sum.h; thread 0 then either writes the sums out
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

struct EpipolarCall {
  const float* flow;
  const unsigned char* mask;
  const float* pose;
  int B, H, W;
  double fx, fy, cx, cy, scale_px, inlier_px;
};

// Argument rules of an entry pair. out[i] of out_bytes[i]: the outputs, none of which may be null or overlap an input or another
// output. The device form (`device`) limits B to gridDim.y before anything else, and its workspace is one more output.
static void epipolar_check_args(const EpipolarCall& c, bool device, const void* const* out, const long* out_bytes, int n_out) {
  if (device) check_plane_batch(c.B, c.H, c.W);
  ATDN_CHECK(c.flow && c.pose, "null argument");
  check_plane_solver(c.B, c.H, c.W, device, c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px, out, n_out);
  const long n = (long)c.H * c.W;
  const void* in[3] = {c.flow, c.mask, c.pose};
  const long in_bytes[3] = {(long)c.B * 2 * n * 4, (long)c.B * n, (long)c.B * 48};
  check_disjoint(in, in_bytes, 3, out, out_bytes, n_out);
}

// Both forms of atdn_epipolar_terms: the checks and the camera
static EpipolarParams epipolar_terms_args(const EpipolarCall& c, double* sums, int* counts, bool device, void* workspace) {
  const void* out[3] = {sums, counts, workspace};
  const long out_bytes[3] = {(long)c.B * PLANE_TERMS * 8, (long)c.B * 12, (long)plane_workspace_size(c.B, c.H, c.W)};
  epipolar_check_args(c, device, out, out_bytes, device ? 3 : 2);
  return epipolar_params(c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px);
}

// Both forms of atdn_epipolar_solve
static EpipolarParams epipolar_solve_args(const EpipolarCall& c, int iters, float* pose_out, double* cost, int* counts, bool device,
                                          void* workspace) {
  const void* out[4] = {pose_out, cost, counts, workspace};
  const long out_bytes[4] = {(long)c.B * 48, (long)c.B * 8, (long)c.B * 16, (long)plane_workspace_size(c.B, c.H, c.W)};
  epipolar_check_args(c, device, out, out_bytes, device ? 4 : 3);
  ATDN_CHECK(iters >= 0 && iters <= 64, "iters must be in [0, 64]");
  return epipolar_params(c.fx, c.fy, c.cx, c.cy, c.scale_px, c.inlier_px);
}

// the launches of a call: plane_run (plane_sum.h) over epipolar_launch_terms
static void epipolar_run(const EpipolarCall& c, const EpipolarParams& cam, int iters, double* sums, int* counts, float* pose_out,
                         double* cost, void* workspace, void* stream) {
  plane_run<EpipolarSolver>([&](const float* pose32, const PlaneWorkspace& ws) {
    epipolar_launch_terms(c.flow, c.mask, pose32, ws, c.B, c.H, c.W, cam, (hipStream_t)stream);
  }, workspace, c.B, c.H, c.W, iters, c.pose, sums, counts, pose_out, cost, (hipStream_t)stream);
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
  const EpipolarCall c{flow, mask, pose, B, H, W, fx, fy, cx, cy, scale_px, inlier_px};
  const EpipolarParams cam = epipolar_terms_args(c, sums, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "workspace and sums must be 8-byte aligned");
  epipolar_run(c, cam, -1, sums, counts, nullptr, nullptr, workspace, stream);
  ATDN_API_END
}

int atdn_epipolar_terms_host(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double scale_px, double inlier_px, double* sums, int* counts) {
  ATDN_API_BEGIN
  const EpipolarCall c{flow, mask, pose, B, H, W, fx, fy, cx, cy, scale_px, inlier_px};
  const EpipolarParams cam = epipolar_terms_args(c, sums, counts, false, nullptr);
  epipolar_terms_host(flow, mask, pose, B, H, W, cam, sums, counts);
  ATDN_API_END
}

int atdn_epipolar_solve(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W, double fx,
                        double fy, double cx, double cy, double scale_px, double inlier_px, int iters, float* pose_out, double* cost,
                        int* counts, void* workspace, void* stream) {
  ATDN_API_BEGIN
  const EpipolarCall c{flow, mask, pose_init, B, H, W, fx, fy, cx, cy, scale_px, inlier_px};
  const EpipolarParams cam = epipolar_solve_args(c, iters, pose_out, cost, counts, true, workspace);
  ATDN_CHECK(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)cost & 7) == 0, "workspace and cost must be 8-byte aligned");
  epipolar_run(c, cam, iters, nullptr, counts, pose_out, cost, workspace, stream);
  ATDN_API_END
}

int atdn_epipolar_solve_host(const float* flow, const unsigned char* mask, const float* pose_init, int B, int H, int W, double fx,
                             double fy, double cx, double cy, double scale_px, double inlier_px, int iters, float* pose_out,
                             double* cost, int* counts) {
  ATDN_API_BEGIN
  const EpipolarCall c{flow, mask, pose_init, B, H, W, fx, fy, cx, cy, scale_px, inlier_px};
  const EpipolarParams cam = epipolar_solve_args(c, iters, pose_out, cost, counts, false, nullptr);
  epipolar_solve_host(flow, mask, pose_init, B, H, W, cam, iters, pose_out, cost, counts);
  ATDN_API_END
}
