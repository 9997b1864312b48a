// Keyframe depth fusion on the device: the geometric-consistency filter of multi-view stereo over the depth bank of the keyframe
// map. For target i = targets[b], fused[b, 0, y, x] = the depth of pixel (x, y) of bank[i] where at least min_views of the sources
// sources[b][.] hold the same surface there (optionally averaged with their estimates), 0 elsewhere; views[b, y, x] = the number
// of agreeing sources; counts[b] = (pixels with a depth, pixels some source saw, pixels kept). The rule — float64, every operation
// rounded on its own — is depth_fuse_relative / depth_fuse_source / depth_fuse_result of depth_fusion_host.h, which this kernel
// calls, so the kernel and the host form evaluate one set of functions. One memset node and one launch on the caller's stream:
// asynchronous, capturable, no host synchronisation, no workspace; targets, sources and poses are read from device memory. Gather
// only: no atomics on the data; the counts are integer sums (pixel_quads.h), the same bits on every call.
//
// Decomposition. Per target pixel 4 bytes in, 5 out, and per source four taps of 4 bytes that neighbouring pixels share (they land
// on neighbouring source pixels: local gathers out of L2) and ~78 float64 operations with seven divisions: arithmetic, not traffic.
// The frame is pixel_quads.h: a thread owns four consecutive flat indices; the views plane anchors the quads (one aligned dword
// per whole quad), fused goes through quad_store, the target depth through quad_load. The sources are a runtime loop in chunks of
// DF_CHUNK: the first DF_CHUNK threads of the workgroup compose one relative pose each (depth_fuse_relative, the host's function)
// into LDS, 12 float64 per source, and every thread then reads them as broadcasts — the poses are wave-uniform, and composing them
// per thread would repeat ~60 float64 operations per source in every thread for the same registers.
#include "../../include/atdn_hip.h"

#include <cmath>
#include <cstdint>

#include "depth_fusion_host.h"
#include "flow_args.h"
#include "pixel_quads.h"

namespace atdn {

constexpr int DF_CHUNK = 16;   // sources per pass through LDS

__global__ __launch_bounds__(PQ_THREADS) void depth_fuse_kernel(const float* __restrict__ bank, const float* __restrict__ poses,
                                                                const int* __restrict__ targets, const int* __restrict__ sources,
                                                                int N, int S, int H, int W, DepthFuseParams c,
                                                                float* __restrict__ fused, unsigned char* __restrict__ views,
                                                                int* __restrict__ counts) {
  __shared__ double rel[DF_CHUNK][DF_REL];
  __shared__ int src[DF_CHUNK];
  const int n = H * W;
  const int b = blockIdx.y;
  float* f = fused + (long)b * n;
  unsigned char* vw = views + (long)b * n;
  const Quad q = quad_of(n, (int)((uintptr_t)vw & 3));
  const int i = targets[b];
  const bool target_ok = i >= 0 && i < N;                      // the same for the whole workgroup
  float zf[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (target_ok) quad_load(q, bank + (long)i * n, zf);
  double X[4][3], zsum[4];
  int cnt[4] = {0, 0, 0, 0}, px[4], py[4];
  bool seen[4] = {false, false, false, false};
  {
    int y = q.lo / W, x = q.lo - y * W;                        // of index lo; the quad may cross the end of a row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      px[k] = x; py[k] = y;
      zsum[k] = (double)zf[k];
      depth_fuse_point((double)zf[k], x, y, c, X[k]);
      if (q.has(k)) {
        if (++x == W) { x = 0; ++y; }
      }
    }
  }
  if (target_ok) {
    for (int s0 = 0; s0 < S; s0 += DF_CHUNK) {
      const int m = S - s0 < DF_CHUNK ? S - s0 : DF_CHUNK;
      if (s0) __syncthreads();                                 // the previous chunk has been read
      if ((int)threadIdx.x < m) {
        const int j = sources[(long)b * S + s0 + threadIdx.x];
        const bool use = j >= 0 && j < N && j != i;
        src[threadIdx.x] = use ? j : -1;
        if (use) depth_fuse_relative(poses + 12L * i, poses + 12L * j, rel[threadIdx.x]);
      }
      __syncthreads();
      for (int s = 0; s < m; ++s) {
        const int j = src[s];
        if (j < 0) continue;
        const float* plane = bank + (long)j * n;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (zf[k] > 0.0f) {                                  // zero outside the quad's part of the plane
            bool ok;
            double zt;
            if (depth_fuse_source(rel[s], plane, X[k], (double)zf[k], px[k], py[k], c, H, W, &ok, &zt)) {
              ++cnt[k];
              zsum[k] = zsum[k] + zt;
            }
            seen[k] = seen[k] || ok;
          }
        }
      }
    }
  }
  int flags[4];
  float out[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = depth_fuse_result(zf[k], cnt[k], zsum[k], seen[k], c, &flags[k]);
  if (q.lo < q.hi) {
    quad_store(q, f, out);
    quad_store_bytes(q, vw, cnt);
  }
  const int bits[3] = {DF_HAS, DF_SEEN, DF_KEPT};
  quad_count<3>(flags, bits, counts + 3 * b);
}

// Argument rules shared by the two entry points below (sources may be null only when S == 0), and the parameters of the call.
static DepthFuseParams depth_fuse_check_args(const float* bank, const float* poses, const int* targets, const int* sources, int N,
                                             int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                                             double max_reproj, double max_rel_depth, int min_views, double min_z, int average,
                                             const float* fused, const unsigned char* views, const int* counts) {
  ATDN_CHECK(bank && poses && targets && fused && views && counts && (sources || S == 0), "null argument");
  check_plane_batch(B, H, W);
  check_pinhole(fx, fy, cx, cy);
  ATDN_CHECK(N >= 1, "the bank is empty (N >= 1)");
  ATDN_CHECK(S >= 0 && S <= 255, "S must be in [0, 255]");
  ATDN_CHECK(min_views >= 1 && min_views <= 255, "min_views must be in [1, 255]");
  ATDN_CHECK(std::isfinite(max_reproj) && max_reproj > 0.0, "max_reproj must be finite and > 0");
  ATDN_CHECK(std::isfinite(max_rel_depth) && max_rel_depth > 0.0, "max_rel_depth must be finite and > 0");
  ATDN_CHECK(std::isfinite(min_z) && min_z > 0.0, "min_z must be finite and > 0");
  const long n = (long)H * W;
  const void* in[4] = {bank, poses, targets, S > 0 ? sources : nullptr};
  const long in_bytes[4] = {(long)N * n * 4, (long)N * 48, (long)B * 4, (long)B * S * 4};
  const void* out[3] = {fused, views, counts};
  const long out_bytes[3] = {(long)B * n * 4, (long)B * n, (long)B * 12};
  check_disjoint(in, in_bytes, 4, out, out_bytes, 3);
  return depth_fuse_params(fx, fy, cx, cy, max_reproj, max_rel_depth, min_views, min_z, average);
}

}  // namespace atdn

using namespace atdn;

int atdn_depth_fuse(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S, int H, int W,
                    double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth, int min_views, double min_z,
                    int average, float* fused, unsigned char* views, int* counts, void* stream) {
  ATDN_API_BEGIN
  const DepthFuseParams c = depth_fuse_check_args(bank, poses, targets, sources, N, B, S, H, W, fx, fy, cx, cy, max_reproj,
                                                  max_rel_depth, min_views, min_z, average, fused, views, counts);
  ATDN_HIP(hipMemsetAsync(counts, 0, (size_t)B * 12, (hipStream_t)stream));
  hipLaunchKernelGGL(depth_fuse_kernel, dim3(quad_blocks((long)H * W, true), (unsigned)B), dim3(PQ_THREADS), 0, (hipStream_t)stream,
                     bank, poses, targets, sources, N, S, H, W, c, fused, views, counts);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

int atdn_depth_fuse_host(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S, int H,
                         int W, double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth, int min_views,
                         double min_z, int average, float* fused, unsigned char* views, int* counts) {
  ATDN_API_BEGIN
  const DepthFuseParams c = depth_fuse_check_args(bank, poses, targets, sources, N, B, S, H, W, fx, fy, cx, cy, max_reproj,
                                                  max_rel_depth, min_views, min_z, average, fused, views, counts);
  depth_fuse_host(bank, poses, targets, sources, N, B, S, H, W, c, fused, views, counts);
  ATDN_API_END
}
