// Warm start of the flow network on video: the previous pair's 1/8-resolution flow pushed forward along itself, to be the
// next pair's flow_init — the GMA wheel's forward_interpolate (whl:GMA/core/utils/utils.py:28-56, used by its evaluate.py),
// which goes to the host and calls scipy.interpolate.griddata(method='nearest') twice. Here it is one launch on the caller's
// stream: asynchronous, capturable, no atomics, no workspace, the same bits on every call.
//
// Rules (warm_start_host.h states them in full and is the float64 host form): source i = y * w + x sits at
// (x + dx_i, y + dy_i) in float64 and is valid when 0 < x1 < w and 0 < y1 < h (strict); every grid point takes the flow of its
// nearest valid source, distance (qx - x1)^2 + (qy - y1)^2 in float64 with every operation rounded on its own (fp contraction
// off: on random flows the best and second-best distance come as close as 3e-6 at 47 x 154, about 20 roundings of fp32), ties
// to the lowest index; no valid source at all gives zeros, where the wheel raises on its empty point set.
//
// Decomposition. Queries alone would be 29 workgroups of 256 at the KITTI grid (47 x 154 = 7238 points) on 256 CUs, so the
// source axis is split too, inside the workgroup: a workgroup of 1024 threads owns QPB = 32 queries, and its 32 x 32 threads are
// (query, source class): thread (q, t) sees the sources j = t (mod 32). That is ceil(7238 / 32) = 227 workgroups of 16 waves
// for one flow. Sources pass through LDS in chunks of CHUNK as (x1, y1) float64, an invalid one as x1 = +inf (its distance
// is +inf and never smaller than anything; nothing is compacted); the two halves of a wave read two LDS addresses per step
// (broadcast reads). Every thread keeps (distance, index) of its best source; the 32 partial results of a query are then reduced
// by the key (distance, index), so the lowest-index rule survives the split.
#include "../../include/atdn_hip.h"

#include <climits>

#include "common.h"
#include "warm_start_host.h"

namespace atdn {

constexpr int WS_QPB = 32;      // queries per workgroup
constexpr int WS_SPLIT = 32;    // source classes per query (threads = WS_QPB * WS_SPLIT)
constexpr int WS_CHUNK = 2048;  // sources staged per pass: 32 KiB of LDS

__global__ __launch_bounds__(WS_QPB* WS_SPLIT) void forward_interpolate_kernel(const float* __restrict__ flow, int h, int w,
                                                                                float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double2 src[WS_CHUNK];
  __shared__ double red_d[WS_SPLIT][WS_QPB];
  __shared__ int red_j[WS_SPLIT][WS_QPB];
  const int n = h * w;
  const float* fx = flow + (long)blockIdx.y * 2 * n;
  const float* fy = fx + n;
  const int tid = threadIdx.x;
  const int ql = tid & (WS_QPB - 1);   // lanes 0..31 and 32..63 of a wave hold the same 32 queries,
  const int t = tid >> 5;              // with two neighbouring source classes
  const int q = blockIdx.x * WS_QPB + ql;
  const int qc = q < n ? q : n - 1;    // (threads past the end work on the last query and write nothing)
  const double qx = (double)(qc % w), qy = (double)(qc / w);
  const double inf = __longlong_as_double(0x7FF0000000000000LL);
  double best = inf;
  int bj = INT_MAX;
  for (int c0 = 0; c0 < n; c0 += WS_CHUNK) {
    const int cnt = min(WS_CHUNK, n - c0);
    __syncthreads();   // the previous chunk has been read by everybody
    for (int k = tid; k < cnt; k += WS_QPB * WS_SPLIT) {
      const int j = c0 + k;
      const double x1 = (double)(j % w) + (double)fx[j], y1 = (double)(j / w) + (double)fy[j];
      const bool valid = x1 > 0.0 && x1 < (double)w && y1 > 0.0 && y1 < (double)h;
      src[k] = make_double2(valid ? x1 : inf, valid ? y1 : 0.0);
    }
    __syncthreads();
    for (int k = t; k < cnt; k += WS_SPLIT) {
      const double2 s = src[k];
      const double ex = qx - s.x, ey = qy - s.y;
      const double xx = ex * ex, yy = ey * ey;
      const double d = xx + yy;
      if (d < best) { best = d; bj = c0 + k; }   // strict, and k rises: the lowest index of this class keeps an equal distance
    }
  }
  red_d[t][ql] = best;
  red_j[t][ql] = bj;
  __syncthreads();
  if (t == 0 && q < n) {
    for (int s = 1; s < WS_SPLIT; ++s) {
      const double d = red_d[s][ql];
      const int j = red_j[s][ql];
      if (d < best || (d == best && j < bj)) { best = d; bj = j; }
    }
    float* ox = out + (long)blockIdx.y * 2 * n;
    const bool found = bj != INT_MAX;    // (an all-invalid class keeps INT_MAX at distance +inf)
    ox[q] = found ? fx[bj] : 0.0f;
    ox[n + q] = found ? fy[bj] : 0.0f;
  }
}

}  // namespace atdn

using namespace atdn;

int atdn_flow_forward_interpolate(const float* flow_low, int B, int h, int w, float* out, void* stream) {
  ATDN_API_BEGIN
  ATDN_CHECK(flow_low && out, "null argument");
  ATDN_CHECK(B >= 1 && B <= 65535 && h >= 1 && w >= 1, "bad batch or grid size");
  ATDN_CHECK((long)h * w <= (1L << 24), "grid too large (h * w <= 2^24)");
  const long n = (long)h * w;
  ATDN_CHECK(disjoint(flow_low, (long)B * 2 * n * 4, out, (long)B * 2 * n * 4), "input and output overlap");
  hipLaunchKernelGGL(forward_interpolate_kernel, dim3((unsigned)cdivl(n, WS_QPB), (unsigned)B), dim3(WS_QPB * WS_SPLIT), 0,
                     (hipStream_t)stream, flow_low, h, w, out);
  ATDN_HIP(hipGetLastError());
  ATDN_API_END
}

// (the host form has always worded its size rules as one)
int atdn_flow_forward_interpolate_host(const float* flow_low, int B, int h, int w, float* out) {
  ATDN_API_BEGIN
  ATDN_CHECK(flow_low && out, "null argument");
  ATDN_CHECK(B >= 1 && h >= 1 && w >= 1 && (long)h * w <= (1L << 24), "bad batch or grid size");
  const long bytes = (long)B * 2 * h * w * 4;
  ATDN_CHECK(disjoint(flow_low, bytes, out, bytes), "input and output overlap");
  forward_interpolate_host(flow_low, B, h, w, out);
  ATDN_API_END
}
