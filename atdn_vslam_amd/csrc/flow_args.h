// Argument rules of the flow-geometry entry points (flow_consistency.hip, two_view.hip, flow_track.hip, pnp.hip, epipolar.hip, depth_fusion.hip, multiview_depth.hip, bundle.hip, ground.hip, voxel_map.hip), shared by each device
// entry point and its host twin in capi.hip, and the overlap rule that the pose solvers (pnp.hip, pose_graph.hip) share.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"
#include "two_view_host.h"

namespace atdn {

// [B, ., H, W] planes walked by pixel_quads.h: B is gridDim.y, and a flat index of a plane times four fits an int. The host forms
// of flow_consistency and two_view have never had the gridDim.y limit (grid_limit = false); their device entry points check it.
inline void check_plane_batch(int B, int H, int W, bool grid_limit = true) {
  ATDN_CHECK(B >= 1 && H >= 1 && W >= 1, "bad batch or image size");
  if (grid_limit) ATDN_CHECK(B <= 65535, "batch too large (B <= 65535)");
  ATDN_CHECK((long)H * W <= (1L << 24), "image too large (H * W <= 2^24)");
}

// in[k] of in_bytes[k] (null: not given), out[i] of out_bytes[i]: no output may overlap an input or another output
inline void check_disjoint(const void* const* in, const long* in_bytes, int n_in, const void* const* out, const long* out_bytes,
                           int n_out) {
  for (int i = 0; i < n_out; ++i) {
    for (int k = 0; k < n_in; ++k)
      if (in[k]) ATDN_CHECK(disjoint(in[k], in_bytes[k], out[i], out_bytes[i]), "an output overlaps an input");
    for (int j = 0; j < i; ++j) ATDN_CHECK(disjoint(out[j], out_bytes[j], out[i], out_bytes[i]), "two outputs overlap");
  }
}

inline void check_pinhole(double fx, double fy, double cx, double cy) {
  ATDN_CHECK(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0 && fy > 0.0, "fx and fy must be finite and > 0");
  ATDN_CHECK(std::isfinite(cx) && std::isfinite(cy), "cx and cy must be finite");
}

// What the argument rules of the dense pose solvers (pnp.hip, epipolar.hip) share: no null output, the plane batch, the pinhole,
// the two pixel scales of the robust loss.
inline void check_plane_solver(int B, int H, int W, bool grid_limit, double fx, double fy, double cx, double cy, double scale_px,
                               double inlier_px, const void* const* out, int n_out) {
  for (int i = 0; i < n_out; ++i) ATDN_CHECK(out[i], "null argument");
  check_plane_batch(B, H, W, grid_limit);
  check_pinhole(fx, fy, cx, cy);
  ATDN_CHECK(std::isfinite(scale_px) && scale_px > 0.0, "scale_px must be finite and > 0");
  ATDN_CHECK(std::isfinite(inlier_px) && inlier_px > 0.0, "inlier_px must be finite and > 0");
}

inline void check_two_view_camera(const TwoViewCamera& cam) {
  check_pinhole(cam.fx, cam.fy, cam.cx, cam.cy);
  ATDN_CHECK(std::isfinite(cam.max_epipolar) && cam.max_epipolar >= 0.0, "max_epipolar must be finite and >= 0");
  ATDN_CHECK(std::isfinite(cam.min_sin2) && cam.min_sin2 >= 0.0, "min_sin2 must be finite and >= 0");
  ATDN_CHECK(std::isfinite(cam.max_depth) && cam.max_depth > 0.0, "max_depth must be finite and > 0");
}

void flow_consistency_check_args(const float* flow_fw, const float* flow_bw, int B, int H, int W, double alpha1, double alpha2,
                                 const unsigned char* mask, const int* count);
void two_view_check_args(const float* flow, const float* pose, const unsigned char* mask, int B, int H, int W,
                         const TwoViewCamera& cam, const float* depth, const int* counts);
void flow_track_check_args(const float* flow, const unsigned char* mask, const float* acc_in, const unsigned char* alive_in, int B,
                           int H, int W, const float* acc_out, const unsigned char* alive_out, const float* pose,
                           const TwoViewCamera& cam, const float* depth, const int* counts);
// out[i] of out_bytes[i], i < n_out: the outputs (a workspace among them); none may be null or overlap an input or another output
void pnp_check_args(const float* depth, const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W,
                    double fx, double fy, double cx, double cy, double scale_px, double inlier_px, double min_z, bool grid_limit,
                    const void* const* out, const long* out_bytes, int n_out);
void epipolar_check_args(const float* flow, const unsigned char* mask, const float* pose, int B, int H, int W, double fx, double fy,
                         double cx, double cy, double scale_px, double inlier_px, bool grid_limit, const void* const* out,
                         const long* out_bytes, int n_out);
// the ground plane (ground.hip): mask may be null, q only where q_optional; out as for pnp_check_args
void ground_check_args(const float* depth, const unsigned char* mask, const double* q, bool q_optional, int B, int H, int W, int y0,
                       int y1, double fx, double fy, double cx, double cy, double scale_rel, double inlier_rel, double min_z,
                       double max_depth, bool grid_limit, const void* const* out, const long* out_bytes, int n_out);
void ground_check_solve(double nx, double ny, double nz, int min_votes, int iters);
// sources may be null only when S == 0
void depth_fuse_check_args(const float* bank, const float* poses, const int* targets, const int* sources, int N, int B, int S,
                           int H, int W, double fx, double fy, double cx, double cy, double max_reproj, double max_rel_depth,
                           int min_views, double min_z, const float* fused, const unsigned char* views, const int* counts);
// depth_init may be null
void multiview_check_args(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                          const float* depth_init, int N, int B, int S, int H, int W, double fx, double fy, double cx, double cy,
                          double scale_px, double inlier_px, double min_z, int min_views, double max_rel_sigma, double max_depth,
                          int iters, const float* depth, const float* info, const unsigned char* views, const int* counts);

// mask may be null; out[i] of out_bytes[i], i < n_out: the outputs (a workspace among them)
void bundle_check_args(const float* acc_bank, const unsigned char* alive_bank, const float* poses, const int* slots,
                       const float* depth_init, const unsigned char* mask, int N, int B, int S, int H, int W, double fx, double fy,
                       double cx, double cy, int stride, int iters, double scale_px, double inlier_px, double min_z, int min_views,
                       bool grid_limit, const void* const* out, const long* out_bytes, int n_out);

// the voxel map (voxel_map.hip): images, mask, indices and pending may be null
void voxel_check_table(const void* table, long capacity);
void voxel_check_integrate(const float* depth, const float* poses, const unsigned char* images, const unsigned char* mask,
                           const int* indices, int N, int K, int H, int W, double fx, double fy, double cx, double cy, int stride,
                           double voxel, double ox, double oy, double oz, double min_z, double max_z, const void* table,
                           long capacity, const unsigned char* pending);
void voxel_check_rehash(const void* src, long src_capacity, const void* dst, long dst_capacity);
void voxel_check_extract(const void* table, long capacity, int min_count, double voxel, double ox, double oy, double oz, long max_out,
                         const float* points, const unsigned char* colors, const int* counts, const int64_t* keys,
                         const int64_t* found);

}  // namespace atdn
