// The argument rules that the geometry entry points (flow_consistency.hip, two_view.hip, flow_track.hip, pnp.hip, epipolar.hip,
// depth_fusion.hip, multiview_depth.hip, bundle.hip, ground.hip, voxel_map.hip, map_view.hip, pose_graph.hip) share. Each module's own rules are
// file-static in its .hip, beside the device entry point and the host twin that both go through them.
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

}  // namespace atdn
