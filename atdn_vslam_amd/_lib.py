"""ctypes binding of libatdn_hip.so (include/atdn_hip.h). There is no fallback: if the
library is missing or a call fails, the caller gets an exception."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ATDN_LIB_PATH: another build of the same library, for A/B timing of two builds inside one GPU job; diagnostics only)
LIB_PATH = os.environ.get("ATDN_LIB_PATH") or os.path.join(_HERE, "libatdn_hip.so")

_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_vp = C.c_void_p

# name -> (restype, argtypes); the single source for the loader and the "exports every symbol" test
SIGNATURES = {
    "atdn_version": (C.c_int, []),
    "atdn_last_error": (C.c_char_p, []),
    "atdn_gma_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int]),
    "atdn_gma_set_low_latency": (C.c_int, [_vp, C.c_int]),
    "atdn_gma_load": (C.c_int, [_vp, C.c_char_p, _vp, _i64p, C.c_int]),
    "atdn_gma_finalize": (C.c_int, [_vp]),
    "atdn_gma_forward": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_gma_forward_predictions": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "atdn_gma_forward_sequence": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_gma_forward_sequence_continued": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_gma_debug_read": (C.c_long, [_vp, C.c_char_p, _vp, C.c_long, _vp]),
    "atdn_gma_profile": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _f32p, _vp]),
    "atdn_gma_profile_mode": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _vp]),
    "atdn_gma_set_range_probe": (C.c_int, [_vp, C.c_int]),
    "atdn_gma_range_rows": (C.c_long, [_vp]),
    "atdn_gma_range_row": (C.c_int, [_vp, C.c_long, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _f32p, _i64p, _i64p]),
    "atdn_range_probe": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _f32p, _i64p, _i64p, _vp]),
    "atdn_range_probe_launch": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp]),
    "atdn_gma_workspace_bytes": (C.c_size_t, [_vp]),
    "atdn_gma_destroy": (None, [_vp]),
    "atdn_device_bytes_live": (C.c_int64, []),
    "atdn_clvo_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    "atdn_clvo_load": (C.c_int, [_vp, C.c_char_p, _vp, _i64p, C.c_int]),
    "atdn_clvo_finalize": (C.c_int, [_vp]),
    "atdn_clvo_encode": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "atdn_clvo_step": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_clvo_last_scan_path": (C.c_int, [_vp]),
    "atdn_clvo_destroy": (None, [_vp]),
    "atdn_vae_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int]),
    "atdn_vae_load": (C.c_int, [_vp, C.c_char_p, _vp, _i64p, C.c_int]),
    "atdn_vae_finalize": (C.c_int, [_vp]),
    "atdn_vae_embedding_shape": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "atdn_vae_encode": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "atdn_vae_scratch_floats": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    "atdn_vae_debug_stage": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_long, _vp]),
    "atdn_vae_destroy": (None, [_vp]),
    "atdn_clvo_trainer_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int]),
    "atdn_clvo_trainer_load": (C.c_int, [_vp, C.c_char_p, _vp, _i64p, C.c_int]),
    "atdn_clvo_trainer_finalize": (C.c_int, [_vp]),
    "atdn_clvo_trainer_forward_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32p, _vp]),
    "atdn_clvo_trainer_gradients": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_long)]),
    "atdn_clvo_trainer_adamw_step": (C.c_int, [_vp, C.c_float, C.c_float, C.c_float, C.c_int, _vp]),
    "atdn_clvo_trainer_set_loss": (C.c_int, [_vp, C.c_float, C.c_int, C.c_int]),
    "atdn_clvo_trainer_loss_terms": (C.c_int, [_vp, _f32p]),
    "atdn_clvo_loss": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _f32p, _vp, _vp, _vp]),
    "atdn_clvo_trainer_read": (C.c_long, [_vp, C.c_char_p, C.c_int, _vp, C.c_long, _vp]),
    "atdn_clvo_trainer_destroy": (None, [_vp]),
    "atdn_pose_transform_f32": (C.c_int, [_vp, _vp, _vp]),
    "atdn_pose_rel2abs": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "atdn_pose_accumulate_f32": (C.c_int, [_vp, _vp, _vp]),
    "atdn_resize_frames": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_resize_frames_mode": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_resize_frames_u8": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_pad_frames": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_ingest_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "atdn_ingest_frames_u8": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "atdn_ingest_destroy": (None, [_vp]),
    "atdn_flow_pack_f16": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_flow_gather_clips": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "atdn_flow_forward_interpolate": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_flow_forward_interpolate_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "atdn_flow_consistency": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp]),
    "atdn_flow_consistency_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp, _vp]),
    "atdn_flow_two_view_depth": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "atdn_flow_two_view_depth_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "atdn_depth_backproject": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "atdn_flow_track_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "atdn_flow_track_step_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, C.c_double,
                                            C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "atdn_depth_fuse": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_depth_fuse_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, _vp, _vp, _vp]),
    "atdn_multiview_depth": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                       C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "atdn_multiview_depth_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                            C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                                            C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp]),
    "atdn_bundle_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "atdn_bundle_terms": (C.c_int, [_vp] * 6 + [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int] + [C.c_double] * 3 + [C.c_int] + [_vp] * 4),
    "atdn_bundle_terms_host": (C.c_int, [_vp] * 6 + [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int] + [C.c_double] * 3 + [C.c_int] +
                               [_vp] * 2),
    "atdn_bundle_adjust": (C.c_int, [_vp] * 6 + [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int] * 2 + [C.c_double] * 3 + [C.c_int] +
                           [_vp] * 6),
    "atdn_bundle_adjust_host": (C.c_int, [_vp] * 6 + [C.c_int] * 5 + [C.c_double] * 4 + [C.c_int] * 2 + [C.c_double] * 3 + [C.c_int] +
                                [_vp] * 4),
    "atdn_pnp_workspace_bytes":(C.c_long, [C.c_int, C.c_int, C.c_int]),
    "atdn_pnp_terms": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "atdn_pnp_terms_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "atdn_pnp_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "atdn_pnp_solve_host": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp]),
    "atdn_epipolar_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "atdn_epipolar_terms": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "atdn_epipolar_terms_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_double, _vp, _vp]),
    "atdn_epipolar_solve": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "atdn_epipolar_solve_host": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_int, _vp, _vp, _vp]),
    "atdn_ground_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "atdn_ground_terms": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 8 + [_vp] * 4),
    "atdn_ground_terms_host": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 8 + [_vp] * 2),
    "atdn_ground_solve": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 11 + [C.c_int] * 2 + [_vp] * 5),
    "atdn_ground_solve_host": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 11 + [C.c_int] * 2 + [_vp] * 3),
    "atdn_ground_classify": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 7 + [_vp] * 3),
    "atdn_ground_classify_host": (C.c_int, [_vp] * 3 + [C.c_int] * 5 + [C.c_double] * 7 + [_vp] * 2),
    "atdn_pose_graph_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "atdn_pose_graph_terms": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "atdn_pose_graph_terms_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp]),
    "atdn_pose_graph_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                        C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "atdn_pose_graph_solve_host": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                             C.c_double, _vp, _vp, _vp, _vp]),
    "atdn_voxel_table_bytes": (C.c_long, [C.c_long]),
    "atdn_voxel_clear": (C.c_int, [_vp, C.c_long, _vp]),
    "atdn_voxel_clear_host": (C.c_int, [_vp, C.c_long]),
    "atdn_voxel_integrate": (C.c_int, [_vp] * 5 + [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_double] * 6 + [C.c_int, _vp,
                                                                                                                 C.c_long, _vp, _vp]),
    "atdn_voxel_integrate_host": (C.c_int, [_vp] * 5 + [C.c_int] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_double] * 6 +
                                  [C.c_int, _vp, C.c_long, _vp]),
    "atdn_voxel_rehash": (C.c_int, [_vp, C.c_long, _vp, C.c_long, _vp]),
    "atdn_voxel_rehash_host": (C.c_int, [_vp, C.c_long, _vp, C.c_long]),
    "atdn_voxel_extract": (C.c_int, [_vp, C.c_long, C.c_int] + [C.c_double] * 4 + [C.c_long] + [_vp] * 6),
    "atdn_voxel_extract_host": (C.c_int, [_vp, C.c_long, C.c_int] + [C.c_double] * 4 + [C.c_long] + [_vp] * 5),
    "atdn_view_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "atdn_view_render": (C.c_int, [_vp] * 3 + [C.c_int, _vp] + [C.c_int] * 3 + [C.c_double] * 6 + [C.c_int] + [C.c_double] * 2 +
                         [C.c_int] + [_vp] * 6),
    "atdn_view_render_host": (C.c_int, [_vp] * 3 + [C.c_int, _vp] + [C.c_int] * 3 + [C.c_double] * 6 + [C.c_int] + [C.c_double] * 2 +
                              [C.c_int] + [_vp] * 4),
    "atdn_voxel_votes": (C.c_int, [_vp, C.c_int] + [_vp] * 3 + [C.c_int] * 4 + [C.c_double] * 8 + [C.c_int] * 2 + [_vp, _vp]),
    "atdn_voxel_votes_host": (C.c_int, [_vp, C.c_int] + [_vp] * 3 + [C.c_int] * 4 + [C.c_double] * 8 + [C.c_int] * 2 + [_vp]),
    "atdn_voxel_remove": (C.c_int, [_vp, C.c_long, _vp, _vp, C.c_long, _vp, _vp]),
    "atdn_voxel_remove_host": (C.c_int, [_vp, C.c_long, _vp, _vp, C.c_long, _vp]),
    "atdn_map_search":(C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "atdn_map_gather_images_u8": (C.c_int, [_vp, C.c_int, C.c_long, _vp, C.c_int, _vp, _vp]),
    "atdn_corr_lookup": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp]),
    "atdn_corr_pyramid": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "atdn_corr_lookup_bricks": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp]),
    "atdn_corr_lookup_bricks_mode": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp, C.c_int, _vp]),
    "atdn_conv2d_nhwc": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_conv2d_nhwc_sf": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "atdn_conv2d_nhwc_sf_epi": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
}

GMA_STAGES = ("fnet", "corr", "pool", "cnet", "attention", "lookup", "motion_encoder", "aggregate", "gru_zr", "gru_q",
              "flow_head", "mask", "gru_ctx", "attn_logits", "agg_vt", "convc1", "gru_zr_v", "gru_q_v")

_lib = None


def lib():
    """The loaded library (loads on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: the HIP extension has not been built (python -m atdn_vslam_amd.build). "
                "There is no CPU fallback for the product path." % LIB_PATH)
        # PyTorch-ROCm ships its own HIP runtime: it must be the one already mapped when this library (linked against
        # libamdhip64 by soname) is loaded, or the process ends up with two runtimes and the second one finds no device
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError("libatdn_hip: " + lib().atdn_last_error().decode("utf-8", "replace"))


def ptr(t):
    """A tensor's data as a `void*` argument of the library; None stays None (a null pointer)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    """The current stream of the current device, as the library's `void* stream` argument."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, device, *args, workspace=None):
    """Entry point `name` for tensors on `device`. A CUDA device: `name(*args, [workspace,] stream)` under that device, on its
    current stream. Otherwise the host twin `name + "_host"` with `args` alone (the convention of every such pair in SIGNATURES:
    the host form takes the device form's arguments without the workspace and the stream)."""
    import torch
    if device.type == "cuda":
        with torch.cuda.device(device):
            if workspace is not None:
                args += (ptr(workspace),)
            check(getattr(lib(), name)(*args, stream()))
    else:
        check(getattr(lib(), name + "_host")(*args))


def workspace(symbol, device, *dims, message=None):
    """The workspace a device entry point asks for through its `*_workspace_bytes` function `symbol(*dims)`: a float64 tensor
    (8-byte aligned) of at least 8 bytes on `device`; None on the host, whose forms take none. A size <= 0 (dimensions out of
    range) raises `message` where one is given, and otherwise leaves the refusal to the entry point."""
    import torch
    if device.type != "cuda":
        return None
    n = int(getattr(lib(), symbol)(*dims))
    if n <= 0 and message:
        raise RuntimeError(message)
    return torch.empty((max(n, 8) + 7) // 8, dtype=torch.float64, device=device)


def load_state(load_fn, handle, state):
    """Feed a {key: tensor/ndarray} state dict to atdn_*_load (float entries only)."""
    import numpy as np
    import torch
    for key, val in state.items():
        if isinstance(val, torch.Tensor):
            if not val.dtype.is_floating_point:
                continue
            arr = val.detach().to("cpu", torch.float32).contiguous().numpy()
        else:
            arr = np.asarray(val)
            if arr.dtype.kind != "f":
                continue
            arr = np.ascontiguousarray(arr, dtype=np.float32)
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape) if arr.ndim else (C.c_int64 * 1)(1)
        check(load_fn(handle, key.encode(), arr.ctypes.data_as(_vp), shape, arr.ndim))
