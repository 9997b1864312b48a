"""`NeuralSLAM` — the caller-facing state machine of atdn_vslam/slam_framework/neural_slam.py on the MI355X path.

Same states (idle -> odometry -> mapping -> relocalization), same call pattern and the same files on disk
(`<keyframes_path>/rgb/%06d.pth` uint8 frames, `poses.pth` [K,12], `MappingVAE_weights.pth`), with the networks
replaced by the HIP modules of this package:

* odometry mode (`neural_slam.py:192-227`): resize to 376x1232, flow (12 iterations), CLVO head, float32 pose
  accumulation, keyframe decision (10 degrees / 15 m since the last keyframe, `neural_slam.py:268-283`);
* relocalization mode (`neural_slam.py:355-399`): MappingVAE embedding of the query, nearest keyframe embedding,
  flow-based refinement against that keyframe's stored frame.

`end_odometry()` persists the keyframe poses like the reference and then creates the map: with trained weights at hand
(`mapping_weights=` or `<keyframes_path>/MappingVAE_weights.pth`) it loads them, otherwise it trains the MappingVAE on
the keyframes (`mapping.create_map`, the reference's `__create_map`: 50 epochs of AdamW on stock PyTorch, a one-off per
mapping run) — then every keyframe is embedded on the HIP path and the state machine enters relocalization.
"""
import copy
import math
import os

import torch

from . import keyframe_dir as kd
from . import transforms
from .keyframe_depth import KeyframeDepthRecorder
from .keyframe_dir import KeyframeDir
from .modules import ATDNVO, MappingVAE, RAFTGMA
from .pipeline import SLAM_SIZE, resize_frames


class Frame:
    """Keyframe record (slam_framework/frame.py): file of the stored frame, predicted pose, latent embedding."""

    def __init__(self, rgb_file_name, pred_pose, code=None):
        self.rgb_file_name = rgb_file_name
        self.pose = pred_pose
        self.embedding = code


class KeyframePolicy:
    """A frame becomes a keyframe when the motion accumulated since the last one exceeds 10 degrees (norm of the yxz
    Euler vector) or 15 m (`NeuralSLAM.__decide_keyframe`, neural_slam.py:268-283). float32 like the reference."""

    def __init__(self, rot_threshold_deg=10.0, translation_threshold=15.0):
        self.rotation_threshold = (rot_threshold_deg / 180) * math.pi
        self.translation_threshold = translation_threshold
        self.propagation = torch.eye(4, dtype=torch.float32)

    def __call__(self, pred_mat):
        self.propagation = self.propagation @ torch.as_tensor(pred_mat, dtype=torch.float32)
        rotation = transforms.matrix2euler(self.propagation[:3, :3])
        translation = self.propagation[:3, -1]
        if torch.norm(rotation) > self.rotation_threshold or torch.norm(translation) > self.translation_threshold:
            self.propagation = torch.eye(4, dtype=torch.float32)
            return True
        return False


def _load_weights(w):
    return torch.load(w, map_location="cpu") if isinstance(w, (str, os.PathLike)) else w


def _homogeneous(poses12):
    p = torch.as_tensor(poses12, dtype=torch.float32).view(-1, 3, 4)
    last = torch.tensor([0.0, 0.0, 0.0, 1.0]).view(1, 1, 4).repeat(len(p), 1, 1)
    return torch.cat([p, last], dim=1)


def _check_options(calib, resident_map, keyframe_depth, loop_closure, refine_pose, fuse_depth, ground, camera_height, voxel_map,
                   map_depth, carve=False):
    """The rules between NeuralSLAM's options; the first one that is broken raises ValueError."""
    if voxel_map and (calib is None or not resident_map):
        raise ValueError("voxel_map=True needs the calibration and the keyframe map in device memory: pass calib= and "
                         "resident_map=True")
    if map_depth not in (False, True, "fill"):
        raise ValueError('map_depth is False, True or "fill", got %r' % (map_depth,))
    if map_depth and not voxel_map:
        raise ValueError("map_depth needs the voxel map: pass voxel_map=True")
    if carve and not voxel_map:
        raise ValueError("carve=True needs the voxel map: pass voxel_map=True")
    if ground and calib is None:
        raise ValueError("ground=True needs the calibration: pass calib=")
    if ground and camera_height is not None and not (math.isfinite(float(camera_height)) and float(camera_height) > 0.0):
        raise ValueError("camera_height must be finite and > 0, got %r" % (camera_height,))
    if fuse_depth and (calib is None or not resident_map):
        raise ValueError("fuse_depth=True needs the calibration and the keyframe map in device memory: pass calib= and "
                         "resident_map=True")
    if refine_pose and calib is None:
        raise ValueError("refine_pose=True needs the calibration: pass calib=")
    if loop_closure and not resident_map:
        raise ValueError("loop_closure=True needs the keyframe map in device memory: pass resident_map=True")
    if keyframe_depth not in ("pair", "track", "multiview", "bundle"):
        raise ValueError('keyframe_depth is "pair", "track" or "multiview", or "bundle", got %r' % (keyframe_depth,))
    if keyframe_depth != "pair" and calib is None:
        raise ValueError('keyframe_depth="%s" needs the calibration: pass calib=' % keyframe_depth)


class NeuralSLAM:
    """Drop-in for `atdn_vslam.slam_framework.neural_slam.NeuralSLAM`.

    args: object with `.device` and `.keyframes_path` (the reference's `Arguments`).
    odometry_weights / flow_weights / mapping_weights: checkpoint path or state dict. `flow_weights` defaults to the
    path the reference's `GMA_Parameters` names. `map_options`: keyword arguments for `mapping.create_map` when
    `end_odometry()` has to train the map itself.
    `resident_map=True` keeps the keyframe map in device memory (keyframe_map.KeyframeMap): keyframe images and embeddings
    sit in HBM banks, a relocalisation query searches them in one launch and takes the keyframe image from the bank instead
    of its file, and `relocalize_batch` answers several queries per call. Files on disk and return values are the same; with
    the default (False) nothing changes.
    `warm_start=True`: in odometry mode every pair of an unbroken run of calls starts from the previous pair's flow, pushed forward
    on the device (RAFTGMA.forward_consecutive; 12 iterations as before). The relocalisation refinement always runs cold: a
    keyframe and a query are not consecutive frames.
    `calib`: (fx, fy, cx, cy) or a 3x3 / 3x4 calibration matrix of the 376 x 1232 grid (depth.resize_calib). In odometry mode the
    pair whose first frame is a keyframe then gives that keyframe its depth (transforms.two_view_depth of the pair's flow and
    predicted pose): `<keyframes_path>/depth/%06d.pth`, float32 [1,376,1232], 0 = no depth, written on the call after the one
    that stored the keyframe — a keyframe that never gets a successor has no file — and `keyframe_points(i)` returns its valid
    pixels as points of the world frame. Without it nothing on disk or in any return value changes.
    `keyframe_depth`: "pair" (the default) is the depth just described. "track" (needs `calib`) uses the whole keyframe interval
    instead of its first pair: a depth.FlowTrack starts at every keyframe and is extended by every pair up to and including the one
    that registers the next keyframe, so each pixel's depth is triangulated over the longest baseline its track survives. The file
    has the same name, shape and dtype; it is written when the next keyframe is registered, or by `end_odometry()` for the last
    keyframe if any pair followed it. Poses and `rgb/` files do not depend on the choice.
    "multiview" (needs `calib`) keeps the last 16 steps of that track (FlowTrack(history=16)) and solves every pixel's depth over
    all of them at once (FlowTrack.multiview, `multiview_options` its keyword arguments), started from the track's depth: the same
    `depth/%06d.pth`, and beside it `depth_info/%06d.pth` (float32 [1,376,1232], the inverse variance of the relative depth for
    unit pixel noise) and `depth_mv_views/%06d.pth` (uint8 [376,1232], the views that agree); `multiview_counts` [1,3] =
    (candidates, solved, valid) of the last keyframe stays on the device. "pair" and "track" change no file, directory or bit.
    "bundle" (needs `calib`) is "multiview" behind a windowed bundle adjustment: FlowTrack.bundle first refines the poses of the
    stored steps jointly with the anchor's depth (transforms.bundle_adjust, `bundle_options` its keyword arguments) and solves the
    multi-view depth against the refined poses. It writes what "multiview" writes and `bundle/%06d.pth`, a dict of `poses`
    (float32 [S,12], anchor <- step, oldest first), `cost` (float64 [2]) and `counts` (int32 [4]); `bundle_cost` [1,2] and
    `bundle_counts` [1,4] of the last keyframe stay on the device. `bundle_pose=True`: when the interval had at most 16 steps —
    the window's last step is then the new keyframe's frame — the new keyframe's pose and the running pose become (anchor pose @
    refined last pose), formed in float64 and stored as float32; otherwise, and with False (the default), the trajectory is that of
    "multiview", bit for bit.
    `refine_pose=True` (needs `calib`): in odometry mode every pair's predicted pose is refined on the pair's own flow
    (transforms.pose_from_flow with its defaults, on the device: the rotation and the direction of t; |t| stays the head's) before
    anything uses it: the "pair" keyframe depth, the poses fed to the flow track, the keyframe policy and the running pose
    (float32 pose @ refined step) all see the refined pose; `last_refine_counts` [1,4] = (candidates, used, inliers, accepted
    steps) of the last pair stays on the device. With False (the default) nothing changes anywhere.
    `fuse_depth=True` (needs `calib` and `resident_map`): at the end of `end_odometry()` — after the loop closure when that is on,
    so with the optimised poses — the keyframe depths are filtered against their neighbours (`fuse_depths`, `fuse_options` its
    keyword arguments): `depth_fused/%06d.pth`, `depth_views/%06d.pth` and `fusion_counts`; `keyframe_points(i, fused=True)` reads
    them. With False (the default) no file, directory or return value changes.
    `ground=True` (needs `calib`): every keyframe depth — the one `keyframe_depth` selects, while it is still on the device — is
    fitted with the road's plane (transforms.ground_plane; `ground_options` its keyword arguments, plus `min_inlier_share` and
    `max_tilt_deg` of transforms.ground_accept). `ground/%06d.pth` holds a dict of `q`, `normal`, `height`, `sums`, `counts`
    (host tensors), `accepted` (bool: ground_accept) and `scale` (float: `camera_height` / height when accepted and a
    `camera_height`, in the units the trajectory should have, is given; 1.0 otherwise). The depth of a keyframe is triangulated
    against the poses of its own interval, so `scale` is the correction of exactly that interval's translations. With a
    `camera_height` and keyframe_depth "track", "multiview" or "bundle", `end_odometry()` also writes `poses_scaled.pth` [K,12]
    float32 = evaluation.rescale_intervals(poses.pth, the scales of keyframes 0 .. K-2). With "pair" the depth carries the scale
    of the keyframe's first pair only, not of the interval, and `poses_scaled.pth` is not written. Nothing is fed back: the
    running pose, `poses.pth`, `poses_closed.pth`, the loop closure, the depth fusion and every other file are what they are
    without it. With False (the default) no file, directory, attribute or bit changes.
    `voxel_map=True` (needs `calib` and `resident_map`): at the end of `end_odometry()` — after the loop closure and the depth
    fusion when those are on, so with the optimised poses and the fused depths — every keyframe's depth and colours are
    accumulated into one voxel-hashed point cloud (`build_voxel_map`, `voxel_options` its keyword arguments): `map.ply` and the
    `voxel_map` attribute. A cold start with the option removes a `map.ply` of an earlier session. With False (the default)
    nothing anywhere changes.
    `map_depth=True` or `"fill"` (needs `voxel_map=True`): after `build_voxel_map()` the cloud is rendered back into every
    keyframe's own pose (`write_map_depth`; `voxel_map.VoxelMap.render` with its defaults): `map_depth/%06d.pth`, float32
    [1,376,1232], 0 = nothing rendered — the depth a keyframe would have had, had it seen what all of them saw. With `"fill"` the
    rendered depth also goes into the depth bank at exactly the pixels that hold 0, so the geometric leg of relocalisation reads
    it. A cold start with the option removes a `map_depth/` of an earlier session. With False (the default) no file, no code path
    and no bit changes anywhere.
    `carve=True` (needs `voxel_map=True`): `build_voxel_map()` carves free space after the last integrate and before `map.ply`
    is written (`KeyframeMap.carve`, `carve_options` its keyword arguments — min_free, ratio, min_support, near, far, rel,
    abs_tol, radius, batch) against the depths it integrated — the fused ones with `fuse_depth`, the depth bank otherwise: a
    voxel that enough keyframes see straight through, and more than confirm it, leaves the cloud. `carve_report` keeps
    `VoxelMap.carve`'s report, `map.ply` holds the carved cloud and `map_depth` renders it. No new file or directory. With
    False (the default) no code path and no bit changes anywhere.
    """

    FLOW_CHECKPOINT = "atdn_vslam/checkpoints/gma-kitti.pth"  # utils/gma_parameters.py

    def __init__(self, args, odometry_weights=None, start_mode=None, flow_weights=None, mapping_weights=None,
                 precision=None, map_options=None, resident_map=False, warm_start=False, calib=None, keyframe_depth="pair",
                 loop_closure=False, loop_options=None, refine_pose=False, fuse_depth=False, fuse_options=None,
                 multiview_options=None, bundle_options=None, bundle_pose=False, ground=False, ground_options=None,
                 camera_height=None, voxel_map=False, voxel_options=None, map_depth=False, carve=False, carve_options=None):
        from .depth import intrinsics
        _check_options(calib, resident_map, keyframe_depth, loop_closure, refine_pose, fuse_depth, ground, camera_height, voxel_map,
                       map_depth, carve)
        self._args = args
        self._base = args.keyframes_path
        self._dir = KeyframeDir(self._base)
        self._device = torch.device(args.device if getattr(args, "device", None) not in (None, "cpu") else "cuda:0")
        self._calib = None if calib is None else intrinsics(calib)
        self._precision = precision
        self._warm_start = bool(warm_start)   # odometry mode only; relocalisation pairs are not consecutive frames
        self._refine_pose = bool(refine_pose)
        self.last_refine_counts = None
        # keyframe depth: the recorder decides which pairs give which keyframe its depth, _record_depth writes what it returns
        self._depth = KeyframeDepthRecorder(keyframe_depth, SLAM_SIZE, self._calib, self._device, multiview_options, bundle_options)
        self._bundle_pose = bool(bundle_pose) and keyframe_depth == "bundle"
        self.multiview_counts = None   # [1,3] int32 (device) of the last multi-view keyframe depth: candidates, solved, valid
        self.bundle_cost = self.bundle_counts = None   # [1,2] float64, [1,4] int32 (device) of the last keyframe's adjustment
        self._ground = bool(ground)
        if ground:
            self._ground_options = dict(ground_options or {})
            self._ground_accept = {k: self._ground_options.pop(k) for k in ("min_inlier_share", "max_tilt_deg")
                                   if k in self._ground_options}
            self._camera_height = None if camera_height is None else float(camera_height)
            self._ground_scales = {}     # keyframe index -> scale of its interval
        # (with "pair" the depth carries the scale of the keyframe's first pair only, not of the interval: no scaled poses)
        self._scale_poses = bool(ground) and camera_height is not None and keyframe_depth != "pair"
        # what end_odometry() does after the map is embedded
        self._map_options = dict(map_options or {})   # keyword arguments of mapping.create_map (e.g. num_epochs)
        self._loop_closure = bool(loop_closure)
        self._loop_options = dict(loop_options or {})
        self.loop_report = None      # the report of the last close_loops()
        self._fuse_depth = bool(fuse_depth)
        self._fuse_options = dict(fuse_options or {})
        self.fusion_counts = None    # [K,3] int32 (host) of the last fuse_depths(): pixels with a depth, seen, kept
        self._fused_device = None    # the fused depths of the last fuse_depths() (device), kept for the voxel map only
        self._voxel_map = bool(voxel_map)
        self._voxel_options = dict(voxel_options or {})
        self.voxel_map = None        # voxel_map.VoxelMap of the last build_voxel_map()
        self._map_depth = map_depth
        self._carve = bool(carve)
        self._carve_options = dict(carve_options or {})
        self.carve_report = None     # VoxelMap.carve's report of the last build_voxel_map() with carve=True
        # frame-by-frame caller that returns a host pose per call (one device synchronisation each): the split-f16 range guard
        # is read after EVERY forward, so no pose computed from clamped activations is ever returned
        self._flow_net = RAFTGMA(max_batch=1, precision=precision, saturation_check_every=1, low_latency=True)
        self._flow_net.load_state_dict(_load_weights(flow_weights if flow_weights is not None else self.FLOW_CHECKPOINT))
        self._flow_net = self._flow_net.to(self._device).eval()
        self._padder = transforms.InputPadder((3,) + SLAM_SIZE)
        self._odometry_net = ATDNVO()
        self._odometry_net.load_state_dict(_load_weights(odometry_weights))
        self._odometry_net = self._odometry_net.to(self._device).eval()
        self._image_buffer = None
        self._mapping_net = None
        self._keyframes = []
        self._policy = KeyframePolicy()
        self._current_pose = torch.eye(4, dtype=torch.float32)
        self._resident = bool(resident_map)
        self._map = None            # keyframe_map.KeyframeMap when resident_map=True
        self._batch_flow_net = None  # relocalize_batch's flow handle (batch > 1), created on first use

        if start_mode == "mapping":
            self._load_keyframes(embed=False)
            self._mode = "odometry"
            self.end_odometry(mapping_weights)
        elif start_mode == "relocalization":
            self._set_mapping_net(mapping_weights if mapping_weights is not None else self._dir.path(kd.WEIGHTS))
            self._load_keyframes(embed=True)
            self._mode = "relocalization"
        else:
            options = dict(calib=calib is not None, fuse_depth=fuse_depth, multiview=keyframe_depth in ("multiview", "bundle"),
                           bundle=keyframe_depth == "bundle", ground=ground, map_depth=map_depth, voxel_map=voxel_map)
            self._dir.prepare_cold_start([name for name, on in options.items() if on])
            self._mode = "idle"
            if self._resident:
                from .keyframe_map import KeyframeMap
                self._map = KeyframeMap(self._device, hw=SLAM_SIZE)

    # ------------------------------------------------------------------ state machine
    def start_odometry(self):
        if self._mode == "idle":
            self._mode = "odometry"
        else:
            print("Odometry cannot be performed in current SLAM stage")

    def end_odometry(self, mapping_weights=None):
        """Persist the keyframe poses (`poses.pth`, [K,12]), create the map (train the MappingVAE on the keyframes, as
        neural_slam.py:160 does; skipped only when `mapping_weights` is given explicitly), embed every keyframe and
        enter relocalization."""
        if self._mode == "odometry" and len(self._keyframes) > 0:
            self._record_depth(self._depth.close(False))
            poses = torch.stack([kf.pose.flatten()[:12] for kf in self._keyframes], dim=0)
            self._dir.save(poses, kd.POSES)
            if self._scale_poses:
                from .evaluation import rescale_intervals
                scales = [self._ground_scales.get(i, 1.0) for i in range(len(self._keyframes) - 1)]
                scaled = torch.from_numpy(rescale_intervals(poses.numpy(), scales)[:, :3, :].reshape(-1, 12)).float()
                self._dir.save(scaled, kd.POSES_SCALED)
            self._mode = "mapping"
            if mapping_weights is None:
                # map creation (neural_slam.py:160,305-352): the reference ALWAYS trains the auto-encoder on the current
                # keyframes here and overwrites MappingVAE_weights.pth — a file left in the directory by an earlier
                # session belongs to another environment and is never picked up. Training runs on stock PyTorch, as in
                # the reference; the embedding it yields runs on the HIP path again. Only an explicit `mapping_weights`
                # argument skips the training.
                from .mapping import create_map
                create_map(self._base, device=self._device, **self._map_options)
                mapping_weights = self._dir.path(kd.WEIGHTS)
            self._set_mapping_net(mapping_weights)
            self._embed_keyframes()
            self._mode = "relocalization"
            if self._loop_closure:
                self.close_loops(**self._loop_options)
            if self._fuse_depth:
                self.fuse_depths(**self._fuse_options)               # after the loop closure: it sees the optimised poses
            if self._voxel_map:
                self.build_voxel_map(**self._voxel_options)          # after both: the optimised poses, the fused depths
                if self._map_depth:
                    self.write_map_depth(fill=self._map_depth == "fill")
        elif len(self._keyframes) == 0:
            print("There is no explored enviromnent yet!")
        elif self._mode == "mapping" and mapping_weights is not None:
            self._set_mapping_net(mapping_weights)
            self._embed_keyframes()
            self._mode = "relocalization"
        else:
            print("Current state is not odometry")

    def close_loops(self, **options):
        """Close the loops of the keyframe map (relocalisation mode, resident map only): `loop_closure.close_loops` with this
        object's networks and calibration (`options`: its keyword arguments, `calib` among them). The optimised poses replace
        the frames' and the map's and are written to `poses_closed.pth` ([K,12]); `poses.pth` stays the raw odometry. Without
        a verified loop nothing changes and no file is written. Returns the report."""
        from . import loop_closure
        if getattr(self, "_map", None) is None:
            raise RuntimeError("close_loops needs the keyframe map in device memory: construct NeuralSLAM(..., resident_map=True)")
        if self._mode != "relocalization":
            raise Exception("SLAM called in invalid state!")
        options.setdefault("calib", self._calib)
        report = loop_closure.close_loops(self._map, self._flow_for_batches(), self._odometry_net, **options)
        self.loop_report = report
        if report["counts"] is not None:
            for i, kf in enumerate(self._keyframes):
                kf.pose = self._map.poses[i].clone()
            self._dir.save(self._map.poses[:, :3, :].reshape(-1, 12).clone(), kd.POSES_CLOSED)
        return report

    @torch.no_grad()
    def fuse_depths(self, **options):
        """Fuse the keyframe depths across the map (resident map and `calib` only): `KeyframeMap.fuse_depths` with this object's
        calibration (`options`: its keyword arguments — window, sources, batch, the thresholds; `replace` too). Writes, for every
        keyframe, `depth_fused/%06d.pth` (float32 [1,H,W], 0 = no depth or rejected) and `depth_views/%06d.pth` (uint8 [H,W], the
        number of agreeing neighbours); `depth/` stays the unfused depth. Sets and returns `fusion_counts` [K,3] int32 (host).
        A map in which no keyframe has a depth writes nothing and returns None."""
        if getattr(self, "_map", None) is None or self._calib is None:
            raise RuntimeError("fuse_depths needs the keyframe map in device memory and the calibration: construct "
                               "NeuralSLAM(..., calib=..., resident_map=True)")
        if self._map.depth_bank is None:
            self.fusion_counts = None
            return None
        fused, views, counts = self._map.fuse_depths(self._calib, **options)
        if self._voxel_map:
            self._fused_device = fused
        fused, views = fused.cpu(), views.cpu()
        self._dir.create(kd.DEPTH_FUSED, kd.DEPTH_VIEWS)
        for i, kf in enumerate(self._keyframes):
            self._dir.save(fused[i:i + 1].clone(), kd.DEPTH_FUSED, kf.rgb_file_name)
            self._dir.save(views[i].clone(), kd.DEPTH_VIEWS, kf.rgb_file_name)
        self.fusion_counts = counts.cpu()
        return self.fusion_counts

    @torch.no_grad()
    def build_voxel_map(self, min_count=1, **options):
        """The map as one coloured point cloud (relocalisation mode, resident map and `calib` only): `KeyframeMap.voxel_map` with
        this object's calibration (`options`: its keyword arguments — voxel, origin, min_z, max_z, capacity, stride, batch) over
        the keyframes' poses as they are now (the optimised ones after a loop closure) and their depths — the fused depths of
        the last `fuse_depths()` of this object when `fuse_depth=True`, the depth bank otherwise. Writes
        `<keyframes_path>/map.ply` (binary little-endian: x y z float, red green blue uchar, count int; the voxels with at least
        `min_count` points in ascending key order; with `carve=True` after free-space carving against the same depths, whose
        report is kept as `self.carve_report`), keeps the VoxelMap as `self.voxel_map` and returns it. A map in which no
        keyframe has a depth writes nothing and returns None."""
        if getattr(self, "_map", None) is None or self._calib is None:
            raise RuntimeError("build_voxel_map needs the keyframe map in device memory and the calibration: construct "
                               "NeuralSLAM(..., calib=..., resident_map=True)")
        if self._mode != "relocalization":
            raise Exception("SLAM called in invalid state!")
        if self._map.depth_bank is None:
            self.voxel_map = None
            return None
        fused = self._fused_device if self._fuse_depth else None
        if fused is not None and int(fused.shape[0]) != len(self._map):
            fused = None
        self.voxel_map = self._map.voxel_map(self._calib, fused=fused, **options)
        if self._carve:
            self.carve_report = self._map.carve(self.voxel_map, self._calib, fused=fused, **self._carve_options)
        self.voxel_map.save_ply(self._dir.path(kd.MAP_PLY), min_count=min_count)
        return self.voxel_map

    @torch.no_grad()
    def render_map(self, poses, **options):
        """`self.voxel_map` seen from arbitrary `poses` ([B,12], [B,3,4] or [B,4,4]; world <- camera; any device) under this
        object's calibration at the map's frame size: `VoxelMap.render` (`options`: min_count, splat, max_splat, near, far).
        Returns `(depth [B,H,W] float32, colors [B,3,H,W] uint8 or None, support [B,H,W] uint8, counts [B,3] int64)` on the
        device."""
        if self.voxel_map is None:
            raise RuntimeError("render_map needs the voxel map: construct NeuralSLAM(..., voxel_map=True) and end the odometry, "
                               "or call build_voxel_map()")
        return self.voxel_map.render(torch.as_tensor(poses).to(self.voxel_map.device), self._calib, SLAM_SIZE, **options)

    @torch.no_grad()
    def write_map_depth(self, fill=False, **options):
        """Render `self.voxel_map` into every keyframe's own pose (`KeyframeMap.render_depths`; `options`: its keyword
        arguments) and write `map_depth/<the frame's name>`, float32 [1,H,W], 0 = nothing rendered. `fill=True` also fills the
        depth bank's zero pixels. Returns the rendered depths [K,H,W] on the device; None (and no file) without a voxel map."""
        if self.voxel_map is None:
            return None
        depths = self._map.render_depths(self.voxel_map, self._calib, fill=fill, **options)
        self._dir.create(kd.MAP_DEPTH)
        host = depths.cpu()
        for i, kf in enumerate(self._keyframes):
            self._dir.save(host[i:i + 1].clone(), kd.MAP_DEPTH, kf.rgb_file_name)
        return depths

    @torch.no_grad()
    def __call__(self, im):
        if self._mode == "odometry":
            im = im.to(self._device)
            im = resize_frames(im if im.dtype == torch.uint8 else im.float(), SLAM_SIZE)   # (uint8: converted inside the resize kernel)
            if im.dtype != torch.float32:
                im = im.float()
            if self._image_buffer is not None:
                im2 = self._padder.pad(im)[0]
                # (pair mode's bits, one feature-network pass per frame while the chain of odometry calls is unbroken)
                _, flow = self._flow_net.forward_consecutive(self._image_buffer, im2, iters=12, warm_start=self._warm_start)
                pred_rot, pred_tr = self._odometry_net(flow)
                rot, tr = pred_rot.squeeze().cpu(), pred_tr.squeeze().cpu()
                pred_mat = transforms.transform(rot, tr)
                if self._refine_pose:
                    refined, _, self.last_refine_counts = transforms.pose_from_flow(flow, pred_mat[None].to(self._device), self._calib)
                    pred_mat = refined[0].cpu()
                    self._current_pose = self._current_pose @ pred_mat
                else:
                    self._current_pose = transforms.accumulate(self._current_pose, rot, tr)  # float32 pose @ pred_mat
                self._record_depth(self._depth.pair(flow, pred_mat))
                if self._policy(pred_mat):
                    self._add_keyframe(im2)
                    self._record_depth(self._depth.close(True))    # (may move the new keyframe's pose: bundle_pose)
                    self._depth.anchor(len(self._keyframes) - 1)
                self._image_buffer = im2
            else:
                self._image_buffer = self._padder.pad(im)[0]
                self._add_keyframe(im)
                self._depth.anchor(0)
            return self._current_pose
        if self._mode == "relocalization":
            q = im.to(self._device).float()
            if q.dim() == 3:
                q = q.unsqueeze(0)
            return self._relocalize(q)
        raise Exception("SLAM called in invalid state!")

    def mode(self):
        return copy.deepcopy(self._mode)

    def to(self, device):
        self._args.device = device
        self._device = torch.device(device)
        self._flow_net = self._flow_net.to(device)
        self._odometry_net = self._odometry_net.to(device)
        if self._mapping_net is not None:
            self._mapping_net = self._mapping_net.to(device)
        self._batch_flow_net = None   # (a resident keyframe map stays where it was built: its search names both devices)
        self._depth.to(self._device)   # keyframe_depth="track": a running track goes along with the networks

    def get_keyframe(self, index):
        return self._keyframes[index]

    def __getitem__(self, index):
        return self._keyframes[index]

    def __len__(self):
        return len(self._keyframes)

    @torch.no_grad()
    def keyframe_points(self, index, fused=False):
        """[3,N] float32 on the device: the pixels of keyframe `index` that have a depth, as points of the world frame — its
        depth file back-projected (depth.project_depth) and moved by the keyframe's pose. Needs `calib`; a keyframe without a
        depth file (no successor yet) raises FileNotFoundError. `fused=True` reads the fused depth (`depth_fused/`, written by
        `fuse_depths`) instead: only the pixels that enough neighbouring keyframes agree on."""
        from .depth import project_depth
        if self._calib is None:
            raise RuntimeError("keyframe_points needs the calibration: construct NeuralSLAM(..., calib=...)")
        kf = self._keyframes[index]
        depth = self._dir.load(kd.DEPTH_FUSED if fused else kd.DEPTH, kf.rgb_file_name).to(self._device)
        points = project_depth(depth, self._calib)
        points = points[:, depth[0] > 0]
        pose = torch.as_tensor(kf.pose, dtype=torch.float32).to(self._device)
        # (three products and three sums per coordinate, element-wise: no GEMM for a 3 x 3 matrix)
        return (pose[:3, 0:1] * points[0:1] + pose[:3, 1:2] * points[1:2]) + (pose[:3, 2:3] * points[2:3] + pose[:3, 3:4])

    # ------------------------------------------------------------------ internals
    def _add_keyframe(self, im):
        """The frame `im` becomes the next keyframe, at the running pose."""
        name = self._dir.path(kd.RGB, len(self._keyframes))
        self._store_keyframe(im, name)
        self._keyframes.append(Frame(name, self._current_pose))

    def _record_depth(self, result):
        """Everything a keyframe_depth.KeyframeDepth leads to (None: nothing): the keyframe's files, the bundle_pose feedback,
        the ground fit, the depth bank."""
        if result is None:
            return
        index, save = result.index, self._dir.save
        if result.poses is not None:
            poses = result.poses[0].to("cpu")
            self.bundle_cost, self.bundle_counts = result.cost, result.counts
            save(dict(poses=poses, cost=result.cost[0].to("cpu"), counts=result.counts[0].to("cpu")), kd.BUNDLE, index)
        if result.info is not None:
            self.multiview_counts = result.multiview_counts
            save(result.info[0].to("cpu"), kd.DEPTH_INFO, index)
            save(result.views[0].to("cpu"), kd.DEPTH_MV_VIEWS, index)
        save(result.depth[0].to("cpu"), kd.DEPTH, index)
        if self._bundle_pose and result.new_keyframe and result.complete:
            # the window's last step is the frame of the keyframe just registered (the last of the list)
            last = torch.eye(4, dtype=torch.float64)
            last[:3, :] = poses[-1].reshape(3, 4).double()
            anchor = torch.as_tensor(self._keyframes[index].pose).double()
            pose = (anchor @ last).float()
            self._keyframes[-1].pose = pose
            self._current_pose = pose
            if self._map is not None:
                self._map.poses[len(self._keyframes) - 1] = pose
        if self._ground:
            ground = transforms.ground_record(result.depth, self._calib, self._ground_options, self._ground_accept, self._camera_height)
            self._ground_scales[index] = ground["scale"]
            save(ground, kd.GROUND, index)
        if self._map is not None:
            self._map.set_depth(index, result.depth[0])

    def _set_mapping_net(self, weights):
        self._mapping_net = MappingVAE()
        self._mapping_net.load_state_dict(_load_weights(weights))
        self._mapping_net = self._mapping_net.to(self._device).eval()

    def _embed(self, rgb):
        rgb = rgb.to(self._device).float()
        if rgb.dim() == 3:
            rgb = rgb.unsqueeze(0)
        return self._mapping_net(rgb)[0]

    def _store_keyframe(self, im, name):
        """Write the keyframe's uint8 image file (neural_slam.py:213,224); with the resident map the same bytes also go into
        the image bank, converted and copied on the device."""
        if self._map is None:
            torch.save(im.to("cpu").byte(), name)
            return
        u8 = im.byte()
        self._map.append(u8, self._current_pose)
        torch.save(u8.to("cpu"), name)

    def _embed_keyframes(self):
        if self._map is None:
            for kf in self._keyframes:
                kf.embedding = self._embed(torch.load(kf.rgb_file_name))
            return
        self._map.embed(self._mapping_net, batch=16)
        for i, kf in enumerate(self._keyframes):
            kf.embedding = self._map.embedding(i)

    def _load_keyframes(self, embed):
        closed = embed and self._dir.exists(kd.POSES_CLOSED)
        if self._resident:
            from .keyframe_map import KeyframeMap
            self._map = KeyframeMap.from_directory(self._base, self._device)
            if closed:                                            # a relocalisation start after a loop closure
                self._map.update_poses(self._dir.load(kd.POSES_CLOSED))
            self._keyframes = [Frame(f, self._map.poses[i].clone()) for i, f in enumerate(self._dir.frames())]
            if embed:
                self._embed_keyframes()
            return
        poses = _homogeneous(self._dir.load(kd.POSES_CLOSED if closed else kd.POSES))
        for i, f in enumerate(self._dir.frames("*")):
            code = self._embed(torch.load(f)) if embed else None
            self._keyframes.append(Frame(f, poses[i], code))

    def _flow_for_batches(self):
        if self._batch_flow_net is None:
            net = RAFTGMA(max_batch=16, precision=self._precision, saturation_check_every=1)
            net.load_state_dict(self._flow_net.state_dict())
            self._batch_flow_net = net.to(self._device).eval()
        return self._batch_flow_net

    @torch.no_grad()
    def relocalize_batch(self, images, top_k=1, refine=True, verify=False, geometric=False):
        """Several relocalisation queries per call (resident map only): `KeyframeMap.relocalize` with this object's
        networks. images [Q,3,376,1232] (or a list of [3,376,1232] frames). Returns host tensors `distances` [Q,K],
        `indices` [Q,top_k] (nearest first), `initial` [Q,4,4], `refined` [Q,4,4]. Every query is refined from the reset
        (zero) state of the pose head, and the state the head carries between `slam(image)` calls is neither read nor
        changed. The flow network runs on a second handle with the same weights (batches of at most 16), created on the
        first call.
        `verify=True` (needs `refine`): every one of the Q * top_k candidates is refined and scored by the forward-backward
        consistency of its two flows; returns `(distances, indices, initial, refined, scores, chosen)` with `scores`
        [Q,top_k] (near 0: the keyframe and the query do not show the same place), `chosen` [Q] the rank with the most
        consistent pixels, and `initial` / `refined` those of the chosen candidate (`KeyframeMap.relocalize`).
        `geometric=True` (needs `refine` and a `calib` at construction) appends `refined_geo` [Q,4,4] and `geo_counts` [Q,4]:
        the pose that the keyframe's depth map and the keyframe -> query flow determine (`transforms.pose_from_depth`, started
        at the pose head's answer, masked by the consistency mask with `verify`), as initial @ pose, and its (candidates,
        used, inliers, accepted steps). A keyframe without a depth gives refined_geo == refined and zero counts."""
        if getattr(self, "_map", None) is None:
            raise RuntimeError("relocalize_batch needs the keyframe map in device memory: construct "
                               "NeuralSLAM(..., resident_map=True)")
        if self._mode != "relocalization":
            raise Exception("SLAM called in invalid state!")
        if isinstance(images, (list, tuple)):
            images = torch.stack([torch.as_tensor(im) for im in images], dim=0)
        if geometric and self._calib is None:
            raise ValueError("geometric=True needs the calibration: construct NeuralSLAM(..., calib=...)")
        return self._map.relocalize(images, self._flow_for_batches(), self._odometry_net, self._mapping_net, top_k=top_k,
                                    refine=refine, verify=verify, geometric=geometric, calib=self._calib if geometric else None)

    def _relocalize(self, image):
        mu = self._mapping_net(image)[0]
        if self._map is None:
            distances = torch.stack([torch.norm(kf.embedding - mu, p=2) for kf in self._keyframes], dim=0)
            closest = self._keyframes[int(torch.argmin(distances))]
            im1 = torch.load(closest.rgb_file_name).unsqueeze(0).to(self._device).float()
        else:
            # resident map: every distance and the nearest keyframe in one launch, its image from the bank
            distances, nearest = self._map.search(mu, top_k=1)
            distances = distances[0]
            closest = self._keyframes[int(nearest[0, 0])]
            im1 = self._map.images([int(nearest[0, 0])])
        initial_pose = closest.pose
        # refinement: odometry between the stored keyframe image and the query (neural_slam.py:386-399); batch 1 on the
        # low-latency flow handle and the stateful head in both cases: the reference's semantics, carried state included
        _, flow = self._flow_net(im1, image, iters=12, test_mode=True)
        pred_rot, pred_tr = self._odometry_net(flow)
        pose_diff = transforms.transform(pred_rot.squeeze().cpu(), pred_tr.squeeze().cpu())
        return initial_pose, initial_pose @ pose_diff, distances.cpu()
