"""Carving in NeuralSLAM: with carve=True map.ply holds the cloud that building without carving and applying the NumPy
restatement (tests/carve_ref.py) to the same depths and poses gives, and carve_report agrees with it. The synthetic weights give
arbitrary flows and depths: this pins files and bits, not accuracy."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carve_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402
from slam_cases import _Args, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu


def test_carve_needs_the_voxel_map(tmp_path):
    from atdn_vslam_amd.slam import NeuralSLAM
    with pytest.raises(ValueError, match="carve"):
        NeuralSLAM(_Args(str(tmp_path)), calib=SLAM_CALIB, resident_map=True, carve=True)


def test_neuralslam_carve(tmp_path):
    """Five synthetic frames, keyframes 0, 2, 4 (as the voxel map's SLAM test), fused depths. The run with carve=True differs
    from the run without in map.ply alone; map.ply and carve_report are those of the restatement."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))
    fuse = dict(fuse_depth=True, fuse_options=dict(window=1, min_views=1, max_reproj=50.0, max_rel_depth=0.5))
    options = dict(voxel=0.5, max_z=80.0, stride=2, capacity=1 << 12)
    # (the synthetic weights leave a handful of voxels, most of which no keyframe confirms: min_support makes the carving bite)
    carve = dict(min_free=1, ratio=0.0, min_support=1, radius=1, rel=0.02, batch=2)
    run = {}
    for name, kw in (("off", {}), ("on", dict(carve=True, carve_options=carve))):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(path)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, voxel_map=True,
                          voxel_options=options, **fuse, **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        slam.end_odometry(mapping_weights=vsd)
        run[name] = (slam, path, poses)
    (off, off_path, off_poses), (slam, path, poses) = run["off"], run["on"]
    assert all(torch.equal(a, b) for a, b in zip(poses, off_poses)) and off.carve_report is None
    assert _tree(path) == _tree(off_path)                                # no new file or directory
    for f in _tree(path):
        if not f.endswith("/") and f != "map.ply":                       # every other file, byte for byte
            assert open(os.path.join(path, f), "rb").read() == open(os.path.join(off_path, f), "rb").read(), f
    assert slam.voxel_map.counts == off.voxel_map.counts                 # the table's counters do not change
    # the restatement on the same depths and poses
    fused, _, _ = slam._map.fuse_depths(SLAM_CALIB, **fuse["fuse_options"])
    depth = fused.cpu().numpy()
    kf_poses = slam._map.poses[:3, :3, :].reshape(3, 12).numpy()
    images = slam._map.image_bank[:3].cpu().numpy()
    ref = V.RefMap(voxel=0.5, max_z=80.0)
    ref.integrate(depth, kf_poses, SLAM_CALIB, images, stride=2)
    uncarved = VoxelMap.load_ply(os.path.join(off_path, "map.ply"))
    pts, col, cnt, _ = ref.extract()
    assert V.same_bits(uncarved[0].numpy(), pts) and V.same_bits(uncarved[1].numpy(), col) and V.same_bits(uncarved[2].numpy(), cnt)
    want, _ = R.carve(ref, depth, kf_poses, SLAM_CALIB, **{k: v for k, v in carve.items() if k != "batch"})
    print("carve report", slam.carve_report)
    assert slam.carve_report == want and want["voxels"] == len(pts) and 0 < want["removed_voxels"] < want["voxels"]
    assert slam.voxel_map.removed == dict(voxels=want["removed_voxels"], points=want["removed_points"])
    pts, col, cnt, _ = ref.extract()
    carved = VoxelMap.load_ply(os.path.join(path, "map.ply"))
    assert V.same_bits(carved[0].numpy(), pts) and V.same_bits(carved[1].numpy(), col) and V.same_bits(carved[2].numpy(), cnt)
    assert len(pts) == want["voxels"] - want["removed_voxels"]
