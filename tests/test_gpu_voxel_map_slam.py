"""The voxel map in the keyframe map and in NeuralSLAM: KeyframeMap.voxel_map against VoxelMap.integrate called by hand and the
NumPy restatement, and NeuralSLAM(..., voxel_map=True) against the map's own call and against a run without the option."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.keyframe_map import KeyframeMap
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_map_ref as V  # noqa: E402
from slam_cases import _Args, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(cloud):
    return tuple(None if t is None else t.cpu().numpy() for t in cloud)


def test_keyframe_map_voxel_map():
    """Five keyframes at 16 x 48 out of a bank that is longer than the map: the cloud equals the restatement and a VoxelMap filled
    by hand, in one batch and in batches of two, with a stride, and from fused depths given in place of the bank."""
    H, W, N = 16, 48, 5
    s = V.scene(H, W, N, 21, special=False)
    m = KeyframeMap(DEV, hw=(H, W), capacity=2)
    P = torch.cat([torch.from_numpy(s["poses"]).view(N, 3, 4), torch.tensor([0.0, 0, 0, 1]).view(1, 1, 4).repeat(N, 1, 1)], dim=1)
    for k in range(N):
        m.append(torch.from_numpy(s["images"][k]), P[k])
    with pytest.raises(RuntimeError, match="depth"):
        m.voxel_map(s["calib"])
    for k in range(N - 1):                                             # the last keyframe never gets a depth
        m.set_depth(k, torch.from_numpy(s["depth"][k]))
    assert m.capacity > N
    depth = s["depth"].copy()
    depth[N - 1] = 0
    want, wc = V.reference(depth, s["poses"], s["calib"], s["images"])
    hand = VoxelMap(DEV, capacity=64)
    hand.integrate(torch.from_numpy(depth).to(DEV), torch.from_numpy(s["poses"]).to(DEV), s["calib"],
                   images=torch.from_numpy(s["images"]).to(DEV))
    for batch in (8, 2):
        vm = m.voxel_map(s["calib"], batch=batch, capacity=64)
        assert vm.counts == wc == hand.counts and V.same_cloud(_np(vm.extract()), want)
    assert all(torch.equal(a, b) for a, b in zip(vm.extract(), hand.extract()))
    strided = m.voxel_map(s["calib"], stride=3, voxel=0.5, min_z=1.0, max_z=30.0)
    want3, wc3 = V.reference(depth, s["poses"], s["calib"], s["images"], stride=3, voxel=0.5, min_z=1.0, max_z=30.0)
    assert strided.counts == wc3 and V.same_cloud(_np(strided.extract()), want3)
    fused = depth.copy()
    fused[:, ::2] = 0
    vf = m.voxel_map(s["calib"], fused=torch.from_numpy(fused).to(DEV))
    wantf, wcf = V.reference(fused, s["poses"], s["calib"], s["images"])
    assert vf.counts == wcf and V.same_cloud(_np(vf.extract()), wantf)
    with pytest.raises(ValueError, match="fused"):
        m.voxel_map(s["calib"], fused=torch.from_numpy(fused[:2]).to(DEV))


def test_neuralslam_voxel_map(tmp_path):
    """Five synthetic frames, every second pair ends in a keyframe: keyframes are frames 0, 2, 4; keyframes 0 and 1 get a depth.
    The synthetic weights give arbitrary flows and depths: this test pins the plumbing — which files appear, that map.ply holds
    what the map's own voxel_map returns from the fused depths, that nothing else changes — not accuracy."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    for kw in (dict(voxel_map=True), dict(voxel_map=True, calib=SLAM_CALIB), dict(voxel_map=True, resident_map=True)):
        with pytest.raises(ValueError, match="voxel_map"):
            NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, **kw)
    fuse = dict(fuse_depth=True, fuse_options=dict(window=1, min_views=1, max_reproj=50.0, max_rel_depth=0.5))
    options = dict(voxel=0.5, max_z=80.0, stride=2, capacity=1 << 12)
    run = {}
    for name, kw in (("off", {}), ("on", dict(voxel_map=True, voxel_options=options))):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(path)
        with open(os.path.join(path, "map.ply"), "w") as f:            # left by an earlier session: only the option clears it
            f.write("stale")
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, **fuse, **kw)
        assert os.path.exists(os.path.join(path, "map.ply")) == (name == "off")
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        assert slam.voxel_map is None
        slam.end_odometry(mapping_weights=vsd)
        run[name] = (slam, path, poses)
    (off, off_path, off_poses), (slam, path, poses) = run["off"], run["on"]
    assert all(torch.equal(a, b) for a, b in zip(poses, off_poses)) and len(slam) == len(off) == 3
    assert off.voxel_map is None and open(os.path.join(off_path, "map.ply")).read() == "stale"
    assert _tree(path) == _tree(off_path)                              # the option adds map.ply and nothing else
    for f in _tree(path):
        if f.endswith(".pth"):                                         # every other file, bit for bit
            a, b = torch.load(os.path.join(path, f)), torch.load(os.path.join(off_path, f))
            assert a.dtype == b.dtype and torch.equal(a, b), f
    # the contents are the map's own call on the fused depths (the bank was not replaced, so the fusion can be repeated)
    fused, _, _ = slam._map.fuse_depths(SLAM_CALIB, **fuse["fuse_options"])
    by_hand = slam._map.voxel_map(SLAM_CALIB, fused=fused, **options)
    print("voxel map counts", slam.voxel_map.counts)
    assert isinstance(slam.voxel_map, VoxelMap) and slam.voxel_map.counts == by_hand.counts
    assert slam.voxel_map.counts["dropped"] == 0 and slam.voxel_map.counts["candidates"] > 0
    cloud = by_hand.extract()
    lp, lc, ln = VoxelMap.load_ply(os.path.join(path, "map.ply"))
    assert len(lp) == slam.voxel_map.counts["voxels"] > 0
    assert torch.equal(lp.view(torch.int32), cloud[0].cpu().view(torch.int32)) and torch.equal(lc, cloud[1].cpu())
    assert torch.equal(ln, cloud[2].cpu())
    raw = open(os.path.join(path, "map.ply"), "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                          b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int count\n"
                          b"end_header\n" % len(lp))
    # on demand in relocalisation mode: the same file; with other options another one
    os.remove(os.path.join(path, "map.ply"))
    again = slam.build_voxel_map(**options)
    assert again is slam.voxel_map and open(os.path.join(path, "map.ply"), "rb").read() == raw
    n3 = slam.build_voxel_map(min_count=3, **options).counts
    assert n3 == by_hand.counts and len(VoxelMap.load_ply(os.path.join(path, "map.ply"))[0]) == int((cloud[2] >= 3).sum())
    # an object without the option builds from the depth bank on demand
    unfused = off.build_voxel_map(**options)
    hand = off._map.voxel_map(SLAM_CALIB, **options)
    assert unfused.counts == hand.counts and all(torch.equal(a, b) for a, b in zip(unfused.extract(), hand.extract()))
    assert unfused.counts["candidates"] >= slam.voxel_map.counts["candidates"]
