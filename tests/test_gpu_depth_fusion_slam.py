"""Keyframe depth fusion in the keyframe map and in NeuralSLAM: KeyframeMap.fuse_depths against transforms.fuse_depths called by
hand, and NeuralSLAM(..., fuse_depth=True) against the map's own call and against a run without the option."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms
from atdn_vslam_amd.keyframe_map import KeyframeMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_fusion_ref import check_reference, scene  # noqa: E402
from slam_cases import _Args, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _map_of(bank, poses, capacity=2):
    N, H, W = bank.shape
    m = KeyframeMap(DEV, hw=(H, W), capacity=capacity)                 # grows on the way
    P = torch.cat([torch.from_numpy(poses).view(N, 3, 4), torch.tensor([0.0, 0, 0, 1]).view(1, 1, 4).repeat(N, 1, 1)], dim=1)
    for k in range(N):
        m.append(torch.zeros(3, H, W, dtype=torch.uint8), P[k])
    return m


def test_keyframe_map_fuse_depths():
    """Five keyframes at 16 x 48 filled with the helper's scene. The result equals transforms.fuse_depths called by hand (and the
    helper) bit for bit, in one batch and in batches of two; the default windows at the ends of the map hold empty slots;
    replace=True swaps the fused depths in, and a second call then differs from the first."""
    H, W, N = 16, 48, 5
    bank, poses, calib, _ = scene(H, W, N, 1)
    m = _map_of(bank, poses)
    with pytest.raises(RuntimeError, match="depth"):
        m.fuse_depths(calib)
    for k in range(N):
        m.set_depth(k, torch.from_numpy(bank[k]))
    assert m.capacity > N                                              # the bank is longer than the map: only its first n planes count
    window = [[-1, -1, 1, 2], [-1, 0, 2, 3], [0, 1, 3, 4], [1, 2, 4, -1], [2, 3, -1, -1]]
    want = check_reference(bank, poses, list(range(N)), window, calib)
    by_hand = transforms.fuse_depths(m.depth_bank[:N], m.poses.to(DEV), list(range(N)), window, calib)
    for batch in (16, 2):
        fused, views, counts = m.fuse_depths(calib, batch=batch)
        assert fused.is_cuda and tuple(fused.shape) == (N, H, W) and tuple(views.shape) == (N, H, W) and tuple(counts.shape) == (N, 3)
        assert torch.equal(fused.view(torch.int32), by_hand[0][:, 0].view(torch.int32))
        assert torch.equal(views, by_hand[1]) and torch.equal(counts, by_hand[2])
        assert np.array_equal(fused.cpu().numpy().view(np.uint32), want[0][:, 0].view(np.uint32))
        assert np.array_equal(views.cpu().numpy(), want[1]) and np.array_equal(counts.cpu().numpy(), want[2])
    assert torch.equal(m.depth_bank[:N].cpu(), torch.from_numpy(bank))    # nothing was written into the bank
    # window = 1, explicit sources, thresholds passed through
    one = m.fuse_depths(calib, window=1, min_views=1, average=False)
    hand = transforms.fuse_depths(m.depth_bank[:N], m.poses.to(DEV), list(range(N)), [[-1, 1], [0, 2], [1, 3], [2, 4], [3, -1]], calib,
                                  min_views=1, average=False)
    assert torch.equal(one[0], hand[0][:, 0]) and torch.equal(one[1], hand[1]) and torch.equal(one[2], hand[2])
    far = m.fuse_depths(calib, sources=[[4], [3], [0], [1], [0]], min_views=1)
    hand = transforms.fuse_depths(m.depth_bank[:N], m.poses.to(DEV), list(range(N)), [[4], [3], [0], [1], [0]], calib, min_views=1)
    assert torch.equal(far[0], hand[0][:, 0]) and torch.equal(far[2], hand[2])
    with pytest.raises(ValueError):
        m.fuse_depths(calib, sources=[[1, 2]])
    # replace: Jacobi (every target saw the unfused bank), then the bank holds the fused depths
    first = m.fuse_depths(calib, replace=True)
    assert torch.equal(first[0].view(torch.int32), by_hand[0][:, 0].view(torch.int32)) and torch.equal(first[2], by_hand[2])
    assert torch.equal(m.depth_bank[:N], first[0])
    second = m.fuse_depths(calib)
    assert not torch.equal(second[0], first[0]) and not torch.equal(second[2], first[2])
    assert (second[2][:, 0] == first[2][:, 2]).all()                   # what was kept is what now has a depth


def test_neuralslam_fuse_depth(tmp_path):
    """Five synthetic frames, every second pair ends in a keyframe: keyframes are frames 0, 2, 4; keyframes 0 and 1 get a depth.
    The synthetic weights give arbitrary flows, so the depths hardly agree: this test pins the plumbing — which files appear,
    that they hold what the map's own fuse_depths returns, that nothing else changes — not accuracy."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    for kw in (dict(fuse_depth=True), dict(fuse_depth=True, calib=SLAM_CALIB), dict(fuse_depth=True, resident_map=True)):
        with pytest.raises(ValueError, match="fuse_depth"):
            NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, **kw)
    options = dict(window=1, min_views=1, max_reproj=50.0, max_rel_depth=0.5)
    run = {}
    for name, kw in (("off", {}), ("on", dict(fuse_depth=True, fuse_options=options))):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(os.path.join(path, "depth_fused"))
        open(os.path.join(path, "depth_fused", "000009.pth"), "w").close()   # left by an earlier session: only the option clears it
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        assert slam.fusion_counts is None
        slam.end_odometry(mapping_weights=vsd)
        run[name] = (slam, path, poses)
    (off, off_path, off_poses), (slam, path, poses) = run["off"], run["on"]
    assert all(torch.equal(a, b) for a, b in zip(poses, off_poses)) and len(slam) == len(off) == 3
    assert off.fusion_counts is None
    names = ["%06d.pth" % i for i in range(3)]
    before = ["depth/000000.pth", "depth/000001.pth"]
    after = ["poses.pth"] + ["rgb/" + n for n in names]
    assert _tree(off_path) == before + ["depth_fused/000009.pth"] + after + ["depth/", "depth_fused/", "rgb/"]
    assert _tree(path) == (before + ["depth_fused/" + n for n in names] + ["depth_views/" + n for n in names] + after +
                           ["depth/", "depth_fused/", "depth_views/", "rgb/"])
    for f in before + after:                                           # every pre-existing file, bit for bit
        a, b = torch.load(os.path.join(path, f)), torch.load(os.path.join(off_path, f))
        assert a.dtype == b.dtype and torch.equal(a, b), f
    # the contents are the map's own call (the bank was not replaced, so it can be repeated)
    fused, views, counts = slam._map.fuse_depths(SLAM_CALIB, **options)
    assert torch.equal(slam.fusion_counts, counts.cpu()) and slam.fusion_counts.dtype == torch.int32 and not slam.fusion_counts.is_cuda
    print("fusion counts", slam.fusion_counts.tolist())
    assert slam.fusion_counts[2].tolist() == [0, 0, 0]                 # keyframe 2 never got a depth
    for i, n in enumerate(names):
        f, v = torch.load(os.path.join(path, "depth_fused", n)), torch.load(os.path.join(path, "depth_views", n))
        assert f.dtype == torch.float32 and tuple(f.shape) == (1, 376, 1232) and not f.is_cuda
        assert v.dtype == torch.uint8 and tuple(v.shape) == (376, 1232) and not v.is_cuda
        assert torch.equal(f[0].view(torch.int32), fused[i].cpu().view(torch.int32)) and torch.equal(v, views[i].cpu())
        assert int((f != 0).sum()) == int(counts[i, 2])
        pts = slam.keyframe_points(i, fused=True)
        assert pts.is_cuda and pts.dtype == torch.float32 and tuple(pts.shape) == (3, int(counts[i, 2]))
        if i < 2:
            assert torch.equal(slam.keyframe_points(i, fused=False), slam.keyframe_points(i))
            # the fused points are those of the same depth through the unfused door
            torch.save(f, os.path.join(off_path, "depth", n))
            assert torch.equal(pts, off.keyframe_points(i))
    # a second explicit call with replace: the bank now holds the fused depths
    again = slam.fuse_depths(replace=True, **options)
    assert torch.equal(again, slam.fusion_counts) and torch.equal(slam._map.depth_bank[:3], fused)
