"""NeuralSLAM(..., ground=True): the files it writes, that every other file is what it is without it, byte for byte, that
ground/%06d.pth holds what transforms.ground_plane and the host helpers give for the keyframe's stored depth, and that
poses_scaled.pth is evaluation.rescale_intervals of poses.pth and the stored scales. The synthetic weights give arbitrary flows and
depths: this pins the plumbing, not accuracy."""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import evaluation, transforms
from atdn_vslam_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args, _bits_flat as _bits, EverySecond, _files, SLAM_CALIB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# wide open: the arbitrary depths of synthetic weights should leave a plane to fit and to accept
PLANE = dict(iters=4, scale_rel=0.5, inlier_rel=0.5, min_z=1e-3, max_depth=1e6, min_votes=1, rows=(0, 376))
ACCEPT = dict(min_inlier_share=0.0, max_tilt_deg=180.0)
CAMERA_HEIGHT = 1.65


def test_neuralslam_ground(tmp_path):
    """Five synthetic frames, every second pair ends in a keyframe (frames 0, 2, 4). keyframe_depth="track" without and with the
    ground fit, and "pair" with it."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    with pytest.raises(ValueError, match="calib"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, ground=True)
    with pytest.raises(ValueError, match="camera_height"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, ground=True, camera_height=0.0)
    on = dict(ground=True, ground_options=dict(PLANE, **ACCEPT), camera_height=CAMERA_HEIGHT)
    run = {}
    for mode, kw in (("off", dict(keyframe_depth="track")), ("track", dict(keyframe_depth="track", **on)),
                     ("pair", dict(keyframe_depth="pair", **on))):
        path = os.path.join(str(tmp_path), mode)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        slam.end_odometry(mapping_weights=vsd)
        run[mode] = (path, poses)
    (off, off_poses), (track, track_poses), (pair, _) = run["off"], run["track"], run["pair"]
    # ground=True changes no pose and no existing file, byte for byte
    assert all(torch.equal(a, b) for a, b in zip(off_poses, track_poses))
    names = ["%06d.pth" % i for i in range(3)]
    assert _files(off) == ["depth/" + n for n in names[:2]] + ["poses.pth"] + ["rgb/" + n for n in names]
    assert _files(track) == sorted(_files(off) + ["ground/" + n for n in names[:2]] + ["poses_scaled.pth"])
    assert not os.path.exists(os.path.join(off, "ground"))
    for f in _files(off):
        assert open(os.path.join(off, f), "rb").read() == open(os.path.join(track, f), "rb").read(), f
    # with "pair" the depth has the scale of one pair, not of the interval: ground files, but no scaled poses
    assert _files(pair) == sorted(["depth/" + n for n in names[:2]] + ["ground/" + n for n in names[:2]] + ["poses.pth"] +
                                  ["rgb/" + n for n in names])
    for path in (track, pair):
        scales = []
        for n in names[:2]:
            g = torch.load(os.path.join(path, "ground", n))
            assert sorted(g) == ["accepted", "counts", "height", "normal", "q", "scale", "sums"]
            depth = torch.load(os.path.join(path, "depth", n))
            for d in (depth, depth.to(DEV)):                                   # the host form and the kernels: the same bits
                q, sums, counts = transforms.ground_plane(d, SLAM_CALIB, **PLANE)
                assert _bits(g["q"], q[0].cpu()) and _bits(g["sums"], sums[0].cpu()) and _bits(g["counts"], counts[0].cpu())
            normal, height = transforms.ground_height(g["q"])
            assert _bits(g["normal"], normal) and _bits(g["height"], height)
            accepted = bool(transforms.ground_accept(g["q"], g["counts"], (0.0, 1.0, 0.0), **ACCEPT))
            assert g["accepted"] is accepted and isinstance(g["scale"], float)
            assert g["scale"] == (CAMERA_HEIGHT / float(height) if accepted else 1.0)
            print(os.path.basename(path), n, "counts", g["counts"].tolist(), "height", float(height), "accepted", accepted, "scale",
                  g["scale"])
            scales.append(g["scale"])
        if path == track:
            stored = torch.load(os.path.join(path, "poses.pth"))
            scaled = torch.load(os.path.join(path, "poses_scaled.pth"))
            want = torch.from_numpy(evaluation.rescale_intervals(stored.numpy(), scales)[:, :3, :].reshape(-1, 12)).float()
            assert scaled.dtype == torch.float32 and tuple(scaled.shape) == (3, 12) and _bits(scaled, want)
            assert any(s != 1.0 for s in scales) and not _bits(scaled, stored)   # a plane was found: the scaling did something
