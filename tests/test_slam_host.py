"""Host logic of the NeuralSLAM drop-in that needs no GPU: keyframe policy, file layout helpers and the option rules of the
constructor, which come before anything touches a device or the directory."""
import os
import types

import numpy as np
import pytest
import torch

from atdn_vslam_amd import transforms
from atdn_vslam_amd.slam import Frame, KeyframePolicy, NeuralSLAM, _homogeneous


def test_keyframe_policy_matches_reference(golden_dir):
    """NeuralSLAM.__decide_keyframe of the imported reference on a scripted motion sequence (keyframes.npz)."""
    g = np.load(os.path.join(golden_dir, "keyframes.npz"))
    policy = KeyframePolicy()
    got = [policy(transforms.transform(torch.from_numpy(r), torch.from_numpy(t))) for r, t in zip(g["rots"], g["trs"])]
    assert np.array_equal(np.array(got, dtype=np.uint8), g["decisions"])
    assert 0 < sum(got) < len(got)


def test_keyframe_policy_thresholds():
    p = KeyframePolicy()
    step = transforms.transform(torch.zeros(3), torch.tensor([0.0, 0.0, 4.0]))
    assert [p(step) for _ in range(4)] == [False, False, False, True]   # 16 m > 15 m on the 4th step, then reset
    assert [p(step) for _ in range(3)] == [False, False, False]
    p = KeyframePolicy()
    turn = transforms.transform(torch.tensor([0.06, 0.0, 0.0]), torch.zeros(3))
    assert [p(turn) for _ in range(3)] == [False, False, True]          # 0.18 rad > 10 degrees = 0.1745 rad


def test_pose_file_layout_round_trip():
    poses = [transforms.transform(torch.tensor([0.1 * i, 0.0, 0.05]), torch.tensor([1.0 * i, 0.0, 2.0])) for i in range(4)]
    rows = torch.stack([p.flatten()[:12] for p in poses])            # what end_odometry writes (neural_slam.py:149-153)
    back = _homogeneous(rows)
    assert back.shape == (4, 4, 4)
    for a, b in zip(back, poses):
        assert torch.equal(a, b)
    f = Frame("x.pth", poses[1])
    assert f.embedding is None and f.rgb_file_name == "x.pth"


# ------------------------------------------------------------------ the option rules, through NeuralSLAM(...) itself
CALIB = (700.0, 700.0, 600.0, 180.0)

# in the order the constructor checks them: (name, keyword arguments that break this rule alone, what the message says)
RULES = [
    ("voxel_map", dict(voxel_map=True), "voxel_map=True needs the calibration and the keyframe map"),
    ("map_depth value", dict(map_depth="x", voxel_map=True, calib=CALIB, resident_map=True), 'map_depth is False, True or "fill", got \'x\''),
    ("map_depth needs voxel_map", dict(map_depth=True), "map_depth needs the voxel map: pass voxel_map=True"),
    ("ground needs calib", dict(ground=True), "ground=True needs the calibration: pass calib="),
    ("camera_height", dict(ground=True, calib=CALIB, camera_height=0.0), "camera_height must be finite and > 0, got 0.0"),
    ("fuse_depth", dict(fuse_depth=True), "fuse_depth=True needs the calibration and the keyframe map"),
    ("refine_pose", dict(refine_pose=True), "refine_pose=True needs the calibration: pass calib="),
    ("loop_closure", dict(loop_closure=True), "loop_closure=True needs the keyframe map in device memory: pass resident_map=True"),
    ("keyframe_depth value", dict(keyframe_depth="x", calib=CALIB), 'keyframe_depth is "pair", "track" or "multiview", or "bundle", got \'x\''),
    ("keyframe_depth needs calib", dict(keyframe_depth="track"), 'keyframe_depth="track" needs the calibration: pass calib='),
]
# both rules of each adjacent pair broken in one call: the first one's message
PAIRS = [
    dict(voxel_map=True, map_depth="x"),
    dict(map_depth="x"),                                            # not a value, and no voxel map either
    dict(map_depth=True, ground=True),
    dict(ground=True, camera_height=0.0),
    dict(ground=True, calib=CALIB, camera_height=0.0, fuse_depth=True),
    dict(fuse_depth=True, refine_pose=True),
    dict(refine_pose=True, loop_closure=True),
    dict(loop_closure=True, keyframe_depth="x"),
    dict(keyframe_depth="x"),                                       # not a value, and not "pair" without a calibration
]


def _construct(tmp_path, **kw):
    root = os.path.join(str(tmp_path), "kf")
    try:
        NeuralSLAM(types.SimpleNamespace(device="cuda:0", keyframes_path=root), **kw)
    finally:
        assert not os.path.exists(root)                             # a refused option set has not touched the directory


@pytest.mark.parametrize("name,kw,message", RULES, ids=[r[0] for r in RULES])
def test_every_rule_raises_its_message(tmp_path, name, kw, message):
    with pytest.raises(ValueError) as e:
        _construct(tmp_path, **kw)
    assert message in str(e.value)


@pytest.mark.parametrize("k", range(len(PAIRS)), ids=["%s > %s" % (RULES[k][0], RULES[k + 1][0]) for k in range(len(PAIRS))])
def test_the_earlier_rule_speaks(tmp_path, k):
    with pytest.raises(ValueError) as e:
        _construct(tmp_path, **PAIRS[k])
    first, second = RULES[k][2], RULES[k + 1][2]
    assert first in str(e.value) and second.split(":")[0] not in str(e.value)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_camera_height_values(tmp_path, bad):
    with pytest.raises(ValueError, match="camera_height must be finite and > 0"):
        _construct(tmp_path, ground=True, calib=CALIB, camera_height=bad)


@pytest.mark.parametrize("mode", ["track", "multiview", "bundle"])
def test_every_track_mode_needs_the_calibration(tmp_path, mode):
    with pytest.raises(ValueError) as e:
        _construct(tmp_path, keyframe_depth=mode)
    assert 'keyframe_depth="%s" needs the calibration' % mode in str(e.value)
