"""NeuralSLAM(..., keyframe_depth="multiview"): the files it writes, that they hold what FlowTrack.multiview() returns for the same
flows and poses, and that nothing "track" writes changes. The synthetic weights give arbitrary flows: this pins the plumbing,
not accuracy."""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import depth as depth_mod
from atdn_vslam_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_neuralslam_multiview_keyframe_depth(tmp_path):
    """Five synthetic frames, every second pair ends in a keyframe: keyframes are frames 0, 2, 4; keyframes 0 and 1 get a depth
    over two steps each. The thresholds are opened wide so that the arbitrary flows leave some valid pixels."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    with pytest.raises(ValueError, match='"pair", "track" or "multiview"'):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, keyframe_depth="stereo")
    with pytest.raises(ValueError, match="calib"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, keyframe_depth="multiview")
    options = dict(min_views=1, max_rel_sigma=1e3, inlier_px=1e3, scale_px=64.0, max_depth=1e6)
    run, events = {}, []
    for mode, kw in (("track", {}), ("multiview", dict(multiview_options=options))):
        path = os.path.join(str(tmp_path), mode)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, keyframe_depth=mode,
                          **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = []
        for k, f in enumerate(frames):
            poses.append(slam(f).clone())
            if k == 0 and mode == "multiview":                         # the track exists now: record what it is fed
                track = slam._depth.track
                assert track.history == 16
                start, extend = track.start, track.extend

                def rec_start():
                    events.append(("start",))
                    return start()

                def rec_extend(flow, pred_mat, mask=None):
                    events.append(("extend", flow.clone(), torch.as_tensor(pred_mat).clone()))
                    return extend(flow, pred_mat, mask)

                track.start, track.extend = rec_start, rec_extend
        slam.end_odometry(mapping_weights=vsd)
        run[mode] = (slam, path, poses)
    (ref, ref_path, ref_poses), (slam, path, poses) = run["track"], run["multiview"]
    assert all(torch.equal(a, b) for a, b in zip(poses, ref_poses)) and len(slam) == len(ref) == 3
    assert ref._depth.track.history == 0 and ref.multiview_counts is None
    names = ["%06d.pth" % i for i in range(3)]
    depth = ["depth/" + n for n in names[:2]]
    after = ["poses.pth"] + ["rgb/" + n for n in names]
    assert _tree(ref_path) == depth + after + ["depth/", "rgb/"]
    assert _tree(path) == (depth + ["depth_info/" + n for n in names[:2]] + ["depth_mv_views/" + n for n in names[:2]] + after +
                           ["depth/", "depth_info/", "depth_mv_views/", "rgb/"])
    for f in after:                                                    # poses and images, bit for bit
        a, b = torch.load(os.path.join(path, f)), torch.load(os.path.join(ref_path, f))
        assert a.dtype == b.dtype and torch.equal(a, b), f
    # the same flows and poses through a track of one's own
    assert [e[0] for e in events] == ["extend", "extend", "start", "extend", "extend", "start"]
    mine = depth_mod.FlowTrack((376, 1232), SLAM_CALIB, DEV, history=16)
    mine.start()
    want = []
    for e in events:
        if e[0] == "start":
            want.append(tuple(t.clone() for t in mine.multiview(**options)) + (mine.depth.clone(),))
            mine.start()
        else:
            mine.extend(e[1], e[2])
    assert len(want) == 2
    assert torch.equal(slam.multiview_counts, want[1][3]) and slam.multiview_counts.is_cuda and tuple(slam.multiview_counts.shape) == (1, 3)
    for i, n in enumerate(names[:2]):
        d, info, views = (torch.load(os.path.join(path, sub, n)) for sub in ("depth", "depth_info", "depth_mv_views"))
        assert d.dtype == torch.float32 and tuple(d.shape) == (1, 376, 1232) and not d.is_cuda
        assert info.dtype == torch.float32 and tuple(info.shape) == (1, 376, 1232) and not info.is_cuda
        assert views.dtype == torch.uint8 and tuple(views.shape) == (376, 1232) and not views.is_cuda
        assert torch.equal(d.view(torch.int32), want[i][0][0].cpu().view(torch.int32))
        assert torch.equal(info.view(torch.int32), want[i][1][0].cpu().view(torch.int32)) and torch.equal(views, want[i][2][0].cpu())
        assert torch.equal((d > 0), (info > 0)) and int((d > 0).sum()) == int(want[i][3][0, 2])
        print("keyframe", i, "counts", want[i][3].tolist())
        assert torch.equal(slam._map.depth_bank[i].cpu(), d[0])        # and the map holds it
        pts = slam.keyframe_points(i)
        assert pts.is_cuda and pts.dtype == torch.float32 and tuple(pts.shape) == (3, int((d > 0).sum()))
        # "track" wrote the depth of the track itself: the one the solve started from
        t = torch.load(os.path.join(ref_path, "depth", n))
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, 376, 1232)
        assert torch.equal(t.view(torch.int32), want[i][4][0].cpu().view(torch.int32))
    assert int(want[0][3][0, 2]) > 0
