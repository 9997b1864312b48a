"""NeuralSLAM(..., keyframe_depth="bundle"): the files it writes, that they hold what FlowTrack.bundle() returns for the same flows
and poses, that the trajectory is that of "multiview" bit for bit unless bundle_pose=True, and what bundle_pose=True stores. The
synthetic weights give arbitrary flows: this pins the plumbing, not accuracy."""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import depth as depth_mod
from atdn_vslam_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args, _bits, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_neuralslam_bundle_keyframe_depth(tmp_path):
    """Five synthetic frames, every second pair ends in a keyframe: keyframes are frames 0, 2, 4; keyframes 0 and 1 get a window
    of two steps each. The thresholds are opened wide so that the arbitrary flows leave some candidates."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    with pytest.raises(ValueError, match="calib"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, keyframe_depth="bundle")
    mv = dict(min_views=1, max_rel_sigma=1e3, inlier_px=1e3, scale_px=64.0, max_depth=1e6)
    ba = dict(min_views=1, stride=4, iters=3, scale_px=64.0, inlier_px=1e3)
    run, events = {}, []
    for mode, kd, kw in (("multiview", "multiview", {}), ("bundle", "bundle", dict(bundle_options=ba)),
                         ("bundle_pose", "bundle", dict(bundle_options=ba, bundle_pose=True))):
        path = os.path.join(str(tmp_path), mode)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, keyframe_depth=kd,
                          multiview_options=mv, **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = []
        for k, f in enumerate(frames):
            poses.append(slam(f).clone())
            if k == 0 and mode == "bundle":                            # the track exists now: record what it is fed
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
    (ref, ref_path, ref_poses), (slam, path, poses), (slam_p, path_p, poses_p) = run["multiview"], run["bundle"], run["bundle_pose"]
    # bundle_pose=False: the trajectory of "multiview", bit for bit
    assert all(torch.equal(a, b) for a, b in zip(poses, ref_poses)) and len(slam) == len(ref) == len(slam_p) == 3
    assert ref.bundle_cost is None and ref.bundle_counts is None
    names = ["%06d.pth" % i for i in range(3)]
    shared = ["depth/" + n for n in names[:2]] + ["depth_info/" + n for n in names[:2]] + ["depth_mv_views/" + n for n in names[:2]]
    after = ["poses.pth"] + ["rgb/" + n for n in names]
    assert _tree(ref_path) == shared + after + ["depth/", "depth_info/", "depth_mv_views/", "rgb/"]
    want_tree = sorted(shared + after + ["bundle/" + n for n in names[:2]]) + ["bundle/", "depth/", "depth_info/", "depth_mv_views/", "rgb/"]
    assert _tree(path) == want_tree and _tree(path_p) == want_tree
    for f in after:
        assert _bits(torch.load(os.path.join(path, f)), torch.load(os.path.join(ref_path, f))), f
    # the same flows and poses through a track of one's own
    assert [e[0] for e in events] == ["extend", "extend", "start", "extend", "extend", "start"]
    mine = depth_mod.FlowTrack((376, 1232), SLAM_CALIB, DEV, history=16)
    mine.start()
    want = []
    for e in events:
        if e[0] == "start":
            want.append(tuple(t.clone() for t in mine.bundle(multiview_options=mv, **ba)))
            mine.start()
        else:
            mine.extend(e[1], e[2])
    assert len(want) == 2
    assert _bits(slam.bundle_cost, want[1][5]) and _bits(slam.bundle_counts, want[1][6]) and _bits(slam.multiview_counts, want[1][4])
    assert slam.bundle_cost.is_cuda and tuple(slam.bundle_cost.shape) == (1, 2) and tuple(slam.bundle_counts.shape) == (1, 4)
    for i, n in enumerate(names[:2]):
        d, info, views, b = (torch.load(os.path.join(path, sub, n)) for sub in ("depth", "depth_info", "depth_mv_views", "bundle"))
        assert _bits(d, want[i][1][0].cpu()) and _bits(info, want[i][2][0].cpu()) and _bits(views, want[i][3][0].cpu())
        assert sorted(b) == ["cost", "counts", "poses"]
        assert _bits(b["poses"], want[i][0][0].cpu()) and tuple(b["poses"].shape) == (2, 12) and b["poses"].dtype == torch.float32
        assert _bits(b["cost"], want[i][5][0].cpu()) and _bits(b["counts"], want[i][6][0].cpu())
        assert int(b["counts"][0]) > 0
        print("keyframe", i, "bundle counts", b["counts"].tolist(), "cost", b["cost"].tolist())
        assert _bits(slam._map.depth_bank[i].cpu(), d[0])
        # the pose does not feed back into the flows or the head: the bundle_pose run solved the same windows
        bp = torch.load(os.path.join(path_p, "bundle", n))
        assert all(_bits(bp[k], b[k]) for k in b)
    # bundle_pose=True: keyframe i + 1 stands at (keyframe i's pose @ refined last pose), float64 product stored as float32
    assert torch.equal(slam_p[0].pose, ref[0].pose) and torch.equal(poses_p[1], ref_poses[1])
    for i in range(2):
        last = torch.eye(4, dtype=torch.float64)
        last[:3] = torch.load(os.path.join(path_p, "bundle", names[i]))["poses"][-1].reshape(3, 4).double()
        expect = (slam_p[i].pose.double() @ last).float()
        assert _bits(slam_p[i + 1].pose, expect) and _bits(poses_p[2 * i + 2], expect)
        assert _bits(slam_p._map.poses[i + 1], expect)
    assert _bits(torch.load(os.path.join(path_p, "poses.pth")), torch.stack([slam_p[i].pose.flatten()[:12] for i in range(3)]))
