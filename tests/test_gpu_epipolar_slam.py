"""The refine_pose option of VisualOdometry and NeuralSLAM: what they keep equals transforms.pose_from_flow and
transforms.two_view_depth called by hand on the same flow and the same predicted pose, and with refine_pose=False nothing moves.
Synthetic weights: the flows are noise and the refined poses mean nothing, but every relation below is exact."""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import depth as depth_mod
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW = (376, 1232)
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (376, 1232))


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


@pytest.fixture(scope="module")
def hsd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def frames():
    return torch.from_numpy(syn.make_frames(4, 376, 1241, seed=8))


class _Spy:
    """Records the arguments and the results of transforms.transform, pose_from_flow and two_view_depth, which go on working."""

    def __init__(self, monkeypatch):
        self.transform, self.refine, self.depth = [], [], []
        real_t, real_r, real_d = transforms.transform, transforms.pose_from_flow, transforms.two_view_depth

        def transform(rot, tr):
            out = real_t(rot, tr)
            self.transform.append(out.clone())
            return out

        def pose_from_flow(flow, pose_init, calib, *a, **kw):
            assert not a and not kw                                   # the defaults of transforms.pose_from_flow
            out = real_r(flow, pose_init, calib)
            self.refine.append((flow.clone(), pose_init.clone(), calib, tuple(t.clone() for t in out)))
            return out

        def two_view_depth(flow, pose, calib, *a, **kw):
            out = real_d(flow, pose, calib, *a, **kw)
            self.depth.append((flow.clone(), torch.as_tensor(pose).clone(), tuple(t.clone() for t in out)))
            return out

        self.real_refine, self.real_depth = real_r, real_d
        monkeypatch.setattr(transforms, "transform", transform)
        monkeypatch.setattr(transforms, "pose_from_flow", pose_from_flow)
        monkeypatch.setattr(transforms, "two_view_depth", two_view_depth)


def _pose44(rows12):
    step = torch.eye(4, dtype=torch.float32)
    step[:3] = rows12.reshape(3, 4).cpu()
    return step


def test_visual_odometry_refines_every_pair(gsd, hsd, frames, monkeypatch):
    from atdn_vslam_amd.pipeline import VisualOdometry
    with pytest.raises(ValueError, match="calib"):
        VisualOdometry(gsd, hsd, device=DEV, refine_pose=True)
    plain = VisualOdometry(gsd, hsd, device=DEV, calib=CALIB)
    want = [(plain(f).clone(), plain.last_depth, plain.last_counts) for f in frames[:3]]
    spy = _Spy(monkeypatch)
    off = VisualOdometry(gsd, hsd, device=DEV, calib=CALIB, refine_pose=False)
    for f, (pose, depth, counts) in zip(frames[:3], want):
        assert torch.equal(off(f), pose) and off.last_refine_counts is None
        assert (depth is None and off.last_depth is None) or (torch.equal(off.last_depth, depth) and torch.equal(off.last_counts, counts))
    assert not spy.refine and len(spy.depth) == 2
    spy.transform.clear()
    spy.depth.clear()
    vo = VisualOdometry(gsd, hsd, device=DEV, calib=CALIB, refine_pose=True)
    prev = vo(frames[0]).clone()
    assert vo.last_refine_counts is None and torch.equal(prev, torch.eye(4))
    for k in (1, 2):
        got = vo(frames[k]).clone()
        assert len(spy.refine) == k and len(spy.depth) == k and len(spy.transform) == k
        flow, init, calib, (pose, cost, counts) = spy.refine[-1]
        assert calib == vo.calib and torch.equal(init.cpu(), spy.transform[-1][:3].reshape(1, 12))      # the head's pose goes in
        by_hand = spy.real_refine(flow, init, CALIB)
        assert all(torch.equal(x, y) for x, y in zip(by_hand, (pose, cost, counts)))
        depth, dcounts = spy.real_depth(flow, by_hand[0], CALIB)
        assert torch.equal(spy.depth[-1][0], flow) and torch.equal(spy.depth[-1][1], pose)
        assert torch.equal(vo.last_depth, depth) and torch.equal(vo.last_counts, dcounts)
        assert vo.last_refine_counts.is_cuda and torch.equal(vo.last_refine_counts, counts)
        assert torch.equal(got, prev @ pose[0].cpu())
        assert torch.equal(pose[0, 3].cpu(), torch.tensor([0.0, 0.0, 0.0, 1.0]))
        prev = got
        print("pair", k, "refine counts", counts.tolist(), "two-view counts", dcounts.tolist())
    vo.reset()
    assert vo.last_refine_counts is None


@pytest.mark.parametrize("mode", ["pair", "track"])
def test_neural_slam_refines_every_pair(gsd, hsd, frames, tmp_path, monkeypatch, mode):
    """Four frames, every second pair ends in a keyframe. refine_pose=False equals the default run bit for bit (poses and depth
    files); refine_pose=True feeds the refined pose to the running pose, the keyframe depth of the pair and the flow track."""
    from atdn_vslam_amd.depth import FlowTrack
    from atdn_vslam_amd.slam import KeyframePolicy, NeuralSLAM

    class EverySecond(KeyframePolicy):
        def __init__(self):
            super().__init__()
            self.calls, self.seen = 0, []

        def __call__(self, pred_mat):
            self.calls += 1
            self.seen.append(torch.as_tensor(pred_mat).clone())
            return self.calls % 2 == 0

    def session(name, **kw):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(path)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, resident_map=True, calib=CALIB, keyframe_depth=mode,
                          **kw)
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        slam._record_depth(slam._depth.close())
        files = sorted(os.listdir(os.path.join(path, "depth")))
        return slam, poses, [torch.load(os.path.join(path, "depth", f)) for f in files]

    with pytest.raises(ValueError, match="calib"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, refine_pose=True)
    _, want_poses, want_depths = session("default")
    spy = _Spy(monkeypatch)
    extended = []
    real_extend = FlowTrack.extend

    def extend(self, flow, pred_mat, mask=None):
        extended.append((flow.clone(), torch.as_tensor(pred_mat).clone()))
        return real_extend(self, flow, pred_mat, mask)

    monkeypatch.setattr(FlowTrack, "extend", extend)
    off, poses, depths = session("off", refine_pose=False)
    assert not spy.refine and off.last_refine_counts is None
    assert all(torch.equal(x, y) for x, y in zip(poses, want_poses))
    assert len(depths) == len(want_depths) > 0 and all(torch.equal(x, y) for x, y in zip(depths, want_depths))
    spy.transform.clear()
    spy.depth.clear()
    extended.clear()
    slam, poses, depths = session("on", refine_pose=True)
    assert len(spy.refine) == 3 and len(spy.transform) == 3 and torch.equal(poses[0], torch.eye(4))
    refined = []
    for k, (flow, init, calib, out) in enumerate(spy.refine):
        assert torch.equal(init.cpu(), spy.transform[k][None])
        by_hand = spy.real_refine(flow, init, CALIB)
        assert all(torch.equal(x, y) for x, y in zip(by_hand, out))
        refined.append(by_hand[0][0].cpu())
        assert torch.equal(poses[k + 1], poses[k] @ refined[k])
        assert torch.equal(slam._policy.seen[k], refined[k])
    assert slam.last_refine_counts.is_cuda and torch.equal(slam.last_refine_counts, spy.refine[-1][3][2])
    if mode == "pair":
        # keyframe 0 gets the depth of pair 0, keyframe 1 (registered by pair 1) that of pair 2
        assert len(spy.depth) == 2 and len(depths) == 2 and not extended
        for (flow, pose, _), k, stored in zip(spy.depth, (0, 2), depths):
            assert torch.equal(flow, spy.refine[k][0]) and torch.equal(pose.cpu(), refined[k][None])
            depth, _ = spy.real_depth(flow, refined[k][None].to(DEV), CALIB)
            assert torch.equal(stored, depth[0].cpu()) and torch.equal(slam._map.depth_bank[len(spy.depth) - 1 if k else 0].cpu(), stored[0])
    else:
        assert len(extended) == 3 and len(depths) == 2
        for k, (flow, pred) in enumerate(extended):
            assert torch.equal(flow, spy.refine[k][0]) and torch.equal(pred, refined[k])
        # the track of keyframe 0 by hand: two steps with the refined poses
        track = FlowTrack(HW, CALIB, DEV)
        track.start()
        for k in (0, 1):
            real_extend(track, extended[k][0], refined[k])
        assert torch.equal(depths[0], track.depth[0].cpu())
    print(mode, "refine counts", [r[3][2].tolist() for r in spy.refine])
