"""Flow track on the GPU: the kernel (atdn_flow_track_step, csrc/flow_track.hip) against the NumPy float64 restatement of the rule
(tests/flow_track_ref.py) and against the library's host form — every bit of acc, alive and depth and every count, exactly, at every
step —, guard values around every output with every buffer at every alignment, a side stream, a captured graph, in place against
out of place, depth.FlowTrack against the same steps by hand, and NeuralSLAM(keyframe_depth="track") on a short synthetic drive."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, depth as depth_mod, synthetic as syn, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_track_ref as R  # noqa: E402
from flow_track_ref import CASES, FULL_CASE, MIN_MARGIN, same_bits, same_steps  # noqa: E402
from slam_cases import _Args, SLAM_CALIB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _n(t):
    return None if t is None else t.cpu().numpy()


def gpu_step(flow, mask, acc, alive, pose, calib, depth, **kw):
    a, l, d, c = transforms.flow_track_step(_dev(flow), _dev(acc), _dev(alive), pose=_dev(pose), calib=calib, mask=_dev(mask),
                                            depth=_dev(depth), **kw)
    torch.cuda.synchronize()
    assert a.is_cuda and l.is_cuda and c.is_cuda and a.dtype == torch.float32 and l.dtype == torch.uint8 and c.dtype == torch.int32
    assert (d is None) == (pose is None)
    return _n(a), _n(l), _n(d), _n(c)


def host_step(flow, mask, acc, alive, pose, calib, depth, **kw):
    a, l, d, c = transforms.flow_track_step(_t(flow), _t(acc), _t(alive), pose=_t(pose), calib=calib, mask=_t(mask),
                                            depth=None if depth is None else _t(depth.copy()), **kw)
    return _n(a), _n(l), _n(d), _n(c)


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, B = 2 sequence of two steps and its reference, computed once."""
    _, H, W, B, seed = FULL_CASE
    flows, poses, masks, calib = R.sequence(H, W, B, seed, steps=2)
    ref, margin = R.reference_sequence(flows, poses, masks, calib)
    assert margin >= MIN_MARGIN, margin
    return flows, poses, masks, calib, ref


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("name,H,W,B,seed", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_helper_and_the_host_form(name, H, W, B, seed, masked):
    """5 x 7 (one workgroup, a ragged last quad); 9 x 33, B = 3 (H * W = 297 is odd: the alive planes of b = 1, 2 start at
    addresses 1 and 2 mod 4, so their quads are cut off the index grid and every float access of them is scalar); 8 x 16, B = 2
    (everything aligned, no tail); 47 x 154, B = 2 (8 workgroups, H * W = 2 mod 4). Four steps, full form and chain-only form."""
    flows, poses, masks, calib = R.sequence(H, W, B, seed)
    for p in (poses, None):
        seq = dict(flows=flows, poses=p, masks=masks if masked else None, calib=calib if p is not None else None, init=None)
        ref, margin = R.reference_sequence(flows, p, seq["masks"], calib)
        assert margin >= MIN_MARGIN
        got = R.run_sequence(gpu_step, seq)
        assert same_steps(got, ref), name
        assert same_steps(got, R.run_sequence(host_step, seq)), name


def test_kernel_at_full_size(full_size):
    """376 x 1232, B = 2, two steps with a mask: 453 workgroups per image."""
    flows, poses, masks, calib, ref = full_size
    got = R.run_sequence(gpu_step, dict(flows=flows, poses=poses, masks=masks, calib=calib, init=None))
    assert same_steps(got, ref)
    c = ref[1][3]
    assert (0 < c[:, 3]).all() and (c[:, 3] < c[:, 2]).all() and (c[:, 2] < c[:, 1]).all() and (c[:, 1] <= c[:, 0]).all()


def test_kernel_equals_the_host_form_on_closed_forms_and_non_finite_values():
    for name, seq in R.special_sequences().items():
        got = R.run_sequence(gpu_step, seq)
        assert same_steps(got, R.run_sequence(host_step, seq)), name
        assert same_steps(got, R.run_sequence(R.helper_step, seq)), name


def test_kernel_outputs_are_fully_written():
    """Pre-filled output buffers with guard values around them; over the four rounds every buffer, input and output, stands at
    every one of its four alignments (floats 0, 4, 8, 12 bytes off the 16-byte grid, bytes 0 .. 3 off the dword grid), in mixed
    combinations. 8 x 16, B = 2 (aligned planes: the shifts alone decide) and 9 x 33, B = 3. Dead pixels' acc_out is the input's."""
    L = _lib.lib()
    for H, W, B, seed in ((8, 16, 2, 4), (9, 33, 3, 3)):
        flows, poses, masks, calib = R.sequence(H, W, B, seed)
        ref, _ = R.reference_sequence(flows, poses, masks, calib)
        acc0, alive0, depth0, _ = ref[1]
        want = ref[2]
        chain = R.reference_step(flows[2], masks[2], acc0, alive0)
        n = B * H * W

        def shifted(values, dtype, shift):
            buf = torch.zeros(values.size + 8, dtype=dtype, device=DEV)
            buf[shift:shift + values.size] = _dev(values).reshape(-1)
            return buf, C.c_void_p(buf[shift:].data_ptr())

        for s in range(4):
            keep = [shifted(flows[2], torch.float32, s), shifted(masks[2], torch.uint8, (s + 1) % 4),
                    shifted(acc0, torch.float32, (s + 2) % 4), shifted(alive0, torch.uint8, (s + 3) % 4)]
            dpose = _dev(poses[2])
            so = {"acc": (s + 1) % 4, "alive": s, "depth": (s + 3) % 4}
            for full in (True, False):
                a_out = torch.full((2 * n + 32,), -7.0, dtype=torch.float32, device=DEV)
                l_out = torch.full((n + 32,), 77, dtype=torch.uint8, device=DEV)
                d_io = torch.full((n + 32,), -7.0, dtype=torch.float32, device=DEV)
                d_io[16 + so["depth"]:16 + so["depth"] + n] = _dev(depth0).reshape(-1)
                cnt = torch.full((4 * B + 2,), -7, dtype=torch.int32, device=DEV)
                _lib.check(L.atdn_flow_track_step(
                    keep[0][1], keep[1][1], keep[2][1], keep[3][1], B, H, W, C.c_void_p(a_out[16 + so["acc"]:].data_ptr()),
                    C.c_void_p(l_out[16 + so["alive"]:].data_ptr()), C.c_void_p(dpose.data_ptr()) if full else None, *calib, 1.0,
                    R.min_sin2_of(0.05), 80.0, C.c_void_p(d_io[16 + so["depth"]:].data_ptr()) if full else None,
                    C.c_void_p(cnt[1:].data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                tag = (H, W, s, full)
                w_acc, w_alive, w_depth, w_counts = want if full else (chain[0], chain[1], depth0, chain[3])
                for name, buf, count, w, guard in (("acc", a_out, 2 * n, w_acc, -7.0), ("alive", l_out, n, w_alive, 77),
                                                   ("depth", d_io, n, w_depth, -7.0)):
                    o, lo = buf.cpu().numpy(), 16 + so[name]
                    assert (o[:lo] == guard).all() and (o[lo + count:] == guard).all(), tag + (name,)
                    assert same_bits(o[lo:lo + count].reshape(w.shape), w), tag + (name,)
                assert cnt.cpu().tolist() == [-7] + w_counts.reshape(-1).tolist() + [-7], tag


def test_kernel_streams_graph_and_in_place(full_size):
    """376 x 1232, B = 2, the second step of the sequence: the same bits on a second call, on a side stream, in place, and from a
    captured graph (the memset of the counts, then the kernel; out of place, so a replay starts from the same state) replayed
    twice with pre-filled outputs."""
    flows, poses, masks, calib, ref = full_size
    H, W, B = 376, 1232, 2
    acc0, alive0, depth0 = (_dev(x) for x in ref[0][:3])
    flow, mask, pose = _dev(flows[1]), _dev(masks[1]), _dev(poses[1])
    want = [_dev(x) for x in ref[1]]

    def check(a, l, d, c, tag):
        assert torch.equal(a.view(torch.int32), want[0].view(torch.int32)) and torch.equal(l, want[1]), tag
        assert torch.equal(d.view(torch.int32), want[2].view(torch.int32)) and torch.equal(c, want[3]), tag

    for tag in ("first", "second"):
        check(*transforms.flow_track_step(flow, acc0, alive0, pose=pose, calib=calib, mask=mask, depth=depth0.clone()), tag)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = depth0.clone()
        out = transforms.flow_track_step(flow, acc0, alive0, pose=pose, calib=calib, mask=mask, depth=d)
    side.synchronize()
    check(*out, "side stream")
    a, l, d, c = acc0.clone(), alive0.clone(), depth0.clone(), torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    got = transforms.flow_track_step(flow, a, l, pose=pose, calib=calib, mask=mask, depth=d, out=(a, l, c))
    assert got[0] is a and got[1] is l and got[2] is d and got[3] is c
    check(a, l, d, c, "in place")
    # captured: static buffers; depth is in/out, so it is restored before every replay, the other outputs are pre-filled
    a_out = torch.empty((B, 2, H, W), dtype=torch.float32, device=DEV)
    l_out = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    d_io = depth0.clone()
    counts = torch.empty((B, 4), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_lib.lib().atdn_flow_track_step(p(flow), p(mask), p(acc0), p(alive0), B, H, W, p(a_out), p(l_out), p(pose), *calib,
                                                   1.0, R.min_sin2_of(0.05), 80.0, p(d_io), p(counts),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, 1e30):
        a_out.fill_(fill)
        l_out.fill_(9)
        counts.fill_(123456)
        d_io.copy_(depth0)
        graph.replay()
        torch.cuda.synchronize()
        check(a_out, l_out, d_io, counts, fill)


def test_kernel_argument_errors():
    L = _lib.lib()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)   # noqa: E731
    flow, acc, acc2, depth, pose = z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 2, 4, 4), z(1, 1, 4, 4), z(1, 12)
    alive, alive2, counts = z(1, 4, 4, dt=torch.uint8), z(1, 4, 4, dt=torch.uint8), z(1, 4, dt=torch.int32)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    base = dict(flow=flow, mask=None, acc_in=acc, alive_in=alive, acc_out=acc2, alive_out=alive2, pose=pose, depth=depth,
                counts=counts, B=1, W=4, fx=5.0, max_depth=80.0)

    def call(**over):
        a = dict(base, **over)
        return L.atdn_flow_track_step(p(a["flow"]), p(a["mask"]), p(a["acc_in"]), p(a["alive_in"]), a["B"], 4, a["W"], p(a["acc_out"]),
                                      p(a["alive_out"]), p(a["pose"]), a["fx"], 5.0, 1.5, 1.5, 1.0, 1e-6, a["max_depth"],
                                      p(a["depth"]), p(a["counts"]), None)

    assert call() == 0 and call(acc_out=acc, alive_out=alive) == 0 and call(pose=None, depth=None) == 0
    assert call(pose=None, depth=None, fx=-1.0, max_depth=0.0) == 0
    for over in (dict(flow=None), dict(acc_in=None), dict(alive_out=None), dict(counts=None), dict(depth=None), dict(pose=None),
                 dict(B=0), dict(B=65536), dict(W=0), dict(fx=0.0), dict(max_depth=float("inf")), dict(acc_out=flow),
                 dict(depth=acc), dict(depth=acc2), dict(alive_out=alive.view(-1)[1:]), dict(counts=pose.view(torch.int32))):
        assert call(**over) != 0, list(over)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(flow, acc, alive.cpu())                                    # alive on the host
    with pytest.raises(RuntimeError, match="max_epipolar"):
        transforms.flow_track_step(flow, acc, alive, pose=torch.eye(4), calib=(5.0, 5.0, 1.5, 1.5), max_epipolar=-1.0)


def test_flow_track_object():
    """depth.FlowTrack on the device against the same steps by hand (the host's float64 pose product included), a restart, and a
    batch of two."""
    flows, rels, calib, Z0 = R.drive(steps=3)
    flows2 = np.concatenate([flows, flows[:, :, :, ::-1].copy()], axis=1)                 # a second, different image
    track = depth_mod.FlowTrack((47, 154), calib, DEV, batch=2, max_epipolar=1.5)
    assert track.acc.is_cuda and track.alive.dtype == torch.uint8 and tuple(track.depth.shape) == (2, 1, 47, 154)
    for attempt in range(2):
        track.start()
        assert track.steps == 0
        P = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
        acc, alive = np.zeros((2, 2, 47, 154), dtype=np.float32), np.ones((2, 47, 154), dtype=np.uint8)
        depth = np.zeros((2, 1, 47, 154), dtype=np.float32)
        for k in range(3):
            counts = track.extend(_dev(flows2[k]), _t(rels[k]))
            P = P @ _t(rels[k])
            acc, alive, depth, c = host_step(flows2[k], None, acc, alive, R.pose_rows(P.numpy()), calib, depth, max_epipolar=1.5)
            assert track.steps == k + 1 and torch.equal(track.pose, P)
            assert same_bits(_n(track.acc), acc) and same_bits(_n(track.alive), alive) and same_bits(_n(track.depth), depth)
            assert np.array_equal(_n(counts), c) and counts is track.counts
        assert (c[:, 3] > 0).all()


def test_flow_track_object_moves_between_devices():
    """FlowTrack.to: a track begun on the host and moved to the device after its first step goes on with the same bits as the
    host form driven by hand (what NeuralSLAM.to relies on for a running track)."""
    flows, rels, calib, Z0 = R.drive(steps=3)
    track = depth_mod.FlowTrack((47, 154), calib, "cpu")
    track.start()
    P = torch.eye(4, dtype=torch.float64)[None]
    acc, alive = np.zeros((1, 2, 47, 154), dtype=np.float32), np.ones((1, 47, 154), dtype=np.uint8)
    depth = np.zeros((1, 1, 47, 154), dtype=np.float32)
    for k in range(3):
        if k == 1:
            assert track.to(DEV) is track and track.acc.is_cuda and track.alive.is_cuda and track.depth.is_cuda and track.steps == 1
        track.extend(_t(flows[k]) if k == 0 else _dev(flows[k]), _t(rels[k]))
        P = P @ _t(rels[k])
        acc, alive, depth, c = host_step(flows[k], None, acc, alive, R.pose_rows(P.numpy()), calib, depth)
        assert same_bits(_n(track.acc), acc) and same_bits(_n(track.alive), alive) and same_bits(_n(track.depth), depth)
        assert np.array_equal(_n(track.counts), c)


# ----------------------------------------------------------------------------- NeuralSLAM with keyframe_depth="track"
class _Recorder:
    """Stands in front of a callable, keeps what it returned (tensors cloned), forwards every other attribute."""

    def __init__(self, fn, owner=None):
        self._fn, self._owner, self.outputs = fn, owner, []

    def __call__(self, *a, **k):
        out = self._fn(*a, **k)
        self.outputs.append(tuple(o.clone() for o in out))
        return out

    def __getattr__(self, name):
        return getattr(self._owner, name)


def _listing(root, sub):
    return sorted(os.listdir(os.path.join(root, sub)))


def test_neuralslam_keyframe_depth_track(tmp_path):
    """Six frames, every third pair ends in a keyframe: keyframes are frames 0 and 3. The track of keyframe 0 is extended by the
    pairs 0, 1, 2 and written when pair 2 registers keyframe 1; the track of keyframe 1 is extended by the pairs 3, 4 and written
    by end_odometry(). The files equal a hand-driven FlowTrack on the recorded flows and poses; poses and rgb/ files are those of
    keyframe_depth="pair" and of calib=None, bit for bit; "pair" writes what it wrote before."""
    from atdn_vslam_amd.slam import KeyframePolicy, NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(6, 376, 1241, seed=8))

    class EveryThird(KeyframePolicy):
        calls = 0

        def __call__(self, pred_mat):
            self.calls += 1
            return self.calls % 3 == 0

    with pytest.raises(ValueError):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, keyframe_depth="track")
    with pytest.raises(ValueError):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, keyframe_depth="chain")
    run = {}
    for name, kw in (("plain", {}), ("pair", dict(calib=SLAM_CALIB, keyframe_depth="pair")),
                     ("track", dict(calib=SLAM_CALIB, keyframe_depth="track"))):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(path)
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, **kw)
        slam._policy = EveryThird()
        slam.start_odometry()
        flows = _Recorder(slam._flow_net.forward_consecutive)
        heads = _Recorder(slam._odometry_net, slam._odometry_net)
        slam._flow_net.forward_consecutive = flows
        slam._odometry_net = heads
        poses, listings = [], []
        for f in frames:
            poses.append(slam(f).clone())
            listings.append(_listing(path, "depth") if kw else None)
        slam._odometry_net = heads._owner
        slam.end_odometry(mapping_weights=vsd)
        run[name] = (slam, path, poses, flows, heads, listings)
    slam, path, poses, flows, heads, listings = run["track"]
    for other in ("plain", "pair"):
        assert all(torch.equal(a, b) for a, b in zip(poses, run[other][2])) and len(run[other][0]) == 2
        assert _listing(run[other][1], "rgb") == _listing(path, "rgb") == ["000000.pth", "000001.pth"]
        for f in _listing(path, "rgb"):
            assert torch.equal(torch.load(os.path.join(path, "rgb", f)), torch.load(os.path.join(run[other][1], "rgb", f)))
        assert torch.equal(torch.load(os.path.join(path, "poses.pth")), torch.load(os.path.join(run[other][1], "poses.pth")))
    # when the files appear: "track" after the pair that registers the next keyframe (the call with frame 3), then end_odometry()
    assert listings == [[], [], [], ["000000.pth"], ["000000.pth"], ["000000.pth"]]
    assert _listing(path, "depth") == ["000000.pth", "000001.pth"]
    # "pair": on the call after the one that stored the keyframe, as before
    assert run["pair"][5] == [[], ["000000.pth"], ["000000.pth"], ["000000.pth"], ["000000.pth", "000001.pth"],
                              ["000000.pth", "000001.pth"]]
    assert _listing(run["pair"][1], "depth") == ["000000.pth", "000001.pth"]
    track = depth_mod.FlowTrack((376, 1232), SLAM_CALIB, DEV)
    for kf, pairs in ((0, (0, 1, 2)), (1, (3, 4))):
        track.start()
        for i in pairs:
            rot, tr = heads.outputs[i]
            track.extend(flows.outputs[i][1], transforms.transform(rot.squeeze().cpu(), tr.squeeze().cpu()))
        stored = torch.load(os.path.join(path, "depth", "%06d.pth" % kf))
        assert stored.dtype == torch.float32 and tuple(stored.shape) == (1, 376, 1232) and not stored.is_cuda
        assert torch.equal(stored.view(torch.int32), track.depth[0].cpu().view(torch.int32)), kf
        print("keyframe", kf, "counts of the last step", track.counts[0].tolist(), "pixels with a depth", int((stored > 0).sum()))
        pts = slam.keyframe_points(kf)
        assert pts.is_cuda and tuple(pts.shape) == (3, int((stored > 0).sum()))
        # "pair" is the first step of the track: the two-view depth of the pair that starts at the keyframe
        rot, tr = run["pair"][4].outputs[pairs[0]]
        first, _ = transforms.two_view_depth(run["pair"][3].outputs[pairs[0]][1],
                                             transforms.transform(rot.squeeze().cpu(), tr.squeeze().cpu())[None], SLAM_CALIB)
        assert torch.equal(torch.load(os.path.join(run["pair"][1], "depth", "%06d.pth" % kf)), first[0].cpu()), kf
