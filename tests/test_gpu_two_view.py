"""Two-view depth on the GPU: the kernel (atdn_flow_two_view_depth, csrc/two_view.hip) against the NumPy float64 restatement of
the rule (tests/two_view_ref.py) and against the library's host form — every depth bit and every count, exactly (the scenes keep
every decision at least 1e-9 from its threshold, asserted on the helper alone) —, atdn_depth_backproject against the CPU
expression and the reference's outputs, and VisualOdometry / NeuralSLAM with a calibration against the same steps done by hand."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, depth as depth_mod
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from two_view_ref import CASES, FULL_CASE, DEFAULTS, check_case, min_sin2_of, reference_batch  # noqa: E402
from slam_cases import _Args, EverySecond, SLAM_CALIB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 4 x the reference's own float32-against-float64 gap on each fixture case (tests/test_two_view_host.py)
PROJECT_TOL = {"5x7": 4 * 3.353e-06, "47x154": 4 * 6.757e-06}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu(flow, pose, calib, mask=None, **kw):
    d, c = transforms.two_view_depth(_dev(flow), _dev(pose), calib, None if mask is None else _dev(mask), **kw)
    torch.cuda.synchronize()
    assert d.is_cuda and c.is_cuda and d.dtype == torch.float32 and c.dtype == torch.int32
    return d.cpu().numpy(), c.cpu().numpy()


def _host(flow, pose, calib, mask=None, **kw):
    d, c = transforms.two_view_depth(torch.from_numpy(np.ascontiguousarray(flow)), torch.from_numpy(np.ascontiguousarray(pose)),
                                     calib, None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)), **kw)
    return d.numpy(), c.numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(flow, pose, calib, ref_depth, ref_counts, mask=None, tag="", **kw):
    """Kernel == helper == host form; returns the kernel's (depth, counts)."""
    depth, counts = _gpu(flow, pose, calib, mask, **kw)
    hdepth, hcounts = _host(flow, pose, calib, mask, **kw)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts), tag
    assert _same_bits(depth, hdepth) and np.array_equal(counts, hcounts), tag
    return depth, counts


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, B = 2 scene and its reference, computed once."""
    _, H, W, B, seed = FULL_CASE
    return check_case(H, W, B, seed)


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_helper_and_the_host_form(name, H, W, B, seed):
    """5 x 7 (one workgroup, nine quads, a ragged last one); 9 x 33, B = 3 (H * W = 297 is odd: the planes of b = 1, 2 start off
    the 16-byte grid and take scalar accesses, b = 0 takes vector accesses and a ragged tail); 8 x 16, B = 2 (everything
    aligned, no tail); 47 x 154, B = 2 (8 workgroups, H * W = 7238 = 2 mod 4)."""
    flow, pose, calib, _, ref_depth, ref_counts = check_case(H, W, B, seed)
    _check(flow, pose, calib, ref_depth, ref_counts, tag=name)
    for b in range(B):                                            # every plane alone, through the 3-d form
        d3, c3 = transforms.two_view_depth(_dev(flow[b]), _dev(pose[b]), calib)
        assert d3.is_cuda and tuple(d3.shape) == (1, H, W) and tuple(c3.shape) == (3,)
        assert _same_bits(d3.cpu().numpy(), ref_depth[b]) and np.array_equal(c3.cpu().numpy(), ref_counts[b])
    score = transforms.epipolar_score(_dev(ref_counts))
    assert score.is_cuda and np.array_equal(score.cpu().numpy(), (ref_counts[:, 1] / ref_counts[:, 0].astype(np.float64)).astype(np.float32))


def test_kernel_one_pixel_image():
    th = 0.1
    R = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
    pose = np.concatenate([R, np.array([[-0.5], [0.0], [0.0]])], axis=1).reshape(1, 12).astype(np.float32)
    z = np.zeros((1, 2, 1, 1), dtype=np.float32)
    calib = (10.0, 10.0, 0.0, 0.0)
    ref_depth, ref_counts, _ = reference_batch(z, pose, calib)
    depth, counts = _check(z, pose, calib, ref_depth, ref_counts)
    assert counts.tolist() == [[1, 1, 1]]
    np.testing.assert_allclose(depth[0, 0, 0, 0], 0.5 / math.tan(th), rtol=1e-6)
    f = z.copy()
    f[0, 1] = -0.5                                                # leaves the image
    ref_depth, ref_counts, _ = reference_batch(f, pose, calib)
    _, counts = _check(f, pose, calib, ref_depth, ref_counts)
    assert counts.tolist() == [[0, 0, 0]]


def test_kernel_with_a_mask_off_the_dword_grid():
    """9 x 33, B = 3: the mask planes of b = 1, 2 start at addresses 1 and 2 mod 4 (byte loads), b = 0 reads dwords; then the
    mask of flow_consistency as it comes from its kernel."""
    H, W, B, seed = 9, 33, 3, 3
    mask = (np.random.RandomState(7).uniform(size=(B, H, W)) < 0.6).astype(np.uint8)
    flow, pose, calib, _, ref_depth, ref_counts = check_case(H, W, B, seed, mask=mask)
    dm = _dev(mask)
    assert dm.data_ptr() % 4 == 0 and (H * W) % 4 == 1
    depth, counts = _check(flow, pose, calib, ref_depth, ref_counts, mask=mask)
    assert (depth[:, 0][mask == 0] == 0).all() and (counts[:, 0] > 0).all()
    _check(flow, pose, calib, np.zeros_like(ref_depth), np.zeros_like(ref_counts), mask=np.zeros_like(mask))
    fc, _ = transforms.flow_consistency(_dev(flow), _dev(-flow))
    d, c = transforms.two_view_depth(_dev(flow), _dev(pose), calib, mask=fc)
    want = reference_batch(flow, pose, calib, fc.cpu().numpy()[:, 0])
    assert _same_bits(d.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])


def test_kernel_outputs_are_fully_written():
    """Pre-filled output buffers with guard values around them, every buffer at every alignment of its vector grid: every depth
    and every count is written, nothing else is. 8 x 16, B = 2 (aligned planes: the shifts alone decide) and 9 x 33, B = 3."""
    for H, W, B, seed in ((8, 16, 2, 4), (9, 33, 3, 3)):
        flow, pose, calib, _, ref_depth, ref_counts = check_case(H, W, B, seed)
        n = B * H * W
        mask = (np.random.RandomState(seed).uniform(size=(B, H, W)) < 0.7).astype(np.uint8)
        ref_m = reference_batch(flow, pose, calib, mask)
        for shift in (0, 1, 2, 3):
            fbuf = torch.zeros(2 * n + 8, dtype=torch.float32, device=DEV)
            fbuf[shift:shift + 2 * n] = _dev(flow).reshape(-1)
            mbuf = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
            mbuf[shift:shift + n] = _dev(mask).reshape(-1)
            out = torch.full((n + 32,), -7.0, dtype=torch.float32, device=DEV)
            cnt = torch.full((3 * B + 2,), -7, dtype=torch.int32, device=DEV)
            dpose = _dev(pose)
            for use_mask, (want_d, want_c, _) in ((False, (ref_depth, ref_counts, 0)), (True, ref_m)):
                out.fill_(-7.0)
                cnt.fill_(-7)
                _lib.check(_lib.lib().atdn_flow_two_view_depth(
                    C.c_void_p(fbuf[shift:].data_ptr()), C.c_void_p(dpose.data_ptr()),
                    C.c_void_p(mbuf[shift:].data_ptr()) if use_mask else None, B, H, W, *calib, 1.0,
                    min_sin2_of(DEFAULTS["min_parallax_deg"]), 80.0, C.c_void_p(out[16 + shift:].data_ptr()),
                    C.c_void_p(cnt[1:].data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert (o[:16 + shift] == -7.0).all() and (o[16 + shift + n:] == -7.0).all(), (H, W, shift, use_mask)
                assert _same_bits(o[16 + shift:16 + shift + n].reshape(B, 1, H, W), want_d), (H, W, shift, use_mask)
                assert cnt.cpu().tolist() == [-7] + want_c.reshape(-1).tolist() + [-7], (H, W, shift, use_mask)


def test_kernel_at_full_size_streams_and_graph(full_size):
    """376 x 1232, B = 2: 453 workgroups per image and a ragged last one. The same bits on a second call, on a side stream, and
    from a captured graph (one linear chain: the memset of the counts, then the kernel) replayed twice."""
    flow, pose, calib, _, ref_depth, ref_counts = full_size
    H, W = 376, 1232
    dflow, dpose = _dev(flow), _dev(pose)
    d1, c1 = transforms.two_view_depth(dflow, dpose, calib)
    d2, c2 = transforms.two_view_depth(dflow, dpose, calib)
    torch.cuda.synchronize()
    assert _same_bits(d1.cpu().numpy(), ref_depth) and np.array_equal(c1.cpu().numpy(), ref_counts)
    assert torch.equal(d1, d2) and torch.equal(c1, c2)
    hd, hc = _host(flow, pose, calib)
    assert _same_bits(hd, ref_depth) and np.array_equal(hc, ref_counts)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d3, c3 = transforms.two_view_depth(dflow, dpose, calib)
    side.synchronize()
    assert torch.equal(d3, d1) and torch.equal(c3, c1)
    # captured: static output buffers, pre-filled before every replay so that unwritten values and un-reset counts would show
    depth = torch.empty((2, 1, H, W), dtype=torch.float32, device=DEV)
    counts = torch.empty((2, 3), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_lib.lib().atdn_flow_two_view_depth(C.c_void_p(dflow.data_ptr()), C.c_void_p(dpose.data_ptr()), None, 2, H, W,
                                                       *calib, 1.0, min_sin2_of(DEFAULTS["min_parallax_deg"]), 80.0,
                                                       C.c_void_p(depth.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, 1e30):
        depth.fill_(fill)
        counts.fill_(123456)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(depth, d1) and torch.equal(counts, c1), fill


def test_kernel_argument_errors():
    z = torch.zeros(1, 2, 4, 4, device=DEV)
    eye = torch.eye(4, device=DEV)[None]
    k = (5.0, 5.0, 1.5, 1.5)
    with pytest.raises(RuntimeError, match="max_epipolar"):
        transforms.two_view_depth(z, eye, k, max_epipolar=-1.0)
    with pytest.raises(RuntimeError, match="max_depth"):
        transforms.two_view_depth(z, eye, k, max_depth=float("inf"))
    with pytest.raises(RuntimeError):
        transforms.two_view_depth(z, eye, k, mask=torch.ones(1, 4, 4, dtype=torch.uint8))      # the mask on the host
    L = _lib.lib()
    pose = torch.zeros(12, device=DEV)
    d = torch.zeros(16, device=DEV)
    c = torch.zeros(3, dtype=torch.int32, device=DEV)
    zp, pp, dp, cp = (C.c_void_p(t.data_ptr()) for t in (z, pose, d, c))
    tail = (1, 4, 4, 5.0, 5.0, 1.5, 1.5, 1.0, 1e-6, 80.0)
    assert L.atdn_flow_two_view_depth(zp, pp, None, *tail, dp, cp, None) == 0
    assert L.atdn_flow_two_view_depth(None, pp, None, *tail, dp, cp, None) != 0
    assert L.atdn_flow_two_view_depth(zp, None, None, *tail, dp, cp, None) != 0
    assert L.atdn_flow_two_view_depth(zp, pp, None, *tail, dp, None, None) != 0
    assert L.atdn_flow_two_view_depth(zp, pp, None, *tail, zp, cp, None) != 0
    assert b"overlap" in L.atdn_last_error()
    assert L.atdn_flow_two_view_depth(zp, pp, None, 1, 4, 0, *tail[3:], dp, cp, None) != 0
    assert L.atdn_flow_two_view_depth(zp, pp, None, 1, 4, 4, 0.0, *tail[4:], dp, cp, None) != 0
    pts = torch.zeros(48, device=DEV)
    assert L.atdn_depth_backproject(dp, 1, 4, 4, 5.0, 5.0, 1.5, 1.5, C.c_void_p(pts.data_ptr()), None) == 0
    assert L.atdn_depth_backproject(dp, 1, 4, 4, 5.0, 5.0, 1.5, 1.5, dp, None) != 0
    assert L.atdn_depth_backproject(None, 1, 4, 4, 5.0, 5.0, 1.5, 1.5, C.c_void_p(pts.data_ptr()), None) != 0
    assert L.atdn_depth_backproject(dp, 1, 4, 4, 5.0, -5.0, 1.5, 1.5, C.c_void_p(pts.data_ptr()), None) != 0
    torch.cuda.synchronize()


def test_backproject_matches_the_cpu_expression_and_the_reference(golden_dir):
    """atdn_depth_backproject against depth.project_depth on the CPU (the same float64 expression: within 1 ulp of float32) and
    against the reference's project_depth (tests/golden/depth.npz) within four times the reference's own float32-against-float64
    gap (test_two_view_host.py: 3.353e-06 at 5 x 7, 6.757e-06 at 47 x 154)."""
    g = np.load(os.path.join(golden_dir, "depth.npz"))
    k3 = torch.from_numpy(g["calib_3x3"])
    for name in [str(n) for n in g["names"]]:
        d = torch.from_numpy(g["depth_" + name])
        cpu = depth_mod.project_depth(d, k3).numpy()
        for dev_pts in (depth_mod.project_depth(d.to(DEV), k3), depth_mod.project_depth(d, k3, device=DEV)):
            assert dev_pts.is_cuda and dev_pts.dtype == torch.float32 and tuple(dev_pts.shape) == cpu.shape
            got = dev_pts.cpu().numpy()
            assert (np.abs(got.astype(np.float64) - cpu) <= np.spacing(np.abs(cpu))).all(), name
            err = float(np.abs(got.astype(np.float64) - g["points_" + name]).max())
            print(name, "largest difference from the reference", err, "allowed", PROJECT_TOL[name])
            assert err <= PROJECT_TOL[name]
    # a batch through the raw entry point: every image is the single call's
    d = _dev(np.stack([g["depth_47x154"], g["depth_47x154"][::-1].copy()]))
    pts = torch.full((2, 3, 47, 154), -7.0, device=DEV)
    fx, fy, cx, cy = depth_mod.intrinsics(k3)
    _lib.check(_lib.lib().atdn_depth_backproject(C.c_void_p(d.data_ptr()), 2, 47, 154, fx, fy, cx, cy, C.c_void_p(pts.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for b in range(2):
        assert torch.equal(pts[b], depth_mod.project_depth(d[b], k3))


# ----------------------------------------------------------------------------- odometry and SLAM with a calibration
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


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


@pytest.fixture(scope="module")
def hsd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def kitti_frames():
    return torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))


def test_visual_odometry_with_a_calibration(gsd, hsd, kitti_frames):
    from atdn_vslam_amd.pipeline import VisualOdometry
    plain = VisualOdometry(gsd, hsd, device=DEV, iters=4)
    vo = VisualOdometry(gsd, hsd, device=DEV, iters=4, calib=SLAM_CALIB)
    assert plain.calib is None and plain.last_depth is None and plain.epipolar_score() is None
    flows = _Recorder(vo.pipe.flow_net.forward_consecutive)
    heads = _Recorder(vo.pipe.head, vo.pipe.head)
    vo.pipe.flow_net.forward_consecutive = flows
    vo.pipe.head = heads
    for i, f in enumerate(kitti_frames[:3]):
        want = plain(f).clone()
        got = vo(f).clone()
        assert torch.equal(got, want), i                          # the poses of calib=None, bit for bit
        assert plain.last_depth is None and plain.last_counts is None
        if i == 0:
            assert vo.last_depth is None and vo.last_counts is None and vo.epipolar_score() is None
            continue
        assert len(flows.outputs) == i and len(heads.outputs) == i
        flow, (rot, tr) = flows.outputs[-1][1], heads.outputs[-1]
        pose = transforms.transform(rot.reshape(-1).cpu(), tr.reshape(-1).cpu())
        depth, counts = transforms.two_view_depth(flow, pose[None], SLAM_CALIB)
        assert tuple(vo.last_depth.shape) == (1, 1, 376, 1232) and tuple(vo.last_counts.shape) == (1, 3)
        assert vo.last_depth.is_cuda and vo.last_counts.is_cuda
        assert torch.equal(vo.last_depth, depth) and torch.equal(vo.last_counts, counts), i
        c = counts[0].tolist()
        assert 0 <= c[2] <= c[1] <= c[0] <= 376 * 1232 and int((depth != 0).sum()) == c[2]
        score = vo.epipolar_score()
        assert isinstance(score, float) and score == (float(np.float32(c[1] / c[0])) if c[0] else 0.0)
        print("pair", i, "counts", c, "score", score)
    vo.pipe.head = heads._owner
    vo.reset()
    assert vo.last_depth is None and vo.last_counts is None


def _listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs) + \
        sorted(os.path.relpath(os.path.join(d, s), root) + "/" for d, ss, _ in os.walk(root) for s in ss)


def test_neuralslam_keyframe_depth(gsd, hsd, kitti_frames, tmp_path):
    """Five frames, every second pair ends in a keyframe: keyframes are frames 0, 2, 4; the pairs (0,1) and (2,3) give keyframes 0
    and 1 their depth, keyframe 2 has no successor and no file."""
    from atdn_vslam_amd.slam import NeuralSLAM

    run = {}
    for name, calib in (("plain", None), ("calib", SLAM_CALIB)):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(os.path.join(path, "depth"))
        open(os.path.join(path, "depth", "000009.pth"), "w").close()    # left by an earlier session: a cold start clears it
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=calib)
        assert _listing(path) == ["depth/", "rgb/"]
        slam._policy = EverySecond()
        slam.start_odometry()
        flows = _Recorder(slam._flow_net.forward_consecutive)
        heads = _Recorder(slam._odometry_net, slam._odometry_net)
        slam._flow_net.forward_consecutive = flows
        slam._odometry_net = heads
        poses = [slam(f).clone() for f in kitti_frames]
        run[name] = (slam, path, poses, flows, heads)
    slam, path, poses, flows, heads = run["calib"]
    for a, b in zip(poses, run["plain"][2]):
        assert torch.equal(a, b)
    assert len(slam) == 3 and len(run["plain"][0]) == 3
    rgb = ["rgb/%06d.pth" % i for i in range(3)]
    assert _listing(run["plain"][1]) == rgb + ["depth/", "rgb/"]        # (the stale directory stays, empty; nothing new appears)
    assert _listing(path) == ["depth/000000.pth", "depth/000001.pth"] + rgb + ["depth/", "rgb/"]
    with pytest.raises(RuntimeError, match="calib"):
        run["plain"][0].keyframe_points(0)
    fx, fy, cx, cy = SLAM_CALIB
    for kf, pair in ((0, 0), (1, 2)):                              # keyframe index -> index of the pair that starts at it
        stored = torch.load(os.path.join(path, "depth", "%06d.pth" % kf))
        assert stored.dtype == torch.float32 and tuple(stored.shape) == (1, 376, 1232) and not stored.is_cuda
        flow, (rot, tr) = flows.outputs[pair][1], heads.outputs[pair]
        pred = transforms.transform(rot.squeeze().cpu(), tr.squeeze().cpu())
        depth, counts = transforms.two_view_depth(flow, pred[None], SLAM_CALIB)
        assert torch.equal(stored, depth[0].cpu()), kf
        print("keyframe", kf, "counts", counts[0].tolist())
        # keyframe_points: back-projection and the keyframe's pose in float64, against the float32 result
        pts = slam.keyframe_points(kf)
        z = stored[0].double()
        valid = z > 0
        assert pts.is_cuda and pts.dtype == torch.float32 and tuple(pts.shape) == (3, int(valid.sum()))
        x = torch.arange(1232, dtype=torch.float64).view(1, -1)
        y = torch.arange(376, dtype=torch.float64).view(-1, 1)
        P = torch.stack([(z * (x - cx)) / fx, (z * (y - cy)) / fy, z])[:, valid]
        T = slam[kf].pose.double()
        want = T[:3, :3] @ P + T[:3, 3:4]
        # float32: the points rounded once, three products and three sums -> 8 * 2^-24 of the sum of magnitudes
        bound = 8 * 2.0 ** -24 * (T[:3, :3].abs() @ P.abs() + T[:3, 3:4].abs())
        assert bool(((pts.cpu().double() - want).abs() <= bound).all()), kf
    with pytest.raises(FileNotFoundError):
        slam.keyframe_points(2)
