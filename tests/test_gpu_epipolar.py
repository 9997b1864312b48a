"""Pose from flow alone on the device: the kernels of atdn_epipolar_terms / atdn_epipolar_solve (transforms.epipolar_terms and
transforms.pose_from_flow on device tensors) against the host form and the NumPy float64 restatement of the rule
(tests/epipolar_ref.py) — every bit of the sums, the pose and the cost, and every count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epipolar_ref import CASES, FULL_CASE, MIN_MARGIN, check_case, solve_batch, terms_batch  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def _cpu(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rows(pose44):
    return np.ascontiguousarray(pose44[..., :3, :]).reshape(pose44.shape[:-2] + (12,))


def _terms(to, flow, pose, calib, mask=None, **kw):
    s, c = transforms.epipolar_terms(to(flow), to(pose), calib, to(mask), **kw)
    assert s.is_cuda == (to is _dev) and c.is_cuda == (to is _dev) and s.dtype == torch.float64 and c.dtype == torch.int32
    return s.cpu().numpy(), c.cpu().numpy()


def _solve(to, flow, pose, calib, mask=None, **kw):
    p, k, c = transforms.pose_from_flow(to(flow), to(pose), calib, to(mask), **kw)
    assert all(t.is_cuda == (to is _dev) for t in (p, k, c))
    assert p.dtype == torch.float32 and k.dtype == torch.float64 and c.dtype == torch.int32
    return _rows(p.cpu().numpy()), k.cpu().numpy(), c.cpu().numpy()


def _equal(got, want, tag=""):
    for g, w in zip(got, want):
        if w.dtype == np.int32:
            assert np.array_equal(g, w), (tag, g.tolist(), w.tolist())
        else:
            assert _same_bits(g, w), tag


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, B = 2 scene and its references (one evaluation, three steps), computed once."""
    _, H, W, B, seed = FULL_CASE
    return check_case(H, W, B, seed, iters=3)


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_helper_and_the_host_form(name, H, W, B, seed, masked):
    """5 x 7 (one chunk, nine quads, a ragged last one); 9 x 33, B = 3 (H * W = 297 is odd: the flow planes of b = 1, 2 start off
    the 16-byte grid and take scalar accesses, the mask planes at addresses 1 and 2 mod 4 take byte loads); 8 x 16, B = 2
    (everything aligned); 47 x 154, B = 2 (8 chunks: their order matters). With and without a mask."""
    c = check_case(H, W, B, seed)
    args = (c["flow"], c["start"], c["calib"])
    if masked:
        mask = (np.random.RandomState(seed).uniform(size=(B, H, W)) < 0.7).astype(np.uint8)
        want_t, want_s, kw = terms_batch(*args, mask), solve_batch(*args, mask, iters=6), dict(iters=6)
        assert min(want_t[2], want_s[3]) >= MIN_MARGIN
        want_t, want_s = want_t[:2], want_s[:3]
    else:
        mask, want_t, want_s, kw = None, c["terms"], c["solve"], {}
    _equal(_terms(_dev, *args, mask), want_t, name)
    _equal(_terms(_cpu, *args, mask), want_t, name)
    _equal(_solve(_dev, *args, mask, **kw), want_s, name)
    _equal(_solve(_cpu, *args, mask, **kw), want_s, name)
    for b in range(B):                                            # every plane alone, through the 3-d form
        m = None if mask is None else mask[b]
        s3, c3 = _terms(_dev, c["flow"][b], c["start"][b], c["calib"], m)
        assert s3.shape == (28,) and c3.shape == (3,)
        _equal((s3, c3), (want_t[0][b], want_t[1][b]), (name, b))
        p3, k3, n3 = _solve(_dev, c["flow"][b], c["start"][b], c["calib"], m, **kw)
        assert p3.shape == (12,) and k3.shape == () and n3.shape == (4,)
        _equal((p3, k3, n3), (want_s[0][b], np.asarray(want_s[1][b]), want_s[2][b]), (name, b))
    if masked:
        s0, c0 = _terms(_dev, *args, np.zeros_like(mask))
        assert (c0 == 0).all() and (_bits(s0) == 0).all()
    else:
        _, tv = transforms.two_view_depth(_dev(c["flow"]), _dev(c["start"]), c["calib"])
        assert np.array_equal(tv.cpu().numpy()[:, :2], want_t[1][:, [0, 2]])


def test_edge_cases_return_the_input_pose_and_iters_zero():
    _, H, W, B, seed = CASES[1]
    c = check_case(H, W, B, seed)
    cand = c["terms"][1][:, 0]
    start = c["start"].copy()
    start[0, [3, 7, 11]] = 0.0                                            # t = 0
    start[1, 0] = np.float32(0.123)
    start[2, 5] = np.nan                                                  # a NaN in R
    mask = np.ones((B, H, W), dtype=np.uint8)
    mask[1] = 0
    pose, cost, counts = _solve(_dev, c["flow"], start, c["calib"], mask)
    assert _same_bits(pose, start) and (_bits(cost) == 0).all()
    assert counts.tolist() == [[int(cand[0]), 0, 0, 0], [0, 0, 0, 0], [int(cand[2]), 0, 0, 0]]
    pose, cost, counts = _solve(_dev, c["flow"], c["start"], c["calib"], iters=0)
    assert _same_bits(pose, c["start"]) and _same_bits(cost, np.ascontiguousarray(c["terms"][0][:, 27]))
    assert np.array_equal(counts[:, :3], c["terms"][1]) and (counts[:, 3] == 0).all()
    f = c["flow"].copy()
    f[1, 0, 4, 16] = np.nan
    f[2, 1, 4, 16] = np.inf
    _equal(_terms(_dev, f, c["start"], c["calib"]), terms_batch(f, c["start"], c["calib"])[:2])


def test_outputs_are_fully_written_and_nothing_else():
    """Guard values around every output, the flow at every alignment of its vector grid, a workspace full of NaN bytes: every
    output is written, nothing else is, and nothing is read from the workspace that the call did not write."""
    _, H, W, B, seed = CASES[1]
    c = check_case(H, W, B, seed)
    n = B * H * W
    L = _lib.lib()
    calib = c["calib"]
    dpose = _dev(c["start"])
    nws = int(L.atdn_epipolar_workspace_bytes(B, H, W))
    for shift in (0, 1, 2, 3):
        fbuf = torch.zeros(2 * n + 8, dtype=torch.float32, device=DEV)
        fbuf[shift:shift + 2 * n] = _dev(c["flow"]).reshape(-1)
        ws = torch.full((nws // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
        sums = torch.full((28 * B + 2,), -7.0, dtype=torch.float64, device=DEV)
        cnt3 = torch.full((3 * B + 2,), -7, dtype=torch.int32, device=DEV)
        head = (C.c_void_p(fbuf[shift:].data_ptr()), None, C.c_void_p(dpose.data_ptr()), B, H, W, *calib, 2.0, 1.0)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.atdn_epipolar_terms(*head, C.c_void_p(sums[1:].data_ptr()), C.c_void_p(cnt3[1:].data_ptr()),
                                         C.c_void_p(ws[1:].data_ptr()), stream))
        pose = torch.full((12 * B + 2,), -7.0, dtype=torch.float32, device=DEV)
        cost = torch.full((B + 2,), -7.0, dtype=torch.float64, device=DEV)
        cnt4 = torch.full((4 * B + 2,), -7, dtype=torch.int32, device=DEV)
        ws.fill_(float("nan"))
        _lib.check(L.atdn_epipolar_solve(*head, 16, C.c_void_p(pose[1:].data_ptr()), C.c_void_p(cost[1:].data_ptr()),
                                         C.c_void_p(cnt4[1:].data_ptr()), C.c_void_p(ws[1:].data_ptr()), stream))
        torch.cuda.synchronize()
        s = sums.cpu().numpy()
        assert s[0] == -7.0 and s[-1] == -7.0 and _same_bits(s[1:-1].reshape(B, 28), c["terms"][0]), shift
        assert cnt3.cpu().tolist() == [-7] + c["terms"][1].reshape(-1).tolist() + [-7], shift
        p = pose.cpu().numpy()
        assert p[0] == -7.0 and p[-1] == -7.0 and _same_bits(p[1:-1].reshape(B, 12), c["solve"][0]), shift
        k = cost.cpu().numpy()
        assert k[0] == -7.0 and k[-1] == -7.0 and _same_bits(k[1:-1], c["solve"][1]), shift
        assert cnt4.cpu().tolist() == [-7] + c["solve"][2].reshape(-1).tolist() + [-7], shift
        w = ws.cpu().numpy()
        assert np.isnan(w[0]) and np.isnan(w[-1])


def test_full_size_two_calls_streams_and_graph(full_size):
    """376 x 1232, B = 2: 453 chunks per image and a ragged last one; one evaluation and three steps against the helper. The same
    bits on a second call, on a side stream, and from a captured graph — a capture fails on any host synchronisation, so the
    replayed single chain of 2 * 4 launches shows that the call has none."""
    _, H, W, B, _ = FULL_CASE
    c = full_size
    f, p = _dev(c["flow"]), _dev(c["start"])
    calib = c["calib"]
    s1, c1 = transforms.epipolar_terms(f, p, calib)
    s2, c2 = transforms.epipolar_terms(f, p, calib)
    a1 = transforms.pose_from_flow(f, p, calib, iters=3)
    a2 = transforms.pose_from_flow(f, p, calib, iters=3)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in (s1, c1) + a1)
    _equal((s1.cpu().numpy(), c1.cpu().numpy()), c["terms"])
    _equal((_rows(a1[0].cpu().numpy()), a1[1].cpu().numpy(), a1[2].cpu().numpy()), c["solve"])
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64)) and torch.equal(c1, c2)
    assert all(torch.equal(x, y) for x, y in zip(a1, a2))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a3 = transforms.pose_from_flow(f, p, calib, iters=3)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a1, a3))
    L = _lib.lib()
    pose = torch.empty((B, 12), dtype=torch.float32, device=DEV)
    cost = torch.empty((B,), dtype=torch.float64, device=DEV)
    counts = torch.empty((B, 4), dtype=torch.int32, device=DEV)
    ws = torch.empty((int(L.atdn_epipolar_workspace_bytes(B, H, W)) // 8,), dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(L.atdn_epipolar_solve(C.c_void_p(f.data_ptr()), None, C.c_void_p(p.data_ptr()), B, H, W, *calib, 2.0, 1.0, 3,
                                         C.c_void_p(pose.data_ptr()), C.c_void_p(cost.data_ptr()), C.c_void_p(counts.data_ptr()),
                                         C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, float("nan")):
        pose.fill_(fill)
        cost.fill_(fill)
        counts.fill_(123456)
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pose, a1[0][:, :3, :].reshape(B, 12)) and torch.equal(cost, a1[1]) and torch.equal(counts, a1[2]), fill


def test_kernel_argument_errors():
    z = torch.zeros(1, 2, 4, 4, device=DEV)
    eye = torch.eye(4, device=DEV)[None]
    k = (5.0, 5.0, 1.5, 1.5)
    with pytest.raises(RuntimeError, match="scale_px"):
        transforms.epipolar_terms(z, eye, k, scale_px=0.0)
    with pytest.raises(RuntimeError, match="iters"):
        transforms.pose_from_flow(z, eye, k, iters=-1)
    with pytest.raises(RuntimeError):
        transforms.pose_from_flow(z, eye, k, mask=torch.ones(1, 4, 4, dtype=torch.uint8))      # the mask on the host
    L = _lib.lib()
    pose = torch.eye(4, device=DEV)[:3].reshape(12).contiguous()
    out = torch.zeros(12, device=DEV)
    cost = torch.zeros(1, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    sums = torch.zeros(28, dtype=torch.float64, device=DEV)
    ws = torch.zeros(int(L.atdn_epipolar_workspace_bytes(1, 4, 4)) // 8 + 1, dtype=torch.float64, device=DEV)
    zp, pp, op, kp, cp, sp, wp = (C.c_void_p(t.data_ptr()) for t in (z, pose, out, cost, cnt, sums, ws))
    tail = (1, 4, 4, 5.0, 5.0, 1.5, 1.5, 2.0, 1.0)
    assert L.atdn_epipolar_terms(zp, None, pp, *tail, sp, cp, wp, None) == 0
    assert L.atdn_epipolar_solve(zp, None, pp, *tail, 2, op, kp, cp, wp, None) == 0
    assert L.atdn_epipolar_terms(zp, None, pp, *tail, sp, cp, None, None) != 0 and b"null" in L.atdn_last_error()
    assert L.atdn_epipolar_solve(zp, None, pp, *tail, 2, op, kp, cp, None, None) != 0
    assert L.atdn_epipolar_terms(None, None, pp, *tail, sp, cp, wp, None) != 0
    assert L.atdn_epipolar_terms(zp, None, pp, *tail, sp, cp, C.c_void_p(ws.data_ptr() + 4), None) != 0
    assert b"aligned" in L.atdn_last_error()
    assert L.atdn_epipolar_solve(zp, None, pp, *tail, 2, pp, kp, cp, wp, None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_epipolar_solve(zp, None, pp, *tail, 2, op, kp, cp, zp, None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_epipolar_solve(zp, None, pp, *tail, 65, op, kp, cp, wp, None) != 0
    assert L.atdn_epipolar_solve(zp, None, pp, 65536, *tail[1:], 2, op, kp, cp, wp, None) != 0
    torch.cuda.synchronize()
