"""Pose from flow alone, host form: atdn_epipolar_terms_host / atdn_epipolar_solve_host through transforms.epipolar_terms and
transforms.pose_from_flow on CPU tensors and through the raw C ABI, against the NumPy float64 restatement of the rule
(tests/epipolar_ref.py) — every bit of the sums, the pose and the cost, and every count —, the gradient against central
differences, the counts against two_view_depth, recovery of the generating pose, the edge cases and every argument error.
Needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epipolar_ref import (CASES, MIN_MARGIN, NOISY_CASE, check_case, gradient_check, pose_errors_deg, solve_batch,  # noqa: E402
                          terms_batch)

IDS = [c[0] for c in CASES]


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _terms(flow, pose, calib, mask=None, **kw):
    s, c = transforms.epipolar_terms(_t(flow), _t(pose), calib, _t(mask), **kw)
    assert s.dtype == torch.float64 and c.dtype == torch.int32 and not s.is_cuda
    return s.numpy(), c.numpy()


def _solve(flow, pose, calib, mask=None, **kw):
    p, cost, c = transforms.pose_from_flow(_t(flow), _t(pose), calib, _t(mask), **kw)
    assert p.dtype == torch.float32 and cost.dtype == torch.float64 and c.dtype == torch.int32 and not p.is_cuda
    return p.numpy(), cost.numpy(), c.numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rows(pose44):
    assert np.array_equal(pose44[..., 3, :], np.broadcast_to(np.array([0, 0, 0, 1], dtype=np.float32), pose44[..., 3, :].shape))
    return np.ascontiguousarray(pose44[..., :3, :]).reshape(pose44.shape[:-2] + (12,))


def _tt(pose12):
    t = pose12.reshape(-1, 3, 4)[:, :, 3].astype(np.float64)
    return (t * t).sum(axis=1)


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=IDS)
def test_host_terms_equal_the_helper(name, H, W, B, seed):
    """margin >= 1e-9 is asserted on the helper alone (check_case); then every bit of the 28 sums and every count at the start
    pose, through the 4-d and the 3-d forms, and at other parameters."""
    c = check_case(H, W, B, seed)
    sums, counts = _terms(c["flow"], c["start"], c["calib"])
    assert _same_bits(sums, c["terms"][0]) and np.array_equal(counts, c["terms"][1])
    assert (counts[:, 1] > 0).all() and (counts[:, 0] < H * W).all()
    for b in range(B):
        s3, c3 = _terms(c["flow"][b], c["start"][b].reshape(3, 4), c["calib"])
        assert s3.shape == (28,) and c3.shape == (3,)
        assert _same_bits(s3, c["terms"][0][b]) and np.array_equal(c3, c["terms"][1][b])
    kw = dict(scale_px=0.5, inlier_px=0.05)
    want = terms_batch(c["flow"], c["start"], c["calib"], **kw)
    assert want[2] >= MIN_MARGIN
    sums, counts = _terms(c["flow"], c["start"], c["calib"], **kw)
    assert _same_bits(sums, want[0]) and np.array_equal(counts, want[1])


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=IDS)
def test_host_solve_equals_the_helper_and_recovers_the_pose(name, H, W, B, seed):
    """Noise-free flow (float32 rounding only), a start 1 degree off in rotation and 8 degrees off in the direction of t, 16
    steps: every bit against the helper, batched and each plane alone; the rotation and the direction of t within 1e-4 degrees of
    the generating pose (the helper gets below 7e-6), t.t kept to 1e-6 (the float32 rounding of the output), a step accepted."""
    c = check_case(H, W, B, seed)
    pose, cost, counts = _solve(c["flow"], c["start"], c["calib"])
    assert pose.shape == (B, 4, 4) and counts.shape == (B, 4)
    assert _same_bits(_rows(pose), c["solve"][0]) and _same_bits(cost, c["solve"][1]) and np.array_equal(counts, c["solve"][2])
    for b in range(B):
        p3, k3, c3 = _solve(c["flow"][b], c["start"][b], c["calib"])
        assert p3.shape == (4, 4) and k3.shape == () and c3.shape == (4,)
        assert _same_bits(_rows(p3), c["solve"][0][b]) and _bits(k3) == _bits(c["solve"][1][b]) and np.array_equal(c3, c["solve"][2][b])
    rot0, dir0 = pose_errors_deg(c["start"], c["true"])
    assert (np.abs(rot0 - 1.0) < 1e-3).all() and (np.abs(dir0 - 8.0) < 1e-3).all()
    rot, dirn = pose_errors_deg(_rows(pose), c["true"])
    print("rotation error (deg)", rot, "direction error (deg)", dirn)
    assert (rot < 1e-4).all() and (dirn < 1e-4).all()
    assert (np.abs(_tt(_rows(pose)) / _tt(c["start"]) - 1.0) <= 1e-6).all()
    assert (counts[:, 3] >= 1).all() and (cost < c["terms"][0][:, 27]).all()
    # fewer steps and other parameters
    kw = dict(iters=5, scale_px=3.0, inlier_px=0.5)
    want = solve_batch(c["flow"], c["start"], c["calib"], **kw)
    assert want[3] >= MIN_MARGIN
    pose, cost, counts = _solve(c["flow"], c["start"], c["calib"], **kw)
    assert _same_bits(_rows(pose), want[0]) and _same_bits(cost, want[1]) and np.array_equal(counts, want[2])


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=IDS)
def test_host_forms_with_a_mask(name, H, W, B, seed):
    c = check_case(H, W, B, seed)
    mask = (np.random.RandomState(seed).uniform(size=(B, 1, H, W)) < 0.7).astype(np.uint8)
    want_t = terms_batch(c["flow"], c["start"], c["calib"], mask[:, 0])
    want_s = solve_batch(c["flow"], c["start"], c["calib"], mask[:, 0], iters=6)
    assert min(want_t[2], want_s[3]) >= MIN_MARGIN
    sums, counts = _terms(c["flow"], c["start"], c["calib"], mask)
    assert _same_bits(sums, want_t[0]) and np.array_equal(counts, want_t[1])
    assert (counts <= c["terms"][1]).all() and (counts[:, 0] < c["terms"][1][:, 0]).all()
    pose, cost, cnt = _solve(c["flow"], c["start"], c["calib"], mask[:, 0] != 0, iters=6)      # a bool mask [B,H,W]
    assert _same_bits(_rows(pose), want_s[0]) and _same_bits(cost, want_s[1]) and np.array_equal(cnt, want_s[2])


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=IDS)
def test_gradient_agrees_with_central_differences(name, H, W, B, seed):
    """Terms 21 .. 26 against central differences (h = 1e-6) of the summed cost over the step (dw, dth), both taken in the helper,
    whose terms the host form equals bit for bit (above): relative 1e-6 of the largest entry (measured: 2e-11 .. 1e-9)."""
    c = check_case(H, W, B, seed)
    for b in range(B):
        g, num = gradient_check(c["flow"][b], c["start"][b], c["calib"])
        rel = np.abs(g - num).max() / np.abs(g).max()
        print(name, b, "relative gradient error", rel)
        assert rel <= 1e-6
        assert _same_bits(np.ascontiguousarray(_terms(c["flow"][b], c["start"][b], c["calib"])[0][21:27]), np.ascontiguousarray(g))


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=IDS)
def test_counts_are_those_of_two_view_depth(name, H, W, B, seed):
    """Same pose, no mask, inlier_px = max_epipolar: candidates = two_view's inside, inliers = two_view's inliers, exactly (the
    prefix of the rule is one shared function)."""
    c = check_case(H, W, B, seed)
    for px in (1.0, 0.05):
        _, counts = _terms(c["flow"], c["start"], c["calib"], inlier_px=px)
        _, tv = transforms.two_view_depth(_t(c["flow"]), _t(c["start"]), c["calib"], max_epipolar=px)
        assert np.array_equal(counts[:, 0], tv.numpy()[:, 0]) and np.array_equal(counts[:, 2], tv.numpy()[:, 1])
        assert (counts[:, 1] == counts[:, 0]).all()
    assert (counts[:, 2] < counts[:, 0]).all()                           # at 0.05 px the start is not all inliers


def test_noisy_scene_with_outliers():
    """94 x 308, 0.2 px Gaussian noise, 30 % gross outliers, 32 steps from 1 / 8 degrees off. The helper alone ends 0.0671 degrees
    off in rotation and 0.527 degrees off in direction (cost 19966.08 -> 11646.61, all 32 steps accepted: under the redescending
    loss the flat rotation/translation valley of a forward motion is descended linearly, a property of the problem); the bounds
    here are those figures times two. The host form must equal the helper bit for bit as well."""
    _, H, W, B, seed = NOISY_CASE
    c = check_case(H, W, B, seed, iters=32, noise_px=0.2, outliers=0.3)
    pose, cost, counts = _solve(c["flow"], c["start"], c["calib"], iters=32)
    assert _same_bits(_rows(pose), c["solve"][0]) and _same_bits(cost, c["solve"][1]) and np.array_equal(counts, c["solve"][2])
    rot0, dir0 = pose_errors_deg(c["start"], c["true"])
    rot, dirn = pose_errors_deg(_rows(pose), c["true"])
    print("cost", c["terms"][0][:, 27], "->", cost, "rotation", rot0, "->", rot, "direction", dir0, "->", dirn, counts.tolist())
    assert (cost <= c["terms"][0][:, 27]).all() and (dirn < dir0).all()
    assert (rot <= 2 * 0.0671).all() and (dirn <= 2 * 0.527).all()
    assert (counts[:, 2] > c["terms"][1][:, 2]).all()                    # more inliers than at the start


def test_edge_cases_return_the_input_pose():
    """t = 0, an all-zero mask, a NaN in the pose: no pixel is used, no step is accepted, the pose comes back bit for bit (not
    a rotation: entry 0 is 0.123), cost +0.0, counts (candidates, 0, 0, 0). iters = 0 is the evaluation alone."""
    _, H, W, B, seed = CASES[1]
    c = check_case(H, W, B, seed)
    cand = c["terms"][1][:, 0]
    start = c["start"].copy()
    start[0, [3, 7, 11]] = 0.0                                            # t = 0
    start[1, 0] = np.float32(0.123)
    start[2, 5] = np.nan                                                  # a NaN in R
    mask = np.ones((B, H, W), dtype=np.uint8)
    mask[1] = 0
    pose, cost, counts = _solve(c["flow"], start, c["calib"], mask)
    assert _same_bits(_rows(pose), start) and (_bits(cost) == 0).all()
    assert counts.tolist() == [[int(cand[0]), 0, 0, 0], [0, 0, 0, 0], [int(cand[2]), 0, 0, 0]]
    sums, cnt = _terms(c["flow"], start, c["calib"], mask)
    assert (_bits(sums) == 0).all() and np.array_equal(cnt, counts[:, :3])
    start[2] = c["start"][2]
    start[2, 7] = np.nan                                                  # a NaN in t
    pose, cost, counts = _solve(c["flow"], start, c["calib"])
    assert _same_bits(_rows(pose)[[0, 2]], start[[0, 2]]) and (counts[[0, 2], 1:] == 0).all() and (_bits(cost[[0, 2]]) == 0).all()
    assert counts[1, 3] >= 1                                              # the one sound problem of the batch is solved
    pose, cost, counts = _solve(c["flow"], c["start"], c["calib"], iters=0)
    assert _same_bits(_rows(pose), c["start"]) and _same_bits(cost, np.ascontiguousarray(c["terms"][0][:, 27]))
    assert np.array_equal(counts[:, :3], c["terms"][1]) and (counts[:, 3] == 0).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_flow_is_not_a_candidate(bad):
    _, H, W, B, seed = CASES[1]
    c = check_case(H, W, B, seed)
    base = c["terms"][1]
    ys, xs = np.mgrid[0:H, 0:W]
    x2, y2 = xs + c["flow"][1, 0].astype(np.float64), ys + c["flow"][1, 1].astype(np.float64)
    pix = tuple(np.argwhere((x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1))[3])     # a candidate
    for ch in (0, 1):
        f = c["flow"].copy()
        f[1, ch][pix] = bad
        sums, counts = _terms(f, c["start"], c["calib"])
        want = terms_batch(f, c["start"], c["calib"])
        assert _same_bits(sums, want[0]) and np.array_equal(counts, want[1])
        assert counts[1, 0] == base[1, 0] - 1 and np.array_equal(counts[[0, 2]], base[[0, 2]])
        assert np.isfinite(sums).all()
        got, want_s = _solve(f, c["start"], c["calib"], iters=3), solve_batch(f, c["start"], c["calib"], iters=3)
        assert _same_bits(_rows(got[0]), want_s[0]) and np.array_equal(got[2], want_s[2])


def test_argument_errors():
    L = _lib.lib()
    H, W = 4, 4
    flow = np.zeros((1, 2, H, W), dtype=np.float32)
    pose = np.eye(4, dtype=np.float32)[:3].reshape(1, 12).copy()
    pose[0, 11] = 1.0
    mask = np.ones((1, H, W), dtype=np.uint8)
    sums = np.full((1, 28), -7.0, dtype=np.float64)
    counts = np.full((1, 4), -7, dtype=np.int32)
    pose_out = np.full((1, 12), -7.0, dtype=np.float32)
    cost = np.full((1,), -7.0, dtype=np.float64)
    outputs = (sums, counts, pose_out, cost)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    good = dict(flow=p(flow), mask=p(mask), pose=p(pose), B=1, H=H, W=W, fx=5.0, fy=5.0, cx=1.5, cy=1.5, scale_px=2.0,
                inlier_px=1.0, iters=2, sums=p(sums), counts=p(counts), pose_out=p(pose_out), cost=p(cost))
    head = ("flow", "mask", "pose", "B", "H", "W", "fx", "fy", "cx", "cy", "scale_px", "inlier_px")

    def terms(**kw):
        a = dict(good, **kw)
        return L.atdn_epipolar_terms_host(*[a[k] for k in head + ("sums", "counts")])

    def solve(**kw):
        a = dict(good, **kw)
        return L.atdn_epipolar_solve_host(*[a[k] for k in head + ("iters", "pose_out", "cost", "counts")])

    def refused(call, **kw):
        """the call fails and nothing is written"""
        for a in outputs:
            a.fill(-7)
        rc = call(**kw)
        return rc != 0 and all((a == -7).all() for a in outputs)

    for call, outs in ((terms, ("sums", "counts")), (solve, ("pose_out", "cost", "counts"))):
        assert call() == 0
        assert call(mask=None) == 0                                      # the mask is the one pointer that may be null
        for name in ("flow", "pose") + outs:
            assert refused(call, **{name: None}), name
            assert b"null" in L.atdn_last_error()
        for name in ("B", "H", "W"):
            assert refused(call, **{name: 0}) and refused(call, **{name: -1}), name
        assert refused(call, H=4097, W=4097) and b"2^24" in L.atdn_last_error()
        for name in ("fx", "fy", "scale_px", "inlier_px"):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                assert refused(call, **{name: v}), (name, v)
        for name in ("cx", "cy"):
            for v in (float("nan"), float("inf"), -float("inf")):
                assert refused(call, **{name: v}), (name, v)
            assert call(**{name: -3.0}) == 0
        for name in outs:
            for inp in (flow, mask, pose):
                before = inp.copy()
                assert call(**{name: p(inp)}) != 0 and b"overlap" in L.atdn_last_error(), name
                assert np.array_equal(inp, before)
        assert call(**{outs[0]: p(counts)}) != 0 and b"overlap" in L.atdn_last_error()
    for v in (-1, 65):
        assert refused(solve, iters=v) and b"iters" in L.atdn_last_error()
    assert solve(iters=0) == 0 and solve(iters=64) == 0
    assert L.atdn_epipolar_workspace_bytes(1, 4, 4) > 0 and L.atdn_epipolar_workspace_bytes(0, 4, 4) == 0
    assert L.atdn_epipolar_workspace_bytes(1, 4097, 4097) == 0
    assert L.atdn_epipolar_workspace_bytes(2, 47, 154) == 2 * L.atdn_epipolar_workspace_bytes(1, 47, 154)
    # the Python layer
    calib = (5.0, 5.0, 1.5, 1.5)
    eye = torch.eye(4)[None]
    with pytest.raises(RuntimeError):
        transforms.epipolar_terms(torch.zeros(3, 4, 4), torch.eye(4), calib)
    with pytest.raises(RuntimeError):
        transforms.pose_from_flow(torch.zeros(2, 2, 4, 4), eye, calib)
    with pytest.raises(RuntimeError):
        transforms.pose_from_flow(torch.zeros(1, 2, 4, 4), eye, calib, mask=torch.ones(1, 4, 5))
    with pytest.raises(RuntimeError, match="iters"):
        transforms.pose_from_flow(torch.zeros(1, 2, 4, 4), eye, calib, iters=65)
    with pytest.raises(RuntimeError, match="scale_px"):
        transforms.epipolar_terms(torch.zeros(1, 2, 4, 4), eye, calib, scale_px=0.0)
    with pytest.raises(ValueError, match="skew"):
        transforms.epipolar_terms(torch.zeros(1, 2, 4, 4), eye, [[5.0, 0.1, 1.5], [0, 5.0, 1.5], [0, 0, 1]])
