"""Two-view depth, host form: atdn_flow_two_view_depth_host through the raw C ABI and through transforms.two_view_depth on CPU
tensors, against the NumPy float64 restatement of the rule (tests/two_view_ref.py) — every depth bit and every count —, closed
forms, every argument error, and the calibration helpers of atdn_vslam_amd/depth.py against their formulas and against the
reference's own outputs (tests/golden/depth.npz). Needs no GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, depth as depth_mod, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from two_view_ref import (CASES, DEFAULTS, MIN_MARGIN, check_case, min_sin2_of, reference_batch, scene,  # noqa: E402
                          two_view_ref)

# 4 x the reference's own float32-against-float64 gap on each fixture case (tests/golden/make_golden_depth.py prints the gaps)
PROJECT_GAP = {"5x7": 3.353e-06, "47x154": 6.757e-06}
PROJECT_TOL = {k: 4.0 * v for k, v in PROJECT_GAP.items()}


def _host(flow, pose, calib, mask=None, **kw):
    d, c = transforms.two_view_depth(torch.from_numpy(np.ascontiguousarray(flow)), torch.from_numpy(np.ascontiguousarray(pose)),
                                     calib, None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)), **kw)
    assert d.dtype == torch.float32 and c.dtype == torch.int32 and not d.is_cuda
    return d.numpy(), c.numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _pose(R=None, t=(0.0, 0.0, 0.0), B=1):
    P = np.concatenate([np.eye(3) if R is None else np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)
    return np.repeat(P.reshape(1, 12), B, axis=0).astype(np.float32)


def _const(B, H, W, u, v):
    f = np.empty((B, 2, H, W), dtype=np.float32)
    f[:, 0], f[:, 1] = u, v
    return f


@pytest.mark.parametrize("name, H, W, B, seed", CASES, ids=[c[0] for c in CASES])
def test_host_form_equals_the_helper(name, H, W, B, seed):
    """The random scenes (disturbance 1.5 px, default thresholds): margin >= 1e-9 and 0 < valid < inliers < inside < H * W are
    asserted on the helper alone (check_case); then every depth bit and every count, through the 4-d and the 3-d form."""
    flow, pose, calib, _, ref_depth, ref_counts = check_case(H, W, B, seed)
    depth, counts = _host(flow, pose, calib)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
    assert np.array_equal((depth != 0).reshape(B, -1).sum(axis=1), ref_counts[:, 2])
    for b in range(B):
        d3, c3 = transforms.two_view_depth(torch.from_numpy(flow[b]), torch.from_numpy(pose[b]).view(3, 4), calib)
        assert tuple(d3.shape) == (1, H, W) and tuple(c3.shape) == (3,)
        assert _same_bits(d3.numpy(), ref_depth[b]) and np.array_equal(c3.numpy(), ref_counts[b])
    # other thresholds, the pose as [B,4,4], the calibration as a 3x4 matrix
    kw = dict(max_epipolar=0.5, min_parallax_deg=0.2, max_depth=30.0)
    want = reference_batch(flow, pose, calib, max_epipolar=0.5, min_sin2=min_sin2_of(0.2), max_depth=30.0)
    assert want[2] >= MIN_MARGIN
    P44 = np.concatenate([pose.reshape(B, 3, 4), np.tile(np.array([0, 0, 0, 1], dtype=np.float32), (B, 1, 1))], axis=1)
    K = torch.tensor([[calib[0], 0, calib[2], 0.1], [0, calib[1], calib[3], 0.2], [0, 0, 1, 0.3]], dtype=torch.float64)
    depth, counts = _host(flow, P44, K, **kw)
    assert _same_bits(depth, want[0]) and np.array_equal(counts, want[1])


@pytest.mark.parametrize("name, H, W, B, seed", CASES[:3], ids=[c[0] for c in CASES[:3]])
def test_host_form_with_a_mask(name, H, W, B, seed):
    mask = (np.random.RandomState(seed).uniform(size=(B, 1, H, W)) < 0.6).astype(np.uint8)
    flow, pose, calib, _, ref_depth, ref_counts = check_case(H, W, B, seed, mask=mask[:, 0])
    full = check_case(H, W, B, seed)
    depth, counts = _host(flow, pose, calib, mask)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
    assert (depth[mask == 0] == 0).all() and _same_bits(depth[mask != 0], full[4][mask != 0])
    assert (counts <= full[5]).all() and (counts[:, 0] < full[5][:, 0]).all()
    d2, c2 = _host(flow, pose, calib, mask[:, 0] != 0)                   # a bool mask [B,H,W]
    assert _same_bits(d2, depth) and np.array_equal(c2, counts)
    d0, c0 = _host(flow, pose, calib, np.zeros_like(mask))               # a mask that removes everything
    assert (d0 == 0).all() and (c0 == 0).all()


def test_noise_free_scene_recovers_the_depth():
    """Disturbance 0 at 47 x 154: every correspondence lies on its epipolar line up to the float32 rounding of flow and pose, and
    every valid depth is the true one within 1e-5 relative (the rule itself shows 6e-6 here: far points with little parallax)."""
    flow, pose, calib, Z = scene(47, 154, 5, 2, 0.0)
    ref_depth, ref_counts, _ = reference_batch(flow, pose, calib)
    v = ref_depth[:, 0] > 0
    assert (ref_counts[:, 1] == ref_counts[:, 0]).all() and v.sum() > 4000
    assert float((np.abs(ref_depth[:, 0] - Z) / Z)[v].max()) <= 1e-5
    depth, counts = _host(flow, pose, calib)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
    score = transforms.epipolar_score(torch.from_numpy(counts))
    assert score.dtype == torch.float32 and score.tolist() == [1.0, 1.0]


def test_sideways_translation_over_a_plane():
    """R = I, t = (t0, 0, 0), a fronto-parallel plane at Z: X2 = X1 - t, so the flow is u = -fx*t0/Z and depth = fx*t0/(-u).
    fx = 64, t0 = 0.5, Z = 8: u = -4, every quantity of the rule exact up to the last steps."""
    H, W = 6, 12
    calib = (64.0, 64.0, 5.0, 2.0)
    flow, pose = _const(2, H, W, -4.0, 0.0), _pose(t=(0.5, 0.0, 0.0), B=2)
    depth, counts = _host(flow, pose, calib)
    ref_depth, ref_counts, _ = reference_batch(flow, pose, calib)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
    assert counts.tolist() == [[H * (W - 4)] * 3] * 2                    # x2 = x - 4 >= 0
    assert (depth[:, 0, :, :4] == 0).all()
    np.testing.assert_allclose(depth[:, 0, :, 4:], 8.0, rtol=2.0 ** -23, atol=0)
    # twice the disparity: half the depth; the opposite sign: behind the cameras, inliers without a depth
    d2, c2 = _host(_const(1, H, W, -8.0, 0.0), pose[:1], calib)
    np.testing.assert_allclose(d2[0, 0, :, 8:], 4.0, rtol=2.0 ** -23, atol=0)
    d3, c3 = _host(_const(1, H, W, 4.0, 0.0), pose[:1], calib)
    assert (d3 == 0).all() and c3.tolist() == [[H * (W - 4), H * (W - 4), 0]]
    # a vertical flow component of 2 px is 2 px off the (horizontal) epipolar line: out at 1 px, in at 2 px
    off = _const(1, H, W, -4.0, 2.0)
    assert _host(off, pose[:1], calib)[1].tolist() == [[(H - 2) * (W - 4), 0, 0]]
    d4, c4 = _host(off, pose[:1], calib, max_epipolar=2.0)
    assert c4.tolist() == [[(H - 2) * (W - 4)] * 3] and _same_bits(d4, reference_batch(off, pose[:1], calib, max_epipolar=2.0)[0])


def test_closed_forms_without_a_depth():
    H, W = 5, 7
    flow, pose, calib, _ = scene(H, W, 2, 1, 1.5)
    # t = 0: the epipolar line is undefined (0/0): no inliers, no depths, but correspondences inside
    fz, pz, _, _ = scene(H, W, 2, 1, 1.5, zero_translation=True)
    depth, counts = _host(fz, pz, calib)
    assert (depth == 0).all() and counts[0, 0] > 0 and counts[0, 1:].tolist() == [0, 0]
    assert np.array_equal(counts, reference_batch(fz, pz, calib)[1])
    assert transforms.epipolar_score(torch.from_numpy(counts)).tolist() == [0.0]
    # a flow that leaves the image everywhere: nothing inside, and a score of 0 instead of 0/0
    depth, counts = _host(_const(1, H, W, float(W), 0.0), pose, calib)
    assert (depth == 0).all() and (counts == 0).all()
    assert transforms.epipolar_score(torch.from_numpy(counts)).tolist() == [0.0]
    # zero flow and forward motion with R = I: the two rays of every pixel are parallel (det = 0 exactly, z1 = 0/0). Even with
    # min_parallax_deg = 0 nothing is valid; every pixel is an inlier except the one at the epipole (n = 0: 0/0)
    z = np.zeros((1, 2, H, W), dtype=np.float32)
    depth, counts = _host(z, _pose(t=(0.0, 0.0, 1.0)), (4.0, 4.0, 3.0, 2.0), min_parallax_deg=0.0)
    assert (depth == 0).all() and counts.tolist() == [[35, 34, 0]]
    assert np.array_equal(counts, reference_batch(z, _pose(t=(0.0, 0.0, 1.0)), (4.0, 4.0, 3.0, 2.0), min_sin2=0.0)[1])
    # a translation of 1e-40 scales every depth below the smallest normal float32: inliers as before, but no valid depth
    # (the rule asks z1 >= FLT_MIN, so a valid pixel never carries the depth 0 that means "none")
    tiny = pose.copy().reshape(1, 3, 4)
    tiny[:, :, 3] = (tiny[:, :, 3].astype(np.float64) * 1e-40).astype(np.float32)
    tiny = tiny.reshape(1, 12)
    assert np.abs(tiny.reshape(3, 4)[:, 3]).max() > 0
    depth, counts = _host(flow, tiny, calib)
    ref_depth, ref_counts, _ = reference_batch(flow, tiny, calib)
    assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
    assert (depth == 0).all() and counts[0, 1] > 0 and counts[0, 2] == 0


def test_one_pixel_image():
    """1 x 1: the only correspondence inside is the pixel itself (zero flow). Principal point at the pixel, a rotation of 0.1 rad
    about y and t = (-0.5, 0, 0): a = (0,0,1), b = (sin, 0, cos), z2 = 0.5/sin, z1 = 0.5/tan."""
    th = 0.1
    R = [[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]]
    z = np.zeros((1, 2, 1, 1), dtype=np.float32)
    pose = _pose(R, (-0.5, 0.0, 0.0))
    depth, counts = _host(z, pose, (10.0, 10.0, 0.0, 0.0))
    ref_depth, ref_counts, _ = reference_batch(z, pose, (10.0, 10.0, 0.0, 0.0))
    assert _same_bits(depth, ref_depth) and counts.tolist() == [[1, 1, 1]] and np.array_equal(counts, ref_counts)
    np.testing.assert_allclose(depth[0, 0, 0, 0], 0.5 / math.tan(th), rtol=1e-6)
    # any non-zero flow leaves a 1 x 1 image
    f = z.copy()
    f[0, 0] = 0.25
    assert _host(f, pose, (10.0, 10.0, 0.0, 0.0))[1].tolist() == [[0, 0, 0]]
    # R = I: parallel rays, an inlier (principal point off the pixel, so the line exists) without a depth
    assert _host(z, _pose(t=(0.0, 0.0, 1.0)), (10.0, 10.0, 0.5, 0.25))[1].tolist() == [[1, 1, 0]]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_flow_touches_its_pixel_only(bad):
    flow, pose, calib, _, base, base_counts = check_case(9, 33, 3, 3)
    pix = tuple(np.argwhere(base[1, 0] > 0)[5])
    for c in (0, 1):
        f = flow.copy()
        f[1, c][pix] = bad
        depth, counts = _host(f, pose, calib)
        ref_depth, ref_counts, _ = reference_batch(f, pose, calib)
        assert _same_bits(depth, ref_depth) and np.array_equal(counts, ref_counts)
        assert np.argwhere(depth != base).tolist() == [[1, 0, pix[0], pix[1]]] and depth[1, 0][pix] == 0
        assert (counts[1] == base_counts[1] - 1).all() and np.array_equal(counts[[0, 2]], base_counts[[0, 2]])
    # a NaN in the pose: that image has correspondences inside and nothing else; the others are untouched
    p = pose.copy()
    p[1, 3] = bad
    depth, counts = _host(flow, p, calib)
    assert (depth[1] == 0).all() and counts[1, 0] == base_counts[1, 0] and counts[1, 2] == 0
    assert _same_bits(depth[[0, 2]], base[[0, 2]])
    assert np.array_equal(counts, reference_batch(flow, p, calib)[1])


def test_argument_errors():
    L = _lib.lib()
    H, W = 4, 4
    flow = np.zeros((1, 2, H, W), dtype=np.float32)
    pose = _pose(t=(0.1, 0.0, 1.0))
    mask = np.ones((1, H, W), dtype=np.uint8)
    depth = np.zeros((1, 1, H, W), dtype=np.float32)
    counts = np.zeros((2, 3), dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    good = dict(flow=p(flow), pose=p(pose), mask=p(mask), B=1, H=H, W=W, fx=5.0, fy=5.0, cx=1.5, cy=1.5, max_epipolar=1.0,
                min_sin2=1e-6, max_depth=80.0, depth=p(depth), counts=p(counts))

    def call(**kw):
        a = dict(good, **kw)
        return L.atdn_flow_two_view_depth_host(a["flow"], a["pose"], a["mask"], a["B"], a["H"], a["W"], a["fx"], a["fy"], a["cx"],
                                               a["cy"], a["max_epipolar"], a["min_sin2"], a["max_depth"], a["depth"], a["counts"])

    assert call() == 0
    assert call(mask=None) == 0                                          # the mask is the one pointer that may be null
    for name in ("flow", "pose", "depth", "counts"):
        assert call(**{name: None}) != 0, name
        assert b"null" in L.atdn_last_error()
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) != 0 and call(**{name: -1}) != 0, name
    assert call(H=4097, W=4097) != 0 and b"2^24" in L.atdn_last_error()   # checked before any byte is touched
    for name in ("fx", "fy"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert call(**{name: v}) != 0, (name, v)
    for name in ("cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert call(**{name: v}) != 0, (name, v)
        assert call(**{name: -3.0}) == 0
    for name in ("max_epipolar", "min_sin2"):
        for v in (-1e-9, float("nan"), float("inf")):
            assert call(**{name: v}) != 0, (name, v)
        assert call(**{name: 0.0}) == 0
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert call(max_depth=v) != 0, v
    # no output on top of an input or of the other output
    assert call(depth=p(flow)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(depth=C.c_void_p(flow.ctypes.data + 4 * H * W)) != 0      # the second plane of the flow
    assert call(depth=p(mask)) != 0
    assert call(counts=p(pose)) != 0
    assert call(counts=p(flow)) != 0
    assert call(counts=p(depth)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(counts=C.c_void_p(depth.ctypes.data + 4 * H * W - 4)) != 0
    # the Python layer
    with pytest.raises(RuntimeError):
        transforms.two_view_depth(torch.zeros(3, 4, 4), torch.eye(4), (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.two_view_depth(torch.zeros(2, 2, 4, 4), torch.eye(4)[None], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.two_view_depth(torch.zeros(1, 2, 4, 4), torch.eye(4)[None], (5.0, 5.0, 1.5, 1.5), mask=torch.ones(1, 4, 5))
    with pytest.raises(RuntimeError, match="max_depth"):
        transforms.two_view_depth(torch.zeros(1, 2, 4, 4), torch.eye(4)[None], (5.0, 5.0, 1.5, 1.5), max_depth=0.0)
    with pytest.raises(ValueError, match="skew"):
        transforms.two_view_depth(torch.zeros(1, 2, 4, 4), torch.eye(4)[None], [[5.0, 0.1, 1.5], [0, 5.0, 1.5], [0, 0, 1]])


def test_epipolar_score():
    c = torch.tensor([[10, 4, 1], [0, 0, 0], [3, 3, 3]], dtype=torch.int32)
    s = transforms.epipolar_score(c)
    assert s.dtype == torch.float32 and s.tolist() == [float(np.float32(0.4)), 0.0, 1.0]
    assert transforms.epipolar_score(c[0]).dim() == 0


def test_resize_calib_formula():
    k = (718.856, 718.856, 607.1928, 185.2157)
    fx, fy, cx, cy = depth_mod.resize_calib(k, (376, 1241), (376, 1232))
    sx = 1232.0 / 1241.0
    assert (fx, fy, cx, cy) == (718.856 * sx, 718.856 * 1.0, (607.1928 + 0.5) * sx - 0.5, (185.2157 + 0.5) * 1.0 - 0.5)
    # half-pixel centres: the image centre stays the image centre, the identity stays the identity
    fx, fy, cx, cy = depth_mod.resize_calib((100.0, 50.0, (640 - 1) / 2.0, (480 - 1) / 2.0), (480, 640), (240, 960))
    assert (fx, fy) == (150.0, 25.0) and cx == pytest.approx((960 - 1) / 2.0, abs=1e-12) and cy == pytest.approx((240 - 1) / 2.0, abs=1e-12)
    assert depth_mod.resize_calib(k, (376, 1241), (376, 1241)) == k
    # a matrix as input
    K = torch.tensor([[100.0, 0, 30.0], [0, 50.0, 20.0], [0, 0, 1]])
    assert depth_mod.resize_calib(K, (10, 20), (20, 10)) == (50.0, 100.0, 30.5 * 0.5 - 0.5, 20.5 * 2 - 0.5)
    assert depth_mod.intrinsics(K) == (100.0, 50.0, 30.0, 20.0)
    assert depth_mod.intrinsics((1.0, 2.0, 3.0, 4.0)) == (1.0, 2.0, 3.0, 4.0)
    for bad in ([[1.0, 0.5, 0], [0, 1, 0], [0, 0, 1]], [[1.0, 0, 0], [0, 1, 0], [0, 0, 2]], (1.0, 0.0, 0.0, 0.0), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            depth_mod.intrinsics(bad)


def test_read_calib_and_project_depth_match_the_reference(golden_dir, tmp_path):
    """Against the reference's own read_calib / project_depth (tests/golden/depth.npz, written by make_golden_depth.py).
    read_calib: exact. project_depth: the reference inverts the float32 calibration matrix and multiplies in float32, this
    package divides in float64 and rounds once. The reference's own float32-against-float64 gap on the fixture (largest absolute
    difference, coordinates up to 80) is 3.353e-06 at 5 x 7 and 6.757e-06 at 47 x 154; four times that is allowed: 1.3412e-05 and
    2.7028e-05."""
    g = np.load(os.path.join(golden_dir, "depth.npz"))
    path = os.path.join(str(tmp_path), "calib.txt")
    with open(path, "w") as f:
        f.write(str(g["calib_text"]))
    k3, k4 = depth_mod.read_calib(path), depth_mod.read_calib(path, include_rect=True)
    assert k3.dtype == torch.float32 and tuple(k3.shape) == (3, 3) and np.array_equal(k3.numpy(), g["calib_3x3"])
    assert k4.dtype == torch.float32 and tuple(k4.shape) == (4, 4) and np.array_equal(k4.numpy(), g["calib_4x4"])
    assert float(k3[0, 0]) == float(np.float32(718.856))                 # row 1 of the file: P1
    assert float(k4[0, 3]) == float(np.float32(-386.1448))
    for name in [str(n) for n in g["names"]]:
        assert float(g["gap_" + name]) <= PROJECT_GAP[name] * 1.0005      # the figures above are the fixture's own
        d = torch.from_numpy(g["depth_" + name])
        pts = depth_mod.project_depth(d, k3)
        assert pts.dtype == torch.float32 and tuple(pts.shape) == (3,) + tuple(d.shape) and not pts.is_cuda
        err = float(np.abs(pts.numpy().astype(np.float64) - g["points_" + name]).max())
        print(name, "largest difference from the reference", err, "allowed", PROJECT_TOL[name])
        assert err <= PROJECT_TOL[name]
        assert torch.equal(pts[2], d) and torch.equal(depth_mod.project_depth(d[None], k3, device="cpu"), pts)
        assert (pts[:, d == 0] == 0).all()
    with pytest.raises(ValueError, match="skew"):
        depth_mod.project_depth(torch.ones(2, 2), torch.tensor([[5.0, 0.1, 1.0], [0, 5.0, 1.0], [0, 0, 1.0]]))
