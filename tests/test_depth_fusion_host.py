"""Keyframe depth fusion, host form: atdn_depth_fuse_host through the raw C ABI and through transforms.fuse_depths on CPU tensors,
against the NumPy float64 restatement of the rule (tests/depth_fusion_ref.py) — every fused bit, every views byte and every
count —, properties that follow from the rule, a closed form, and every argument error. Needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_fusion_ref import (CASES, all_sources, analytic_depth, check_case, check_reference, fuse_ref,  # noqa: E402
                              reference_batch, scene)

# The NumPy helper's own largest relative distance |fused - Z| / Z from the analytic plane depth Z on the disturbance-free scene
# (47 x 154, N = 6, seed 1, no outlier block; test_closed_form prints it): with averaging the agreeing sources' estimates are
# bilinear reads of a depth that is not linear in the pixel, without it the only gap is the float32 rounding of the bank.
PLANE_GAP = {True: 7.3092e-03, False: 5.9376e-08}
PLANE_TOL = {k: 4.0 * v for k, v in PLANE_GAP.items()}

_p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731


def _raw(bank, poses, targets, sources, calib, max_reproj=1.0, max_rel_depth=0.01, min_views=2, min_z=0.1, average=True):
    """atdn_depth_fuse_host through ctypes on NumPy buffers."""
    N, H, W = bank.shape
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    B = len(targets)
    sources = np.ascontiguousarray(sources, dtype=np.int32).reshape(B, -1)
    S = sources.shape[1]
    fused = np.full((B, 1, H, W), -7.0, dtype=np.float32)
    views = np.full((B, H, W), 99, dtype=np.uint8)
    counts = np.full((B, 3), -5, dtype=np.int32)
    L = _lib.lib()
    rc = L.atdn_depth_fuse_host(_p(bank), _p(poses), _p(targets), _p(sources) if S else None, N, B, S, H, W, *calib, max_reproj,
                                max_rel_depth, min_views, min_z, 1 if average else 0, _p(fused), _p(views), _p(counts))
    assert rc == 0, L.atdn_last_error()
    return fused, views, counts


def _host(bank, poses, targets, sources, calib, **kw):
    f, v, c = transforms.fuse_depths(torch.from_numpy(np.ascontiguousarray(bank)), torch.from_numpy(np.ascontiguousarray(poses)),
                                     targets, sources, calib, **kw)
    assert f.dtype == torch.float32 and v.dtype == torch.uint8 and c.dtype == torch.int32 and not f.is_cuda
    return f.numpy(), v.numpy(), c.numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same(got, want):
    return _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("average", [True, False], ids=["average", "plain"])
@pytest.mark.parametrize("name, H, W, N, seed, min_views", CASES, ids=[c[0] for c in CASES])
def test_host_form_equals_the_helper(name, H, W, N, seed, min_views, average):
    """All N targets in one call, every other view a source. margin >= 1e-9, 0 < kept < seen < has < H * W per target and three
    distinct `views` values are asserted on the helper alone (check_case); then every bit, through both doors."""
    bank, poses, calib, _, targets, sources, fused, views, counts = check_case(H, W, N, seed, min_views, average)
    want = (fused, views, counts)
    assert _same(_raw(bank, poses, targets, sources, calib, min_views=min_views, average=average), want)
    got = _host(bank, poses, targets, sources, calib, min_views=min_views, average=average)
    assert _same(got, want)
    assert tuple(got[0].shape) == (N, 1, H, W) and tuple(got[1].shape) == (N, H, W) and tuple(got[2].shape) == (N, 3)
    assert np.array_equal((got[0] != 0).reshape(N, -1).sum(axis=1), counts[:, 2])
    # the other forms of the arguments: poses [N,3,4] and [N,4,4], index tensors, a calibration matrix
    P34 = torch.from_numpy(poses).view(N, 3, 4)
    P44 = torch.cat([P34, torch.tensor([0.0, 0, 0, 1]).view(1, 1, 4).repeat(N, 1, 1)], dim=1)
    K = torch.tensor([[calib[0], 0, calib[2]], [0, calib[1], calib[3]], [0, 0, 1]], dtype=torch.float64)
    for P in (P34, P44):
        f, v, c = transforms.fuse_depths(torch.from_numpy(bank), P, torch.from_numpy(targets).long(), torch.from_numpy(sources), K,
                                         min_views=min_views, average=average)
        assert _same((f.numpy(), v.numpy(), c.numpy()), want)
    # other thresholds
    kw = dict(max_reproj=0.5, max_rel_depth=0.004, min_views=1, min_z=0.5, average=average)
    want = check_reference(bank, poses, targets, sources, calib, strict=False, **kw)
    assert _same(_host(bank, poses, targets, sources, calib, **kw), want)


def test_empty_slots_change_no_bit():
    """-1, out-of-range and self slots inserted anywhere: the same bits as the list without them."""
    name, H, W, N, seed, mv = CASES[1]
    bank, poses, calib, _, targets, sources, fused, views, counts = check_case(H, W, N, seed, mv)
    padded = np.empty((N, 7), dtype=np.int32)
    for i in range(N):
        a, b, c = sources[i]
        padded[i] = [[-1, a, N, b, i, c, -2 ** 31], [i, i, a, b, N + 5, -3, c], [a, b, c, -1, -1, -1, 2 ** 31 - 1],
                     [N, -1, i, a, b, c, i]][i % 4]
    assert _same(_host(bank, poses, targets, padded, calib, min_views=mv), (fused, views, counts))
    assert _same(_raw(bank, poses, targets, padded, calib, min_views=mv), (fused, views, counts))
    assert _same(check_reference(bank, poses, targets, padded, calib, min_views=mv), (fused, views, counts))
    wide = padded.astype(np.int64)
    wide[wide == -2 ** 31], wide[wide == 2 ** 31 - 1] = -2 ** 40, 2 ** 32 + 1    # outside int32: still outside the bank, no wrap-around
    assert _same(_host(bank, poses, targets, torch.from_numpy(wide), calib, min_views=mv), (fused, views, counts))


def test_an_inconsistent_source_leaves_the_pixel_alone():
    """Where source s is not consistent at a pixel, fused and views there are those of the run without s (the pixel's `seen` may
    differ: it is a count, not a pixel value)."""
    name, H, W, N, seed, mv = CASES[3]
    bank, poses, calib, _, targets, sources, _, _, _ = check_case(H, W, N, seed, mv)
    i = 2
    full = fuse_ref(bank, poses, i, list(sources[i]), calib, min_views=mv)
    got = _host(bank, poses, [i], sources[i:i + 1], calib, min_views=mv)
    assert _same_bits(got[0][0, 0], full["fused"]) and np.array_equal(got[1][0], full["views"])
    for s in range(sources.shape[1]):
        rest = np.delete(sources[i], s)[None]
        f, v, _ = _host(bank, poses, [i], rest, calib, min_views=mv)
        out = ~full["consistent"][s]
        assert 0 < out.sum() < out.size
        assert _same_bits(f[0, 0][out], got[0][0, 0][out]) and np.array_equal(v[0][out], got[1][0][out])
        assert (v[0][~out].astype(int) + 1 == got[1][0][~out]).all()


def test_no_source_no_depth():
    name, H, W, N, seed, mv = CASES[2]
    bank, poses, calib, _ = scene(H, W, N, seed)
    for got in (_host(bank, poses, [0, 2], np.zeros((2, 0), dtype=np.int32), calib, min_views=1),
                _raw(bank, poses, [0, 2], np.zeros((2, 0), dtype=np.int32), calib, min_views=1),
                _host(bank, poses, [0, 2], [[-1, 0], [2, N]], calib, min_views=1)):
        assert (got[0] == 0).all() and (got[1] == 0).all()
        assert got[2].tolist() == [[int((bank[0] > 0).sum()), 0, 0], [int((bank[2] > 0).sum()), 0, 0]]


def test_identical_views():
    """The same pose (R = I, so the relative pose is exactly the identity) and the same depth map in every view, with holes of
    their own in two of the sources; fx, fy powers of two and an integer principal point make u = x and v = y exactly. Then every
    source whose four taps at (x, y) are free of holes agrees, n is their number and fused == z, averaged or not."""
    H, W, N = 6, 11, 4
    rs = np.random.RandomState(3)
    z = rs.uniform(2.0, 30.0, size=(H, W)).astype(np.float32)
    bank = np.repeat(z[None], N, axis=0)
    bank[0][rs.uniform(size=(H, W)) < 0.1] = 0
    bank[2][rs.uniform(size=(H, W)) < 0.2] = 0
    bank[3][rs.uniform(size=(H, W)) < 0.2] = 0
    poses = np.repeat(np.array([[1, 0, 0, 0.3, 0, 1, 0, -0.1, 0, 0, 1, 2.0]], dtype=np.float32), N, axis=0)
    calib = (8.0, 16.0, 5.0, 2.0)

    def free(d):                                                          # all four taps of (x, y): itself, right, below, both
        g = np.pad(d > 0, ((0, 1), (0, 1)), mode="edge")
        return g[:-1, :-1] & g[:-1, 1:] & g[1:, :-1] & g[1:, 1:]

    has = bank[0] > 0
    n = np.where(has, sum(free(bank[j]).astype(int) for j in (1, 2, 3)), 0)
    for average in (True, False):
        for mv in (1, 3):
            f, v, c = _host(bank, poses, [0], [[1, 2, 3]], calib, min_views=mv, average=average)
            assert np.array_equal(v[0], n)
            kept = has & (n >= mv)
            assert _same_bits(f[0, 0], np.where(kept, bank[0], 0).astype(np.float32))
            assert c.tolist() == [[int(has.sum()), int((has & (n > 0)).sum()), int(kept.sum())]]
            assert 0 < kept.sum() and (mv == 1 or kept.sum() < has.sum())   # source 1 has no hole: it agrees everywhere
            assert _same((f, v, c), reference_batch(bank, poses, [0], [[1, 2, 3]], calib, min_views=mv, average=average)[:3])


def test_target_outside_the_bank():
    name, H, W, N, seed, mv = CASES[2]
    bank, poses, calib, _ = scene(H, W, N, seed)
    targets, sources = [N, 1, -1], [[0, 1], [0, 2], [0, 1]]
    for got in (_host(bank, poses, targets, sources, calib, min_views=1), _raw(bank, poses, targets, sources, calib, min_views=1)):
        for b in (0, 2):
            assert (got[0][b] == 0).all() and (got[1][b] == 0).all() and (got[2][b] == 0).all()
        assert got[2][1, 2] > 0
        assert _same(got, reference_batch(bank, poses, targets, sources, calib, min_views=1)[:3])


@pytest.mark.parametrize("average", [True, False], ids=["average", "plain"])
def test_closed_form(average):
    """The disturbance-free scene (no outlier block; holes stay): every kept depth against the analytic depth of the planes. The
    helper's own gap is printed and compared with the figure written down above; the host form may be four times that off."""
    name, H, W, N, seed, mv = CASES[3]
    bank, poses, calib, Z = scene(H, W, N, seed, disturbance=0.0, outlier=1.0)
    for k in range(N):
        assert np.array_equal(Z[k], analytic_depth(poses[k], calib, H, W))
    targets, sources = all_sources(N)
    fused, views, counts = check_reference(bank, poses, targets, sources, calib, strict=False, min_views=mv, average=average)
    kept = fused[:, 0] > 0
    assert kept.sum() > 0.7 * N * H * W
    gap = float((np.abs(fused[:, 0].astype(np.float64) - Z) / Z)[kept].max())
    print("helper's largest relative distance from the analytic depth:", gap, "written down:", PLANE_GAP[average])
    assert gap <= PLANE_GAP[average] * 1.0005
    f, v, c = _host(bank, poses, targets, sources, calib, min_views=mv, average=average)
    err = float((np.abs(f[:, 0].astype(np.float64) - Z) / Z)[f[:, 0] > 0].max())
    print("host form:", err, "allowed", PLANE_TOL[average])
    assert np.array_equal(f[:, 0] > 0, kept) and err <= PLANE_TOL[average]


def test_argument_errors():
    L = _lib.lib()
    N, B, S, H, W = 3, 2, 2, 4, 4
    bank = np.ones((N, H, W), dtype=np.float32)
    poses = np.repeat(np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=np.float32), N, axis=0)
    targets = np.array([0, 1], dtype=np.int32)
    sources = np.array([[1, 2], [0, 2]], dtype=np.int32)
    fused = np.zeros((B, 1, H, W), dtype=np.float32)
    views = np.zeros((B, H, W), dtype=np.uint8)
    counts = np.zeros((B + 1, 3), dtype=np.int32)
    good = dict(bank=_p(bank), poses=_p(poses), targets=_p(targets), sources=_p(sources), N=N, B=B, S=S, H=H, W=W, fx=5.0, fy=5.0,
                cx=1.5, cy=1.5, max_reproj=1.0, max_rel_depth=0.01, min_views=1, min_z=0.1, average=1, fused=_p(fused),
                views=_p(views), counts=_p(counts))
    order = ["bank", "poses", "targets", "sources", "N", "B", "S", "H", "W", "fx", "fy", "cx", "cy", "max_reproj", "max_rel_depth",
             "min_views", "min_z", "average", "fused", "views", "counts"]

    def call(**kw):
        a = dict(good, **kw)
        return L.atdn_depth_fuse_host(*[a[k] for k in order])

    assert call() == 0 and call(average=0) == 0 and call(average=7) == 0
    for name in ("bank", "poses", "targets", "sources", "fused", "views", "counts"):
        assert call(**{name: None}) != 0, name
        assert b"null" in L.atdn_last_error()
    assert call(sources=None, S=0) == 0                                   # the one pointer that may be null, and only then
    for name in ("B", "H", "W", "N"):
        assert call(**{name: 0}) != 0 and call(**{name: -1}) != 0, name
    assert call(B=65536) != 0 and b"65535" in L.atdn_last_error()          # checked before any byte is touched
    assert call(H=4097, W=4097) != 0 and b"2^24" in L.atdn_last_error()
    assert call(S=-1) != 0 and call(S=256) != 0
    assert call(min_views=0) != 0 and call(min_views=256) != 0 and call(min_views=255) == 0
    for name in ("fx", "fy"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert call(**{name: v}) != 0, (name, v)
    for name in ("cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert call(**{name: v}) != 0, (name, v)
        assert call(**{name: -3.0}) == 0
    for name in ("max_reproj", "max_rel_depth", "min_z"):
        for v in (0.0, -1e-9, float("nan"), float("inf")):
            assert call(**{name: v}) != 0, (name, v)
            assert name.encode() in L.atdn_last_error()
    # every output against every input and against the other outputs; fusing into the bank in place is an overlap
    n = H * W
    assert call(fused=_p(bank)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(fused=C.c_void_p(bank.ctypes.data + 4 * n)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(fused=C.c_void_p(bank.ctypes.data + 4 * n * (N - 1)), B=1) != 0
    assert call(views=_p(bank)) != 0 and call(counts=_p(bank)) != 0
    for out in ("fused", "views", "counts"):
        for inp in (poses, targets, sources):
            assert call(**{out: _p(inp)}) != 0, out
            assert b"overlap" in L.atdn_last_error()
    assert call(views=_p(fused)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(counts=_p(fused)) != 0 and call(counts=_p(views)) != 0
    assert call(counts=C.c_void_p(fused.ctypes.data + 4 * B * n - 4)) != 0
    assert call(sources=_p(fused), S=0) == 0                               # an unused pointer is not an input
    # the Python layer
    tb, tp = torch.from_numpy(bank), torch.from_numpy(poses)
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(tb[0], tp, [0], [[1]], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(tb, tp[:2], [0], [[1]], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(tb, tp, [0, 1], [[1]], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(tb, tp, [], [], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(tb, tp, torch.tensor([0.0]), [[1]], (5.0, 5.0, 1.5, 1.5))
    with pytest.raises(RuntimeError, match="min_views"):
        transforms.fuse_depths(tb, tp, [0], [[1]], (5.0, 5.0, 1.5, 1.5), min_views=0)
    with pytest.raises(RuntimeError, match="max_reproj"):
        transforms.fuse_depths(tb, tp, [0], [[1]], (5.0, 5.0, 1.5, 1.5), max_reproj=0.0)
    with pytest.raises(ValueError, match="skew"):
        transforms.fuse_depths(tb, tp, [0], [[1]], [[5.0, 0.1, 1.5], [0, 5.0, 1.5], [0, 0, 1]])
