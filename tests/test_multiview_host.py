"""Multi-view keyframe depth, the host form (atdn_multiview_depth_host, csrc/multiview_depth_host.h) against the NumPy float64
restatement of the rule (tests/multiview_ref.py): every depth and information bit, every views byte and every count, exactly
(the scenes keep every decision at least 1e-9 from its threshold, asserted on the helper alone); closed forms, non-finite inputs,
argument errors, per-pixel optimality and the statistics the feature is for. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiview_ref as R  # noqa: E402
from two_view_ref import two_view_ref  # noqa: E402


def _host(acc, alive, poses, slots, calib, depth_init=None, **kw):
    out = transforms.multiview_depth(torch.from_numpy(np.ascontiguousarray(acc)), torch.from_numpy(np.ascontiguousarray(alive)),
                                     torch.from_numpy(np.ascontiguousarray(poses)), np.asarray(slots).tolist(), calib,
                                     depth_init=None if depth_init is None else torch.from_numpy(np.ascontiguousarray(depth_init)), **kw)
    d, i, v, c = out
    assert d.dtype == torch.float32 and i.dtype == torch.float32 and v.dtype == torch.uint8 and c.dtype == torch.int32
    return tuple(t.numpy() for t in out)


def _host_case(sc, slots, init, **kw):
    return _host(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], init, **kw)


CASE_ITERS = [(c, it) for c in R.CASES for it in ((0, 1, 4) if c[0].startswith("47x154") else (4,))]


@pytest.mark.parametrize("case, iters", CASE_ITERS, ids=["%s_it%d" % (c[0], it) for c, it in CASE_ITERS])
def test_host_form_equals_the_reference(case, iters):
    """5 x 7, B = 1, S = 2; 9 x 33, B = 3, S = 5 with skipped slots (-1 and N), an odd plane and another view list per problem;
    47 x 154, S = 8 with 0, 1 and 4 steps. R.reference asserts on the helper alone that every problem takes every branch:
    0 < valid < solved < candidates < H * W, a start from depth_init, one from the linear solution, a rejected step (iters > 0)."""
    sc, slots, init, want, _ = R.reference(case, iters)
    assert R.same_outputs(_host_case(sc, slots, init, iters=iters, **case[8]), want)


def test_without_an_initial_depth_and_one_problem_of_a_batch():
    case = R.CASES[1]
    name, H, W, B, S, N, seed, opts, kw, skipped = case
    sc, slots, init, want, _ = R.reference(case)
    d, i, v, c, margin, per = R.reference_batch(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], None)
    assert margin >= R.MIN_MARGIN and not any(o["from_init"].any() for o in per)
    assert R.same_outputs(_host_case(sc, slots, None), (d, i, v, c))
    for b in range(B):                                               # a problem alone gives its part of the batch
        got = _host_case(sc, slots[b], init[b:b + 1])
        assert R.same_outputs(got, tuple(w[b:b + 1] for w in want)), b


def test_returned_depth_is_no_worse_than_its_starts():
    """Per-pixel optimality on the helper's cost function, at the bits the library returns (the reference equals them): at every
    solved pixel cost(rho) <= the cost of whichever starts existed, and a valid depth is (float)(1 / rho)."""
    for case in R.CASES:
        sc, slots, init, want, per = R.reference(case)
        assert R.same_outputs(_host_case(sc, slots, init, **case[8]), want)
        for b, o in enumerate(per):
            pr, rho, solved = o["problem"], o["rho"], o["solved"]
            safe = np.where(solved, rho, 1.0)
            cost = pr.evaluate(safe)[2]
            with np.errstate(all="ignore"):
                lin = pr.linear()
                c_lin = pr.evaluate(np.where(o["has_lin"], lin[0] / lin[1], 1.0))[2]
                c_init = pr.evaluate(np.where(o["has_init"], 1.0 / init[b, 0].astype(np.float64), 1.0))[2]
            assert (o["has_lin"] | o["has_init"]).sum() == solved.sum() > 0
            assert (cost <= c_lin)[o["has_lin"]].all() and (cost <= c_init)[o["has_init"]].all()
            assert (cost < c_lin)[o["has_lin"]].any()                # and the steps do something
            assert np.array_equal(want[0][b, 0][o["valid"]], (1.0 / rho[o["valid"]]).astype(np.float32))


# ------------------------------------------------------------------ closed forms
# 24 x 40, four views, a camera of 60 pixels focal length and a wall no farther than 40 m: enough parallax off the image centre
CLEAN = dict(H=24, W=40, N=4, seed=2)


def _clean():
    return R.scene(CLEAN["H"], CLEAN["W"], CLEAN["N"], CLEAN["seed"], far=40.0, calib=(60.0, 60.0, 19.8, 11.3))


def _rounding_bound(info, W, S):
    """The relative depth error that float32 rounding alone can cause on noise-free views: each flow component is off by at most
    half an ulp, delta <= 2^-24 * W pixels; to first order the least-squares estimate moves by sum(J rho delta) / sum((J rho)^2)
    <= |delta| / sqrt(info) with |delta| <= sqrt(2 S) delta (Cauchy-Schwarz; the weights are 1 to 1e-12 at such residuals); the
    depth itself is rounded to float32 once (2^-24). Doubled: the second-order terms and the float64 arithmetic are far below."""
    delta = 2.0 ** -24 * W
    return 2.0 * (2.0 ** -24 + np.sqrt(2.0 * S) * delta / np.sqrt(info))


def test_noise_free_views_return_the_true_depth():
    sc = _clean()
    N = CLEAN["N"]
    for init in (None, (1.3 * sc["Z"]).astype(np.float32)[None, None]):
        d, i, v, c = _host(sc["acc"], sc["alive"], sc["poses"], [list(range(N))], sc["calib"], init)
        ok = d[0, 0] > 0
        assert c[0, 2] == ok.sum() > 200
        err = np.abs(d[0, 0].astype(np.float64) - sc["Z"]) / sc["Z"]
        assert (err[ok] <= _rounding_bound(i[0, 0][ok].astype(np.float64), CLEAN["W"], N)).all()
        assert (v[0][ok] >= 2).all() and (i[0, 0][ok] >= 16.0).all() and (d[0, 0][ok] <= 80.0).all()
        assert (i[0, 0][~ok] == 0).all()


def test_no_baseline_solves_nothing():
    """Every t = 0: den = 0, the linear start is 0/0; without an initial depth no pixel is solved, but they are candidates."""
    sc = _clean()
    poses = sc["poses"].copy()
    poses[:, 3::4] = 0.0
    d, i, v, c = _host(sc["acc"], sc["alive"], poses, [[0, 1, 2, 3]], sc["calib"])
    assert c[0, 0] > 0 and c[0, 1] == 0 and c[0, 2] == 0
    assert not d.any() and not i.any() and not v.any()


def test_a_single_view_agrees_with_the_two_view_depth():
    """S = 1, min_views = 1 on a noise-free view, asking for sigma_z / z <= 1 only (a single view a metre ahead has little
    parallax): where both rules give a depth it has the same sign and size. Both estimators are exact on exact data; float32
    rounding of the flow moves the multi-view depth by at most _rounding_bound (4e-6 at info >= 16, 1/sqrt(info) times that
    below) and the two-view depth by a like amount at the same parallax, so 1e-4 at info >= 16 and 4e-4 at info >= 1 are ten times
    what rounding explains and far below any real disagreement (a wrong sign, a swapped pose convention, another scale)."""
    sc = _clean()
    for k in (0, 3):
        d, i, v, c = _host(sc["acc"], sc["alive"], sc["poses"], [[k]], sc["calib"], min_views=1, max_rel_sigma=1.0)
        z2, _, _ = two_view_ref(sc["acc"][k], sc["poses"][k], sc["calib"], sc["alive"][k])
        both = (d[0, 0] > 0) & (z2 > 0)
        assert both.sum() > 200
        rel = np.abs(d[0, 0].astype(np.float64) - z2) / np.where(both, z2, 1.0)
        well = both & (i[0, 0] >= 16.0)
        assert (rel[well] <= 1e-4).all() and (rel[both] <= 4e-4).all() and (k == 0 or well.sum() > 50)
        assert (v[0][d[0, 0] > 0] == 1).all()


def test_too_few_observations_is_no_candidate():
    sc = _clean()
    alive = sc["alive"].copy()
    alive[1:, :, :7] = 0                                              # the left columns: seen by view 0 alone
    alive[:, 3, :] = 0                                                # a row: by nobody
    ref = R.multiview_ref(sc["acc"], alive, sc["poses"], [0, 1, 2, 3], sc["calib"])
    d, i, v, c = _host(sc["acc"], alive, sc["poses"], [[0, 1, 2, 3]], sc["calib"])
    assert R.same_outputs((d[0, 0], i[0, 0], v[0], c[0]), (ref["depth"], ref["info"], ref["views"], ref["counts"]))
    assert not ref["cand"][:, :7].any() and not ref["cand"][3].any() and ref["cand"][5, 10:28].all()
    assert not d[0, 0][:, :7].any() and not v[0][:, :7].any() and c[0, 0] == ref["cand"].sum() < d[0, 0].size
    _, _, v1, c1 = _host(sc["acc"], alive, sc["poses"], [[0, 1, 2, 3]], sc["calib"], min_views=1)
    assert c1[0, 0] > c[0, 0] and (v1[0][:, :7] == 1).any() and not v1[0][3].any()      # with min_views = 1 they are solved


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
def test_non_finite_flow_removes_that_view_at_that_pixel_only(bad):
    sc = _clean()
    slots = [[0, 1, 2, 3], [3, 2, 1, 0]]
    clean = _host(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"])
    for ch in (0, 1):
        acc, alive = sc["acc"].copy(), sc["alive"].copy()
        acc[2, ch, 20, 33] = bad
        alive[2, 20, 33] = 0                                           # the same inputs with that view dead at that pixel
        want = _host(sc["acc"], alive, sc["poses"], slots, sc["calib"])
        got = _host(acc, sc["alive"], sc["poses"], slots, sc["calib"])
        assert R.same_outputs(got, want)
        assert clean[0][0, 0, 20, 33] > 0 and got[0][0, 0, 20, 33] > 0  # three views are left
        keep = np.ones(clean[0].shape, dtype=bool)
        keep[:, :, 20, 33] = False
        assert np.array_equal(got[0][keep], clean[0][keep]) and np.array_equal(got[1][keep], clean[1][keep])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
def test_non_finite_pose(bad):
    """In one pose, rotation or translation: the reference's bits; a problem that does not list the view is untouched; where the
    view is observed the linear start fails, so without an initial depth nothing is solved there."""
    sc = _clean()
    slots = np.array([[0, 1, 2], [0, 3, 2]], dtype=np.int32)
    init = np.repeat((1.1 * sc["Z"]).astype(np.float32)[None, None], 2, axis=0)
    clean = _host(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], init)
    for j in (0, 5, 11):
        poses = sc["poses"].copy()
        poses[1, j] = bad
        d, i, v, c, _, per = R.reference_batch(sc["acc"], sc["alive"], poses, slots, sc["calib"], init)
        got = _host(sc["acc"], sc["alive"], poses, slots, sc["calib"], init)
        assert R.same_outputs(got, (d, i, v, c)), j
        assert all(R.same_bits(g[1], w[1]) for g, w in zip(got, clean)), j
        none = _host(sc["acc"], sc["alive"], poses, slots, sc["calib"])
        seen = per[0]["problem"].views[1]["obs"]
        assert seen.any() and not none[0][0, 0][seen].any() and not none[2][0][seen].any()
        assert none[3][0, 1] < clean[3][0, 1] and np.array_equal(none[3][1], _host(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"])[3][1])


# ------------------------------------------------------------------ argument errors
def test_argument_errors_are_refused_with_a_message():
    L = _lib.lib()
    N, B, S, H, W = 3, 2, 2, 4, 5
    n = H * W
    arr = dict(acc_bank=np.zeros((N, 2, H, W), np.float32), alive_bank=np.ones((N, H, W), np.uint8),
               poses=np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (N, 1)), slots=np.array([[0, 1], [1, 2]], np.int32),
               depth_init=np.zeros((B, 1, H, W), np.float32), depth=np.zeros((B, 1, H, W), np.float32),
               info=np.zeros((B, 1, H, W), np.float32), views=np.zeros((B, H, W), np.uint8), counts=np.zeros((B, 3), np.int32))
    ptr = {k: C.c_void_p(a.ctypes.data) for k, a in arr.items()}
    num = dict(N=N, B=B, S=S, H=H, W=W, fx=5.0, fy=5.0, cx=2.0, cy=1.5, scale_px=4.0, inlier_px=2.0, min_z=0.1, min_views=2,
               max_rel_sigma=0.25, max_depth=80.0, iters=4)

    def call(**kw):
        a = dict(ptr, **{k: v for k, v in kw.items() if k in ptr})
        s = dict(num, **{k: v for k, v in kw.items() if k in num})
        return L.atdn_multiview_depth_host(a["acc_bank"], a["alive_bank"], a["poses"], a["slots"], a["depth_init"], s["N"], s["B"],
                                           s["S"], s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"], s["scale_px"], s["inlier_px"],
                                           s["min_z"], s["min_views"], s["max_rel_sigma"], s["max_depth"], s["iters"], a["depth"],
                                           a["info"], a["views"], a["counts"])

    def refused(word, **kw):
        assert call(**kw) != 0, kw
        msg = L.atdn_last_error()
        assert msg and word.encode() in msg, (kw, msg)

    assert call() == 0 and call(depth_init=None) == 0 and call(iters=0) == 0 and call(iters=16) == 0 and call(min_views=1) == 0
    for name in ptr:
        if name != "depth_init":
            refused("null", **{name: None})
    refused("N >= 1", N=0)
    for bad in (dict(B=0), dict(H=0), dict(W=0)):
        refused("bad batch or image size", **bad)
    refused("B <= 65535", B=65536)
    refused("H * W <= 2^24", H=4097, W=4096)
    refused("S must be", S=0)
    refused("S must be", S=17)
    refused("min_views", min_views=0)
    refused("min_views", min_views=S + 1)
    refused("iters", iters=-1)
    refused("iters", iters=17)
    for name in ("fx", "fy"):
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused("fx and fy", **{name: bad})
    for name in ("cx", "cy"):
        for bad in (np.nan, np.inf, -np.inf):
            refused("cx and cy", **{name: bad})
    for name in ("scale_px", "inlier_px", "min_z", "max_rel_sigma", "max_depth"):
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused(name, **{name: bad})
    for out, size in (("depth", 4 * B * n), ("info", 4 * B * n), ("views", B * n), ("counts", 12 * B)):
        for inp in ("acc_bank", "alive_bank", "poses", "slots", "depth_init"):
            refused("overlaps an input", **{out: ptr[inp]})
        # the last byte of the output on the first byte of an input
        refused("overlaps an input", **{out: C.c_void_p(arr["acc_bank"].ctypes.data - size + 1)})
    for a, b in (("depth", "info"), ("depth", "views"), ("depth", "counts"), ("info", "views"), ("info", "counts"), ("views", "counts")):
        refused("two outputs overlap", **{b: ptr[a]})
    with pytest.raises(RuntimeError, match="flow bank"):
        transforms.multiview_depth(torch.zeros(3, H, W), torch.ones(3, H, W, dtype=torch.uint8), torch.zeros(3, 12), [[0]], (5.0, 5.0, 2.0, 1.5))
    with pytest.raises(RuntimeError, match="min_views"):
        transforms.multiview_depth(torch.from_numpy(arr["acc_bank"]), torch.from_numpy(arr["alive_bank"]), torch.from_numpy(arr["poses"]),
                                   [[0]], (5.0, 5.0, 2.0, 1.5))
    with pytest.raises(RuntimeError, match="integers"):
        transforms.multiview_depth(torch.from_numpy(arr["acc_bank"]), torch.from_numpy(arr["alive_bank"]), torch.from_numpy(arr["poses"]),
                                   torch.tensor([[0.0, 1.0]]), (5.0, 5.0, 2.0, 1.5))


# ------------------------------------------------------------------ what the feature is for
@pytest.fixture(scope="module")
def stat_scene():
    """48 x 160, 8 views a metre apart, 0.3 px Gaussian noise on every correspondence, true poses: the scene, the depth the flow
    track's own rule leaves (the last valid two-view triangulation, by flow_track_ref) and the multi-view solve started from it."""
    o = dict(R.STAT_CASE)
    sc = R.scene(o.pop("H"), o.pop("W"), o.pop("N"), o.pop("seed"), **o)
    track = R.last_valid_two_view(sc["acc"], sc["alive"], sc["poses"], sc["calib"])
    d, i, v, c = _host(sc["acc"], sc["alive"], sc["poses"], [list(range(R.STAT_CASE["N"]))], sc["calib"], track[None, None])
    return sc, track, d[0, 0], i[0, 0]


def test_information_is_calibrated(stat_scene):
    """sigma_z / z = noise / sqrt(info): the median of |z - z_true| / (z_true * 0.3 / sqrt(info)) over the valid pixels is that of
    |N(0, 1)|, 0.6745, if the information is what it says; the issue's bounds are [0.5, 0.9]."""
    sc, _, d, info = stat_scene
    ok = d > 0
    assert ok.sum() > 2000
    ratio = np.abs(d[ok].astype(np.float64) - sc["Z"][ok]) / (sc["Z"][ok] * R.STAT_CASE["noise"] / np.sqrt(info[ok].astype(np.float64)))
    med = float(np.median(ratio))
    print("median |error| / sigma = %.4f over %d pixels" % (med, ok.sum()))
    assert 0.5 <= med <= 0.9, med


def test_median_error_is_below_the_flow_tracks(stat_scene):
    sc, track, d, _ = stat_scene
    both = (d > 0) & (track > 0)
    assert both.sum() > 2000
    Z = sc["Z"][both]
    e_mv = float(np.median(np.abs(d[both].astype(np.float64) - Z) / Z))
    e_tr = float(np.median(np.abs(track[both].astype(np.float64) - Z) / Z))
    print("median relative error: multi-view %.5f, last valid two-view %.5f over %d pixels" % (e_mv, e_tr, both.sum()))
    assert e_mv < e_tr, (e_mv, e_tr)
