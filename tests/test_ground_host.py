"""Ground plane, host form: atdn_ground_*_host through transforms.ground_terms / ground_plane / ground_classify on CPU tensors
against the NumPy float64 restatement of the rule (tests/ground_ref.py) — every bit of q, the 10 sums, the residual plane and the
flags, and every count —, the vote's known answers, accuracy on a tilted plane, on a street with obstacles and along a drive whose
translations are off by a factor, the helpers, and every argument error. Needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, depth as depth_mod, evaluation, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_track_ref as FT  # noqa: E402
import ground_ref as G  # noqa: E402
from ground_ref import CASES, CASE_MIN_VOTES, CASE_N0, H_TRUE, OPTS, same_bits  # noqa: E402
from multiview_ref import euler_yxz  # noqa: E402

LEVEL = (0.0, 1.0, 0.0)
CLASSIFY = {k: v for k, v in OPTS.items() if k != "scale_rel"}


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,H,W,rows,seed", CASES, ids=[c[0] for c in CASES])
def test_host_form_equals_the_restatement(name, H, W, rows, seed, B):
    """The case table, with and without mask, from the vote and from q_init, 0 and 6 steps: q, the 10 sums and the 6 counts of the
    solve, the sums and counts of ground_terms at its q, the residual plane and the flags of ground_classify — bit for bit."""
    depth, mask, calib, q0 = G.case_inputs(H, W, B, seed)
    kw = dict(rows=rows, **OPTS)
    planes = 0
    for masked, voted, iters in G.variants():
        m = mask if masked else None
        want = G.solve_batch(depth, calib, CASE_N0, None if voted else q0, m, iters=iters, min_votes=CASE_MIN_VOTES, **kw)
        q, sums, counts = transforms.ground_plane(_t(depth), calib, CASE_N0, None if voted else _t(q0), _t(m), iters=iters,
                                                  min_votes=CASE_MIN_VOTES, **kw)
        assert q.dtype == torch.float64 and sums.dtype == torch.float64 and counts.dtype == torch.int32 and not q.is_cuda
        assert same_bits(q.numpy(), want[0]) and same_bits(sums.numpy(), want[1]) and np.array_equal(counts.numpy(), want[2])
        assert (counts[:, 5] == -1).all() if not voted else (counts[:, 5] >= 0).all()
        planes += int((counts[:, 1] > 0).sum())
        if iters:
            assert (counts[:, 3] > 0).all()                                   # steps were taken: the step's bits are compared
        ts, tc = transforms.ground_terms(_t(depth), q, calib, _t(m), **kw)
        wts, wtc = G.terms_batch(depth, want[0], calib, m, **kw)
        assert same_bits(ts.numpy(), wts) and np.array_equal(tc.numpy(), wtc)
        assert same_bits(ts.numpy(), sums.numpy()) and np.array_equal(tc.numpy(), counts[:, :3].numpy())
        res, on = transforms.ground_classify(_t(depth), q, calib, _t(m), rows=rows, **CLASSIFY)
        wres, won = G.classify_batch(depth, want[0], calib, m, rows=rows, **CLASSIFY)
        assert tuple(res.shape) == (B, 1, H, W) and res.dtype == torch.float32 and on.dtype == torch.uint8
        assert same_bits(res.numpy(), wres) and same_bits(on.numpy(), won)
        assert int(on.sum()) == int(counts[:, 2].sum())
        y0, y1 = G.default_rows(calib, H) if rows is None else rows
        assert not res[:, :, :y0].any() and not res[:, :, y1:].any() and not on[:, :y0].any()
    assert planes == 8 * B                                                    # every variant found a plane in every image


def test_single_plane_forms():
    """[H,W] depth and [3] q: the batch axis is added and dropped; the default rows are those below the principal point."""
    depth, mask, calib, q0 = G.case_inputs(9, 33, 1, 2)
    q, sums, counts = transforms.ground_plane(_t(depth[0]), calib, LEVEL, iters=2, min_votes=3, **OPTS)
    q4, sums4, counts4 = transforms.ground_plane(_t(depth[:, None]), calib, LEVEL, iters=2, min_votes=3, rows=G.default_rows(calib, 9),
                                                 **OPTS)
    assert tuple(q.shape) == (3,) and tuple(sums.shape) == (10,) and tuple(counts.shape) == (6,)
    assert torch.equal(q, q4[0]) and torch.equal(sums, sums4[0]) and torch.equal(counts, counts4[0])
    assert transforms.ground_rows(calib, 9) == (4, 9) and counts[0] == 5 * 33
    res, on = transforms.ground_classify(_t(depth[0]), q, calib, **CLASSIFY)
    assert tuple(res.shape) == (1, 9, 33) and tuple(on.shape) == (9, 33)


# ------------------------------------------------------------------ the vote, known answers
VOTE_CALIB = (8.0, 8.0, 3.5, -0.5)        # every row of the image lies below the principal point


VOTE_OPTS = dict(OPTS, max_depth=2000.0)  # row 0 has ay = 1/16 exactly: a depth of 16 h stands at height h under the level normal


def _vote(depth, min_votes=1):
    q, sums, counts = transforms.ground_plane(_t(depth), VOTE_CALIB, LEVEL, iters=0, min_votes=min_votes, rows=(0, 1), **VOTE_OPTS)
    return q.numpy(), sums.numpy(), counts.numpy()


def _bin_of(height):
    m, e = np.frexp(height)
    return int((e - 1 + 4) * 32 + np.floor((2 * m - 1) * 32))


def test_vote_constant_height_lands_in_its_bin():
    """One row (ay = 1/16 exactly) of depth 16 h: every pixel's height is h; the mode is h's bin with all votes, and the start is
    the level normal over the bin's centre."""
    for h in (1.65, 0.3, 17.0):
        z = np.full((1, 1, 8), np.float32(16.0 * h), dtype=np.float32)
        hh = float(z[0, 0, 0]) / 16.0
        q, _, counts = _vote(z)
        k = _bin_of(hh)
        assert counts[0].tolist() == [8, 8, counts[0, 2], 0, 8, k]
        assert q[0, 0] == 0.0 and q[0, 2] == 0.0 and q[0, 1] == 1.0 / G.bin_centre(k)
        assert abs(1.0 / q[0, 1] / hh - 1.0) <= 1.0 / 64.0 + 1e-12           # the centre is within half a bin of the height


def test_vote_range_and_bin_edges():
    """Heights exactly at 2^-4 (bin 0), at the bin edges 1.0 (bin 128) and 1 + 1/32 (bin 129), and the last float32 step below
    2^6 (bin 319) are in; 2^6 is out, and so is the last float32 step below 2^-4: used pixels that do not vote."""
    for h, k in ((2.0 ** -4, 0), (1.0, 128), (1.0 + 1.0 / 32.0, 129), (64.0 * (1 - 2.0 ** -24), 319)):
        q, _, counts = _vote(np.full((1, 1, 4), np.float32(16.0 * h)), min_votes=4)
        assert counts[0, :2].tolist() == [4, 4] and counts[0, 4:].tolist() == [4, k], (h, counts)
    for h in (2.0 ** 6, 2.0 ** -4 * (1 - 2.0 ** -24)):
        q, s, counts = _vote(np.full((1, 1, 4), np.float32(16.0 * h)))
        assert not q.any() and not s.any() and not counts.any(), (h, counts)


def test_vote_tie_goes_to_the_lower_bin_and_min_votes():
    """Two groups of three pixels four bins apart: equal smoothed counts, the lower bin wins. One more pixel in the upper group
    and it wins. With min_votes above the mode there is no plane: q = 0, sums = 0, all counts 0."""
    lo, hi = G.bin_centre(100), G.bin_centre(104)
    z = np.array([[[16 * lo] * 3 + [16 * hi] * 3 + [0.0, 0.0]]], dtype=np.float32)
    q, _, counts = _vote(z)
    assert counts[0, :2].tolist() == [8, 6] and counts[0, 4:].tolist() == [3, 100]
    z[0, 0, 6] = 16 * hi
    q, _, counts = _vote(z)
    assert counts[0, 4:].tolist() == [4, 104]
    q, s, counts = transforms.ground_plane(_t(z), VOTE_CALIB, LEVEL, iters=3, min_votes=5, rows=(0, 1), **VOTE_OPTS)
    assert not counts.any()
    assert same_bits(q.numpy(), np.zeros((1, 3))) and same_bits(s.numpy(), np.zeros((1, 10)))
    # neighbours count: two pixels in bin 100 and two in bin 101 are a mode of four in bin 100 (the lowest of the equal 100, 101)
    z = np.array([[[16 * G.bin_centre(100)] * 2 + [16 * G.bin_centre(101)] * 2]], dtype=np.float32)
    q, _, counts = _vote(z, min_votes=4)
    assert counts[0, 4:].tolist() == [4, 100]


# ------------------------------------------------------------------ accuracy
def _errors(q, normal, height):
    q = np.asarray(q)
    h = float(G.height_of(q))
    return abs(h - height) / height, float(np.abs(q * h - normal).max())


def test_accuracy_on_a_tilted_plane_without_noise():
    """A noise-free plane 1.65 m below a camera pitched by 3 and rolled by 2 degrees, in float32 depth at 47 x 154, level prior,
    8 steps: the host form recovers h and n to 10 x what the NumPy restatement yields on the same input. Measured (restatement
    and host form alike, they agree to the bit): relative error of h 1.1e-09, largest error of a component of n 2.2e-10 — the
    float32 rounding of the depths, averaged over 3696 pixels."""
    n = G.tilt_normal(3.0, 2.0)
    depth, calib = G.plane_depth(47, 154, n, H_TRUE)
    ref = G.solve_ref(depth, calib, LEVEL, iters=8, min_votes=8, **OPTS)
    q, sums, counts = transforms.ground_plane(_t(depth), calib, LEVEL, iters=8, min_votes=8, **OPTS)
    eh_ref, en_ref = _errors(ref[0], n, H_TRUE)
    eh, en = _errors(q.numpy(), n, H_TRUE)
    print("tilted plane: restatement h %.3e n %.3e, host form h %.3e n %.3e" % (eh_ref, en_ref, eh, en))
    assert 0 < eh_ref < 1e-6 and 0 < en_ref < 1e-6              # float32 depths: the restatement itself is this good
    assert eh <= 10 * eh_ref and en <= 10 * en_ref
    assert counts[1] == counts[2] == 3696                        # every pixel of the band is an inlier
    normal, height = transforms.ground_height(q)
    assert abs(float(height) - H_TRUE) / H_TRUE <= 10 * eh_ref and float((normal - _t(n)).abs().max()) <= 10 * en_ref
    # the height is known to the relative depth noise times sigma: 3696 pixels on three parameters, sigma is a few per cent
    sigma = float(transforms.ground_sigma(q, sums))
    assert 1.0 / np.sqrt(3696.0) < sigma < 0.2


STREET = dict(H=47, W=154, seed=1)


def test_accuracy_on_a_street_with_obstacles():
    """multiview_ref.scene's street at 47 x 154 (the wall covers half of the rows below the horizon) with 2 % depth noise, 20 %
    holes and 5 % gross outliers, at depth scales 1 and 0.8: the error of h against scale x 1.65 is at most 2 x the restatement's
    on the same input, and under 5 %. Measured (both, they agree to the bit): 0.30 % at both scales."""
    for scale in (1.0, 0.8):
        depth, calib = G.street_depth(STREET["H"], STREET["W"], STREET["seed"], scale=scale)
        ref = G.solve_ref(depth, calib, LEVEL, iters=8, min_votes=8, **OPTS)
        q, sums, counts = transforms.ground_plane(_t(depth), calib, LEVEL, iters=8, min_votes=8, **OPTS)
        e_ref = abs(float(G.height_of(ref[0])) / (scale * H_TRUE) - 1.0)
        e = abs(float(G.height_of(q.numpy())) / (scale * H_TRUE) - 1.0)
        print("street, scale %.1f: restatement %.4f, host form %.4f, counts %s" % (scale, e_ref, e, counts.tolist()))
        assert e <= 2 * e_ref and e < 0.05
        assert bool(transforms.ground_accept(q, counts, LEVEL, min_inlier_share=0.2, max_tilt_deg=10.0))


def test_the_vote_is_needed():
    """On the restatement alone: on the street above, a solve without the vote from q_init at twice the true height ends with
    fewer than 10 % of the inliers the vote's solve ends with (measured: 11 against 1357) — under a redescending loss of scale
    5 % a start 50 % off sees no gradient from the road and settles on the few pixels that happen to lie on its plane."""
    depth, calib = G.street_depth(STREET["H"], STREET["W"], STREET["seed"])
    voted = G.solve_ref(depth, calib, LEVEL, iters=8, min_votes=8, **OPTS)
    blind = G.solve_ref(depth, calib, q_init=np.array(LEVEL) / (2 * H_TRUE), iters=8, **OPTS)
    print("inliers: vote %d, from twice the height %d" % (voted[2][2], blind[2][2]))
    assert voted[2][2] > 1000 and blind[2][2] < 0.1 * voted[2][2]


@pytest.fixture(scope="module")
def drive_scales():
    """Per translation factor: (recovered scale of the host form, of the restatement) on the track depth of the drive."""
    flows, rels, calib, Z0 = FT.drive(**FT.DRIVE)
    out = {}
    for factor in (0.85, 1.0, 1.2):
        track = depth_mod.FlowTrack((FT.DRIVE["H"], FT.DRIVE["W"]), calib, "cpu")
        track.start()
        for k in range(len(flows)):
            rel = rels[k].copy()
            rel[:3, 3] *= factor
            track.extend(_t(flows[k]), _t(rel))
        q, sums, counts = transforms.ground_plane(track.depth, calib, LEVEL, iters=8, min_votes=8, **OPTS)
        ref = G.solve_ref(track.depth[0, 0].numpy(), calib, LEVEL, iters=8, min_votes=8, **OPTS)
        _, height = transforms.ground_height(q)
        out[factor] = (H_TRUE / float(height[0]), H_TRUE / float(G.height_of(ref[0])), counts[0].tolist())
    return out


@pytest.mark.parametrize("factor", [0.85, 1.0, 1.2])
def test_scale_along_the_drive(drive_scales, factor):
    """What the feature is for. flow_track_ref.drive (47 x 154, 8 steps, 0.3 px flow noise) through FlowTrack on the host with
    every pair's translation multiplied by 0.85 / 1 / 1.2, then ground_plane on the track's depth with camera_height 1.65: the
    recovered scale camera_height / h is within 2 x the restatement's own error of 1 / factor. Measured (both): the scale is off
    by 1.27 % / 1.21 % / 0.95 % (1.1615 / 0.9879 / 0.8254 against 1.1765 / 1 / 0.8333)."""
    scale, scale_ref, counts = drive_scales[factor]
    e, e_ref = abs(scale * factor - 1.0), abs(scale_ref * factor - 1.0)
    print("drive x %.2f: scale %.4f (true %.4f), off by %.4f; restatement off by %.4f; counts %s" %
          (factor, scale, 1 / factor, e, e_ref, counts))
    assert e <= 2 * e_ref and e < 0.05


# ------------------------------------------------------------------ helpers and errors
def test_rescale_intervals():
    """Three keyframes: the relative motions' translations times (2, 0.5), re-chained — against the chain written out by hand
    with 4 x 4 products. Scale 1 everywhere returns the input's bits."""
    rs = np.random.RandomState(3)
    P = [np.eye(4)]
    for k in range(2):
        M = np.eye(4)
        M[:3, :3] = euler_yxz(rs.uniform(-0.3, 0.3, 3))
        M[:3, 3] = rs.uniform(-1, 1, 3) + [0, 0, 2]
        P.append(P[-1] @ M)
    P = np.stack(P).astype(np.float32).astype(np.float64)
    want = [P[0]]
    for i, s in enumerate((2.0, 0.5)):
        rel = np.linalg.inv(P[i]) @ P[i + 1]
        rel[:3, 3] *= s
        want.append(want[-1] @ rel)
    got = evaluation.rescale_intervals(P, [2.0, 0.5])
    assert got.dtype == np.float64 and got.shape == (3, 4, 4)
    np.testing.assert_allclose(got, np.stack(want), rtol=0, atol=1e-6)      # P is float32-rounded: R R^T = I to 1e-7
    np.testing.assert_array_equal(got[:, :3, :3], P[:, :3, :3])
    np.testing.assert_allclose(got[1, :3, 3], P[0, :3, 3] + 2.0 * (P[1, :3, 3] - P[0, :3, 3]), rtol=0, atol=1e-15)
    np.testing.assert_allclose(got[2, :3, 3], got[1, :3, 3] + 0.5 * (P[2, :3, 3] - P[1, :3, 3]), rtol=0, atol=1e-15)
    rows = P[:, :3, :].reshape(3, 12)
    same = evaluation.rescale_intervals(rows, [1.0, 1.0])
    assert same_bits(same[:, :3, :].reshape(3, 12), rows)
    assert same_bits(evaluation.rescale_intervals(torch.from_numpy(rows).float(), np.ones(2)), P)
    for bad in ([1.0], [1.0, 0.0], [1.0, np.nan], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            evaluation.rescale_intervals(P, bad)


def test_height_sigma_and_accept_helpers():
    q = torch.tensor([[0.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.3, 0.4, 0.0]], dtype=torch.float64)
    normal, height = transforms.ground_height(q)
    assert torch.equal(height, torch.tensor([2.0, 0.0, 2.0], dtype=torch.float64))
    assert torch.allclose(normal, torch.tensor([[0, 1.0, 0], [0, 0, 0], [0.6, 0.8, 0]], dtype=torch.float64), atol=1e-15)
    # H = 4 I: u = q / |q|^2 = (0, 2, 0), u^T H^-1 u = 1
    sums = torch.zeros((3, 10), dtype=torch.float64)
    sums[:, 0] = sums[:, 3] = sums[:, 5] = 4.0
    sigma = transforms.ground_sigma(q, sums)
    assert abs(float(sigma[0]) - 1.0) < 1e-15 and torch.isinf(sigma[1]) and abs(float(sigma[2]) - 1.0) < 1e-15
    assert torch.isinf(transforms.ground_sigma(q[0], torch.zeros(10, dtype=torch.float64)))
    counts = torch.tensor([[10, 10, 5, 0, 0, 0], [0, 0, 0, 0, 0, 0], [10, 10, 5, 0, 0, 0]], dtype=torch.int32)
    assert transforms.ground_accept(q, counts, LEVEL, min_inlier_share=0.5, max_tilt_deg=40.0).tolist() == [True, False, True]
    assert transforms.ground_accept(q, counts, LEVEL, min_inlier_share=0.6, max_tilt_deg=40.0).tolist() == [False, False, False]
    assert transforms.ground_accept(q, counts, LEVEL, min_inlier_share=0.5, max_tilt_deg=30.0).tolist() == [True, False, False]


def _solve_args(depth, mask, q_init, B, H, W, q, sums, counts, **over):
    v = dict(y0=0, y1=H, fx=8.0, fy=8.0, cx=1.0, cy=1.0, nx=0.0, ny=1.0, nz=0.0, scale_rel=0.05, inlier_rel=0.05, min_z=0.1,
             max_depth=80.0, min_votes=1, iters=2)
    v.update(over)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
    return (p(depth), p(mask), p(q_init), B, H, W, v["y0"], v["y1"], v["fx"], v["fy"], v["cx"], v["cy"], v["nx"], v["ny"], v["nz"],
            v["scale_rel"], v["inlier_rel"], v["min_z"], v["max_depth"], v["min_votes"], v["iters"], p(q), p(sums), p(counts))


def test_argument_errors_of_every_entry_point():
    L = _lib.lib()
    B, H, W = 2, 4, 6
    depth = np.ones((B, H, W), dtype=np.float32)
    mask = np.ones((B, H, W), dtype=np.uint8)
    q0 = np.zeros((B, 3))
    q, sums, counts = np.zeros((B, 3)), np.zeros((B, 10)), np.zeros((B, 6), dtype=np.int32)
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, B, H, W, q, sums, counts)) == 0
    assert L.atdn_ground_solve_host(*_solve_args(depth, None, None, B, H, W, q, sums, counts)) == 0
    bad = [dict(y0=-1), dict(y0=2, y1=2), dict(y1=H + 1), dict(fx=0.0), dict(fy=np.nan), dict(cx=np.inf), dict(cy=np.nan),
           dict(ny=0.0), dict(nx=np.nan), dict(nz=np.inf), dict(scale_rel=0.0), dict(scale_rel=np.inf), dict(inlier_rel=-1.0),
           dict(inlier_rel=np.nan), dict(min_z=0.0), dict(min_z=np.inf), dict(max_depth=0.0), dict(max_depth=np.inf),
           dict(min_votes=0), dict(iters=-1), dict(iters=65)]
    for over in bad:
        assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, B, H, W, q, sums, counts, **over)) != 0, over
        assert L.atdn_last_error()
    for nulls in ((None, mask, q0, q, sums, counts), (depth, mask, q0, None, sums, counts), (depth, mask, q0, q, None, counts),
                  (depth, mask, q0, q, sums, None)):
        d, m, qi, qq, ss, cc = nulls
        assert L.atdn_ground_solve_host(*_solve_args(d, m, qi, B, H, W, qq, ss, cc)) != 0
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, 0, H, W, q, sums, counts)) != 0
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, B, 4097, 4097, q, sums, counts, y1=1)) != 0     # H * W > 2^24
    # overlap: an output on an input, two outputs on each other
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, B, H, W, q0, sums, counts)) != 0
    inside = sums.reshape(-1)[:3 * B].reshape(B, 3)
    assert np.shares_memory(inside, sums)
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, q0, B, H, W, inside, sums, counts)) != 0
    # alignment of q
    raw = np.zeros(8 * 3 * B + 8, dtype=np.uint8)
    off = raw[4:4 + 24 * B].view(np.uint8)
    assert off.ctypes.data % 8 == 4
    assert L.atdn_ground_solve_host(*_solve_args(depth, mask, off, B, H, W, q, sums, counts)) != 0
    # the Python layer: shapes, devices of the pieces, the missing q
    t = torch.from_numpy
    with pytest.raises(RuntimeError):
        transforms.ground_plane(t(depth)[:, None, None], (8.0, 8.0, 1.0, 1.0), **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_plane(t(depth), (8.0, 8.0, 1.0, 1.0), mask=t(mask)[:1], **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_plane(t(depth), (8.0, 8.0, 1.0, 1.0), q_init=t(q0)[:1], **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_plane(t(depth), (8.0, 8.0, 1.0, 1.0), normal_prior=(0.0, 1.0), **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_plane(t(depth), (8.0, 8.0, 1.0, 7.0), **OPTS)            # no row below the principal point
    with pytest.raises(RuntimeError):
        transforms.ground_terms(t(depth), None, (8.0, 8.0, 1.0, 1.0), **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_classify(t(depth), None, (8.0, 8.0, 1.0, 1.0), **CLASSIFY)
    with pytest.raises(RuntimeError):
        transforms.ground_terms(t(depth), t(q0), (8.0, 8.0, 1.0, 1.0), rows=(3, 2), **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_classify(t(depth), t(q0), (8.0, 8.0, 1.0, 1.0), rows=(0, 5), **CLASSIFY)
    with pytest.raises(RuntimeError):
        transforms.ground_terms(t(depth), t(q0), (8.0, 8.0, 1.0, 1.0), **dict(OPTS, scale_rel=0.0))
    with pytest.raises(RuntimeError):
        transforms.ground_classify(t(depth), t(q0), (8.0, 8.0, 1.0, 1.0), **dict(CLASSIFY, inlier_rel=float("nan")))
