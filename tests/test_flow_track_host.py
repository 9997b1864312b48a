"""Flow track, host form: atdn_flow_track_step_host through the raw C ABI and through transforms.flow_track_step on CPU tensors,
against the NumPy float64 restatement of the rule (tests/flow_track_ref.py) — every bit of acc, alive and depth and every count, at
every step —, its composition from the chain-only form and the two-view rule, closed forms, non-finite inputs, every argument
error, and what the feature is for: the depth of a drive gets better with every frame of the keyframe interval. Needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, depth as depth_mod, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_track_ref as R  # noqa: E402
from flow_track_ref import CASES, MIN_MARGIN, same_bits, same_steps  # noqa: E402


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _n(t):
    return None if t is None else t.numpy()


def host_step(flow, mask, acc, alive, pose, calib, depth, **kw):
    """transforms.flow_track_step on CPU tensors, out of place: the inputs keep their values."""
    a, l, d, c = transforms.flow_track_step(_t(flow), _t(acc), _t(alive), pose=_t(pose), calib=calib, mask=_t(mask),
                                            depth=None if depth is None else _t(depth.copy()), **kw)
    assert a.dtype == torch.float32 and l.dtype == torch.uint8 and c.dtype == torch.int32 and not a.is_cuda
    assert (d is None) == (pose is None)
    return _n(a), _n(l), _n(d), _n(c)


@pytest.fixture(scope="module")
def specials():
    return R.special_sequences()


@pytest.fixture(scope="module")
def special_refs(specials):
    """The NumPy helper's results, per step, for every special sequence."""
    return {name: R.run_sequence(R.helper_step, seq) for name, seq in specials.items()}


@pytest.fixture(scope="module")
def special_host(specials):
    """The HOST FORM's results (transforms.flow_track_step on CPU tensors), per step, for every special sequence: what the
    closed-form and non-finite tests below assert on."""
    return {name: R.run_sequence(host_step, seq) for name, seq in specials.items()}


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("name,H,W,B,seed", CASES, ids=[c[0] for c in CASES])
def test_host_form_equals_the_helper(name, H, W, B, seed, masked):
    """Random sequences of 4 steps (smooth scene flows with a 1.5-pixel disturbance plus noise: tracks leave the image). On the
    helper alone first: the two-view margin >= 1e-9 at every step, and without a mask 0 < valid < inliers < inside <= alive < H * W
    at some step of every image. Then every bit and every count at every step, full form and chain-only form."""
    flows, poses, masks, calib = R.sequence(H, W, B, seed)
    ref, margin = R.reference_sequence(flows, poses, masks if masked else None, calib)
    assert margin >= MIN_MARGIN, margin
    if not masked:
        for b in range(B):
            assert any(0 < c[b, 3] < c[b, 2] < c[b, 1] <= c[b, 0] < H * W for _, _, _, c in ref), [r[3][b].tolist() for r in ref]
    seq = dict(flows=flows, poses=poses, masks=masks if masked else None, calib=calib, init=None)
    assert same_steps(R.run_sequence(host_step, seq), ref)
    chain_ref, _ = R.reference_sequence(flows, None, masks if masked else None, calib)
    chain = R.run_sequence(host_step, dict(seq, poses=None, calib=None))
    assert same_steps(chain, chain_ref)
    for (a, l, _, c), (a2, l2, d2, c2) in zip(ref, chain):
        assert same_bits(a, a2) and same_bits(l, l2) and d2 is None and (c2[:, 1:] == 0).all() and np.array_equal(c2[:, 0], c[:, 0])


def test_three_dimensional_form_and_input_forms():
    """A 3-d flow with acc [2,H,W] and alive [H,W]; a bool alive and mask; the pose as [3,4] and [B,4,4]: the same bits."""
    flows, poses, masks, calib = R.sequence(9, 33, 3, 3)
    ref, _ = R.reference_sequence(flows, poses, masks, calib)
    acc0, alive0, depth0, _ = ref[0]
    want_a, want_l, want_d, want_c = ref[1]
    for b in range(3):
        a, l, d, c = transforms.flow_track_step(_t(flows[1, b]), _t(acc0[b]), _t(alive0[b]) != 0, pose=_t(poses[1, b]).view(3, 4),
                                                calib=calib, mask=_t(masks[1, b]) != 0, depth=_t(depth0[b].copy()))
        assert tuple(a.shape) == (2, 9, 33) and tuple(l.shape) == (9, 33) and tuple(d.shape) == (1, 9, 33) and tuple(c.shape) == (4,)
        assert same_bits(_n(a), want_a[b]) and same_bits(_n(l), want_l[b]) and same_bits(_n(d), want_d[b])
        assert np.array_equal(_n(c), want_c[b])
    a, l, d, c = transforms.flow_track_step(_t(flows[1]), _t(acc0), _t(alive0)[:, None], pose=_t(R.pose_mats(poses[1])), calib=calib,
                                            mask=_t(masks[1])[:, None], depth=_t(depth0.copy()))
    assert same_bits(_n(a), want_a) and same_bits(_n(l), want_l) and same_bits(_n(d), want_d) and np.array_equal(_n(c), want_c)
    # depth=None starts from zeros
    a, l, d, c = transforms.flow_track_step(_t(flows[0]), _t(np.zeros_like(acc0)), _t(np.ones_like(alive0)), pose=_t(poses[0]),
                                            calib=calib, mask=_t(masks[0]))
    assert same_bits(_n(d), ref[0][2]) and np.array_equal(_n(c), ref[0][3])


def test_raw_abi_with_odd_offsets():
    """The host entry through ctypes, every buffer inside a guarded allocation at an odd offset: the helper's bits, guards intact."""
    H, W, B = 9, 33, 3
    flows, poses, masks, calib = R.sequence(H, W, B, 3)
    ref, _ = R.reference_sequence(flows, poses, masks, calib)
    acc0, alive0, depth0, _ = ref[0]
    n = H * W

    def guarded(values, dtype, off):
        buf = np.full(values.size + 16, 77, dtype=dtype)
        buf[off:off + values.size] = values.reshape(-1)
        return buf, buf[off:off + values.size]

    a_buf, a_out = guarded(np.zeros(B * 2 * n), np.float32, 3)
    l_buf, l_out = guarded(np.zeros(B * n), np.uint8, 5)
    d_buf, d_io = guarded(depth0, np.float32, 1)
    c_buf, c_out = guarded(np.zeros(B * 4), np.int32, 7)
    ins = [np.ascontiguousarray(x) for x in (flows[1], masks[1], acc0, alive0, poses[1])]
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    rc = _lib.lib().atdn_flow_track_step_host(p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), B, H, W, p(a_out), p(l_out), p(ins[4]),
                                              *calib, 1.0, R.min_sin2_of(0.05), 80.0, p(d_io), p(c_out))
    assert rc == 0, _lib.lib().atdn_last_error()
    assert same_bits(a_out.reshape(B, 2, H, W), ref[1][0]) and same_bits(l_out.reshape(B, H, W), ref[1][1])
    assert same_bits(d_io.reshape(B, 1, H, W), ref[1][2]) and np.array_equal(c_out.reshape(B, 4), ref[1][3])
    for buf, view in ((a_buf, a_out), (l_buf, l_out), (d_buf, d_io), (c_buf, c_out)):
        rest = np.ones(buf.size, dtype=bool)
        start = (view.ctypes.data - buf.ctypes.data) // buf.itemsize
        rest[start:start + view.size] = False
        assert (buf[rest] == 77).all()


@pytest.mark.parametrize("name,H,W,B,seed", CASES, ids=[c[0] for c in CASES])
def test_full_form_is_chain_then_two_view(name, H, W, B, seed):
    """The full form equals the chain-only form followed by two_view_depth(acc_out, pose, mask=alive_out), with
    depth = where(d != 0, d, depth_in); counts 1-3 are that call's counts."""
    flows, poses, masks, calib = R.sequence(H, W, B, seed)
    full = R.run_sequence(host_step, dict(flows=flows, poses=poses, masks=masks, calib=calib, init=None))
    acc, alive = np.zeros((B, 2, H, W), dtype=np.float32), np.ones((B, H, W), dtype=np.uint8)
    depth = np.zeros((B, 1, H, W), dtype=np.float32)
    for k in range(len(flows)):
        acc, alive, none, c = host_step(flows[k], masks[k], acc, alive, None, None, None)
        d, c2 = transforms.two_view_depth(_t(acc), _t(poses[k]), calib, mask=_t(alive))
        depth = np.where(d.numpy() != 0, d.numpy(), depth)
        assert same_bits(acc, full[k][0]) and same_bits(alive, full[k][1]) and same_bits(depth, full[k][2])
        assert np.array_equal(full[k][3][:, 0], c[:, 0]) and np.array_equal(full[k][3][:, 1:], c2.numpy())


def test_specials_equal_the_helper(specials, special_refs, special_host):
    """Every closed-form and non-finite sequence of the helper module: the host form has the helper's bits at every step."""
    assert sorted(special_host) == sorted(special_refs) == sorted(specials) and len(specials) >= 69
    for name in specials:
        assert same_steps(special_host[name], special_refs[name]), name


def test_zero_flow_keeps_everything(special_host):
    for acc, alive, depth, counts in special_host["zero"]:
        assert (acc.view(np.uint32) == 0).all() and (alive == 1).all() and (counts[:, 0] == 6 * 12).all()


def test_constant_flow_is_the_running_sum(special_host):
    """(0.75, -0.5) per step: the sums are exact, and a track is alive exactly while every intermediate position is inside. A step
    reads the flow where the track stands, so after step k the track is alive iff the positions after 0 .. k-1 steps are inside."""
    H, W = 6, 12
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok = np.ones((H, W), dtype=bool)
    last = np.zeros((2, H, W))
    for k, (acc, alive, _, counts) in enumerate(special_host["const"]):
        x, y = xs + 0.75 * k, ys - 0.5 * k                       # where the track stands before step k + 1
        ok &= (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        last = np.where(ok, np.stack([np.full((H, W), 0.75 * (k + 1)), np.full((H, W), -0.5 * (k + 1))]), last)
        for b in range(2):
            assert np.array_equal(alive[b] != 0, ok) and np.array_equal(acc[b], last.astype(np.float32)) and counts[b, 0] == ok.sum()
    assert 0 < ok.sum() < H * W


def test_sideways_translation_over_a_plane_chained(special_host):
    """The two-view test's plane, chained: fx = 64, Z = 8, 0.25 m sideways per step -> -2 px per step. After k steps the flow is
    -2k, the baseline 0.25k, and the depth fx * 0.25k / 2k = 8 at every pixel whose track is alive and inside, at every step."""
    H, W = 6, 12
    for k, (acc, alive, depth, counts) in enumerate(special_host["plane"]):
        gone = 2 * (k + 1)                                         # columns whose correspondence left the image
        assert (acc[:, 0, :, 2 * k:] == -2.0 * (k + 1)).all() and (alive[:, :, 2 * k:] == 1).all() and (alive[:, :, :2 * k] == 0).all()
        assert counts.tolist() == [[H * (W - 2 * k)] + [H * (W - gone)] * 3] * 2
        np.testing.assert_allclose(depth[:, 0, :, 2:], 8.0, rtol=2.0 ** -23, atol=0)      # once valid, kept: the latest wins
        assert (depth[:, 0, :, :2] == 0).all()


def test_affine_field_against_its_closed_form(special_host):
    """flow(p) = A p + b chained N = 6 times: p_N = M^N p + (M^(N-1) + .. + I) b with M = I + A, in float64. Bilinear reading of an
    affine field is exact up to rounding, so the gap is the float32 rounding of the field and of acc at every step: bound
    N * 2^-23 * max(1, max |acc|). Measured: 8.3e-07 (bound 6.1e-06) over the 673 of 960 tracks that stay inside."""
    N, H, W = R.AFFINE["N"], R.AFFINE["H"], R.AFFINE["W"]
    M = np.eye(2) + R.AFFINE["A"]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    p = np.stack([xs, ys])
    for _ in range(N):
        p = np.einsum("ij,jhw->ihw", M, p) + R.AFFINE["b"][:, None, None]
    acc, alive, _, counts = special_host["affine"][-1]
    live = alive[0] != 0
    want = p - np.stack([xs, ys])
    gap = np.abs(acc[0].astype(np.float64) - want)[:, live].max()
    bound = N * 2.0 ** -23 * max(1.0, np.abs(acc[0][:, live]).max())
    print("affine chain: gap %.3e, bound %.3e, %d tracks alive" % (gap, bound, live.sum()))
    assert 0 < live.sum() < H * W and gap <= bound


def test_a_dead_pixel_stays_dead(specials, special_host):
    """Dead on entry (outside, NaN payloads, or simply marked dead): the +4 px flow would carry (3, 2) back inside, but it stays
    dead at both steps, its acc bits and its depth untouched, counted nowhere."""
    acc0, alive0, depth0 = specials["dead"]["init"]
    dead = [(2, 3), (1, 1), (4, 4), (3, 0)]
    for acc, alive, depth, counts in special_host["dead"]:
        for y, x in dead:
            assert alive[0, y, x] == 0 and same_bits(acc[0, :, y, x], acc0[0, :, y, x]) and depth[0, 0, y, x] == 3.0
    first = special_host["dead"][0]
    assert first[3][0, 0] == 6 * 12 - 4 and first[1].sum() == 6 * 12 - 4


def test_mask_is_read_at_the_nearest_pixel(special_host):
    acc, alive, _, counts = special_host["mask"][0]
    dead = {(0, 2), (0, 3), (1, 3), (3, 5), (3, 11), (4, 7), (5, 7)}
    assert {tuple(i) for i in np.argwhere(alive[0] == 0)} == dead and counts[0, 0] == 6 * 12 - len(dead)
    assert acc[0, 0, 1, 2] == np.float32(0.49) and acc[0, 0, 2, 2] == 0.5          # x1 = 2.49 reads (2), x1 = 2.5 reads (3): both set


def test_one_pixel_image(special_host):
    for acc, alive, depth, counts in special_host["1x1"]:
        assert alive.tolist() == [[[1]]] and (acc == 0).all() and counts[0, 0] == 1 and counts[0, 1] == 1 and depth[0, 0, 0, 0] == 0


def test_alive_bytes_other_than_0_and_1(specials, special_host):
    alive0 = specials["alive_bytes"]["init"][1]
    acc, alive, _, counts = special_host["alive_bytes"][0]
    assert np.array_equal(alive, (alive0 != 0).astype(np.uint8)) and counts[0, 0] == (alive0 != 0).sum()
    assert (acc[0][:, alive0[0] != 0] == 0.25).all() and (acc[0][:, alive0[0] == 0] == 0).all()


def test_largest_float32_in_a_tap(special_host):
    """FLT_MAX + 3 rounds to FLT_MAX: alive with acc = (FLT_MAX, -FLT_MAX), dead at the next step (outside), acc kept."""
    big = np.finfo(np.float32).max
    for k, (acc, alive, depth, counts) in enumerate(special_host["float_max"]):
        for x in (0, 3):
            assert acc[0, :, 2, x].tolist() == [big, -big] and alive[0, 2, x] == (1 if k == 0 else 0) and depth[0, 0, 2, x] == 0
        assert alive[0].sum() == 6 * 12 - (0 if k == 0 else 2)


@pytest.mark.parametrize("bad", ["nan", "pinf", "ninf"])
def test_non_finite_values_touch_their_pixels_only(specials, special_host, bad):
    """In acc_in: those pixels die and keep their bits. In one of the four taps, also with weight zero: every pixel that reads the
    tap dies, no other pixel changes. In the pose: the chain is unaffected and no depth is written."""
    base_seq = dict(specials["acc_" + bad], init=None)
    base = R.run_sequence(host_step, base_seq)
    acc0 = specials["acc_" + bad]["init"][0]
    got = special_host["acc_" + bad]
    changed = np.zeros((9, 33), dtype=bool)
    changed[5, 7] = changed[6, 8] = True
    for (a, l, d, c), (ba, bl, bd, bc) in zip(got, base):
        assert (l[0][changed] == 0).all() and same_bits(a[0][:, changed], acc0[0][:, changed]) and (d[0, 0][changed] == 0).all()
        assert same_bits(a[0][:, ~changed], ba[0][:, ~changed]) and same_bits(l[0][~changed], bl[0][~changed])
        assert same_bits(d[0, 0][~changed], bd[0, 0][~changed])
    for frac in ("frac", "int"):
        for t, (ty, tx) in enumerate(((2, 4), (2, 5), (3, 4), (3, 5))):
            for c in (0, 1):
                name = "tap%d%d_%s_%s" % (t, c, frac, bad)
                clean = R.run_sequence(host_step, dict(specials[name], flows=specials["acc_" + bad]["flows"]))
                a, l, d, _ = special_host[name][0]
                ca, cl, cd, _ = clean[0]
                readers = np.zeros((9, 33), dtype=bool)
                readers[ty - 1:ty + 1, tx - 1:tx + 1] = True       # pixels standing on themselves whose 2 x 2 taps hold (ty, tx)
                readers[2, 4] = True                                # the pixel standing at (4.25, 2.5) or (4, 2)
                assert l[0, 2, 4] == 0 and (l[0][readers] == 0).all() and (d[0, 0][readers] == 0).all(), name
                assert same_bits(a[0][:, ~readers], ca[0][:, ~readers]) and same_bits(l[0][~readers], cl[0][~readers]), name
                assert same_bits(d[0, 0][~readers], cd[0, 0][~readers]), name
    for j in (0, 5, 11):
        for (a, l, d, c), (ba, bl, bd, bc) in zip(special_host["pose%d_%s" % (j, bad)], base):
            assert same_bits(a, ba) and same_bits(l, bl) and c[0, 0] == bc[0, 0] and (d == 0).all() and c[0, 3] == 0


def test_in_place_equals_out_of_place():
    flows, poses, masks, calib = R.sequence(9, 33, 3, 3)
    ref, _ = R.reference_sequence(flows, poses, masks, calib)
    acc, alive = torch.zeros(3, 2, 9, 33), torch.ones(3, 9, 33, dtype=torch.uint8)
    depth, counts = torch.zeros(3, 1, 9, 33), torch.zeros(3, 4, dtype=torch.int32)
    for k in range(len(flows)):
        a, l, d, c = transforms.flow_track_step(_t(flows[k]), acc, alive, pose=_t(poses[k]), calib=calib, mask=_t(masks[k]),
                                                depth=depth, out=(acc, alive, counts))
        assert a is acc and l is alive and d is depth and c is counts
        assert same_bits(_n(acc), ref[k][0]) and same_bits(_n(alive), ref[k][1]) and same_bits(_n(depth), ref[k][2])
        assert np.array_equal(_n(counts), ref[k][3])


def test_flow_track_object_on_the_host():
    """depth.FlowTrack with CPU tensors: start / extend against the same steps by hand (the float64 pose product included)."""
    flows, rels, calib, Z0 = R.drive(steps=3)
    track = depth_mod.FlowTrack((47, 154), calib, "cpu", max_depth=60.0)
    track.acc.fill_(5.0)
    track.start()
    assert track.steps == 0 and (track.acc == 0).all() and (track.alive == 1).all() and (track.depth == 0).all()
    P = torch.eye(4, dtype=torch.float64)[None]
    acc, alive = np.zeros((1, 2, 47, 154), dtype=np.float32), np.ones((1, 47, 154), dtype=np.uint8)
    depth = np.zeros((1, 1, 47, 154), dtype=np.float32)
    for k in range(3):
        counts = track.extend(_t(flows[k]), _t(rels[k]))
        P = P @ _t(rels[k])
        acc, alive, depth, c = host_step(flows[k], None, acc, alive, R.pose_rows(P.numpy()), calib, depth, max_depth=60.0)
        assert track.steps == k + 1 and torch.equal(track.pose, P)
        assert same_bits(_n(track.acc), acc) and same_bits(_n(track.alive), alive) and same_bits(_n(track.depth), depth)
        assert np.array_equal(_n(counts), c) and counts is track.counts
    with pytest.raises(TypeError):
        depth_mod.FlowTrack((4, 4), calib, "cpu", max_parallax=1.0)


def test_depth_improves_along_the_drive():
    """What the feature is for. Ground plane and slanted wall at 47 x 154, 8 forward steps of about 1 m, 0.3 px of Gaussian noise
    on every flow, the latest valid triangulation wins: the median relative depth error after step 8 is at most half of that after
    step 1 (theory for a surviving track: 1/sqrt(8) = 0.35), and no fewer pixels have a depth. Measured: 0.1311 -> 0.0413 (ratio
    0.32), 5855 -> 6140 pixels. Without noise the chain itself costs a median of 1.6e-05 after 8 steps (bound 1e-4)."""
    for noise in (R.DRIVE["noise"], 0.0):
        flows, rels, calib, Z0 = R.drive(**dict(R.DRIVE, noise=noise))
        P, poses = np.eye(4)[None], []
        for rel in rels:
            P = P @ rel[None]
            poses.append(R.pose_rows(P))
        steps = R.run_sequence(host_step, dict(flows=flows, poses=np.stack(poses), masks=None, calib=calib, init=None))
        errors = R.drive_errors([s[2][0, 0] for s in steps], Z0)
        print("drive, noise %.1f: (median relative error, pixels) per step = %s" % (noise, errors))
        if noise:
            assert errors[7][0] <= 0.5 * errors[0][0]
            assert errors[7][1] >= errors[0][1]
        else:
            assert errors[7][0] <= 1e-4


def test_argument_errors():
    L = _lib.lib()
    H, W = 4, 4
    z = lambda *s, dt=np.float32: np.zeros(s, dtype=dt)   # noqa: E731
    flow, acc, acc2, depth, pose = z(1, 2, H, W), z(1, 2, H, W), z(1, 2, H, W), z(1, 1, H, W), z(1, 12)
    alive, alive2, mask, counts = z(1, H, W, dt=np.uint8), z(1, H, W, dt=np.uint8), z(1, H, W, dt=np.uint8), z(1, 4, dt=np.int32)
    p = lambda x: None if x is None else C.c_void_p(x.ctypes.data)   # noqa: E731
    base = dict(flow=flow, mask=mask, acc_in=acc, alive_in=alive, B=1, H=H, W=W, acc_out=acc2, alive_out=alive2, pose=pose, fx=5.0,
                fy=5.0, cx=1.5, cy=1.5, max_epipolar=1.0, min_sin2=1e-6, max_depth=80.0, depth=depth, counts=counts)

    def call(**over):
        a = dict(base, **over)
        return L.atdn_flow_track_step_host(p(a["flow"]), p(a["mask"]), p(a["acc_in"]), p(a["alive_in"]), a["B"], a["H"], a["W"],
                                           p(a["acc_out"]), p(a["alive_out"]), p(a["pose"]), a["fx"], a["fy"], a["cx"], a["cy"],
                                           a["max_epipolar"], a["min_sin2"], a["max_depth"], p(a["depth"]), p(a["counts"]))

    assert call() == 0 and call(mask=None) == 0
    assert call(acc_out=acc, alive_out=alive) == 0                                   # in place
    assert call(pose=None, depth=None) == 0                                          # chain only ...
    assert call(pose=None, depth=None, fx=float("nan"), max_depth=-1.0) == 0         # ... ignores calibration and thresholds
    assert call(pose=None) != 0 and b"depth" in L.atdn_last_error()                 # chain only takes no depth
    assert call(depth=None) != 0
    for name in ("flow", "acc_in", "alive_in", "acc_out", "alive_out", "counts"):
        assert call(**{name: None}) != 0, name
    for over in (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=1 << 13, W=(1 << 11) + 1),
                 dict(fx=0.0), dict(fy=-1.0), dict(fx=float("inf")), dict(fy=float("nan")), dict(cx=float("nan")),
                 dict(cy=float("inf")), dict(max_epipolar=-1.0), dict(max_epipolar=float("inf")), dict(min_sin2=-1e-9),
                 dict(min_sin2=float("nan")), dict(max_depth=0.0), dict(max_depth=float("inf"))):
        assert call(**over) != 0, over
    # overlaps: an output with an input, with another output, and a partial overlap of the in-place pairs
    both = z(2, 2, H, W)
    half = both.reshape(-1)
    for over in (dict(acc_out=flow), dict(depth=flow[:, :1]), dict(alive_out=mask), dict(depth=acc), dict(acc_out=acc, depth=acc),
                 dict(acc_in=half[:32], acc_out=half[16:48]), dict(depth=acc2), dict(alive_in=alive, alive_out=alive.reshape(-1)[1:]),
                 dict(counts=pose.view(np.int32)), dict(counts=depth.view(np.int32))):
        assert call(**over) != 0, list(over)
    t = torch.zeros
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(2, 4, 4), t(1, 2, 4, 4), t(4, 4))                       # acc not of the flow's shape
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(3, 4, 4), t(3, 4, 4), t(4, 4))                          # not a flow
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 5))                 # alive of another size
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), pose=torch.eye(4))           # a pose without calib
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), depth=t(1, 1, 4, 4))         # depth without a pose
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), pose=torch.eye(4), calib=(5.0, 5.0, 1.5, 1.5),
                                   depth=t(1, 1, 4, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), out=(t(1, 2, 4, 4), t(1, 4, 4)))   # alive_out not uint8
    with pytest.raises(RuntimeError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), pose=torch.eye(4), calib=(5.0, 5.0, 1.5, 1.5),
                                   max_depth=0.0)
    with pytest.raises(ValueError):
        transforms.flow_track_step(t(1, 2, 4, 4), t(1, 2, 4, 4), t(1, 4, 4), pose=torch.eye(4),
                                   calib=[[5.0, 0.1, 1.5], [0, 5.0, 1.5], [0, 0, 1]])
