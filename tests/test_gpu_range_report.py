"""Range report on the GPU (through the C ABI): the probe kernel alone against torch, the rows of a probed forward against the
debug taps (exactly) and against the fp64 walker of tests/test_range_report_host.py, the report against the saturation guard
on rescaled checkpoints, no interference with the module it is called on, and the command-line driver in a child process.
Out-of-range VALUES are ordinary data for both paths (the saturation tests of test_gpu_round3.py run the same checkpoints)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from atdn_vslam_amd import _lib  # noqa: E402
from atdn_vslam_amd import synthetic as syn  # noqa: E402
from atdn_vslam_amd.modules import RAFTGMA  # noqa: E402
from test_range_report_host import LIMIT, REQUIRED_ONCE, REQUIRED_PER_ITERATION, scaled_state, walk  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEXT = float(np.nextafter(np.float32(65504), np.float32(np.inf)))

# Largest relative difference between a row's max |x| and the fp64 walker's, over all rows of the synthetic checkpoint at
# 160x512 / 8 iterations, measured on an MI355X: 2.586e-6, at the row ("flow", 0) (test_rows_against_the_fp64_walker prints it).
# The bound is 10x that, capped at 1e-3 (a headroom figure coarser than 0.1 % answers no question).
MEASURED_REL = 2.586e-6
REL_TOL = min(10 * MEASURED_REL, 1e-3)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _probe(view_base, rows, cols, ld):
    """The kernel alone on `rows` x `cols` values with pitch `ld` starting at view_base[0]."""
    mx, over, nonf = C.c_float(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().atdn_range_probe(C.c_void_p(view_base.data_ptr()), rows, cols, ld, C.byref(mx), C.byref(over),
                                           C.byref(nonf), _stream()))
    return mx.value, over.value, nonf.value


def _ref(v):
    """The same three numbers with torch on the same device values; on the bit patterns, so that no arithmetic mode (denormal
    flushing, NaN handling of max) can touch the yardstick."""
    b = v.contiguous().view(torch.int32) & 0x7FFFFFFF
    nf = b >= 0x7F800000
    mx_bits = int(torch.where(nf, torch.zeros_like(b), b).max())
    mx = float(np.array([mx_bits], dtype=np.uint32).view(np.float32)[0])
    return mx, int(((b > 0x477FE000) & ~nf).sum()), int(nf.sum())


def _view(buf, off, rows, cols, ld):
    return torch.as_strided(buf, (rows, cols), (ld, 1), off)


SMALL_SHAPES = [(1, 1, 1), (7, 3, 3), (7, 3, 5), (1280, 126, 384), (64, 324, 352), (3, 4100, 4104), (5, 4097, 4100), (33, 2, 4),
                (2, 5000, 5004)]


def _contents(v, kind):
    """Fills the valid view `v` ([rows, cols], strided) in place."""
    rows, cols = v.shape
    g = torch.Generator(device="cpu").manual_seed(rows * 7919 + cols)
    data = (torch.randn(rows, cols, generator=g) * 50.0).to(v.device)
    if kind == "normal":
        v.copy_(data)
    elif kind == "zeros":
        v.zero_()
    elif kind == "negative zero":
        v.fill_(-0.0)
    elif kind == "denormals":
        bits = torch.randint(1, 0x7FFFFF, (rows, cols), generator=g, dtype=torch.int32)   # zero exponent: below the smallest normal
        bits[rows // 2, cols // 2] = 0x7FFFFF
        v.copy_((bits | (torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int32) << 31)).view(torch.float32).to(v.device))
    elif kind == "single 65504":
        v.copy_(data)
        v[rows // 2, cols // 2] = -65504.0              # representable: not over
    elif kind == "nextafter":
        v.copy_(data)
        v[rows // 2, cols // 2] = NEXT                  # the first value the format cannot hold
    elif kind == "infinities":
        v.copy_(data)
        v[0, 0] = float("inf")
        v[rows - 1, cols - 1] = float("-inf")
    elif kind == "nan":
        v.copy_(data)
        v[rows // 2, 0] = float("nan")
    elif kind == "max first":
        v.copy_(data)
        v[0, 0] = -7.0e4
    elif kind == "max last":
        v.copy_(data)
        v[rows - 1, cols - 1] = 7.0e4
    elif kind == "max in the tail of a middle row":
        v.copy_(data)
        v[rows // 2, cols - 1] = 7.0e4
    else:
        raise KeyError(kind)


KINDS = ["normal", "zeros", "negative zero", "denormals", "single 65504", "nextafter", "infinities", "nan", "max first", "max last",
         "max in the tail of a middle row"]
EXPECT = {"zeros": (0.0, 0, 0), "negative zero": (0.0, 0, 0)}


def test_kernel_alone_small_shapes_offsets_and_contents():
    """Every shape at 0, 4, 8 and 12 bytes off a 16-byte boundary, every kind of content; the padding between the rows and
    around the view is NaN, so a read outside the valid part shows."""
    for rows, cols, ld in SMALL_SHAPES:
        for off in range(4):
            buf = torch.full((off + rows * ld + 8,), float("nan"), dtype=torch.float32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            v = _view(buf, off, rows, cols, ld)
            for kind in KINDS:
                _contents(v, kind)
                got = _probe(buf[off:], rows, cols, ld)
                want = _ref(v)
                assert got == want, (rows, cols, ld, off, kind, got, want)
                if kind in EXPECT:
                    assert got == EXPECT[kind]
                if kind == "denormals":                      # the copy moved the bit patterns: nothing was flushed on the way
                    assert got == (float(np.array([0x7FFFFF], dtype=np.uint32).view(np.float32)[0]), 0, 0) and got[0] > 0
                if kind == "single 65504":
                    assert got == (65504.0, 0, 0)
                if kind == "nextafter":
                    assert got == (NEXT, 1, 0)
                if kind == "infinities":
                    assert got[2] == min(2, rows * cols) and got[0] < 1e3
                if kind == "nan":
                    assert got[2] == 1 and got[1] == 0 and got[0] < 1e3
                if kind.startswith("max"):
                    assert got[0] == 7.0e4 and got[1] == 1
                if kind == "normal":
                    assert got[0] == float(v.abs().max())
                    assert _probe(buf[off:], rows, cols, ld) == got          # repeated: the slot is zeroed per call


def test_kernel_alone_large_views():
    """The KITTI-size attention shape (7238 x 7238, pitch 7296) and one row of 2^30 + 12 values (> 4 GiB: 64-bit indexing)."""
    rows, cols, ld = 7238, 7238, 7296
    for off in (0, 1):
        buf = torch.full((off + rows * ld,), float("nan"), dtype=torch.float32, device=DEV)
        v = _view(buf, off, rows, cols, ld)
        v.normal_()
        assert _probe(buf[off:], rows, cols, ld) == _ref(v)
        v[rows - 1, cols - 1] = -9.0e4
        v[17, 4001] = float("nan")
        v[4000, 3] = NEXT
        got = _probe(buf[off:], rows, cols, ld)
        assert got == _ref(v) == (9.0e4, 2, 1)
        del buf, v
    n = (1 << 30) + 12
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    buf.normal_()
    for off in (0, 3):
        v = buf[off:off + n]
        base = _ref(v)
        assert _probe(v, 1, n, n) == base and base[1] == 0 and base[2] == 0
        saved = v[[0, n // 2, n - 1]].clone()
        v[n - 1] = 8.0e4                                 # the last value: in the 4-byte tail, behind 2^32 bytes
        assert _probe(v, 1, n, n) == (8.0e4, 1, 0)
        v[0] = -9.0e4                                    # the first value
        v[n // 2] = float("inf")
        assert _probe(v, 1, n, n) == _ref(v) == (9.0e4, 2, 1)
        v[[0, n // 2, n - 1]] = saved
    del buf
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ probed forwards
def _module(sd, precision=None, **kw):
    net = RAFTGMA(precision=precision, **kw)
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def _frames(n, h, w, seed):
    return torch.from_numpy(syn.make_frames(n, h, w, seed=seed)).to(DEV)


def _read_rows(h):
    L = _lib.lib()
    n = L.atdn_gma_range_rows(h)
    assert n >= 0
    name = C.create_string_buffer(128)
    it, lim, mx, over, nonf = C.c_int(), C.c_int(), C.c_float(), C.c_int64(), C.c_int64()
    rows = []
    for i in range(n):
        _lib.check(L.atdn_gma_range_row(h, i, name, len(name), C.byref(it), C.byref(lim), C.byref(mx), C.byref(over), C.byref(nonf)))
        rows.append((name.value.decode(), it.value, bool(lim.value), mx.value, over.value, nonf.value))
    return rows


def test_rows_equal_the_debug_taps_exactly_and_probe_off_restores_the_bits():
    """B = 2 pairs on a handle built for 3: the taps return whole buffers, the rows cover the pairs of the forward only."""
    H, W, B, iters = 160, 512, 2, 3
    N = (H // 8) * (W // 8)
    ldN = (N + 31) // 32 * 32
    net = _module(syn.to_torch(syn.make_gma_state(seed=1)), precision="f32", max_batch=3)
    fr = _frames(3, H, W, seed=3)
    low0, up0 = net(fr[0:2], fr[1:3], iters=iters, test_mode=True)
    h = net._handles[net._key(H, W)][0]
    L = _lib.lib()
    assert L.atdn_gma_range_rows(h) == 0
    _lib.check(L.atdn_gma_set_range_probe(h, 1))
    low1, up1 = net(fr[0:2], fr[1:3], iters=iters, test_mode=True)
    rows = _read_rows(h)
    assert torch.equal(up1, up0) and torch.equal(low1, low0)          # the probe only reads
    by = {(r[0], r[1]): r for r in rows}
    assert len(by) == len(rows)
    last = iters - 1

    def tap(name, nrows, ld, cols):
        t = net.debug_read(name, (nrows, ld), H, W)
        return float(t[:, :cols].abs().max())
    want = {("fnet.conv2", -1): tap("fmap", 2 * B * N, 256, 256), ("att.qk", -1): tap("qk", B * N, 256, 256),
            ("att.attn", -1): tap("attn", B * N, ldN, N), ("corr_lookup", last): tap("corrfeat", B * N, 352, 324),
            ("encoder.convc1", last): tap("cor1", B * N, 256, 256), ("gru.h2", last): tap("net", B * N, 128, 128),
            ("flow", last): tap("flow4", B * N, 4, 2), ("mask", -1): tap("mask", B * N, 576, 576)}
    for l in range(4):
        hw = (H // 8 >> l) * (W // 8 >> l)
        want[("corr.%d" % l, -1)] = tap("pyr%d" % l, B * N, hw, hw)
    for key, w in want.items():
        assert by[key][3] == w, (key, by[key][3], w)                  # a maximum has no rounding: no tolerance
        assert by[key][4] == 0 and by[key][5] == 0
    assert by[("flow_up", -1)][3] == float(up1.abs().max()) and by[("flow_low", -1)][3] == float(low1.abs().max())
    # switched off again: the rows of the last probed forward stay readable, the handle gives the bits it gave before
    _lib.check(L.atdn_gma_set_range_probe(h, 0))
    low2, up2 = net(fr[0:2], fr[1:3], iters=iters, test_mode=True)
    assert torch.equal(up2, up0) and torch.equal(low2, low0)
    assert _read_rows(h) == rows


def test_rows_against_the_fp64_walker():
    """Synthetic checkpoint, 160x512, 8 iterations: every required row present, per-iteration rows for each iteration, max |x|
    within REL_TOL of the fp64 walker's, nothing over, the default path clamps nothing and agrees with the f32 path.
    Largest relative difference measured on an MI355X: 2.586e-6 at ("flow", 0) (MEASURED_REL above; the test prints the figure
    and its row), so the bound is 2.586e-5."""
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    fr = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    Wk = walk(sd, fr[0:1], fr[1:2], 8, dtype=torch.float64)
    net = _module(sd)
    rep = net.range_report(fr[0:1].to(DEV), fr[1:2].to(DEV), iters=8)
    by = {(r.name, r.iteration): r for r in rep.rows}
    assert len(by) == len(rep.rows)
    for n in REQUIRED_ONCE:
        assert (n, -1) in by, n
        assert len(rep.find(n)) == 1, n
    for n in REQUIRED_PER_ITERATION:
        assert [r.iteration for r in rep.find(n)] == list(range(8)), n
    order = [r.name for r in rep.rows]
    assert order.index("fnet.conv1.raw") < order.index("fnet.conv2") < order.index("corr.0") < order.index("cnet.conv1.out") \
        < order.index("att.qk") < order.index("att.logits") < order.index("att.attn") < order.index("corr_lookup") < order.index("mask.0")
    worst = (0.0, None)
    for key, r in by.items():
        assert key in Wk.rows, "the walker has no row %r" % (key,)
        w = Wk.rows[key][0]
        rel = abs(r.max_abs - w) / w if w > 0 else abs(r.max_abs)
        worst = max(worst, (rel, key))
        assert r.over == 0 and r.nonfinite == 0, key
    print("largest relative difference of a row's max |x| to the fp64 walker: %.3e at %r (bound %.1e)" % (worst[0], worst[1], REL_TOL))
    print("largest tensor: corr.0 = %.4f (walker %.4f); worst limited row %s = %.4f, headroom %.1fx; flow_diff %.2e px; %.2f s"
          % (by[("corr.0", -1)].max_abs, Wk.rows[("corr.0", -1)][0], rep.worst.name, rep.worst.max_abs, rep.headroom, rep.flow_diff,
             rep.seconds))
    assert worst[0] <= REL_TOL, worst
    assert not by[("corr.0", -1)].limited and not by[("att.logits", -1)].limited and by[("corr_lookup", 0)].limited
    assert rep.verdict == "in range" and rep.first_over is None
    assert rep.default_clamped == 0
    assert rep.flow_diff <= 1e-3


def _invariants(rep):
    limited_over = any(r.limited and (r.over + r.nonfinite) > 0 for r in rep.rows)
    if limited_over:
        assert rep.default_clamped > 0, "a limited row is over the limit and the default path counted no clamp"
    if rep.verdict == "in range":
        assert rep.default_clamped == 0
    assert (rep.verdict == "out of range") == limited_over


IN_RANGE_CASES = [("unscaled", {}), ("fnet.conv2 x8", {"fnet.conv2": 8.0}), ("gru x4", {"update_block.gru.": 4.0}),
                  ("flow_head.conv1 x4", {"update_block.flow_head.conv1": 4.0}), ("att.to_qk x4", {"att.to_qk": 4.0})]


@pytest.mark.parametrize("label,scales", IN_RANGE_CASES, ids=[c[0] for c in IN_RANGE_CASES])
def test_report_predicts_the_guard_in_range(label, scales):
    sd = scaled_state(scales)
    fr = _frames(2, 160, 512, seed=3)
    rep = _module(sd).range_report(fr[0:1], fr[1:2], iters=8)
    _invariants(rep)
    assert all(r.over == 0 and r.nonfinite == 0 for r in rep.rows), [r for r in rep.rows if r.over or r.nonfinite]
    assert rep.verdict == "in range" and rep.default_clamped == 0 and rep.exit_status == 0
    if label == "fnet.conv2 x8":
        # the oracle's volume: 1.28e3 (2.0e4 as raw dot products, before corr.py's division by sqrt(256) that the stored volume carries)
        assert 1.2e3 < rep.find("corr.0", -1).max_abs < 1.35e3


def test_report_predicts_the_guard_fnet_conv2_x16():
    """fnet.conv2 x16, 4 iterations. On the oracle (oracle.gma_ref, fp32 and fp64) the stored volume peaks at 5.107e3 — the
    8.2e4 quoted for this case is the raw dot product, before corr.py:62 divides by sqrt(256) = 16; the stored volume, on both
    GPU paths and in the reference, carries the division — and the lookup's samples peak at the same 5.107e3 (iteration 0 samples
    the volume at integer coordinates). So nothing is over here: in range, no clamp, and corr.0 is not limited. The case the
    `limited` flag exists for — volume over, samples in range — is the next test."""
    sd = scaled_state({"fnet.conv2": 16.0})
    frh = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    Wk = walk(sd, frh[0:1], frh[1:2], 4, dtype=torch.float64)
    rep = _module(sd).range_report(frh[0:1].to(DEV), frh[1:2].to(DEV), iters=4)
    _invariants(rep)
    c0 = rep.find("corr.0", -1)
    assert not c0.limited
    assert abs(c0.max_abs - Wk.rows[("corr.0", -1)][0]) <= REL_TOL * c0.max_abs and 5.0e3 < c0.max_abs < 5.2e3
    assert max(r.max_abs for r in rep.find("corr_lookup")) < 6.0e3
    assert all(r.over == 0 and r.nonfinite == 0 for r in rep.rows)
    assert rep.verdict == "in range" and rep.default_clamped == 0


def test_report_predicts_the_guard_volume_over_but_not_limited():
    """Why the `limited` flag exists: fnet.conv2 x64 with the lookup moved off the matches (flow_init = (24, 12) px, one
    iteration). On the oracle (fp32 and fp64) the volume holds 7 values over 65504 (peak 8.17e4; 2 more in level 1) while the
    samples peak at 4.86e4 and every other tensor lies below that. The default path keeps the pyramid in plain fp32
    (corr_bricks.hip), so the report says "in range" and the default path must not clamp; if it did, the flag would be wrong
    and the invariants catch it."""
    sd = scaled_state({"fnet.conv2": 64.0})
    frh = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    fi = torch.zeros(1, 2, 20, 64)
    fi[:, 0], fi[:, 1] = 24.0, 12.0
    Wk = walk(sd, frh[0:1], frh[1:2], 1, dtype=torch.float64, flow_init=fi)
    assert Wk.rows[("corr.0", -1)][1] == 7 and Wk.rows[("corr.1", -1)][1] == 2 and Wk.rows[("corr_lookup", 0)][0] < 5.0e4
    rep = _module(sd).range_report(frh[0:1].to(DEV), frh[1:2].to(DEV), iters=1, flow_init=fi.to(DEV))
    _invariants(rep)
    c0 = rep.find("corr.0", -1)
    assert not c0.limited and c0.over == 7 and 8.0e4 < c0.max_abs < 8.3e4
    assert rep.find("corr.1", -1).over == 2 and not rep.find("corr.1", -1).limited
    assert rep.find("corr_lookup", 0).max_abs < 5.0e4 and rep.find("flow_init", -1).max_abs == 24.0
    assert rep.first_over is None
    assert rep.verdict == "in range" and rep.default_clamped == 0


def test_report_predicts_the_guard_lookup_samples_over():
    """fnet.conv2 x64: lookup samples up to 8.2e4, with 7 / 6 / 5 / 4 of them over in iterations 0-3 on the oracle; bracketed by
    the walker's counts at 65504 (1 +- 1e-4), so that a sample sitting on the limit may fall either side. (The stored volume
    peaks at the same 8.17e4 on the oracle — 1.3e6 as raw dot products, before the division by sqrt(256).)"""
    sd = scaled_state({"fnet.conv2": 64.0})
    frh = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    lo, hi = LIMIT * (1 - 1e-4), LIMIT * (1 + 1e-4)
    Wk = walk(sd, frh[0:1], frh[1:2], 4, dtype=torch.float64, thresholds=(lo, hi))
    rep = _module(sd).range_report(frh[0:1].to(DEV), frh[1:2].to(DEV), iters=4)
    _invariants(rep)
    for it, oracle_count in enumerate((7, 6, 5, 4)):
        w = Wk.rows[("corr_lookup", it)]
        assert w[3][hi] == w[3][lo] == oracle_count, (it, w)             # the yardstick: both brackets equal the oracle's count
        r = rep.find("corr_lookup", it)
        print("corr_lookup iteration %d: %d over (walker %d..%d), max %.6g (walker %.6g)" % (it, r.over, w[3][hi], w[3][lo], r.max_abs, w[0]))
        assert w[3][hi] <= r.over <= w[3][lo], (it, r, w)
        assert r.limited and r.nonfinite == 0
    assert (rep.first_over.name, rep.first_over.iteration) == ("corr_lookup", 0)
    assert max(r.max_abs for r in rep.rows if r.limited and r.name != "corr_lookup") < 1.2e4   # every convolution output stays below
    c0, w0 = rep.find("corr.0", -1), Wk.rows[("corr.0", -1)]
    assert not c0.limited and w0[3][hi] <= c0.over <= w0[3][lo] and abs(c0.max_abs - w0[0]) <= REL_TOL * w0[0]
    assert rep.verdict == "out of range" and rep.default_clamped > 0 and rep.exit_status == 3


def test_report_predicts_the_guard_context_network_over():
    """cnet.conv1 x3e5 (BatchNorm is folded: everything behind the stem grows): the first row over is the first cnet row."""
    sd = scaled_state({"cnet.conv1": 3e5})
    frh = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    Wk = walk(sd, frh[0:1], frh[1:2], 2)
    rep = _module(sd).range_report(frh[0:1].to(DEV), frh[1:2].to(DEV), iters=2)
    _invariants(rep)
    first_cnet = next(r for r in rep.rows if r.name.startswith("cnet."))
    assert first_cnet.name == "cnet.conv1.out"
    assert (rep.first_over.name, rep.first_over.iteration) == (first_cnet.name, -1)
    # the same rows are over as on the oracle (rows within 0.1 % of the limit on the oracle may fall either side)
    near = {k for k, v in Wk.rows.items() if abs(v[0] - LIMIT) <= 1e-3 * LIMIT}
    want = {k for k, v in Wk.rows.items() if v[1] + v[2] > 0} - near
    got = {(r.name, r.iteration) for r in rep.rows if r.over + r.nonfinite > 0} - near
    print("rows over: %d on the GPU, %d on the oracle; peak %.3g" % (len(got), len(want), max(r.max_abs for r in rep.rows)))
    assert got == want
    assert rep.verdict == "out of range" and rep.default_clamped > 0


def test_report_predicts_the_guard_clamps_outside_the_stored_activations():
    """att.to_qk x512: q and k stay below 6e4, the logits reach 2.6e6 and are not limited, no limited row is over — and the
    default path clamps in the attention matrix's encode (test_gpu_round3.py::test_h3_encode_saturation_is_counted)."""
    fr = _frames(2, 160, 512, seed=3)
    rep = _module(scaled_state({"att.to_qk": 512.0})).range_report(fr[0:1], fr[1:2], iters=2)
    _invariants(rep)
    assert rep.find("att.qk", -1).max_abs < 6e4 and rep.find("att.qk", -1).limited
    lg = rep.find("att.logits", -1)
    assert not lg.limited and 2.0e6 < lg.max_abs < 3.2e6 and lg.over > 0
    assert rep.first_over is None
    assert rep.default_clamped > 0
    assert rep.verdict == "clamps outside the stored activations" and rep.exit_status == 3


def test_no_interference_with_the_module():
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    fr = _frames(4, 160, 512, seed=3)
    other = _frames(2, 160, 512, seed=9)
    net = _module(sd)
    low0, up0 = net(fr[0:1], fr[1:2], iters=4, test_mode=True)
    checks, handles = net.saturation_checks, dict(net._handles)
    rep = net.range_report(other[0:1], other[1:2], iters=4)
    assert rep.verdict == "in range" and len(rep.rows) > 100
    assert net.precision == "split_f16" and not net.fell_back and net.saturation_checks == checks and net._handles == handles
    low1, up1 = net(fr[0:1], fr[1:2], iters=4, test_mode=True)
    assert torch.equal(up1, up0) and torch.equal(low1, low0)
    assert net.saturation_checks == checks and net.check_saturation() == 0
    # a forward_consecutive chain started before the report goes on as a continued call after it
    # (the chain is keyed on the frame OBJECT: `prev` must be the tensor that was `cur` of the call before, so index once)
    f = [fr[i] for i in range(4)]
    ref = _module(sd)
    want = [ref.forward_consecutive(f[i], f[i + 1], iters=4) for i in range(3)]
    net2 = _module(sd)
    got = [net2.forward_consecutive(f[0], f[1], iters=4)]
    tail = net2._stream_tail
    assert tail is not None and tail[0] is f[1]
    net2.range_report(other[0:1], other[1:2], iters=2, check_default=False)
    assert net2._stream_tail is tail
    calls = []
    L = _lib.lib()
    real = L.atdn_gma_forward_sequence_continued

    class Spy:
        def __getattr__(self, name):
            if name == "atdn_gma_forward_sequence_continued":
                return lambda *a: (calls.append(1), real(*a))[1]
            return getattr(L, name)
    old = _lib._lib
    _lib._lib = Spy()
    try:
        got.append(net2.forward_consecutive(f[1], f[2], iters=4))
    finally:
        _lib._lib = old
    assert calls == [1]                                                  # a continued call: frame 1's features were reused
    got.append(net2.forward_consecutive(f[2], f[3], iters=4))
    for (gl, gu), (wl, wu) in zip(got, want):
        assert torch.equal(gu, wu) and torch.equal(gl, wl)
    # modules of the other precisions
    for prec in ("f32", "f16"):
        m = _module(sd, precision=prec)
        r = m.range_report(other[0:1], other[1:2], iters=2)
        assert m.precision == prec and r.verdict == "in range" and r.default_clamped == 0 and not m._handles
        assert r.rows[:3] == net2.range_report(other[0:1], other[1:2], iters=2, check_default=False).rows[:3]
    # the probe is refused on a split-f16 handle, with a message that says why
    h = C.c_void_p()
    _lib.check(L.atdn_gma_create(C.byref(h), 160, 512, 1, 1))
    try:
        assert L.atdn_gma_set_range_probe(h, 1) != 0
        msg = L.atdn_last_error().decode()
        assert "exact-fp32" in msg and "ATDN_PRECISION_F32" in msg
        _lib.check(L.atdn_gma_set_range_probe(h, 0))                    # switching it off is always allowed
    finally:
        L.atdn_gma_destroy(h)


def test_kitti_size_report_and_the_driver_in_a_child_process(tmp_path):
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    fr = _frames(2, 376, 1232, seed=3)
    net = _module(sd)
    t0 = time.perf_counter()
    rep = net.range_report(fr[0:1], fr[1:2], iters=12)
    wall = time.perf_counter() - t0
    print(rep)
    print("KITTI-size report (1 pair, 376x1232, 12 iterations): %.2f s wall; worst limited row %s = %.4f, headroom %.1fx"
          % (wall, rep.worst.name, rep.worst.max_abs, rep.headroom))
    names = {r.name for r in rep.rows}
    assert set(REQUIRED_ONCE) <= names
    for n in REQUIRED_PER_ITERATION:
        assert [r.iteration for r in rep.find(n)] == list(range(12)), n
    assert rep.verdict == "in range" and rep.default_clamped == 0
    assert rep.worst.limited and rep.headroom > 100 and rep.find("corr.0", -1).max_abs < 100
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "atdn_vslam_amd.range_report"]
    p = subprocess.run(cmd + ["--synthetic", "--json"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout)
    assert d["verdict"] == "in range" and d["pairs"] == 1 and d["default_clamped"] == 0
    w = rep.worst
    assert (d["worst"]["name"], d["worst"]["iteration"], d["worst"]["max_abs"]) == (w.name, w.iteration, w.max_abs)
    bad = tmp_path / "bad.pth"
    torch.save(scaled_state({"cnet.conv1": 3e5}), str(bad))
    p = subprocess.run(cmd + ["--flow-weights", str(bad), "--synthetic", "--size", "160x512", "--iters", "2"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert "verdict: out of range" in p.stdout and "cnet.conv1.out" in p.stdout
