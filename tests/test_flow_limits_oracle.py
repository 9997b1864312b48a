"""The flow network's lower size limit and the yardstick of tests/test_gpu_flow_limits.py, on the CPU oracle alone.

(i) Below 128x128 the reference has no result. Level 3 of the correlation pyramid is H/64 x W/64 cells; bilinear_sampler
(utils/utils.py:63-64) normalises a coordinate by (H_l - 1), which is 0 for a one-cell level: 0/0 or x/0, then (inf + 1) * 0 in
grid_sample's un-normalisation. The first non-finite tensor is the lookup, in exactly its 81 level-3 channels 243..323; everything
computed from it, the flow included, is non-finite. At 128x128 (a 2x2 level 3) every tensor is finite.

(ii) The GPU test bounds max|x_hip - x64| by min(M * max|x32 - x64| + floor, TOL). The cap TOL only means something where the fp32
oracle itself is well inside it: for every case of that test (flow_limits_cases.CASES and INIT_CASES) and every compared tensor,
max|x32 - x64| <= TOL / 2. Measured (frames seed 4, make_gma_state(seed=1), 12 iterations), worst pair per geometry:

    frames     flow_low  flow_up  lookup0  net1     | one iteration from flow_init: lookup0  flow_low  flow_up
    152x216    8.4e-6    3.5e-5   2.7e-5   1.1e-6   |                               2.0e-5   4.4e-6    3.6e-5
    248x264    9.2e-6    3.7e-5   1.1e-5   1.3e-6   |                               1.5e-5   3.8e-6    3.7e-5
    128x1024   4.2e-5    9.2e-5   1.5e-5   1.1e-6
    1024x128   2.5e-5    7.8e-5   2.5e-5   1.4e-6

The nearest to its half: lookup0 at 152x216 pair 2 (2.7e-5 of 5e-5) and flow_low at 128x1024 pair 1 (4.2e-5 of 1e-4). The
figures move by tens of per cent with the host's thread count (another summation order in the CPU convolutions: lookup0 between
1.0e-5 and 2.7e-5 over the pairs and two hosts). `pytest -s` prints every figure ("YARDSTICK" lines).
"""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from oracle import gma_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_limits_cases as lim  # noqa: E402
import test_gpu_flow_geometry as fg  # noqa: E402   (helpers and constants only: its tests stay in its own module)

L3 = set(range(243, 324))   # lookup channels of pyramid level 3: 3 * 81 .. 4 * 81 - 1


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return fg._sd()


def _forward(sd, hw, dtype, iters):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    fr = torch.from_numpy(syn.make_frames(2, hw[0], hw[1], seed=fg.SEED_FRAMES)).to(dtype)
    taps = {}
    low, up = gma_ref.gma_forward(sd, fr[0:1], fr[1:2], iters=iters, taps=taps)
    return low, up, taps


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("hw", lim.REJECTED, ids=lambda hw: "%dx%d" % hw)
def test_reference_is_not_finite_below_128(sd, hw, dtype):
    low, up, taps = _forward(sd, hw, dtype, 2)
    assert min(hw[0] // 64, hw[1] // 64) == 1                       # a one-cell-high or one-cell-wide level 3
    for k in ("fmap1", "fmap2", "net0", "inp", "attn"):            # everything before the lookup is finite
        assert bool(torch.isfinite(taps[k]).all()), k
    assert all(bool(torch.isfinite(p).all()) for p in taps["pyramid"])
    bad = ~torch.isfinite(taps["lookup0"])                          # [1, 324, H8, W8]: the first non-finite tap
    assert set(torch.nonzero(bad.any(dim=3).any(dim=2)[0]).flatten().tolist()) == L3
    assert bool(bad[:, 243:324].all())                              # every pixel of every level-3 channel
    for k in ("mf0", "mfg0", "net1", "delta0"):
        assert not bool(torch.isfinite(taps[k]).all()), k
    assert not bool(torch.isfinite(low).any()) and not bool(torch.isfinite(up).any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_reference_is_finite_at_128(sd, dtype):
    low, up, taps = _forward(sd, (128, 128), dtype, fg.ITERS)
    assert bool(torch.isfinite(taps["lookup0"]).all()) and bool(torch.isfinite(low).all()) and bool(torch.isfinite(up).all())


def _tol(key, o64):
    if key.startswith(("flow_low", "low1")):
        return fg.TOL_LOW
    if key.startswith(("flow_up", "up1")):
        return fg.TOL_UP
    if key == "attn":
        return 1e-6 + 1e-4 * float(o64["attn"].max())
    return fg.TOL_ACT


def _assert_half_tol(tag, o32, o64):
    bad = []
    for k in sorted(o64):
        e = float((o32[k].double() - o64[k].double()).abs().max())
        tol = _tol(k, o64)
        print("YARDSTICK %s %s err_32=%.3e tol=%.1e" % (tag, k, e, tol))
        if not (bool(torch.isfinite(o64[k]).all()) and e <= 0.5 * tol):
            bad.append("%s: %.3e > %.1e / 2" % (k, e, tol))
    assert not bad, "%s: %s" % (tag, "; ".join(bad))


@pytest.mark.parametrize("hw", sorted(lim.SEQ), ids=lambda hw: "%dx%d" % hw)
def test_fp32_oracle_is_within_half_of_every_tolerance(sd, hw):
    """Every pair the GPU cases compare, every tensor they compare (fg._oracle_pair's dictionary), twelve iterations."""
    n, pairs = lim.SEQ[hw]
    assert {c[1] for c in lim.CASES if c[0] == hw} <= set(range(1, n)) and max(pairs) < n - 1
    frames = torch.from_numpy(syn.make_frames(n, hw[0], hw[1], seed=fg.SEED_FRAMES))
    rows = fg._rows((hw[0] // 8) * (hw[1] // 8))
    for i in pairs:
        o32, o64 = (fg._oracle_pair(sd, frames, i, dt, rows, False) for dt in (torch.float32, torch.float64))
        _assert_half_tol("%dx%d/p%d" % (hw[0], hw[1], i), o32, o64)


@pytest.mark.parametrize("hw", sorted({c[0] for c in lim.INIT_CASES}), ids=lambda hw: "%dx%d" % hw)
def test_flow_init_probes_and_their_yardstick(sd, hw):
    """The planted flow_init does what its comments say, in the oracle: integer and half-pixel weights, windows that leave the
    map, two pixels that sample nothing at any level; and the fp32 oracle stays within half of every tolerance under it."""
    H8, W8 = hw[0] // 8, hw[1] // 8
    fi, where, outside = lim.make_flow_init(hw)
    assert tuple(fi.shape) == (1, 2, H8, W8) and float(fi.abs().max()) == 64.0
    assert len(set(where.values())) == len(where) and where["far_corner_last_pixel"] == (H8 - 1, W8 - 1)
    assert all(lim.windows_outside_everywhere(hw, fi, yx) for yx in outside)
    assert not any(lim.windows_outside_everywhere(hw, fi, yx) for k, yx in where.items() if not k.startswith("outside"))
    frames = torch.from_numpy(syn.make_frames(lim.SEQ[hw][0], hw[0], hw[1], seed=fg.SEED_FRAMES))
    o32, o64 = (lim.oracle_flow_init(sd, frames, fi, dt) for dt in (torch.float32, torch.float64))
    assert set(o64) == set(lim.INIT_KEYS)
    _assert_half_tol("%dx%d/flow_init" % hw, o32, o64)
    look = o64["lookup0"].reshape(H8, W8, 324)
    for y, x in outside:
        assert bool((look[y, x] == 0).all())
    for k, (y, x) in where.items():
        if not k.startswith("outside"):
            # a window that is partly inside samples something at level 0; the ones at the border sample padding too
            assert float(look[y, x, :81].abs().max()) > 0, k
    y, x = where["last_is_first"]       # coords (-4, -4): of level 0's 81 samples only offset (+4, +4) = channel 80 hits a cell
    # (the others sit at -1 or beyond, up to the rounding of the reference's normalise / denormalise round trip)
    assert float(look[y, x, 80].abs()) > 1e-3 and float(look[y, x, :80].abs().max()) < 1e-9
    y, x = where["neg_frac_l3"]
    assert -1 < (x + float(fi[0, 0, y, x])) / 8 < 0 and -1 < (y + float(fi[0, 1, y, x])) / 8 < 0


def test_the_library_and_the_range_report_refuse_what_the_reference_cannot_compute():
    """The C ABI's check needs no device: every size of (i) is refused with the reason, 128x128 is accepted; the range
    report's argument check draws the same line."""
    import ctypes as C

    from atdn_vslam_amd import _lib, range_report
    L = _lib.lib()
    for H, W in lim.REJECTED + [(64, 1024), (1024, 120)]:
        for precision in (0, 1, 2):
            h = C.c_void_p()
            assert L.atdn_gma_create(C.byref(h), H, W, 1, precision) != 0
            msg = L.atdn_last_error()
            assert b"at least 128x128" in msg and b"level 3 of the correlation pyramid needs at least 2x2 cells" in msg
            assert b"H/64 - 1" in msg
    h = C.c_void_p()
    assert L.atdn_gma_create(C.byref(h), 120, 132, 1, 1) != 0 and b"multiple of 8" in L.atdn_last_error()
    _lib.check(L.atdn_gma_create(C.byref(h), 128, 128, 1, 1))
    L.atdn_gma_destroy(h)
    for size in ("64x64", "120x136", "136x120"):
        with pytest.raises(SystemExit):
            range_report.parse_args(["--synthetic", "--size", size])
    assert range_report.parse_args(["--synthetic", "--size", "128x128"]).size == (128, 128)
