"""CPU checks of tests/f16_exact_ref.py: the inputs of tests/test_gpu_f16_kernels.py have the properties that make bit equality
the right demand of a FAST (plain-f16) kernel, and that make the demand sharp. Per convolution case:
  * float16(x) == hi_x, and float16(w * 2^p) * 2^-p == hi_w for the p pack_conv_sf chooses;
  * max (sum |x^| |w^| + |b|) < 2^24 quanta of 1/4: every partial sum, in any order, is exact in fp32;
  * fast_ref is exact in fp32 and survives the split-f16 store (under 2^22 quanta, and hi + lo reproduces it);
  * |full_ref - fast_ref| > 16 ulp of the result in >= 0.99 of the outputs (measured 0.9956 - 0.9975 over the 28 cases): the
    full three-product kernel's answer is visibly another one, so a FAST kernel that leaks a lo fragment, drops a chunk or
    misplaces a tap cannot return fast_ref;
  * a cut case (f16_exact_ref.CUTS) gets the kernel of the case it stands for.
And for the correlation shapes: the pooled target levels stay f16 numbers with a zero lo part, and the sums stay under 2^24
quanta at every level, so levels 0-3 are held to bit equality on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_exact_ref as ex  # noqa: E402

CASES = ex.conv_cases()


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def test_value_sets():
    """Every hi + lo rounds to hi in f16 with a normal, nonzero lo; +-2 would not do (the reason it is left out)."""
    for h in ex.HI:
        for l in ex.LO:
            v = np.float32(np.float64(h) + np.float64(l))
            assert np.float64(v) == np.float64(h) + np.float64(l)
            assert np.float32(np.float16(v)) == h
            r = np.float16(v - np.float32(np.float16(v)))
            assert np.float32(r) == l and abs(float(r)) >= 2.0 ** -14
    assert np.float32(np.float16(np.float32(2.0 - 3 * 2.0 ** -12))) != np.float32(2.0)
    assert all(float(h * g / ex.QUANTUM).is_integer() for h in ex.HI for g in ex.HI)


def test_cut_cases_keep_their_kernel():
    conv, stride2, halo, run = ex._tables()
    originals = set(conv + stride2 + halo + run)
    assert set(ex.CUTS) <= originals
    for orig, cut in ex.CUTS.items():
        assert orig[:7] == cut[:7], "a cut changes the image count and size only"
        assert ex.kernel_plan(orig) == ex.kernel_plan(cut), (orig, ex.kernel_plan(orig), cut, ex.kernel_plan(cut))
        assert cut[7] * cut[8] * cut[9] < orig[7] * orig[8] * orig[9]
    for c in run:   # the tile-form bits give the forms their names say, except the run length 42 the run tiles do not serve
        assert ex.kernel_plan(c, 1) == ("halo", 8, 128)
        run_length = c[7] if c[2] == 5 else c[8]
        assert ex.kernel_plan(c, 2) == (("run", 8, 128) if run_length >= 43 else ex.kernel_plan(c))
    plans = {ex.kernel_plan(c) for _, c in CASES}
    assert plans >= {("halo", 4, 64), ("halo", 8, 32), ("halo", 8, 64), ("halo", 8, 96), ("halo", 8, 128), ("halo", 12, 64),
                     ("run", 8, 128), ("gemm", 64, 64), ("gemm", 128, 32), ("gemm", 128, 96)}, plans


@pytest.mark.parametrize("nc", CASES, ids=[ex.case_id(c) for c in CASES])
def test_exact_conv_inputs(nc):
    _, case = nc
    e = ex.exact_conv(case)
    assert np.array_equal(ex.round_inputs(e["x"]), e["hi_x"])
    assert ex.pack_exponent(e["w"]) == -1
    assert np.array_equal(ex.round_weights(e["w"]), e["hi_w"])
    lo_x = (e["x"] - e["hi_x"]).astype(np.float16)
    assert np.all(lo_x != 0) and np.all(np.abs(lo_x.astype(np.float32)) >= 2.0 ** -14)
    quanta = ex.exact_conv_magnitude(case) / ex.QUANTUM
    fast, full = e["fast_ref"], e["full_ref"]
    assert quanta < 2 ** 24, quanta
    assert torch.equal(fast.float().double(), fast)
    q = fast / ex.QUANTUM
    assert torch.equal(q, q.round())
    if case[1] % 32 == 0:
        assert float(q.abs().max()) < 2 ** 22
        assert np.array_equal(ex.sf_roundtrip(fast.float().numpy()), fast.float().numpy())
    share = float(((full - fast).abs() > ex.ULP_GAP * ex.ulp32(fast)).double().mean())
    print("EXACT-HOST %s: max quanta %.3g, max |fast_ref| %.4g, share of outputs > %d ulp apart %.4f, median |full - fast| %.3g"
          % (ex.case_id(nc), quanta, float(fast.abs().max()), ex.ULP_GAP, share, float((full - fast).abs().median())))
    assert share >= ex.MIN_SHARE, share


@pytest.mark.parametrize("shape", ex.CORR_SHAPES, ids=["%dx%dx%dx%d" % s for s in ex.CORR_SHAPES])
def test_exact_corr_inputs(shape):
    C = shape[1]
    hi1, f1, hi2, f2 = ex.corr_features(shape)
    assert np.array_equal(ex.round_inputs(f1), hi1) and np.array_equal(f2, hi2)
    levels = ex.pooled_levels(f2)
    mags = ex.corr_mag(hi1, levels, C)
    for l, (t, m) in enumerate(zip(levels, mags)):
        assert t.shape[2] == shape[2] >> l and t.shape[3] == shape[3] >> l
        v = t.numpy()
        assert np.array_equal(v.astype(np.float16).astype(np.float64), v), "level %d leaves f16: lo would not be 0" % l
        quantum = 0.5 * 0.5 / 4 ** l
        assert np.array_equal(v / (0.5 / 4 ** l), np.round(v / (0.5 / 4 ** l)))
        assert float(m.max()) / quantum < 2 ** 24, (l, float(m.max()) / quantum)
    # split-f16 arithmetic (fast = 0) on these features: the bound of the GPU test tells the modes apart — the hi x hi product
    # alone, i.e. a kernel that lost the source's lo halves, lies outside it at every level
    full, hi_only = ex.corr_levels(f1, levels, C), ex.corr_levels(hi1, levels, C)
    full_mags = ex.corr_mag(f1, levels, C)
    for l in range(4):
        assert float(((full[l] - hi_only[l]).abs() / ex.corr_split_bound(C, full_mags[l])).max()) > 1, l
    # the second run: lo != 0 in the target as well, level 0 only
    hi1b, f1b, hi2b, f2b = ex.corr_features(shape, target_lo=True)
    assert np.array_equal(ex.round_inputs(f1b), hi1b) and np.array_equal(ex.round_inputs(f2b), hi2b)
    assert np.all((f2b - hi2b).astype(np.float16) != 0)
    # and the full product differs visibly from the hi x hi one there (the fast = 1 run is not blind)
    fast = ex.corr_levels(hi1b, [torch.from_numpy(hi2b.astype(np.float64))], C)[0]
    full = ex.corr_levels(f1b, [torch.from_numpy(f2b.astype(np.float64))], C)[0]
    share = float(((full - fast).abs() > ex.ULP_GAP * ex.ulp32(fast)).double().mean())
    print("EXACT-HOST corr %s: share of level-0 entries > %d ulp apart %.4f" % (shape, ex.ULP_GAP, share))
    assert share >= ex.MIN_SHARE, share


def test_decoded_split_values_give_their_hi_half_except_at_midpoints():
    """cor1 of the FAST lookup kernel is compared with float16(samples) of the DECODED samples: that is the hi half the kernel
    multiplied with, except where the decoded value is an exact f16 midpoint — there it may be the other neighbour, and
    f16_midpoint_gap says so and by how much."""
    r = np.random.RandomState(0)
    v = r.normal(0, 8, 1 << 21).astype(np.float32)
    h = r.normal(0, 8, 4096).astype(np.float16)
    h = h[(h.view(np.uint16) & 1) == 1]                                    # odd neighbours
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float32)
    mid = ((h.astype(np.float64) + up.astype(np.float64)) / 2).astype(np.float32)
    planted = np.nextafter(mid, h.astype(np.float32))                      # one fp32 step on the odd neighbour's side
    v = np.concatenate([v, planted, mid])
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    d = hi.astype(np.float32) + lo.astype(np.float32)
    back, gap = d.astype(np.float16), ex.f16_midpoint_gap(d)
    wrong = back != hi
    assert np.all(hi[-len(mid) - len(planted):-len(mid)] == h) and wrong[-len(mid) - len(planted):-len(mid)].all()
    assert not wrong[-len(mid):].any() and np.all(gap[-len(mid):] > 0)
    assert np.all(gap[wrong] > 0)
    assert np.array_equal(np.abs(back.astype(np.float64) - hi.astype(np.float64))[wrong], gap[wrong])
    assert float((gap[:1 << 21] > 0).mean()) < 2.0 ** -10     # rare among ordinary values: three 13-bit patterns of 2^13


def test_probe_coordinates_and_split_rule():
    for shape in ex.CORR_SHAPES:
        import flow_limits_cases as lim
        coords, outside = ex.probe_coords(shape)
        assert coords.shape == (shape[0], 2, shape[2], shape[3]) and len(outside) == 2
        fi = torch.from_numpy(coords[0:1] - np.stack(np.meshgrid(np.arange(shape[3], dtype=np.float32),
                                                                 np.arange(shape[2], dtype=np.float32)))[None])
        for yx in outside:
            assert lim.windows_outside_everywhere((shape[2] * 8, shape[3] * 8), fi, yx)
    # attention x V key ranges of a low-latency handle (attention.hip: attn_v_splits): the two geometries of the network test
    assert ex.attn_v_splits(1, (152 // 8) * (216 // 8)) == 2
    assert ex.attn_v_splits(1, (128 // 8) * (128 // 8)) == 1
