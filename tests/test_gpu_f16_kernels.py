"""The f16 fast mode (precision "f16": the FAST builds, which issue the hi x hi MFMA alone) kernel by kernel.

FAST is a second instantiation of every matrix kernel with its own operand loads and MFMA schedule; end to end it is held to
0.03 / 0.15 px, which hides a leaked lo fragment, a dropped K chunk or a wrong tap at a ragged edge. Here:

a. Exact convolutions. Inputs of tests/f16_exact_ref.py (x = hi + lo, w = hi + lo, float16(x) == hi, every hi * hi a multiple of
   1/4, every partial sum exact in fp32 in ANY order; tests/test_f16_exact_host.py asserts all of that on the CPU): a FAST kernel
   must return conv(hi_x, hi_w) + b bit for bit — torch.equal — through the fp32 store (sf_store = 8) and the split-f16 store (9),
   for every case of CONV_CASES (Cin % 32 == 0), STRIDE2_CASES, HALO_CASES and RUN_CASES (the largest cut to the smallest size with
   the same kernel, f16_exact_ref.CUTS), and for the run / rectangular tile forms of the 1x5 / 5x1 cases (bits 4 / 2 with 8).
   The same inputs WITHOUT bit 3 must give the full product: within 2e-5 * max|full_ref| of conv(x, w) + b (the bound of
   test_split_f16_halo_kernels_match_fp64, whose outputs are O(1), scaled to these: max|full_ref| is 410 - 2330, so 0.008 - 0.047)
   and not the bits of fast_ref, which shows that bit 3 selects another kernel (the two references differ by 0.015 - 0.072 in the
   median and by more than 16 ulp in 99.6 % of the outputs).
b. Random operands (N(0, 1) inputs, uniform weights * sqrt(3 / K): what the small-bit inputs cannot reach — subnormal hi parts of
   tiny weights, mixed exponents) against fp64 on the ROUNDED operands x^ = float16(x), w^ = float16(w 2^p) 2^-p, elementwise within
   (T + 4) 2^-24 (conv(|x^|, |w^|) + |b|), T = Cin KH KW, plus 2^-22 |out| + 3e-8 for the split-f16 store: any fp32 summation order.
c. Correlation and lookup through atdn_corr_lookup_bricks_mode(fast = 1): corr_bricks_kernel<true> at (2, 256, 20, 64) and
   corr_bricks_kernel_k160<true> at (1, 160, 17, 25) (odd at every level, N no multiple of 128). Source features hi + lo, target
   features multiples of 0.5 with lo = 0: their 2x2 averages stay f16 numbers with lo = 0 at every level (multiples of 1/8, 1/32,
   1/128), so ALL FOUR levels must equal (sum hi_src * pooled_tgt) * fp32(1 / sqrt(C)), rounded once, bit for bit; a second run
   with lo != 0 in the target too holds level 0 to the same. The K = 160 kernel in split-f16 arithmetic (fast = 0), which no
   direct test reached: within (3 K + 3) 2^-24 scale sum |a| |b| (three MFMAs per product, no lo x lo term with lo_tgt = 0).
   cor1 of lookup_conv_kernel<true, true> against its own operands, relu(sum float16(samples) w^ + b) in fp64 with `samples` read
   back from the same call: within (324 + 4) 2^-24 (sum |s^| |w^| + |b|) + 2^-22 |out| + 3e-8 + sum_k gap_k |w^_k|, where gap_k is
   the f16 spacing at sample k if it decodes to an EXACT f16 midpoint and 0 otherwise (f16_exact_ref.f16_midpoint_gap). The last
   term corrects the bound as first derived, which took float16(hi + lo) == hi for granted: the sampling kernel stores hi =
   f16(v), lo = f16(v - hi), and v - hi has up to 12 significant bits of which lo keeps 11, so a v one fp32 step beside a midpoint
   on the ODD neighbour's side gets lo = exactly half a spacing and decodes to the midpoint, which float16 rounds to the EVEN
   neighbour; a v that is the midpoint decodes to the same number with hi even. The decoded value cannot tell the two apart
   (3 of 2^13 bit patterns: 621 of 829,440 and 80 of 137,700 samples here), the FAST kernel multiplies the hi it stored, and one
   f16 spacing of a sample of 16 - 32 times a weight of 0.05 is 7.5e-4 against a bound of ~2e-4. Measured without the term: 11 of
   2,560 and 2 of 425 rows over the bound by up to 3.7 x, every one of them holding a midpoint sample; with it, none.
   tests/test_f16_exact_host.py plants such values and checks the function. Coordinates: the probe set of
   flow_limits_cases.make_flow_init in pair 0, uniform +-9 px in pair 1.
d. The f16 handle in low-latency form, RAFTGMA(precision="f16", low_latency=True), at 152x216 (N = 513, 17 chunks: two key ranges,
   attn_v3_kernel<true, true> + attn_reduce_kernel — run by no other test) and at 128x128 (one range: the non-split kernel under
   the parallel graph branches): _check_f16_kernels of tests/test_gpu_aggregate_fold.py (agg against attn @ mf, the rebuilt
   motion_global), the flows within 0.03 / 0.15 px of the fp64 oracle after one and two iterations, sf_clamped == 0, and the agg
   tap within 2 (N + 8) 2^-24 max|mf| of the default f16 handle's when their attn and mf taps are bit-equal (fp32 reassociation
   over the key ranges). The split rule is restated in f16_exact_ref.attn_v_splits and asserted (> 1 and == 1).

Measured on the MI355X (100 tests, 9.2 s for the file, the slowest test 0.8 s; all passed on their first run but cor1, whose
bound was corrected as described under c; no kernel needed a fix):
  a. all 53 (case, store) runs and all 24 tile-form runs torch.equal to fast_ref. The split-f16 kernel on the same inputs:
     1.3e-5 - 8.7e-4 of a bound of 0.008 - 0.047, never fast_ref's bits.
  b. worst error / bound 0.027 (1x1 stride-2 GEMM-shaped, T = 96), otherwise 0.000 - 0.010: the bound is linear in T, the error
     of a random sum grows like sqrt(T); max error 8.3e-7 - 3.9e-6.
  c. all four levels bit-equal at both shapes, level 0 with a split target too; samples against the fp64 sampler 7.3e-5 on 25.1 and
     2.9e-5 on 22.1; cor1 worst error / bound 0.786 (C = 256) and 0.652 (C = 160); the K = 160 kernel in split-f16 arithmetic
     0.0005 - 0.0013 of its bound (max error 9.5e-7 on level 0).
  d. 152x216 low-latency f16: agg against its own operands 1.98e-4 of 1.30e-3, rebuilt motion_global 2.4e-7 (4.7e-6 inside its
     bound), flow_low / flow_up 8.5e-4 / 3.7e-3 px after one iteration and 1.3e-3 / 6.7e-3 px after two (of 0.03 / 0.15); attn
     and mf taps bit-equal to the default f16 handle's, agg 3.6e-7 apart (bound 8.0e-5, two key ranges). 128x128: 3.43e-4 of
     1.05e-3, 2.4e-7, 5.6e-4 / 2.5e-3 and 1.2e-3 / 4.2e-3 px; agg identical to the default handle's (one range).
  Teeth: a scratch build (not in the tree) whose FAST halo kernels drop the last K chunk (3x3) or read one lo fragment in place
  of a hi fragment (1x5 / 5x1; same memory accesses as the split-f16 build) fails all 70 halo-path tests of a and b and none of the
  23 GEMM-path ones, which it does not touch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f16_exact_ref as ex  # noqa: E402
import flow_limits_cases as lim  # noqa: E402
from atdn_vslam_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAST = 8   # bit 3 of atdn_conv2d_nhwc_sf_epi's sf_store

CASES = ex.conv_cases()
STORE_CASES = [(nc, st) for nc in CASES for st in (0, 1) if st == 0 or nc[1][1] % 32 == 0]
RUN_STORE_CASES = [(nc, st) for nc in CASES if nc[0] == "run" for st in (0, 1)]


def _store_id(p):
    return "%s-%s" % (ex.case_id(p[0]), "sf" if p[1] else "f32")


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


def _conv(case, x, w, b, sf_store):
    """x [nimg, Cin, H, W], w [Cout, Cin, KH, KW], b [Cout] fp32 arrays -> [nimg, Cout, Ho, Wo] fp32 CPU tensor."""
    cin, cout, kh, kw, stride, ph, pw, H, W, nimg = case
    ho, wo = ex.conv_out(H, kh, stride, ph), ex.conv_out(W, kw, stride, pw)
    xd = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().to(DEV)
    wt, bt = torch.from_numpy(w).contiguous(), torch.from_numpy(b).contiguous()
    out = torch.full((nimg, ho, wo, cout), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().atdn_conv2d_nhwc_sf_epi(_vp(xd), nimg, H, W, cin, _vp(wt), _vp(bt), cout, kh, kw, stride, ph, pw,
                                                  int(sf_store), _vp(out), _stream()))
    torch.cuda.synchronize()
    return out.cpu().permute(0, 3, 1, 2)


def _mismatch(got, want):
    bad = got != want
    n = int(bad.sum())
    if n == 0:
        return "equal"
    i = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d differ, first at %s: got %r want %r, max |diff| %.4g" % (
        n, bad.numel(), i, float(got[i]), float(want[i]), float((got.double() - want.double()).abs().max()))


# ----------------------------------------------------------------------------- a. exact convolutions
@pytest.mark.parametrize("p", STORE_CASES, ids=[_store_id(p) for p in STORE_CASES])
def test_fast_conv_returns_the_hi_product_exactly(p):
    """(a) of the module docstring: bit 3 -> conv(hi_x, hi_w) + b exactly; without it -> conv(x, w) + b within
    2e-5 * max|full_ref| and other bits."""
    (_, case), store = p
    e = ex.exact_conv(case)
    want = e["fast_ref"].float()
    got = _conv(case, e["x"], e["w"], e["b"], FAST | store)
    assert torch.equal(got, want), _mismatch(got, want)
    full = _conv(case, e["x"], e["w"], e["b"], store)
    err, scale = float((full.double() - e["full_ref"]).abs().max()), float(e["full_ref"].abs().max())
    print("F16-EXACT %s: split-f16 kernel max error %.3g of bound %.3g" % (_store_id(p), err, 2e-5 * scale))
    assert bool(torch.isfinite(full).all()) and err < 2e-5 * scale, (err, 2e-5 * scale)
    assert not torch.equal(full, want), "sf_store without bit 3 returned the plain-f16 product"


@pytest.mark.parametrize("p", RUN_STORE_CASES, ids=[_store_id(p) for p in RUN_STORE_CASES])
def test_fast_tile_forms_return_the_same_bits(p):
    """FAST run tiles (bit 2) and FAST rectangular 8 x 16 x 128 tiles (bit 1) of the 1x5 / 5x1 kernels: equal to each other and
    to fast_ref (the product's own choice for these small grids, 4 x 16 x 64, is the case of the test above)."""
    (_, case), store = p
    e = ex.exact_conv(case)
    want = e["fast_ref"].float()
    run = _conv(case, e["x"], e["w"], e["b"], FAST | 4 | store)
    rect = _conv(case, e["x"], e["w"], e["b"], FAST | 2 | store)
    assert torch.equal(run, rect), _mismatch(run, rect)
    assert torch.equal(run, want), _mismatch(run, want)


def test_conv_entry_rejects_bad_store_words():
    x = torch.zeros(1, 8, 8, 32, device=DEV)
    w, out = torch.zeros(32, 32, 3, 3), torch.zeros(1, 8, 8, 32, device=DEV)
    for word in (-1, 6, 7, 14, 15, 16):
        rc = _lib.lib().atdn_conv2d_nhwc_sf_epi(_vp(x), 1, 8, 8, 32, _vp(w), None, 32, 3, 3, 1, 1, 1, word, _vp(out), _stream())
        assert rc != 0 and b"sf_store" in _lib.lib().atdn_last_error(), word


# ----------------------------------------------------------------------------- b. random operands
@pytest.mark.parametrize("k", range(len(CASES)), ids=[ex.case_id(c) for c in CASES])
def test_fast_conv_random_operands_within_the_derived_bound(k):
    """(b) of the module docstring. One epilogue per case: the split-f16 store for every other case that has one."""
    _, case = CASES[k]
    store = 1 if case[1] % 32 == 0 and k % 2 == 0 else 0
    r = ex.random_conv(case)
    got = _conv(case, r["x"], r["w"], r["b"], FAST | store).double()
    assert bool(torch.isfinite(got).all())
    err, bound = (got - r["ref"]).abs(), ex.random_conv_bound(case, r, store)
    ratio = float((err / bound).max())
    print("F16-RANDOM %s %s: worst error / bound %.3f (max error %.3g)" % (ex.case_id(CASES[k]), "sf" if store else "f32", ratio,
                                                                          float(err.max())))
    assert ratio <= 1.0, ratio


# ----------------------------------------------------------------------------- c. correlation and lookup
def _corr(f1, f2, fast, coords=None, convc1=None):
    """f1, f2 [B, C, H8, W8] fp32 arrays -> (four levels [B * N, H_l * W_l], samples [B * N, 324], cor1 [B * N, 256]), CPU."""
    B, Cc, H8, W8 = f1.shape
    N = H8 * W8
    a = torch.from_numpy(f1).permute(0, 2, 3, 1).reshape(B, N, Cc).contiguous().to(DEV)
    b = torch.from_numpy(f2).permute(0, 2, 3, 1).reshape(B, N, Cc).contiguous().to(DEV)
    pyr = [torch.full((B * N, (H8 >> l) * (W8 >> l)), float("nan"), device=DEV) for l in range(4)]
    null = C.c_void_p(None)
    c = samples = cor1 = wv = bv = None
    if coords is not None:
        c = torch.from_numpy(coords).permute(0, 2, 3, 1).reshape(B * N, 2).contiguous().to(DEV)
        samples = torch.full((B * N, 324), float("nan"), device=DEV)
        wv, bv = torch.from_numpy(convc1[0]).contiguous(), torch.from_numpy(convc1[1]).contiguous()
        cor1 = torch.full((B * N, 256), float("nan"), device=DEV)
    opt = lambda t: _vp(t) if t is not None else null   # noqa: E731
    _lib.check(_lib.lib().atdn_corr_lookup_bricks_mode(_vp(a), _vp(b), B, H8, W8, Cc, opt(c), *[_vp(p) for p in pyr], opt(samples),
                                                       opt(wv), opt(bv), opt(cor1), int(fast), _stream()))
    torch.cuda.synchronize()
    return [p.cpu() for p in pyr], None if samples is None else samples.cpu(), None if cor1 is None else cor1.cpu()


@pytest.mark.parametrize("shape", ex.CORR_SHAPES, ids=["%dx%dx%dx%d" % s for s in ex.CORR_SHAPES])
def test_fast_correlation_levels_are_exact_and_cor1_matches_its_operands(shape):
    """(c) of the module docstring, fast = 1."""
    from oracle import gma_ref
    B, Cc, H8, W8 = shape
    hi1, f1, hi2, f2 = ex.corr_features(shape)
    coords, outside = ex.probe_coords(shape)
    wc, bc = ex.convc1_weights()
    pyr, samples, cor1 = _corr(f1, f2, 1, coords, (wc, bc))
    want = ex.corr_levels(hi1, ex.pooled_levels(f2), Cc)
    for l in range(4):
        assert torch.equal(pyr[l], want[l].float()), "level %d: %s" % (l, _mismatch(pyr[l], want[l].float()))
    # target features with lo != 0 as well: level 0
    hi1b, f1b, hi2b, f2b = ex.corr_features(shape, target_lo=True)
    pyrb, _, _ = _corr(f1b, f2b, 1)
    wantb = ex.corr_levels(hi1b, [torch.from_numpy(hi2b.astype(np.float64))], Cc)[0].float()
    assert torch.equal(pyrb[0], wantb), "level 0 with a split target: %s" % _mismatch(pyrb[0], wantb)
    # the sampling code on that (exact) pyramid against the oracle's bilinear sampler in fp64, at the bound of
    # test_product_corr_kernels_match_oracle
    ref = gma_ref.corr_lookup([w.reshape(B * H8 * W8, 1, H8 >> l, W8 >> l) for l, w in enumerate(want)],
                              torch.from_numpy(coords).double())
    ref = ref.permute(0, 2, 3, 1).reshape(B * H8 * W8, 324)
    assert bool(torch.isfinite(samples).all()) and bool(torch.isfinite(cor1).all())
    e_s, scale = float((samples.double() - ref).abs().max()), float(ref.abs().max())
    assert e_s < 2e-5 * max(1.0, scale), (e_s, scale)
    # cor1 of the FAST fused kernel against its own operands
    s_np = samples.numpy()
    s_hat = torch.from_numpy(ex.round_inputs(s_np)).double()
    tie_gap = torch.from_numpy(ex.f16_midpoint_gap(s_np)).double()
    w_hat = torch.from_numpy(ex.round_weights(wc)).double()
    bias = torch.from_numpy(bc).double()
    own = torch.relu(s_hat @ w_hat.t() + bias)
    mag = s_hat.abs() @ w_hat.abs().t() + bias.abs()
    base = (324 + 4) * 2.0 ** -24 * mag + 2.0 ** -22 * own + 3e-8
    bound = base + tie_gap @ w_hat.abs().t()
    err = (cor1.double() - own).abs()
    ratio = float((err / bound).max())
    over = (err > base).any(1)
    print("F16-CORR %s fast: samples against fp64 %.3g (max %.3g); cor1 worst error / bound %.3f (max error %.3g); %d of %d samples "
          "are f16 midpoints, in %d rows; %d rows exceed the bound without the midpoint term, %d of them hold a midpoint"
          % (shape, e_s, scale, ratio, float(err.max()), int((tie_gap > 0).sum()), tie_gap.numel(), int((tie_gap > 0).any(1).sum()),
             int(over.sum()), int((over & (tie_gap > 0).any(1)).sum())))
    assert ratio <= 1.0, ratio
    for y, x in outside:     # windows outside the map at every level: exact zeros, relu(bias) to the store's error
        n = y * W8 + x
        assert bool((samples[n] == 0).all()), (y, x)
        assert float((cor1[n].double() - torch.relu(bias)).abs().max()) <= 2.0 ** -22 * float(bias.abs().max()) + 3e-8, (y, x)


def test_k160_correlation_in_split_f16_arithmetic():
    """corr_bricks_kernel_k160<false> on caller features (the network reaches it only with its folded head): all four levels
    within (3 K + 3) 2^-24 scale sum |a| |b| of the fp64 product of the full operands."""
    shape = ex.CORR_SHAPES[1]
    Cc = shape[1]
    _, f1, _, f2 = ex.corr_features(shape)
    pyr, _, _ = _corr(f1, f2, 0)
    levels = ex.pooled_levels(f2)
    want, mag = ex.corr_levels(f1, levels, Cc), ex.corr_mag(f1, levels, Cc)
    for l in range(4):
        bound = ex.corr_split_bound(Cc, mag[l])
        err = (pyr[l].double() - want[l]).abs()
        ratio = float((err / bound).max())
        print("F16-CORR k160 split-f16 level %d: worst error / bound %.4f (max error %.3g)" % (l, ratio, float(err.max())))
        assert bool(torch.isfinite(pyr[l]).all()) and ratio <= 1.0, (l, ratio)


def test_corr_entry_rejects_other_channel_counts_and_modes():
    f = torch.zeros(1, 16 * 16, 128, device=DEV)
    null = C.c_void_p(None)
    rc = _lib.lib().atdn_corr_lookup_bricks_mode(_vp(f), _vp(f), 1, 16, 16, 128, *([null] * 9), 1, _stream())
    assert rc != 0 and b"256 or 160" in _lib.lib().atdn_last_error()
    f = torch.zeros(1, 16 * 16, 160, device=DEV)
    rc = _lib.lib().atdn_corr_lookup_bricks_mode(_vp(f), _vp(f), 1, 16, 16, 160, *([null] * 9), 2, _stream())
    assert rc != 0 and b"fast must be" in _lib.lib().atdn_last_error()


# ----------------------------------------------------------------------------- d. the f16 handle in low-latency form
@pytest.mark.timeout(600)
@pytest.mark.parametrize("hw", [lim.ODD, (128, 128)], ids=["152x216-two-key-ranges", "128x128-one-key-range"])
def test_f16_low_latency_handle(hw):
    """(d) of the module docstring."""
    import test_gpu_aggregate_fold as af
    import test_gpu_flow_geometry as fg
    from atdn_vslam_amd import synthetic as syn
    H, W = hw
    N = (H // 8) * (W // 8)
    ldN = (N + 31) // 32 * 32
    splits = ex.attn_v_splits(1, N)
    assert (splits > 1) if hw == lim.ODD else (splits == 1), splits
    sd = af._state()
    frames = torch.from_numpy(syn.make_frames(2, H, W, seed=af.SEED_FRAMES))
    o64 = af.oracle_pair(sd, frames, 0, torch.float64)
    f1, f2 = frames[0:1].to(DEV), frames[1:2].to(DEV)
    taps = {}
    for ll in (True, False):
        net = fg._net(sd, 1, "f16", ll)
        low1, up1 = net(f1, f2, iters=1, test_mode=True)
        torch.cuda.synchronize()
        taps[ll] = {k: net.debug_read(k, s, H, W)[0].cpu() for k, s in (("agg", (1, N, 128)), ("x", (1, N, 384)), ("attn", (1, N, ldN)))}
        tag = "%dx%d/B1/f16%s" % (H, W, "/ll" if ll else "")
        af._check_f16_kernels(tag, sd, taps[ll]["attn"], taps[ll]["x"], taps[ll]["agg"])
        if ll:
            low2, up2 = net(f1, f2, iters=2, test_mode=True)
            torch.cuda.synchronize()
            for name, got, key, tol in (("flow_low@1", low1, "low1", af.F16_LOW), ("flow_up@1", up1, "up1", af.F16_UP),
                                        ("flow_low@2", low2, "low2", af.F16_LOW), ("flow_up@2", up2, "up2", af.F16_UP)):
                e = float((got[0].cpu().double() - o64[key]).abs().max())
                print("PARITY-F16 %s %s err=%.3e bound=%.3e" % (tag, name, e, tol))
                assert bool(torch.isfinite(got).all()) and e <= tol, (tag, name, e)
        assert fg._sf_clamped(net, hw) == 0.0, tag
        del net
        torch.cuda.empty_cache()
    a, b = taps[True], taps[False]
    # (the 126 convolved channels of the motion features, as in _check_f16_kernels: the two flow channels behind them are
    # overwritten by the iteration's flow update, which follows the aggregate and inherits its reassociation)
    if torch.equal(a["attn"], b["attn"]) and torch.equal(a["x"][:, 128:254], b["x"][:, 128:254]):
        mx = float(a["x"][:, 128:254].abs().max())
        d = float((a["agg"].double() - b["agg"].double())[:, :126].abs().max())
        bound = 2 * (N + 8) * 2.0 ** -24 * mx
        print("PARITY-F16 %dx%d agg low-latency against default: %.3e bound %.3e (%d key ranges)" % (H, W, d, bound, splits))
        assert d <= bound, (d, bound)
        if splits == 1:
            assert d == 0.0   # one range: the same kernel on the same operands
    else:
        print("PARITY-F16 %dx%d: the two handles' attn / mf taps are not bit-equal (the parallel branches changed an operand of "
              "attention x V): their agg taps are not compared" % (H, W))
