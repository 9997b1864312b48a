"""Inputs for which the f16 fast mode (precision "f16": FAST builds that issue the hi x hi MFMA alone) has ONE right answer, bit
for bit, and the two fp64 references that go with them. Shared by tests/test_f16_exact_host.py (CPU: the inputs have the
properties claimed here) and tests/test_gpu_f16_kernels.py (GPU: the kernels return those bits).

A FAST kernel computes wscale * sum f16(x) * f16(w * 2^p) + b with fp32 accumulation; wscale = 2^-p is the power of two that
pack_conv_sf chooses (max |w * 2^p| in [1, 2)), so it commutes with every rounding. Operands here are x = hi + lo, w = hi + lo with
    hi in {+-2.5, +-3, +-3.5}   (not +-2: with a lo of the opposite sign the sum falls into the binade below, where the f16
                                 spacing is 2^-10, and may round elsewhere)
    lo in {+-1, +-2, +-3} * 2^-12
    b  integer in [-8, 8]
so that
  * float16(x) == hi exactly (f16 spacing in [2, 4) is 2^-9, |lo| < 2^-10) and lo is a normal f16 number: after the conversion to
    split-f16 every lo half of both operands is nonzero;
  * every product hi * hi is a multiple of 1/4 and every partial sum of a convolution, in any order, is an integer count of such
    quanta far below 2^24: fp32 accumulation is exact whatever the tile shape, the chunk order or the MFMA's internal order;
  * the result, a few thousand quanta, is exact in fp32 and in the split-f16 store (hi + lo of 11 bits each).
A correct FAST kernel therefore returns fast_ref = conv(hi_x, hi_w) + b exactly, while the full three-product kernel returns
full_ref = conv(x, w) + b to fp32 accuracy, which differs from fast_ref by more than 16 ulp in over 99 % of the outputs (asserted
on the CPU): one leaked lo fragment, one dropped chunk, one wrong tap or pad changes bits.

The case tables are those of tests/test_gpu_parity.py and tests/test_gpu_run_tiles.py, which were chosen to land on each tile plan
and ragged edge. The four largest are cut to the smallest image count / height that conv_sf6_plan and choose_tile (restated in
kernel_plan below, for the two plain epilogues of the test entry) still give the same kernel.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HI = np.array([-3.5, -3.0, -2.5, 2.5, 3.0, 3.5], dtype=np.float32)
LO = (np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32) * np.float32(2.0 ** -12)).astype(np.float32)
QUANTUM = 0.25          # every hi * hi product and every bias is a multiple of it
ULP_GAP = 16            # |full_ref - fast_ref| is held to exceed this many ulp of the result ...
MIN_SHARE = 0.99        # ... in at least this share of the outputs


def split_operand(r, shape, hi_set=HI, lo_set=LO):
    """-> (hi, hi + lo), both fp32 and exact."""
    hi = r.choice(hi_set, size=shape).astype(np.float32)
    lo = r.choice(lo_set, size=shape).astype(np.float32)
    x = (hi.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64))
    return hi, x


def pack_exponent(w):
    """The p of pack_conv_sf (weights.h): w * 2^p has its largest magnitude in [1, 2)."""
    mx = float(np.abs(np.asarray(w, dtype=np.float32)).max())
    return 1 - int(np.frexp(np.float32(mx))[1]) if mx > 0 else 1


def round_weights(w):
    """What a FAST kernel multiplies with: float16(w * 2^p) * 2^-p (fp32 array in, fp32 array out, exact)."""
    p = pack_exponent(w)
    return np.ldexp(np.ldexp(np.asarray(w, dtype=np.float32), p).astype(np.float16).astype(np.float32), -p)


def round_inputs(x):
    """The hi half of the split-f16 conversion: float16(x)."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def f16_midpoint_gap(d):
    """For DECODED split-f16 values d = hi + lo (fp32): the f16 spacing at d where d lies exactly half way between two f16
    numbers, 0 elsewhere. Only there the hi half cannot be told from d: the value that was split may have been the midpoint
    itself (hi = the even neighbour, which float16(d) returns) or one fp32 step beside it on the odd neighbour's side (hi = the
    odd neighbour, and lo = f16(v - hi), 12 significant bits rounded to 11, came out as exactly half a spacing)."""
    d = np.asarray(d, dtype=np.float32)
    h = d.astype(np.float16)
    hf = h.astype(np.float64)
    r = d.astype(np.float64) - hf
    nb = np.nextafter(h, np.where(r > 0, np.inf, -np.inf).astype(np.float16)).astype(np.float64)
    tie = (r != 0) & np.isfinite(nb) & (2.0 * d.astype(np.float64) == hf + nb)
    return np.where(tie, np.abs(nb - hf), 0.0)


def sf_roundtrip(v):
    """Decoded split-f16 store of fp32 values: hi = f16(v), lo = f16(v - hi), hi + lo in fp32 (sf.h)."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi + lo


# ----------------------------------------------------------------------------- convolution cases
# (Cin, Cout, KH, KW, stride, padH, padW, H, W, nimg)
def _tables():
    import test_gpu_parity as gp
    import test_gpu_run_tiles as rt
    conv = [c[:10] for c in gp.CONV_CASES if c[0] % 32 == 0]
    stride2 = [(ci, co, 3, 3, 2, 1, 1, H, W, n) for ci, co, H, W, n in gp.STRIDE2_CASES]
    halo = [(ci, co, kh, kw, 1, ph, pw, H, W, n) for ci, co, kh, kw, ph, pw, H, W, n in gp.HALO_CASES]
    run = [(ci, co, kh, kw, 1, kh // 2, kw // 2, H, W, n) for ci, co, kh, kw, H, W, n in rt.RUN_CASES]
    return conv, stride2, halo, run


def cdiv(a, b):
    return -(-a // b)


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def kernel_plan(case, tile_form=0):
    """The kernel conv_sf_dispatch gives this shape under EpiBias<ACT_NONE> / SfBias<ACT_NONE> (plain channel-vector epilogues, no
    normalise-on-load; the FAST flag does not enter for them): ("halo", th, bn) / ("run", 8, 128) of conv_sf6_plan (conv_sf6.h) or
    ("gemm", BM, BN) of choose_tile (conv_dispatch.h). Host arithmetic only; tests/test_f16_exact_host.py holds the cut cases to
    the plans of the originals with it."""
    cin, N, kh, kw, stride, ph, pw, H, W, nimg = case
    Ho, Wo = conv_out(H, kh, stride, ph), conv_out(W, kw, stride, pw)
    if stride == 1 and (kh, kw) in ((3, 3), (1, 5), (5, 1)) and cin % 32 == 0 and N >= 4:
        k3 = kh == 3
        tiles = nimg * cdiv(Wo, 16) * cdiv(Ho, 8)
        bn = 64
        if N <= 32 and k3:
            bn = 32
        elif N == 96 and k3:
            bn = 96
        else:
            best = cdiv(N, 64) * 64
            for c in (128, 256):
                if cdiv(N, c) * c <= best:
                    best, bn = cdiv(N, c) * c, c
        while bn > 64 and bn != 96 and tiles * cdiv(N, bn) < 300:
            bn //= 2
        if not k3:
            bn = min(bn, 128)
        fits12 = k3 and bn in (64, 96) and cdiv(Ho, 12) * 12 * 100 <= cdiv(Ho, 8) * 8 * 103
        L = W if kh == 1 else H
        run_ok = (not k3) and ph == kh // 2 and pw == kw // 2 and (L + 126) // L <= 3
        if not k3 and tile_form == 1:
            return ("halo", 8, 128)
        if run_ok and tile_form == 2:
            return ("run", 8, 128)
        if bn == 64 and tiles * cdiv(N, 64) < 300:
            return ("halo", 4, 64)
        if fits12 and nimg * cdiv(Wo, 16) * cdiv(Ho, 12) * cdiv(N, bn) >= 512:
            return ("halo", 12, bn)
        if run_ok and bn == 128:
            return ("run", 8, 128)
        return ("halo", 8, bn)
    HoWo = Ho * Wo
    if N <= 32:
        return ("gemm", 128, 32)
    if N % 96 == 0 and N % 64 != 0:
        return ("gemm", 128, 96)
    t128 = nimg * cdiv(HoWo, 128)
    pad128 = cdiv(N, 128) * 128 - N
    if N >= 128 and pad128 * 20 <= N and t128 * cdiv(N, 128) >= 400:
        return ("gemm", 128, 128)
    if t128 * cdiv(N, 64) >= 384:
        return ("gemm", 128, 64)
    return ("gemm", 64, 64)


# original case -> the cut case that runs (same plan, same ragged edges: the widths and odd heights are kept)
CUTS = {
    # 12 x 16 x 64 halo tiles need >= 512 of them: 2 x 39 x 8 = 624 (was 2 x 39 x 16); the last tile row keeps 8 live rows of 12
    (64, 64, 3, 3, 1, 1, 1, 188, 616, 2): (64, 64, 3, 3, 1, 1, 1, 92, 616, 2),
    # 8 x 16 x 128 halo tiles need >= 300 tiles of 8 x 16: 50 images of 2 x 3 tiles, one live row / column in the last ones
    (128, 128, 3, 3, 1, 1, 1, 47, 154, 5): (128, 128, 3, 3, 1, 1, 1, 9, 33, 50),
    # GEMM-shaped 128 x 96 (N % 96 == 0: at any size) and 64 x 64 (fewer than 384 / 2 tiles of 128 rows: at any smaller size)
    (64, 96, 3, 3, 2, 1, 1, 188, 616, 2): (64, 96, 3, 3, 2, 1, 1, 46, 616, 1),
    (96, 128, 3, 3, 2, 1, 1, 94, 308, 3): (96, 128, 3, 3, 2, 1, 1, 94, 308, 1),
    # 8 x 16 x 64 halo tiles, N = 192 = 3 blocks: >= 100 tiles against 4-row tiles, < 512 / 3 twelve-row tiles: 2 x 60
    (256, 192, 3, 3, 1, 1, 1, 47, 154, 3): (256, 192, 3, 3, 1, 1, 1, 47, 154, 2),
    # run tiles by the product's own rule (128-wide blocks: >= 150 tiles of 8 x 16 at N = 256, >= 300 at N = 128; run length >= 43)
    (384, 256, 1, 5, 1, 0, 2, 47, 154, 4): (384, 256, 1, 5, 1, 0, 2, 9, 49, 19),     # 19 x 2 x 4 = 152; 441 pixels = 3 tiles + 57
    (384, 128, 5, 1, 1, 2, 0, 47, 154, 6): (384, 128, 5, 1, 1, 2, 0, 47, 17, 25),    # 25 x 6 x 2 = 300; 799 pixels = 6 tiles + 31
    # 8 x 16 x 64 halo tiles, N = 126 = 2 blocks, the second partial: 150 <= tiles < 300 (128-wide from 300 on): 3 x 60
    (256, 126, 3, 3, 1, 1, 1, 47, 154, 4): (256, 126, 3, 3, 1, 1, 1, 47, 154, 3),
}


def conv_cases():
    """-> (list of (table name, case)), the large cases replaced by their cuts."""
    conv, stride2, halo, run = _tables()
    out = []
    for name, table in (("conv", conv), ("stride2", stride2), ("halo", halo), ("run", run)):
        out += [(name, CUTS.get(c, c)) for c in table]
    return out


def case_id(nc):
    name, c = nc
    return "%s-%dto%d-%dx%d-s%d-%dx%dx%d" % ((name,) + tuple(c[:5]) + tuple(c[7:10]))


def case_seed(case):
    return (sum((i + 1) * 7919 * int(v) for i, v in enumerate(case)) + 17) & 0x7FFFFFFF


# ----------------------------------------------------------------------------- operands and references
def _conv64(x, w, b, case):
    _, _, _, _, stride, ph, pw = case[:7]
    return F.conv2d(torch.from_numpy(np.asarray(x, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64)),
                    None if b is None else torch.from_numpy(np.asarray(b, dtype=np.float64)), stride=stride, padding=(ph, pw))


_exact_cache = {}


def exact_conv(case):
    """-> dict: x, w, b (fp32 arrays, NCHW / torch weight layout), hi_x, hi_w, fast_ref, full_ref (fp64 tensors). Computed once
    per case and shared by the tests of that case; callers must not write into it."""
    if case not in _exact_cache:
        if len(_exact_cache) >= 2:     # the tests of one case run next to each other: two entries are enough
            _exact_cache.pop(next(iter(_exact_cache)))
        cin, cout, kh, kw, _, _, _, H, W, nimg = case
        r = np.random.RandomState(case_seed(case))
        hi_x, x = split_operand(r, (nimg, cin, H, W))
        hi_w, w = split_operand(r, (cout, cin, kh, kw))
        b = r.randint(-8, 9, size=(cout,)).astype(np.float32)
        _exact_cache[case] = {
            "x": x, "w": w, "b": b, "hi_x": hi_x, "hi_w": hi_w,
            "fast_ref": _conv64(hi_x, hi_w, b, case), "full_ref": _conv64(x, w, b, case)}
    return _exact_cache[case]


def exact_conv_magnitude(case):
    """max of conv(|hi_x|, |hi_w|) + |b|: what any partial sum of the FAST kernel, in any order, stays below."""
    e = exact_conv(case)
    return float(_conv64(np.abs(e["hi_x"]), np.abs(e["hi_w"]), np.abs(e["b"]), case).max())


def random_conv(case):
    """The operands of the existing fp64 tests (N(0, 1) inputs, uniform weights * sqrt(3 / K), bias +-0.5) with the fp64
    convolution of the ROUNDED operands and the magnitude sum of the derived bound.
    -> dict: x, w, b (fp32 arrays), ref, mag (fp64 tensors)."""
    cin, cout, kh, kw, _, _, _, H, W, nimg = case
    r = np.random.RandomState(case_seed(case) ^ 0x5A5A)
    x = r.normal(0, 1, (nimg, cin, H, W)).astype(np.float32)
    w = (r.uniform(-1, 1, (cout, cin, kh, kw)) * np.sqrt(3.0 / (cin * kh * kw))).astype(np.float32)
    b = r.uniform(-0.5, 0.5, (cout,)).astype(np.float32)
    xr, wr = round_inputs(x), round_weights(w)
    return {"x": x, "w": w, "b": b, "ref": _conv64(xr, wr, b, case), "mag": _conv64(np.abs(xr), np.abs(wr), np.abs(b), case)}


def random_conv_bound(case, r, sf_store):
    """Elementwise bound of a FAST convolution against r["ref"]: (T + 4) * 2^-24 * (conv(|x^|, |w^|) + |b|), T = Cin * KH * KW —
    T - 1 additions in any order, each within 2^-24 relative of its partial sum, which is at most the magnitude sum (first-order
    sum (T - 1) u, with the second-order terms and the multiplication by the power-of-two wscale inside the spare units), the bias
    add and one more for a fused form of it. The split-f16 store adds its representation error 2^-22 |out| + 3e-8 (sf.h)."""
    cin, _, kh, kw = case[:4]
    bound = (cin * kh * kw + 4) * 2.0 ** -24 * r["mag"]
    if sf_store:
        bound = bound + 2.0 ** -22 * r["ref"].abs() + 3e-8
    return bound


def ulp32(v):
    """Spacing of fp32 at |v| (fp64 tensor in, fp64 tensor out)."""
    a = v.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ----------------------------------------------------------------------------- correlation and lookup
CORR_SHAPES = [(2, 256, 20, 64), (1, 160, 17, 25)]   # (B, C, H8, W8)
TGT = np.arange(-7, 8, dtype=np.float32) * np.float32(0.5)    # target hi parts: multiples of 0.5 in [-3.5, 3.5]


def corr_scale(C):
    """The entry's scale 1 / sqrt(C) as the library forms it, in fp32 (1/16 for C = 256)."""
    return np.float32(1.0) / np.sqrt(np.float32(C))


def corr_features(shape, target_lo=False):
    """-> (hi1, f1, hi2, f2) fp32 [B, C, H8, W8]: source features hi + lo; target features multiples of 0.5 with lo = 0 (their 2x2
    averages stay exact at every level) or, target_lo, hi + lo like the source (level 0 only)."""
    r = np.random.RandomState(1000 + shape[1] + (1 if target_lo else 0))
    hi1, f1 = split_operand(r, shape)
    if target_lo:
        hi2, f2 = split_operand(r, shape)
    else:
        hi2 = r.choice(TGT, size=shape).astype(np.float32)
        f2 = hi2.copy()
    return hi1, f1, hi2, f2


def pooled_levels(f2):
    """fp64 [B, C, H_l, W_l] for l = 0..3: 2x2 averages with floor sizes, as avg_pool2d(2, stride 2)."""
    lv = [torch.from_numpy(np.asarray(f2, dtype=np.float64))]
    for _ in range(3):
        lv.append(F.avg_pool2d(lv[-1], 2, stride=2))
    return lv


def corr_levels(src, levels, C):
    """fp64 [B * N, H_l * W_l] per level: (sum_c src[p, c] * level[q, c]) * fp32(1 / sqrt(C)), the product with the scale taken
    exactly (rounding it to fp32 is the kernel's one rounding when the sum is exact)."""
    B = src.shape[0]
    a = torch.from_numpy(np.asarray(src, dtype=np.float64)).reshape(B, C, -1).transpose(1, 2)     # [B, N, C]
    s = float(corr_scale(C))
    return [(a @ t.reshape(B, C, -1)).reshape(-1, t.shape[2] * t.shape[3]) * s for t in levels]


def corr_mag(src, levels, C):
    """fp64 per level: sum_c |src| |level| (before the scale)."""
    B = src.shape[0]
    a = torch.from_numpy(np.abs(np.asarray(src, dtype=np.float64))).reshape(B, C, -1).transpose(1, 2)
    return [(a @ t.abs().reshape(B, C, -1)).reshape(-1, t.shape[2] * t.shape[3]) for t in levels]


def corr_split_bound(C, mag):
    """Elementwise bound of a split-f16 correlation level (three MFMAs per product: hi x hi, hi x lo, lo x hi) against the fp64
    product of the full operands, for operands that split exactly and a target with lo = 0 (no lo x lo term is dropped):
    3 C products summed in fp32 in any order, the scale and the store: (3 C + 3) 2^-24 scale sum |a| |b|."""
    return (3 * C + 3) * 2.0 ** -24 * float(corr_scale(C)) * mag


def probe_coords(shape):
    """[B, 2, H8, W8] fp32 (x, y): the grid plus the flow_init of tests/flow_limits_cases.py (uniform +-6 px and its planted probes:
    integer, half, negative fraction, each border, far corner, fully outside) in pair 0, uniform +-9 px in the others.
    -> (coords, [(y, x) of pair 0's pixels whose windows miss the map at every level])."""
    import flow_limits_cases as lim
    B, _, H8, W8 = shape
    fi, _, outside = lim.make_flow_init((H8 * 8, W8 * 8))
    ys, xs = np.meshgrid(np.arange(H8, dtype=np.float32), np.arange(W8, dtype=np.float32), indexing="ij")
    grid = np.stack([xs, ys])[None].repeat(B, 0)
    off = np.random.RandomState(5).uniform(-9, 9, (B, 2, H8, W8)).astype(np.float32)
    off[0] = fi[0].numpy()
    return (grid + off).astype(np.float32), outside


def convc1_weights(seed=3):
    r = np.random.RandomState(seed)
    w = (r.uniform(-1, 1, (256, 324)) * np.sqrt(3.0 / 324)).astype(np.float32)
    b = r.uniform(-0.5, 0.5, (256,)).astype(np.float32)
    return w, b


# ----------------------------------------------------------------------------- attention x V key ranges
def attn_v_splits(B, N):
    """attn_v_splits of attention.hip for a low-latency handle: key ranges of attention x V (1: the non-split kernel)."""
    RT, Q = cdiv(N, 32), cdiv(N, 32)
    tiles = B * cdiv(RT, 8)
    n = min(8, max(1, 256 // max(tiles, 1)))
    while n > 1 and cdiv(Q, n) < 8:
        n -= 1
    return n
