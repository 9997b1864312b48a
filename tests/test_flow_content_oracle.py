"""The content cases of tests/test_gpu_flow_content.py (flow_content_cases.py) on the CPU oracle alone: they are finite, they are
what they claim, and the yardstick of the GPU test binds.

(i) Every tensor fg._oracle_pair returns is finite in fp64 and fp32 for every (geometry, content) a GPU case compares.

(ii) The contents, asserted on the fp64 oracle. black / white / grey / checker: the stem convolution's output (7x7, stride 2) has
per-channel variance EXACTLY 0 over the outputs whose window is whole, in fnet and cnet; all variance comes from the zero-padding
border. Largest rstd of fnet's first InstanceNorm: grey 315 (1 / sqrt(eps) = 316: eps IS the variance), faint 125, lowcontrast
114; black / white 11.7 at 128x128, 16.3 at 184x328, 26.1 at 376x1232 (border-only variance, its share shrinks with the map),
checker 15.9; textured 9.9, sky_road 6.4 to 7.1. Attention rows of black / white / grey: max / min < 2 (1.74 at most) among the
features 4 or more from the map's edge; over ALL features 1.95 for grey, but 5e11 (white) and 2e20 (black): the border features'
logits stand far from the interior's, so "uniform" holds for the interior only. Largest weight: grey 4.50e-3 at 128x128 (uniform:
3.91e-3), black 8.9e-2, white 0.34. `identical` has fmap1 == fmap2 bit for bit. max |corr|: 19 to 25 at 128x128, 33 (black,
grey) and 44 (white) at 184x328, 58 (sky_road) and 82 (black) at 376x1232.

(iii) The caps. max|x_hip - x64| <= min(M * max|x32 - x64| + FLOOR * max|x64|, cap) only means something where the fp32 oracle is
well inside cap: for every (case, tensor) max|x32 - x64| <= cap / 2, with cap the stated tolerance of test_gpu_flow_geometry.py
and, for pyr0..3 and lookup0, TOL_ACT * max(1, max|x64| / 25). A (case, tensor) that is not must be in cc.RELATIVE_CAP, where
1e-3 * max|x64| (parity_check.CAP) takes the cap's place; the list holds pyr0 and lookup0 of `grey` at both geometries and
test_the_exception_list_is_grey_correlations_only keeps it to correlation tensors of grey pairs.

Measured (8 threads, make_gma_state(seed=1), twelve iterations; max|x32 - x64|):

    frames, content           flow_low  flow_up  fmap1    pyr0     lookup0  its cap  max|corr|  net1     attn / its cap
    128x128  black            1.2e-5    6.6e-5   4.2e-6   1.2e-5   1.3e-5   1.0e-4   19.3       3.0e-6   0.20
    128x128  white            9.0e-6    5.3e-5   4.0e-6   9.7e-6   1.0e-5   1.0e-4   24.7       2.7e-6   0.055
    128x128  grey             3.4e-6    1.7e-5   2.7e-5   5.6e-5   5.6e-5   1.0e-4   19.1       7.4e-7   0.002    <- RELATIVE_CAP
    128x128  lowcontrast      4.2e-6    1.7e-5   1.5e-5   2.0e-5   2.0e-5   1.0e-4   4.6        7.1e-7   0.002
    128x128  faint            4.1e-6    1.4e-5   1.0e-5   1.3e-5   1.2e-5   1.0e-4   10.1       5.2e-7   0.002
    128x128  identical        5.4e-6    2.0e-5   4.0e-6   8.0e-6   6.6e-6   1.0e-4   11.0       7.5e-7   0.016
    128x128  half_saturated   9.0e-6    3.6e-5   4.6e-6   9.8e-6   9.8e-6   1.0e-4   13.7       2.8e-6   0.047
    128x128  top_black        6.5e-6    3.4e-5   5.2e-6   1.0e-5   1.0e-5   1.0e-4   16.5       4.3e-6   0.055
    128x128  checker          9.8e-6    4.1e-5   4.3e-6   1.1e-5   1.1e-5   1.0e-4   19.5       2.4e-6   0.050
    128x128  impulse          1.1e-5    6.0e-5   5.6e-6   1.3e-5   1.2e-5   1.0e-4   17.1       3.2e-6   0.18
    128x128  sky_road         8.9e-6    3.4e-5   4.9e-6   1.3e-5   9.9e-6   1.0e-4   18.0       3.6e-6   0.030
    128x128  textured         5.5e-6    2.0e-5   4.0e-6   7.1e-6   7.1e-6   1.0e-4   9.2        8.1e-7   0.016
    184x328  black            1.5e-5    6.5e-5   4.7e-6   3.9e-5   4.7e-5   1.3e-4   32.7       3.0e-6   0.14
    184x328  white            1.4e-5    9.2e-5   5.7e-6   2.9e-5   4.2e-5   1.8e-4   44.3       2.7e-6   0.079
    184x328  grey             1.2e-5    4.8e-5   2.5e-5   6.5e-5   5.2e-5   1.3e-4   33.2       1.2e-6   0.001    <- RELATIVE_CAP
    184x328  lowcontrast      1.2e-5    4.4e-5   1.7e-5   2.5e-5   2.4e-5   1.0e-4   4.4        7.6e-7   0.001
    184x328  sky_road         1.3e-5    4.9e-5   5.0e-6   1.7e-5   1.6e-5   1.0e-4   21.2       3.1e-6   0.032
    376x1232 sky_road         5.6e-5    1.8e-4   6.6e-6   2.5e-5   6.8e-5   2.3e-4   58.1       3.8e-6   0.033
    376x1232 black            4.7e-5    1.9e-4   8.3e-6   6.0e-5   9.7e-5   3.3e-4   81.8       3.4e-6   0.037

Nearest to half a cap outside the list: 184x328 grey pyr0 at 0.49 of its cap (listed anyway: lookup0 of the same case moved
between 5.2e-5 and 5.8e-5 over two hosts) and lookup0 0.39, then 184x328 black lookup0 0.36, grey pyr1 0.35 (3.5e-5 of 1e-4), 376x1232
black lookup0 0.30 and sky_road flow_low 0.28; everything else is below a quarter. As tests/test_flow_limits_oracle.py notes, the
figures move by tens of per cent with the host's thread count. `pytest -s` prints every figure ("YARDSTICK" and "CONTENT" lines).

Why grey is the hard one: 128 is the one level whose normalised value 2 * (128 / 255) - 1 = 2^-8 cancels almost completely; the
half-ulp rounding of the intermediate 0.50196 leaves the fp32 value 1.51e-5 (relative) off, where 127 or 120 are at 6e-8. With eps
as the variance, fnet's first norm is linear in that value, so the whole feature map of the fp32 oracle is 1.5e-5 off, relatively:
the fp64 oracle run on the frame level that the fp32 one effectively sees differs from grey by 1.9e-5 (fmap), 7.8e-5 / 4.6e-5 /
2.8e-5 / 1.5e-5 (pyr0..3) at 184x328 - the fp32 oracle's whole error (2.5e-5; 6.5e-5 / 3.5e-5 / 2.7e-5 / 1.5e-5).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_content_cases as cc  # noqa: E402
import parity_check  # noqa: E402
import test_gpu_flow_geometry as fg  # noqa: E402   (helpers and constants only: its tests stay in its own module)

ORACLED = cc.oracled()
IDS = ["%dx%d-%s" % (hw[0], hw[1], c) for hw, c in ORACLED]


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return fg._sd()


@pytest.fixture(scope="module")
def oracle(sd):
    """(geometry, content) -> (frames, fp32 oracle, fp64 oracle), each computed once per module."""
    cache = {}

    def get(hw, content):
        if (hw, content) not in cache:
            frames = torch.from_numpy(cc.make_pair(content, hw))
            rows = fg._rows((hw[0] // 8) * (hw[1] // 8))
            cache[(hw, content)] = (frames,) + tuple(fg._oracle_pair(sd, frames, 0, dt, rows, False) for dt in (torch.float32, torch.float64))
        return cache[(hw, content)]
    return get


def test_the_constants_are_those_of_the_modules_they_come_from():
    assert (cc.TOL_LOW, cc.TOL_UP, cc.TOL_ACT) == (fg.TOL_LOW, fg.TOL_UP, fg.TOL_ACT) and cc.REL_CAP == parity_check.CAP
    assert (fg.M, fg.FLOOR) == (9.0, 1e-6) and cc.SEED_FRAMES == fg.SEED_FRAMES
    assert set(cc.MODES) == {(c[2], c[3]) for c in fg.CASES}
    for name, hw, contents, pos, modes, rev in cc.MIXED:
        assert max(pos) < len(contents) and set(modes) <= set(cc.MODES)
        if rev:    # every position is oracled, so the reversed launch is too
            assert pos == tuple(range(len(contents)))


@pytest.mark.parametrize("case", ORACLED, ids=IDS)
def test_the_fp64_oracle_is_finite(oracle, case):
    _, o32, o64 = oracle(*case)
    for k in sorted(o64):
        assert bool(torch.isfinite(o64[k]).all()) and bool(torch.isfinite(o32[k]).all()), k


def _stem(sd, frames, net):
    """fp64 output of the stem convolution (7x7, stride 2) of `net` on both frames, and its interior: the outputs whose window
    touches no zero padding, rows / columns 2 .. (size - 4) // 2."""
    im = 2 * (frames.double() / 255.0) - 1.0
    y = F.conv2d(im, sd[net + "conv1.weight"].double(), sd[net + "conv1.bias"].double(), stride=2, padding=3)
    H, W = frames.shape[2:]
    return y, y[:, :, 2:(H - 4) // 2 + 1, 2:(W - 4) // 2 + 1]


def _rstd1(y):
    return 1.0 / torch.sqrt(y.var(dim=(2, 3), unbiased=False) + 1e-5)


FLAT_RSTD = 30.0


@pytest.mark.parametrize("case", ORACLED, ids=IDS)
def test_the_contents_are_what_they_claim(sd, oracle, case):
    hw, content = case
    frames, _, o64 = oracle(hw, content)
    y, inner = _stem(sd, frames, "fnet.")
    rstd = _rstd1(y)
    var_in = float(inner.var(dim=(2, 3), unbiased=False).max())
    print("CONTENT %dx%d %s stem interior var %.3e, whole-map var %.3e .. %.3e, rstd of fnet.norm1 max %.1f, max|pyr0| %.1f, attn max %.2e"
          % (hw[0], hw[1], content, var_in, float(y.var(dim=(2, 3), unbiased=False).min()), float(y.var(dim=(2, 3), unbiased=False).max()),
             float(rstd.max()), float(o64["pyr0"].abs().max()), float(o64["attn"].max())))
    if content in cc.CONSTANTS or content in cc.BORDER_ONLY:
        # the stem's output is one value per channel wherever the window is whole; only the border varies
        assert var_in == 0.0
        assert float(y.var(dim=(2, 3), unbiased=False).min()) > 0.0
        assert float(rstd.max()) > 10.0
    if content in cc.CONSTANTS:
        for net in ("cnet.",):
            assert float(_stem(sd, frames, net)[1].var(dim=(2, 3), unbiased=False).max()) == 0.0
        # near-uniform attention away from the border features
        H8, W8 = hw[0] // 8, hw[1] // 8
        keep = torch.zeros(H8, W8, dtype=torch.bool)
        keep[cc.BORDER:H8 - cc.BORDER, cc.BORDER:W8 - cc.BORDER] = True
        keep = keep.flatten()
        rows = fg._rows(H8 * W8)
        a = o64["attn"][keep[rows]][:, keep]
        ratio = float((a.max(dim=1).values / a.min(dim=1).values).max())
        full = float((o64["attn"].max(dim=1).values / o64["attn"].min(dim=1).values).max())
        print("CONTENT %dx%d %s attention row max/min: interior %.3f, all features %.3f" % (hw[0], hw[1], content, ratio, full))
        assert ratio < 2.0
        if content == "grey":
            assert full < 2.0
    if content in cc.FLAT:
        assert float(rstd.max()) > FLAT_RSTD
    if content == "identical":
        assert torch.equal(o64["fmap1"], o64["fmap2"])


@pytest.mark.parametrize("case", ORACLED, ids=IDS)
def test_fp32_oracle_is_within_half_of_every_cap(oracle, case):
    """Every tensor the GPU cases compare (fg._oracle_pair's dictionary). A (case, tensor) outside half of its absolute cap must
    be listed in cc.RELATIVE_CAP, where REL_CAP * max|x64| takes the cap's place."""
    hw, content = case
    _, o32, o64 = oracle(hw, content)
    bad = []
    for k in sorted(o64):
        e = float((o32[k].double() - o64[k].double()).abs().max())
        scale = float(o64[k].double().abs().max())
        tol = cc.absolute_cap(k, scale)
        listed = (hw, content, cc.tensor_key(k)) in cc.RELATIVE_CAP
        print("YARDSTICK %dx%d/%s %s err_32=%.3e max64=%.3e cap=%.2e%s" % (hw[0], hw[1], content, k, e, scale, tol,
                                                                          " RELATIVE_CAP %.2e" % (cc.REL_CAP * scale) if listed else ""))
        if listed:
            assert cc.cap(hw, content, k, scale) == cc.REL_CAP * scale
            if not e <= 0.5 * cc.REL_CAP * scale:
                bad.append("%s (listed): %.3e > %.2e / 2" % (k, e, cc.REL_CAP * scale))
        else:
            assert cc.cap(hw, content, k, scale) == tol
            if not e <= 0.5 * tol:
                bad.append("%s: %.3e > %.2e / 2" % (k, e, tol))
    assert not bad, "%dx%d/%s: %s" % (hw[0], hw[1], content, "; ".join(bad))


def test_the_exception_list_is_grey_correlations_only():
    never = ("flow_low", "flow_up", "fmap1", "fmap2", "inp", "net1", "mask1", "mf0", "mfg0", "cor1", "attn")
    assert len(set(cc.RELATIVE_CAP)) == len(cc.RELATIVE_CAP)
    for hw, content, key in cc.RELATIVE_CAP:
        assert key in cc.CORR_KEYS and key not in never
        assert content == "grey" and (hw, content) in ORACLED
    # a launch is held to the list through its positions: a listed tensor belongs to a pair that IS grey
    for _, hw, contents, pos, _, _ in cc.MIXED:
        for p in pos:
            for k in cc.CORR_KEYS:
                if (hw, contents[p], k) in cc.RELATIVE_CAP:
                    assert contents[p] == "grey"
