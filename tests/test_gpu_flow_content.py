"""GMA flow network against the fp64 oracle on flat, saturated and mixed-content frames: the image CONTENT no other test feeds it.

Every other parity test uses synthetic.make_frames (one well-textured canvas), and every launch with B > 1 takes consecutive frames
of one sequence. Here (tests/flow_content_cases.py; tests/test_flow_content_oracle.py shows on the CPU that the cases are what they
claim and that the fp32 oracle is within half of every cap): constant 0 / 255 / 128 frames, 128 +- 1, a texture compressed to
+- 4 levels, a frame against itself, half-saturated and part-black frames, a pixel-pitch checker, a lone moving pixel, a sky / texture
/ road frame - a channel whose variance is small against its mean through the InstanceNorm chain (the stem's M2 partials, the
statistics epilogues, the two-level fp64 merge with its clamped between-group term, the normalise-on-load loaders, in_apply_sf_kernel;
rstd up to 315), near-uniform attention rows, correlation rows of near-identical entries and correlations up to 82 - and launches
whose pairs are unlike each other, where per-image statistics that leaked between images would show.

Yardstick, Checker and _check_taps are those of tests/test_gpu_flow_geometry.py (M = 9, FLOOR = 1e-6, flow_low 2e-4 px, flow_up 1e-3
px, activations 1e-4, attention 1e-6 + 1e-4 * max), with one derived cap: pyr0..3 and lookup0 get 1e-4 * max(1, max|x64| / 25) (the
suite's 1e-4 was stated for correlations of O(1) - O(25)); and pyr0 / lookup0 of `grey` are held to the same M-bound under
1e-3 * max|x64| (cc.RELATIVE_CAP: the fp32 oracle itself is not within half of the absolute cap there).

Tests. `test_flow_stages_on_flat_and_saturated_frames`: every tap after one iteration, flow after one and twelve, sf_clamped == 0;
all twelve contents at 128x128 (black, grey, lowcontrast, sky_road also in f32 and low-latency), five at 184x328 (partial 32-row
statistics groups), sky_road at 376x1232. `test_a_pair_does_not_depend_on_its_neighbours`: [black, textured, white] and [grey,
sky_road, lowcontrast] at 128x128, forward and reversed, [white, sky_road, black] at 184x328, all in split-f16, f32 and low-latency;
sky_road / black / sky_road at positions 0 / 7 / 15 of a B = 16 launch at 376x1232 (split-f16, f32). The oracled positions meet the
yardstick, and every position is torch.equal in fmap, x, net, mask, flow_low and flow_up after twelve iterations to the same position
of a launch of B copies of its own pair on the same handle. `test_sequence_modes_through_a_flat_frame`: a clip, a continued clip and
forward_consecutive on the low-latency handle over [textured, black, textured, lowcontrast, textured] give pair mode's bits.

Measured on the MI355X (39 tests, 1355 comparisons, all pass). Every neighbour, reversal and sequence comparison is bit-equal in all
modes: no kernel is exempt.

The defect these frames found. On the first run 184x328-grey-split_f16 exceeded the absolute cap on pyr1 (1.553e-4 of 1e-4) and pyr2
(1.142e-4), with fmap at 6.5e-5, pyr0 3.10e-4, lookup0 3.08e-4 (need_m 4.7); the exact-fp32 mode on the same frames had pyr1 1.200e-4.
Not statistics indexing (per-channel mean of fmap's error 2.3e-6 against 6.5e-5 of per-pixel residual; mixed launches bit-equal),
not the input (the img4 tap equals the fp32 oracle's value bit for bit and its split hi + lo is exact). Projected on the fp64
oracle's response to the input level, fmap's error was an effective relative input error of 1.57e-5 (fp32 oracle), 1.63e-5 (f32 mode),
2.3e-5 (split-f16) - the shared rounding of 2 * (128 / 255) - 1 - plus a residual of 1.6e-5 / 4.2e-5 / 6.4e-5: an excess in both
independent modes. Cause: the per-group sum of the InstanceNorm statistics (stem_sf.hip, MODE_RAW_STATS epilogue; conv_mfma.h, kStats
epilogue) was a running fp32 sum. On a constant frame a group's 32 values are one DC level v (up to 0.1, the bias), the partial sums
k * v round at every step and round THE SAME WAY in every group of the image, so the error does not average out: the channel mean
ends up about 4 ulp off where the border deviations that carry all the variance are 1e-3 (variance 6e-8 to 4e-6 against eps 1e-5),
and rstd = 315 multiplies it. The reference accumulates its statistics in double. Fix: the group is summed in fp64 and rounded once.
After it, 184x328 grey split-f16: fmap 2.4e-5 (fp32 oracle 2.5e-5), pyr0..3 1.03e-4 / 6.4e-5 / 4.0e-5 / 2.1e-5, lookup0 9.5e-5
(need_m at most 1.17); 128x128 grey: pyr0 3.9e-5 split-f16 and 4.3e-5 f32 where they were 1.47e-4 and 1.11e-4 (fp32 oracle 5.4e-5).

The two-pass encoder plumbing (cc.TWO_PASS, precision "split_f16_two_pass": the f16 mode's op sequence in split-f16 arithmetic —
stem_sf_kernel<1> / <2> and the separate in_apply_sf_kernel passes, which no flat frame had ever reached). Cases: black, grey,
lowcontrast, sky_road at 128x128; grey, lowcontrast, sky_road at 184x328; the three B = 3 launches (both orders at 128x128); the clip
and the continued clip of the sequence test. 10 more parametrisations, 396 comparisons, every neighbour / reversal / sequence
comparison bit-equal. stem_sf_kernel<1> still had the running fp32 group sum described above. With it every case passed, but grey stood
at twice the one-pass path's error and against the cap: 184x328 fmap 5.0e-5, pyr0..3 1.62e-4 / 9.90e-5 (cap 1e-4) / 4.6e-5 / 2.4e-5,
lookup0 1.63e-4 (need_m 2.24); 128x128 fmap 4.0e-5, pyr0 9.4e-5. With the group summed in fp64 and rounded once (the same fix): 184x328
fmap 2.4e-5, pyr0..3 1.15e-4 / 6.6e-5 / 4.2e-5 / 2.1e-5, lookup0 1.07e-4 (need_m 1.27); 128x128 fmap 2.5e-5, pyr0 3.9e-5 — the one-pass
path's figures. Worst need_m after the fix: 128x128 black 1.42 (net1), grey 2.23 (attn), lowcontrast 2.10 (attn), sky_road 0.94 (net1);
184x328 grey 1.81 (attn), lowcontrast 2.44 (attn), sky_road 2.24 (net1); [black, textured, white] 1.55 (attn, textured), [grey, sky_road,
lowcontrast] 2.23 (attn, grey), both orders alike; [white, sky_road, black] 2.24 (net1, sky_road). Closest to a cap: 184x328 grey pyr1,
6.6e-5 of 1e-4.

Worst need_m = (max|x_hip - x64| - FLOOR * max|x64|) / max|x32 - x64| per case (PARITY-WORST lines):
    128x128 split-f16   black 1.53 (mfg0)   white 1.26 (net1)   grey 2.23 (attn)   lowcontrast 2.10 (attn)   faint 1.59 (attn)
                        identical 1.55 (attn)   half_saturated 1.48 (net1)   top_black 1.49 (net1)   checker 1.34 (net1)
                        impulse 1.45 (net1)   sky_road 0.94 (net1)   textured 1.55 (attn)
    128x128 f32         black 2.36 (net1)   grey 0.67 (flow_low@1)   lowcontrast 1.05 (fmap2)   sky_road 1.55 (flow_low@1)
    128x128 low-latency black 1.53 (mfg0)   grey 2.23 (attn)   lowcontrast 2.10 (attn)   sky_road 0.94 (net1)
    184x328 split-f16   black 1.44 (net1)   white 1.25 (net1)   grey 1.81 (attn)   lowcontrast 2.44 (attn)   sky_road 2.26 (net1)
    184x328 f32         sky_road 2.73 (attn)          376x1232 split-f16   sky_road 1.74 (net1)
    [black, textured, white] B = 3, forward and reversed alike: split-f16 1.55 (attn, textured)   f32 2.46 (net1, white)
                        low-latency 1.55 (attn, textured)
    [grey, sky_road, lowcontrast] B = 3, both orders: split-f16 2.23 (attn, grey)   f32 1.55 (flow_low@1, sky_road)   low-latency 2.23
    [white, sky_road, black] 184x328 B = 3: split-f16 2.26 (net1, sky_road)   f32 2.73 (attn, sky_road)   low-latency 2.28 (net1)
    376x1232 B = 16: split-f16 1.74 (net1, sky_road at 0)   f32 5.14 (mfg0, sky_road at 0: 2.8e-5 of the 1e-4 cap where the fp32
                        oracle is at 4.6e-6; the suite's largest, the geometry file's worst is 2.36)
Closest to a cap: 184x328 grey pyr1 6.4e-5 of 1e-4 and lookup0 9.5e-5 of 1.33e-4 (the fp32 oracle there: 3.4e-5 and 5.8e-5). The flat
contents need no more than the textured ones; the largest flat figures are attention rows whose largest weight is 1.15 x uniform
(2.1 to 2.4). `pytest -s` prints every comparison.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_content_cases as cc  # noqa: E402
import test_gpu_flow_geometry as fg  # noqa: E402
from test_gpu_flow_geometry import sd  # noqa: E402,F401   (module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = fg.DEV
ITERS = fg.ITERS


@pytest.fixture(scope="module")
def oracle(sd):
    """(geometry, content) -> (fp32 oracle, fp64 oracle) of the content's pair, each computed once per module."""
    cache = {}

    def get(hw, content):
        if (hw, content) not in cache:
            frames = torch.from_numpy(cc.make_pair(content, hw))
            rows = fg._rows((hw[0] // 8) * (hw[1] // 8))
            cache[(hw, content)] = tuple(fg._oracle_pair(sd, frames, 0, dt, rows, False) for dt in (torch.float32, torch.float64))
        return cache[(hw, content)]
    return get


def _to_dev(pairs):
    """[pair [2,3,H,W], ...] -> (image1 [B,3,H,W], image2 [B,3,H,W]) on the device."""
    return (torch.from_numpy(np.stack([p[0] for p in pairs])).to(DEV), torch.from_numpy(np.stack([p[1] for p in pairs])).to(DEV))


def _compare(chk, net, oracle, hw, names, pos, f1, f2):
    """The comparisons of test_gpu_flow_geometry._run_case for the positions `pos` of one launch whose position p holds the
    pair named names[p]: every tap after one iteration, flow_low / flow_up after one and after twelve. Returns the twelve-iteration
    (flow_low, flow_up)."""
    B = len(names)
    rows = fg._rows((hw[0] // 8) * (hw[1] // 8))
    res = {p: oracle(hw, names[p]) for p in pos}

    def cap(p, key, x64, tol):
        return cc.cap(hw, names[p], key, float(x64.double().abs().max()))
    low1, up1 = net(f1, f2, iters=1, test_mode=True)
    torch.cuda.synchronize()
    fg._check_taps(chk, net, hw, B, pos, rows, res, cap=cap)
    for p in pos:
        chk("p%d/flow_low@1" % p, low1[p], res[p][0]["low1"], res[p][1]["low1"], cc.TOL_LOW)
        chk("p%d/flow_up@1" % p, up1[p], res[p][0]["up1"], res[p][1]["up1"], cc.TOL_UP)
    low, up = net(f1, f2, iters=ITERS, test_mode=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(up).all()), chk.case
    for p in pos:
        chk("p%d/flow_low" % p, low[p], res[p][0]["flow_low"], res[p][1]["flow_low"], cc.TOL_LOW)
        chk("p%d/flow_up" % p, up[p], res[p][0]["flow_up"], res[p][1]["flow_up"], cc.TOL_UP)
    return low, up


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("case", cc.CASES, ids=[cc.case_id(c) for c in cc.CASES])
def test_flow_stages_on_flat_and_saturated_frames(sd, oracle, case):
    """Every stage tap after one iteration and the flow after one and twelve, one pair of each content per launch."""
    hw, content, precision, ll = case
    tag = "%dx%d/%s/%s%s" % (hw[0], hw[1], content, precision, "/ll" if ll else "")
    net = fg._net(sd, 1, precision, ll)
    chk = fg.Checker(tag)
    f1, f2 = _to_dev([cc.make_pair(content, hw)])
    _compare(chk, net, oracle, hw, (content,), (0,), f1, f2)
    clamped = fg._sf_clamped(net, hw)
    del net
    torch.cuda.empty_cache()
    assert clamped == 0.0, tag
    chk.finish()


STATE = (("fmap", 256), ("x", 384), ("net", 128), ("mask", 576))


def _state(net, hw, B, low, up):
    """What a launch left behind after its twelfth iteration, per position: fmap [2, B, N, 256] (both images' features), the GRU
    input x (context | motion features | aggregate) [B, N, 384], the hidden state [B, N, 128], the mask [B, N, 576], the flows."""
    H, W = hw
    N = (H // 8) * (W // 8)
    s = {"fmap": net.debug_read("fmap", (2, B, N, 256), H, W).transpose(0, 1)}
    for k, c in STATE[1:]:
        s[k] = net.debug_read(k, (B, N, c), H, W)
    s["flow_low"], s["flow_up"] = low.cpu(), up.cpu()
    return s


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("case", cc.MIXED_CASES, ids=[cc.mixed_id(c) for c in cc.MIXED_CASES])
def test_a_pair_does_not_depend_on_its_neighbours(sd, oracle, case):
    """Unlike pairs side by side in one launch (a black pair between a textured and a white one). The oracled positions meet the
    fp64 yardstick; and EVERY position p is bit-identical, in its feature maps, GRU input, hidden state, mask and flows after
    twelve iterations, to position p of a launch of the same B (same handle: the same kernels and tiles) whose B positions all
    hold pair p, so that the neighbours are the only difference. The reversed launch is compared in the same two ways and, position
    for position, with the forward one. No kernel of the network reduces across images, so nothing is exempt from bit-equality."""
    (name, hw, names, pos, _, reverse), precision, ll = case
    B = len(names)
    tag = "%s/B%d/%s%s" % (name, B, precision, "/ll" if ll else "")
    net = fg._net(sd, B, precision, ll)
    pairs = [cc.mixed_pair(n, hw) for n in names]
    chks, states = [], []
    for rev in ((False, True) if reverse else (False,)):
        order = list(range(B))[::-1] if rev else list(range(B))
        chk = fg.Checker(tag + ("/reversed" if rev else ""))
        f1, f2 = _to_dev([pairs[i] for i in order])
        low, up = _compare(chk, net, oracle, hw, [names[i] for i in order], [order.index(p) for p in pos], f1, f2)
        states.append((order, _state(net, hw, B, low, up)))
        chks.append(chk)
    differ = []
    for i in range(B):                                     # the launch in which every position holds pair i
        f1, f2 = _to_dev([pairs[i]] * B)
        low, up = net(f1, f2, iters=ITERS, test_mode=True)
        torch.cuda.synchronize()
        alone = _state(net, hw, B, low, up)
        for order, mixed in states:
            p = order.index(i)
            differ += ["%s position %d (%s) %s" % ("reversed" if order[0] else "forward", p, names[i], k)
                       for k in alone if not torch.equal(mixed[k][p], alone[k][p])]
        del alone
    if reverse:
        (_, fwd), (_, bwd) = states
        differ += ["forward position %d / reversed position %d: %s" % (p, B - 1 - p, k)
                   for p in range(B) for k in fwd if not torch.equal(fwd[k][p], bwd[k][B - 1 - p])]
    clamped = fg._sf_clamped(net, hw)
    del net, states
    torch.cuda.empty_cache()
    assert not differ, "%s: not bit-identical to the launch without neighbours:\n  " % tag + "\n  ".join(differ)
    assert clamped == 0.0, tag
    for chk in chks:
        chk.finish()


@pytest.mark.timeout(1200)
def test_sequence_modes_through_a_flat_frame(sd):
    """tests/test_gpu_round3.py::test_clip_modes_are_bit_identical_to_pair_mode, for a clip that passes through a black and a
    low-contrast frame: each shared frame's feature maps and statistics slot serve the pair before and the pair after it. A clip
    on the default handle, and the same frames one per call through forward_consecutive on the low-latency handle, give the bits
    of pair mode on the same handle. The clip and the continued clip also on the two-pass encoder plumbing (cc.TWO_PASS): there
    run_encoder_sf takes first_img and the clip's private buffers through the stem's two passes and the in_apply_sf passes."""
    hw = cc.SMALL
    fr = torch.from_numpy(cc.sequence_frames(hw)).to(DEV)
    for precision in ("split_f16", cc.TWO_PASS[0]):
        net = fg._net(sd, 4, precision, False)
        low_p, up_p = net(fr[0:4], fr[1:5], iters=ITERS, test_mode=True)
        low_s, up_s = net.forward_sequence(fr, iters=ITERS)
        assert torch.equal(low_s, low_p) and torch.equal(up_s, up_p), precision
        net.forward_sequence(fr[0:2], iters=ITERS)                                  # a clip that ends on the black frame ...
        low_c, up_c = net.forward_sequence(fr[1:5], iters=ITERS, continued=True)    # ... continued from it
        assert torch.equal(low_c, low_p[1:4]) and torch.equal(up_c, up_p[1:4]), precision
        assert bool(torch.isfinite(up_p).all()), precision
        assert fg._sf_clamped(net, hw) == 0.0, precision
        del net
    ll = fg._net(sd, 1, "split_f16", True)
    frames = [fr[t].clone() for t in range(5)]
    chain = [ll.forward_consecutive(frames[t], frames[t + 1], iters=ITERS) for t in range(4)]
    for t in range(4):
        low_1, up_1 = ll(frames[t][None], frames[t + 1][None], iters=ITERS, test_mode=True)
        assert torch.equal(chain[t][0], low_1) and torch.equal(chain[t][1], up_1), t
    assert fg._sf_clamped(ll, hw) == 0.0
    del ll
    torch.cuda.empty_cache()
