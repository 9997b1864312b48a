"""The feature head folded into the correlation (weights.h: pack_fnet_head_folded): the split-f16 / f16 paths
correlate the source frame's folded head output (128 -> 129 channels, padded to 160) with the target's pre-head features + one
constant channel instead of two 256-channel head outputs. `-m gpu`, through the module.

Shapes: 136x200 (17x25 at 1/8: odd at every pyramid level, N = 425 is no multiple of the 128-pixel strip, the last brick column
and row are partial at every level) and 128x160 (the smallest frame the network accepts). Two pairs on a handle built for three.
Checkpoints: the synthetic one, and the same with fnet.conv2.bias x 32, so that the constant channel carries real weight
(b . b / 16 grows from 0.003 to 3.4 of a |corr| <= 20).

Figures of the parent commit's library that this file compares against were measured with that library on the same inputs (one
MI355X, profiles/corr_fold_ab.txt); they are constants here because a checkout holds one library."""
import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import RAFTGMA
from oracle import gma_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(136, 200), (128, 160)]
STATES = ["base", "bias32"]
B, MAXB = 2, 3

# max |pyr_l - fp64| over the four levels of the PARENT commit's split-f16 handle, same inputs: {(state, H, W): error}
PARENT_PYR_ERR = {
    ("base", 136, 200): 9.167e-06, ("base", 128, 160): 1.027e-05, ("bias32", 136, 200): 1.012e-05, ("bias32", 128, 160): 1.045e-05,
}
# sf_clamped of the PARENT commit's library after one forward with fnet.conv2 x 64: {(H, W): count}
PARENT_CLAMPED_X64 = {(136, 200): 2, (128, 160): 0}


def _state(which, conv2_mul=1.0):
    sd = syn.make_gma_state(seed=1)
    if which == "bias32":
        sd["fnet.conv2.bias"] = (sd["fnet.conv2.bias"] * 32).astype(np.float32)
    for k in ("fnet.conv2.weight", "fnet.conv2.bias"):
        sd[k] = (sd[k] * conv2_mul).astype(np.float32)
    return syn.to_torch(sd)


def _frames(n, H, W):
    return torch.from_numpy(syn.make_frames(n, H, W, seed=7))


def _net(sd, precision):
    net = RAFTGMA(max_batch=MAXB, precision=precision)
    net.load_state_dict(sd)
    return net.to(DEV).eval()


_ORACLE = {}


def _oracle(which, H, W):
    """fp64 feature maps of frames 0..4 and the pyramid of the pairs (0, 1), (1, 2): computed once, never modified."""
    key = (which, H, W)
    if key not in _ORACLE:
        sd = {k: v.double() for k, v in _state(which).items()}
        x = 2 * (_frames(5, H, W).double() / 255.0) - 1
        with torch.no_grad():
            fm = gma_ref.encoder(x, sd, "fnet.", "instance")
            pyr = gma_ref.corr_pyramid(fm[0:2], fm[1:3])
        _ORACLE[key] = (fm, pyr)
    return _ORACLE[key]


def pyr_errors(which, H, W, precision):
    """max |pyr_l tap - fp64| per level after a forward of the pairs (0, 1), (1, 2)."""
    n = (H // 8) * (W // 8)
    net = _net(_state(which), precision)
    fr = _frames(5, H, W).to(DEV)
    net(fr[0:2], fr[1:3], iters=1, test_mode=True)
    _, ref = _oracle(which, H, W)
    errs = []
    for l in range(4):
        hw = (H // 8 >> l) * (W // 8 >> l)
        got = net.debug_read("pyr%d" % l, (B * n, hw), H, W)
        errs.append(float((got.double() - ref[l].reshape(B * n, hw)).abs().max()))
    return errs


def clamped_after_forward(H, W, conv2_mul):
    """The device's saturation counter after one forward (2 pairs, 2 iterations) with fnet.conv2 x conv2_mul."""
    fr = _frames(3, H, W).to(DEV)
    drain = _net(_state("base"), "split_f16")    # the counter is one per device: whatever an earlier test left in it is read
    drain._sat_pending = False                   # (and published) here, before the module under test has a handle
    drain(fr[0:1], fr[1:2], iters=1, test_mode=True)
    drain.check_saturation(raise_on_clamp=False)
    net = _net(_state("base", conv2_mul), "split_f16")
    net._sat_pending = False                     # no automatic check (it would raise): the count is read below
    net(fr[0:2], fr[1:3], iters=2, test_mode=True)
    return net.check_saturation(raise_on_clamp=False)


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("H,W", SHAPES)
def test_pyramid_taps_against_fp64(which, H, W):
    """Bound: the 1e-4 that tests/test_gpu_parity.py applies to the same taps, for the split-f16 and the exact-fp32 handle; and
    the folded form stays within 2x the parent library's error (the 22-bit operand emulation saw 1.6x: more is a bug).
    Measured, max over the levels, split-f16 new / parent / f32 handle: see profiles/corr_fold_ab.txt."""
    e_sf = pyr_errors(which, H, W, "split_f16")
    e_32 = pyr_errors(which, H, W, "f32")
    parent = PARENT_PYR_ERR[(which, H, W)]
    print("%s %dx%d: pyr0..3 max error split_f16 %s | f32 %s | parent split_f16 (max) %s"
          % (which, H, W, ["%.2e" % e for e in e_sf], ["%.2e" % e for e in e_32], parent))
    assert max(e_sf) < 1e-4 and max(e_32) < 1e-4
    assert max(e_sf) <= 2 * parent


@pytest.mark.parametrize("H,W", SHAPES)
def test_samples_outside_the_map_are_exactly_zero(H, W):
    """bias x 32 and integer flow_init in +-(W8 + 40): windows leave the map on every side, wholly and in part, at every level.
    A sample (corr.py:32-53: level l, x = cx / 2^l + d_i, y = cy / 2^l + d_j, channel 81 l + 9 i + j) has no cell of the map
    among its four neighbours iff x <= -1 or x >= W_l or y <= -1 or y >= H_l; grid_sample's zero padding makes it exactly 0.
    (Positions exactly ON those four bounds are left out: the reference maps a position through normalised coordinates and
    back, utils.py:63-66, and the lookup kernel reproduces that rounding: x = W_l can come back as W_l - 1 ulp, a weight of
    1e-7 on the last cell, in the reference as here. Every other position is at least 1/8 cell away from a bound.)
    The lookup reads the padding cells of the bricked levels (cells past H_l / W_l inside the last brick row / column) like
    any other cell, so this is also the check that those cells hold exact zeros: their constant channel is 0 with the rest of
    the row. Positions are exact in fp32 (integers / 2^l)."""
    h8, w8 = H // 8, W // 8
    n = h8 * w8
    r = np.random.RandomState(11)
    fi = np.stack([r.randint(-(w8 + 40), w8 + 41, (B, h8, w8)), r.randint(-(h8 + 40), h8 + 41, (B, h8, w8))], 1).astype(np.float32)
    net = _net(_state("bias32"), "split_f16")
    fr = _frames(3, H, W).to(DEV)
    net(fr[0:2], fr[1:3], iters=1, flow_init=torch.from_numpy(fi).to(DEV), test_mode=True)
    got = net.debug_read("corrfeat", (B * n, 352), H, W)[:, :324].reshape(B, h8, w8, 4, 9, 9)
    ys, xs = np.meshgrid(np.arange(h8), np.arange(w8), indexing="ij")
    cx, cy = xs[None] + fi[:, 0], ys[None] + fi[:, 1]
    d = np.arange(-4, 5, dtype=np.float64)
    whole = part = 0
    for l in range(4):
        hl, wl = h8 >> l, w8 >> l
        sx = (cx / 2 ** l)[..., None, None] + d[None, None, None, :, None]
        sy = (cy / 2 ** l)[..., None, None] + d[None, None, None, None, :]
        out = torch.from_numpy((sx < -1) | (sx > wl) | (sy < -1) | (sy > hl))
        inside = torch.from_numpy((sx > -1) & (sx < wl) & (sy > -1) & (sy < hl))
        g = got[:, :, :, l]
        assert bool((g[out] == 0).all()), (l, float(g[out].abs().max()))
        assert float(g[inside].abs().max()) > 1.0                    # ... and the rest carries the correlation
        allout = out.reshape(B, h8, w8, 81).all(-1)
        whole += int(allout.sum())
        part += int((out.reshape(B, h8, w8, 81).any(-1) & ~allout).sum())
    assert whole > 100 and part > 100, (whole, part)


def test_fmap_tap_keeps_its_meaning_in_every_mode():
    """debug_read("fmap") = W f + b, [slot][N][256], rebuilt on the debug path: within 3e-5 x max of the exact-fp32 handle's tap
    (the bound of tests/test_gpu_round2.py) in pair mode, clip mode and a continued clip (whose slot 0 is the carried frame)."""
    H, W = 136, 200
    n = (H // 8) * (W // 8)
    fr = _frames(5, H, W).to(DEV)
    sd = _state("bias32")
    new, old = _net(sd, "split_f16"), _net(sd, "f32")

    def taps(frames_of_slots):
        a = new.debug_read("fmap", (2 * MAXB, n, 256), H, W)
        b = old.debug_read("fmap", (2 * MAXB, n, 256), H, W)
        return a[:len(frames_of_slots)], b[frames_of_slots]

    old(fr[0:2], fr[1:3], iters=1, test_mode=True)                 # f32 slots: frames 0, 1 | 1, 2
    new(fr[0:2], fr[1:3], iters=1, test_mode=True)                 # pair mode: the same slots
    a, b = taps([0, 1, 2, 3])
    tol = 3e-5 * max(1.0, float(b.abs().max()))
    assert float(b.abs().max()) > 0.1 and float((a - b).abs().max()) < tol
    new.forward_sequence(fr[0:3], iters=1)                         # clip: slots = frames 0, 1, 2
    a, b = taps([0, 1, 3])
    assert float((a - b).abs().max()) < tol
    old(fr[2:4], fr[3:5], iters=1, test_mode=True)                 # f32 slots: frames 2, 3 | 3, 4
    new.forward_sequence(fr[2:5], iters=1, continued=True)         # continued clip: slots = frames 2 (carried), 3, 4
    a, b = taps([0, 1, 3])
    assert float(b.abs().max()) > 0.1 and float((a - b).abs().max()) < 3e-5 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("H,W", SHAPES)
def test_modes_agree_bit_for_bit(H, W):
    """A clip, continued clips (one of them after a clip of another length: the carried frame's row feeds both the head and
    the target side) and the same pairs in pair mode give the same bits."""
    net = _net(_state("bias32"), "split_f16")
    fr = _frames(5, H, W).to(DEV)
    low_p, up_p = net(fr[0:3], fr[1:4], iters=2, test_mode=True)                  # pair mode, 3 pairs
    low_s, up_s = net.forward_sequence(fr[0:4], iters=2)                          # one clip
    assert torch.equal(up_s, up_p) and torch.equal(low_s, low_p)
    net.forward_sequence(fr[0:2], iters=2)                                        # clip of one pair ...
    low_c, up_c = net.forward_sequence(fr[1:4], iters=2, continued=True)          # ... continued by a clip of two
    assert torch.equal(up_c, up_p[1:3]) and torch.equal(low_c, low_p[1:3])
    low_d, up_d = net.forward_sequence(fr[3:5], iters=2, continued=True)          # ... continued by a clip of one
    low_1, up_1 = net(fr[3:4], fr[4:5], iters=2, test_mode=True)
    assert torch.equal(up_d, up_1) and torch.equal(low_d, low_1)
    for b in range(3):                                                            # single pairs
        _, up_b = net(fr[b:b + 1], fr[b + 1:b + 2], iters=2, test_mode=True)
        assert torch.equal(up_b, up_p[b:b + 1]), b


@pytest.mark.parametrize("H,W", SHAPES)
def test_scaled_head_clamps_no_more_than_before(H, W):
    """fnet.conv2 x 64 (|corr| x 4096): the folded layer's power-of-two scale follows W, so nothing is clamped that the
    unfolded path did not clamp: the saturation counter after a forward equals the parent library's on the same inputs."""
    got = clamped_after_forward(H, W, 64.0)
    print("%dx%d, fnet.conv2 x 64: sf_clamped %d, parent library %s" % (H, W, got, PARENT_CLAMPED_X64[(H, W)]))
    assert got == PARENT_CLAMPED_X64[(H, W)]
