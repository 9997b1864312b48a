"""MappingVAE encoder (csrc/vae.hip) stage by stage against the fp64 oracle, at the geometries where it can go wrong.

Every stage (the stem and the six residual blocks, read back as the next layer reads them: channels-last with the pixel padding)
and `mu` are compared with oracle/vae_ref.py run in fp64. The yardstick of each tensor is the fp32 CPU oracle's own error on it:

    max|x_hip - x64| <= min(M * max|x32 - x64| + 1e-6 * max|x64|,  1e-3 * max|x64|)

Calibrated once on the MI355X: the worst (max|x_hip - x64| - 1e-6 * max|x64|) / max|x32 - x64| over every tensor of every case
(the Mish-tail case included) was 0.305 (the output of block 5, 127x191, B = 2; next 0.135 for the same tensor at 376x1232, B = 1, and 0.129 for block 2 at
65x65); M is at most 4x that. Relative to its own max|x64| no tensor was further from fp64 than 1.3e-6, so nothing needs the 1e-3 cap,
and the fp32 oracle's own error is 2.9e-7 to 1.2e-6 of max|x64| throughout. Running `pytest -s` prints every comparison ("PARITY" lines).

Geometries: 64x64 (the smallest accepted frame, a 1x1 embedding), 65x65 (odd at every level: 33/17/9/5/3/2), 127x191, 200x333,
375x1242 (a raw KITTI frame of sequence 03: 188x621 after the first block) and 376x1232. A stride-2 layer writes
ceil(h/2) x ceil(w/2) pixels, so at every odd size the first block's maps are larger than 4*H*W floats per image; every handle
here is created with max_batch = B (a fresh module per case), so that no slack of a larger handle hides an overrun.

Tile shapes (conv_dispatch.h choose_tile; N = output channels, tiles of 128 pixels per image x images): layers with N <= 32 always run
128x32. At 376x1232 the N = 64 layers (conv.1 and the skip of block 4, conv.0 of block 5: 24x77 pixels, 15 tiles per image) run 64x64
below B = 26 and 128x64 from B = 26 (15 * 26 >= 384); the N = 128 layers at 12x39 pixels (conv.1 and the skip of block 5, conv.0 of
block 6: 4 tiles per image) run 64x64 below B = 48 and 128x64 from B = 48 (4 * 48 * 2 >= 384); the N = 128 layers at 6x20 (block 6, mean_lin:
one tile per image) run 64x64 at every batch a handle accepts (B <= 64), and 128x128 (400 tiles) and 128x96 (N % 96) are out of the
VAE's reach. So B = 1, 26 and 48 reach every shape the encoder can run. The batches of 26 and 48 repeat five distinct frames (image b is
frame b % 5): the oracle runs on five frames, and every one of the B outputs is compared with its own frame's."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from atdn_vslam_amd import _lib
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import MappingVAE
from oracle import vae_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

M, FLOOR, CAP = 1.2, 1e-6, 1e-3      # observed 0.305
CHANNELS = (3, 16, 16, 32, 64, 128, 128)
KITTI_FRAMES = 5
CASES = [(64, 64, 1), (65, 65, 3), (127, 191, 2), (200, 333, 3), (375, 1242, 2), (376, 1232, 1), (376, 1232, 26), (376, 1232, 48)]


def _net(sd):
    net = MappingVAE()
    net.load_state_dict(sd)
    return net


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _oracle(sd, frames):
    """{name: (x32, x64)} channels-last on the CPU: the seven stages and mu."""
    out = {}
    runs = []
    for s in (sd, _f64(sd)):
        taps = {}
        taps["mu"] = vae_ref.vae_encode(s, frames, taps)
        runs.append(taps)
    for k in runs[0]:
        out[k] = tuple(r[k].permute(0, 2, 3, 1).contiguous() for r in runs)
    return out


@pytest.fixture(scope="module")
def vsd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return syn.to_torch(syn.make_vae_state(seed=2))


@pytest.fixture(scope="module")
def tail_sd(vsd):
    """The stem's weights x 60 and the first block's x 4: pre-activations far beyond +-20 on both sides."""
    sd = dict(vsd)
    sd["encoder.0.conv.weight"] = vsd["encoder.0.conv.weight"] * 60.0
    for k in ("conv.0.conv", "conv.1.conv", "skip_layer"):
        sd["encoder.1.%s.weight" % k] = vsd["encoder.1.%s.weight" % k] * 4.0
    return sd


@pytest.fixture(scope="module")
def oracle(vsd):
    """(H, W) -> (frames, {name: (x32, x64)}), computed once per geometry."""
    cache = {}

    def get(H, W, n):
        if (H, W) not in cache:
            frames = torch.from_numpy(syn.make_frames(n, H, W, seed=300 + H + W))
            cache[(H, W)] = (frames, _oracle(vsd, frames))
        assert cache[(H, W)][0].shape[0] == n
        return cache[(H, W)]
    return get


class Checker:
    """Collects every comparison (for the calibration table) and every violation (reported together at the end). `hip` is a
    device tensor [B, ...]; image b is compared with reference b % n (x32, x64: CPU tensors [n, ...])."""

    def __init__(self, case, m=M, floor=FLOOR):
        self.case, self.m, self.floor, self.rows, self.bad = case, m, floor, [], []

    def __call__(self, name, hip, x32, x64):
        n = min(hip.shape[0], x64.shape[0])
        assert hip.shape[1:] == x64.shape[1:], (name, hip.shape, x64.shape)
        assert bool(torch.isfinite(hip).all()), name
        r64 = x64[:n].to(hip.device)
        e_hip = max(float((hip[b].double() - r64[b % n]).abs().max()) for b in range(hip.shape[0]))
        scale, e32 = float(x64[:n].abs().max()), float((x32[:n].double() - x64[:n]).abs().max())
        bound = min(self.m * e32 + self.floor * scale, CAP * scale)
        need = max(0.0, e_hip - self.floor * scale) / e32 if e32 > 0 else (0.0 if e_hip <= self.floor * scale else float("inf"))
        self.rows.append((name, e_hip / scale if scale else e_hip, e32 / scale if scale else e32, need))
        if not e_hip <= bound:
            self.bad.append("%s: max|hip-64| %.3e > bound %.3e (max|64| %.3e, max|32-64| %.3e)" % (name, e_hip, bound, scale, e32))

    def finish(self):
        for name, rel, rel32, need in self.rows:
            print("PARITY %s %s rel_hip=%.3e rel_32=%.3e need_m=%.3g" % (self.case, name, rel, rel32, need))
        worst = max(self.rows, key=lambda r: r[3])
        print("PARITY-WORST %s %s need_m=%.3g" % (self.case, worst[0], worst[3]))
        assert not self.bad, "%s:\n  " % self.case + "\n  ".join(self.bad)


def _check_all_stages(chk, net, images, want):
    """Every stage tap and mu of a fresh module (max_batch = B) against the oracle; the pad lane of the 3-channel maps is 0."""
    B, _, H, W = images.shape
    stages = MappingVAE.layer_plan(H, W)[0]
    for k in range(7):
        tap = net.debug_stage(images, k)
        c = CHANNELS[k]
        assert tuple(tap.shape) == (B,) + stages[k] and stages[k][2] >= c
        if stages[k][2] > c:
            assert float(tap[..., c:].abs().max()) == 0.0, "pad lane of stage %d" % k
        chk("enc%d" % k, tap[..., :c], *want["enc%d" % k])
    mu = net(images)[0]
    chk("mu", mu.permute(0, 2, 3, 1), *want["mu"])
    rows, hw = net.encode_rows(images)
    assert hw == stages[6][:2] and torch.equal(rows.view(B, hw[0], hw[1], 128), mu.permute(0, 2, 3, 1))
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,W,B", CASES, ids=["%dx%d-B%d" % c for c in CASES])
def test_every_stage_matches_the_fp64_oracle(vsd, oracle, H, W, B):
    n = KITTI_FRAMES if (H, W) == (376, 1232) else B
    frames, want = oracle(H, W, n)
    images = frames[torch.arange(B) % n].to(DEV)
    chk = Checker("%dx%d/B%d" % (H, W, B))
    _check_all_stages(chk, _net(vsd), images, want)
    chk.finish()


def test_mish_tails_match_the_fp64_oracle(tail_sd):
    """65x65, B = 3, with pre-activations of the stem and of all three Mish of the first block beyond +-20 on both sides (asserted
    on the fp64 oracle): the `x > 20` branch of mishf_ on one side and, below -104, expf underflowing to 0 on the other."""
    frames = torch.from_numpy(syn.make_frames(3, 65, 65, seed=31))
    sd, x = _f64(tail_sd), vae_ref.normalize_rgb(frames.double())
    pre = {"stem": F.conv2d(x, sd["encoder.0.conv.weight"], sd["encoder.0.conv.bias"], padding=3)}
    e0 = vae_ref._bn(F.mish(pre["stem"]), sd, "encoder.0.bn")
    p = "encoder.1"
    pre["conv.0"] = F.conv2d(e0, sd[p + ".conv.0.conv.weight"], sd[p + ".conv.0.conv.bias"], padding=1)
    y = vae_ref._bn(F.mish(pre["conv.0"]), sd, p + ".conv.0.bn")
    pre["conv.1"] = F.conv2d(y, sd[p + ".conv.1.conv.weight"], sd[p + ".conv.1.conv.bias"], stride=2, padding=1)
    y = vae_ref._bn(F.mish(pre["conv.1"]), sd, p + ".conv.1.bn")
    pre["sum"] = y + F.conv2d(e0, sd[p + ".skip_layer.weight"], sd[p + ".skip_layer.bias"], stride=2)
    for k, v in pre.items():
        print("PREACT %s min=%.1f max=%.1f" % (k, float(v.min()), float(v.max())))
        assert float(v.min()) < -20.0 and float(v.max()) > 20.0, k
    assert float(pre["stem"].min()) < -104.0 and float(pre["conv.0"].min()) < -104.0
    want = _oracle(tail_sd, frames)
    assert torch.equal(want["enc1"][1], vae_ref._bn(F.mish(pre["sum"]), sd, p + ".out_block.1").permute(0, 2, 3, 1))
    chk = Checker("mish-tails/65x65/B3")
    _check_all_stages(chk, _net(tail_sd), frames.to(DEV), want)
    chk.finish()


@pytest.fixture(scope="module")
def small():
    """Three frames at 127x191 on the device."""
    return torch.from_numpy(syn.make_frames(3, 127, 191, seed=47)).to(DEV)


def _rows(net, images):
    return net(images)[0].permute(0, 2, 3, 1).contiguous()


def test_repeated_split_and_smaller_batches_give_the_same_bits(vsd, small):
    net = _net(vsd)
    first = _rows(net, small)
    assert torch.equal(_rows(net, small), first)                                    # a second call
    single = _net(vsd)
    ones = torch.cat([_rows(single, small[b:b + 1]) for b in range(3)])
    assert torch.equal(ones, first)                                                 # B = 3 against three calls at B = 1
    assert net._handles[net._key(127, 191)][3] == 3
    assert torch.equal(_rows(net, small[1:2]), first[1:2])                          # B = 1 on the handle of 3, after a call at 3 ...
    assert torch.equal(_rows(net, small[1:3]), _rows(_net(vsd), small[1:3]))        # ... and B = 2, against a fresh handle
    for k in range(7):                                                              # the stage read does not disturb the product call
        assert torch.equal(net.debug_stage(small, k), _net(vsd).debug_stage(small, k)), k
    assert torch.equal(_rows(net, small), first)


def test_encode_rows_into_a_bank_and_a_side_stream_give_the_same_bits(vsd, small):
    net = _net(vsd)
    mu = net(small)[0]
    h, w = mu.shape[2:]
    bank = torch.full((5, h * w * 128), 7.0, device=DEV)
    rows, hw = net.encode_rows(small, out=bank[1:4])
    assert hw == (h, w) and rows.data_ptr() == bank[1].data_ptr()
    assert torch.equal(bank[1:4].view(3, h, w, 128), mu.permute(0, 2, 3, 1))
    assert float(bank[0].min()) == 7.0 and float(bank[4].max()) == 7.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mu_side = net(small)[0]
        tap_side = net.debug_stage(small, 3)
    side.synchronize()
    assert torch.equal(mu_side, mu) and torch.equal(tap_side, net.debug_stage(small, 3))


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_frame_does_not_poison_the_handle(vsd, value):
    """126x190 (even, so that 4*H*W floats would hold every map: this is about the pad lane alone; 63x95 after the first block). One pixel of one frame is NaN or +-Inf: that call's output may be anything, but the next clean call on the same handle gives the
    bits of a fresh handle, at every stage. (The 3-channel maps travel as 4 floats per pixel; the layer that reads them multiplies
    the pad lane by a zero weight, and 0 * NaN is NaN: the lane has to be written by every call, not once at finalize(). With the
    lane zeroed once, the clean call after a NaN frame returned NaN in 1536 of the 2304 elements of mu.)"""
    net = _net(vsd)
    small = torch.from_numpy(syn.make_frames(3, 126, 190, seed=53)).to(DEV)
    bad = small.clone()
    bad[1, 2, 60, 100] = value
    out = net(bad)[0]
    assert not bool(torch.isfinite(out[1]).all())
    fresh = _net(vsd)
    for k in range(7):
        assert torch.equal(net.debug_stage(small, k), fresh.debug_stage(small, k)), k
    clean = net(small)[0]
    assert bool(torch.isfinite(clean).all()) and torch.equal(clean, fresh(small)[0])


def test_argument_edges_are_rejected_and_a_later_call_is_sound(vsd, small, oracle):
    L = _lib.lib()
    h = C.c_void_p()
    for H, W in ((63, 64), (64, 63), (63, 63), (4097, 4096)):                       # below 64, and H * W > 2^24
        assert L.atdn_vae_create(C.byref(h), H, W, 1) != 0
        assert b"frame size out of range" in L.atdn_last_error()
    for B in (0, 65):
        assert L.atdn_vae_create(C.byref(h), 64, 64, B) != 0
        assert b"max_batch out of range" in L.atdn_last_error()
    out = torch.empty((3, 2 * 3 * 128), device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
    assert L.atdn_vae_create(C.byref(h), 127, 191, 2) == 0                          # never finalised
    assert L.atdn_vae_encode(h, ptr(small), 1, ptr(out), None) != 0
    assert b"not finalized" in L.atdn_last_error()
    L.atdn_vae_destroy(h)
    net = _net(vsd)
    want = _rows(net, small[:2])
    good = net._handles[net._key(127, 191)][0]                                      # max_batch = 2
    for B in (3, 0):
        assert L.atdn_vae_encode(good, ptr(small), B, ptr(out), None) != 0
        assert b"max_batch" in L.atdn_last_error()
    assert L.atdn_vae_debug_stage(good, ptr(small), 2, 7, ptr(out), out.numel(), None) != 0
    assert L.atdn_vae_debug_stage(good, ptr(small), 2, 6, ptr(out), 2 * 2 * 3 * 128 - 1, None) != 0
    assert L.atdn_vae_encode(good, None, 2, ptr(out), None) != 0
    torch.cuda.synchronize()
    assert torch.equal(_rows(net, small[:2]), want)                                 # the good handle is untouched ...
    frames, ref = oracle(127, 191, 2)
    chk = Checker("127x191/B2/after-rejections")
    chk("mu", _rows(net, frames.to(DEV)), *ref["mu"])                               # ... and still right
    chk.finish()
