"""The MappingVAE encoder's layer plan (csrc/vae_plan.h through atdn_vae_scratch_floats; host only) against an independent
restatement of the stack in Python: the stem (7x7, stride 1, padding 3) and six residual blocks, each conv.0 (3x3, stride 1,
padding 1, at the block's input size and channels), a skip convolution (1x1, stride 2, no padding) and conv.1 (3x3, stride 2,
padding 1). Every buffer must hold every map that vae.hip writes into it. `4*H*W` floats per image, the sizing this plan replaced,
hold them only when H and W are both even: the table below is the overrun it had."""
import ctypes as C

import pytest

from atdn_vslam_amd import _lib
from atdn_vslam_amd.keyframe_map import embedding_hw
from atdn_vslam_amd.modules import MappingVAE

CHANNELS = (3, 16, 16, 32, 64, 128, 128)
SIZES = [(200, 333), (375, 1242), (376, 1232), (370, 1226), (1232, 376)]
# (H, W) -> floats per image by which the first block's skip convolution and output exceeded 4*H*W
OLD_OVERRUN = {(65, 65): 524, (127, 191): 1276, (200, 333): 800, (375, 1242): 4968, (376, 1232): 0, (370, 1226): 0, (64, 64): 0}


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def pix(c):
    return 4 if c <= 4 else 16 if c <= 16 else -(-c // 32) * 32


def restated(H, W):
    """([(h, w, floats per pixel) per stage], {buffer: [floats per image of every map written to it]})."""
    writes = {"in4": [H * W * 4], "bufA": [], "bufB": [], "bufS": []}
    h, w = conv_out(H, 7, 1, 3), conv_out(W, 7, 1, 3)
    stages = [(h, w, pix(CHANNELS[0]))]
    writes["bufA"].append(h * w * pix(CHANNELS[0]))
    for i in range(6):
        cin, cout = CHANNELS[i], CHANNELS[i + 1]
        writes["bufB"].append(conv_out(h, 3, 1, 1) * conv_out(w, 3, 1, 1) * pix(cin))
        writes["bufS"].append(conv_out(h, 1, 2, 0) * conv_out(w, 1, 2, 0) * pix(cout))
        h, w = conv_out(h, 3, 2, 1), conv_out(w, 3, 2, 1)
        writes["bufA"].append(h * w * pix(cout))
        stages.append((h, w, pix(cout)))
    return stages, writes


def _check(H, W):
    stages, floats = MappingVAE.layer_plan(H, W)
    want_stages, writes = restated(H, W)
    assert stages == want_stages, (H, W)
    for name, maps in writes.items():
        assert floats[name] == max(maps), (H, W, name, floats[name], maps)   # covers every map, and is no larger than the largest
    return stages, floats, writes


def test_plan_covers_every_stage_for_every_size_from_64_to_160():
    for H in range(64, 161):
        for W in range(64, 161):
            _check(H, W)


@pytest.mark.parametrize("hw", SIZES, ids=lambda v: "%dx%d" % v)
def test_plan_covers_every_stage_at_the_sizes_in_use(hw):
    stages, _, _ = _check(*hw)
    assert stages[6][:2] == embedding_hw(hw)


def test_four_floats_per_input_pixel_hold_the_maps_only_at_even_sizes():
    for (H, W), over in OLD_OVERRUN.items():
        _, floats, writes = _check(H, W)
        old = 4 * H * W
        assert writes["bufS"][0] - old == over and writes["bufA"][1] - old == over, (H, W)
        assert max(floats.values()) == old + over
    for H in range(64, 161):
        for W in range(64, 161):
            floats = MappingVAE.layer_plan(H, W)[1]
            assert (max(floats.values()) > 4 * H * W) == bool(H % 2 or W % 2), (H, W)


def test_sizes_the_plan_refuses():
    L = _lib.lib()
    floats, stages = (C.c_long * 4)(), (C.c_int * 21)()
    for H, W in ((0, 64), (64, 0), (-3, 64), (4097, 4096)):
        assert L.atdn_vae_scratch_floats(H, W, floats, stages) != 0
        assert b"frame size" in L.atdn_last_error()
    assert L.atdn_vae_scratch_floats(64, 64, None, stages) != 0
    assert L.atdn_vae_scratch_floats(4096, 4096, floats, stages) == 0
    assert floats[0] == 4 * 4096 * 4096
