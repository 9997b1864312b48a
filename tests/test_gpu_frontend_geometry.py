"""Frame front-end (atdn_vslam_amd/csrc/frontend.hip: resize, uint8 ingest, replicate padding) against the fp64 reference of
tests/resize_ref.py at the tile tails, ratio limits and launch slices of its kernels.

Yardstick (as in tests/test_gpu_flow_geometry.py): the error of torch's own fp32 CPU op on the same input,

    max|hip - ref64| <= M * max|torch32 - ref64| + FLOOR * 255

on uint8 noise (values 0..255, full local contrast: the worst input for weight rounding). ref64 is numpy fp64 and shares no
code with ATen (tests/test_resize_ref_host.py pins it to F.interpolate in fp64 to 1e-9); torch32 is F.interpolate in fp32 on
the CPU. Where torch32 equals ref64 exactly (identity tables) the bound is the floor alone. Every case runs with a uint8 and
an fp32 source (outputs must be torch.equal) and with antialiasing on and off; every output buffer is pre-filled with NaN and
followed by a NaN guard row, so an unwritten element and a write past the end both show.

Calibration: see CALIBRATION below the imports (worst need 0.958 at past_boundary, plain bilinear; M = 4). `pytest -s` prints one PARITY line per comparison.

Kernels and the cases that reach them (tests/resize_ref.py CASES; each with both source types and both modes):
  resize_rows_kernel (Hin == Hout, 4 Win <= 5 Wout, planes <= 65535; 256 columns x 8 rows per block, source span in LDS)
      rows_tail_1249  (13,321)->(13,257)  ratio 1.249, last row block of 5 rows, second column block of ONE column
      rows_125_span   (9,645)->(9,516)    exactly 1.25 = the dispatch boundary: three column blocks, the last of 4 columns, a
                                          1-row tail, and the largest LDS span (antialias: 321 source columns for block 0)
      rows_upscale    (8,40)->(8,50)      width up-scaling, one partial column block, no row tail
      identity_capi   (5,300)->(5,300)    identity tables (resize_frames returns its input, so through the C ABI): output equals
                                          the input bit for bit
      and the 6-plane calls of planes_65538 below
  resize_kernel<T, true> (Hin == Hout otherwise)
      past_boundary   (13,322)->(13,257)  one source pixel past 4 Win <= 5 Wout
      idy_333x / idy_35x / idy_375x / idy_4x   (8,100)->(8,30), (8,112)->(8,32), (8,120)->(8,32), (8,128)->(8,32): antialias
                                          rows of 6-7, 7, 7-8 and 8 taps (3.5x has 7 taps everywhere; 8-tap rows need 2s > 7)
      planes_65538    21,846 frames (4,10)->(4,9): more planes than grid.z holds, so the rows kernel is declined; five slices
                      of 16,383 planes, the last of 6. Its first 6 and last 6 planes must be torch.equal to 6-plane calls,
                      which go through resize_rows_kernel ("same products in the same order")
  resize_kernel<T, false> (both axes)
      both_down (21,37)->(13,29), both_up (7,9)->(19,23), mixed (30,20)->(9,40), one_pixel (1,1)->(8,8)
      two_slices      911 frames (16,12)->(24,10): 2,733 planes x 24 rows = 65,592 > 65,535 grid rows: a slice of 2,730 planes
                      and one of 3; the last 6 planes must be torch.equal to a 6-plane call on those planes alone
  ratio guard of make_table_aa: idy_4x is the largest ratio every width supports; (8,129)->(8,32) and (8,160)->(8,32), on either
      axis, must raise and leave the output untouched; plain bilinear at 5x has no limit
  pad_replicate_kernel: InputPadder at (1,1), (8,8), (7,9), (161,515); asymmetric pads on (5,6) through the C ABI; 4 frames of
      (370,1226) -> 5,558,784 elements, beyond the 4,194,304 of one trip of the 16,384-block grid: the grid-stride loop's
      second trip
  FrameIngest: (21,37)->(13,29), six clips of 4, 1, 3, 4, 2, 4 frames through the two staging slots

What a broken kernel would fail (reasoned from the code, not run):
  nrow fixed at 8            rows_tail_1249, rows_125_span, identity_capi: the last row block of the last plane writes 3 (7, 3)
                             rows past the end -> the NaN guard row is overwritten (and earlier planes' tail blocks race with
                             the next plane's first rows)
  span capped 16 lower       rows_125_span, antialias: block 0 needs source columns 0..320 (321 > 320), so column 255 reads an
                             LDS element nobody staged -> parity against fp64 (and torch.equal between neighbouring runs)
  slice offset d0 with Hin   two_slices: the second slice lands at plane 2730 * 16/24 -> the last 3 planes stay NaN
  pad loop's stride dropped  the 4 x (370,1226) pad: elements from 4,194,304 on stay NaN (one trip), or never ends (stride 0)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.pipeline import FrameIngest, resize_frames

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# CALIBRATION (MI355X, FLOOR 1e-6, the 75 PARITY lines of this file): the worst (max|hip - ref64| - FLOOR * 255) /
# max|torch32 - ref64| was 0.958, past_boundary (13,322)->(13,257) without antialiasing, both source types: max|hip - ref64| =
# max|torch32 - ref64| = 6.09e-3 (the fp32 rounding of the source coordinate times the full contrast of noise). In 65 of the 75
# comparisons the kernel's error equals torch's to the printed digits, and 46 stay within the floor alone. M = 4 (4.2x the
# worst need).
M, FLOOR = 4.0, 1e-6


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n, row):
    """n output floats followed by a guard row, all NaN."""
    return torch.full((n + row,), float("nan"), dtype=torch.float32, device=DEV)


def _split(buf, n, shape, what):
    torch.cuda.synchronize()
    out, guard = buf[:n].view(shape), buf[n:]
    assert bool(torch.isnan(guard).all()), "%s: wrote past the end of its output" % what
    return out


def _resize_raw(x, size, antialias):
    """atdn_resize_frames_mode / _u8 into a NaN-filled, guarded buffer -> (return code, buffer, n)."""
    x = x.contiguous()
    planes = int(x.numel() // (x.shape[-2] * x.shape[-1]))
    n = planes * size[0] * size[1]
    buf = _guarded(n, size[1])
    fn = _lib.lib().atdn_resize_frames_u8 if x.dtype == torch.uint8 else _lib.lib().atdn_resize_frames_mode
    rc = fn(C.c_void_p(x.data_ptr()), planes, x.shape[-2], x.shape[-1], size[0], size[1], int(bool(antialias)),
            C.c_void_p(buf.data_ptr()), _stream())
    return rc, buf, n


def _resize(x, size, antialias):
    rc, buf, n = _resize_raw(x, size, antialias)
    _lib.check(rc)
    out = _split(buf, n, tuple(x.shape[:-2]) + tuple(size), "resize %s" % (tuple(x.shape),))
    assert not bool(torch.isnan(out).any()), "resize %s -> %s left output elements unwritten" % (tuple(x.shape), size)
    return out


def _pad(x, l, r, t, b):
    x = x.contiguous()
    H, W = x.shape[-2:]
    planes = int(x.numel() // (H * W))
    n = planes * (H + t + b) * (W + l + r)
    buf = _guarded(n, W + l + r)
    _lib.check(_lib.lib().atdn_pad_frames(C.c_void_p(x.data_ptr()), planes, H, W, l, r, t, b, C.c_void_p(buf.data_ptr()), _stream()))
    out = _split(buf, n, tuple(x.shape[:-2]) + (H + t + b, W + l + r), "pad %s" % (tuple(x.shape),))
    assert not bool(torch.isnan(out).any()), "pad %s left output elements unwritten" % (tuple(x.shape),)
    return out


def _references(u8, size, antialias):
    """(fp64 reference, torch's fp32 CPU result) of uint8 frames [n,3,H,W] (numpy)."""
    r64 = torch.from_numpy(rr.resize(u8, size, antialias))
    t32 = F.interpolate(torch.from_numpy(u8).float(), size=list(size), mode="bilinear", align_corners=False, antialias=antialias)
    return r64, t32.double()


def _parity(case, name, hip, t32, r64):
    hip = hip.detach().cpu().double()
    assert hip.shape == r64.shape, (case, name, hip.shape, r64.shape)
    assert bool(torch.isfinite(hip).all()), (case, name)
    e_hip, e32 = float((hip - r64).abs().max()), float((t32 - r64).abs().max())
    floor = FLOOR * 255.0
    need = max(0.0, e_hip - floor) / e32 if e32 > 0 else (0.0 if e_hip <= floor else float("inf"))
    print("PARITY %s %s err_hip=%.3e err_32=%.3e need_m=%.3g" % (case, name, e_hip, e32, need))
    assert e_hip <= M * e32 + floor, "%s %s: max|hip-64| %.3e > %g * %.3e + %.3e" % (case, name, e_hip, M, e32, floor)


def _mode(antialias):
    return "aa" if antialias else "plain"


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("case", [c[0] for c in rr.CASES])
def test_resize_against_fp64(case, antialias):
    _, n, hw, size = rr.CASE[case]
    u8 = rr.noise_u8(case)
    r64, t32 = _references(u8, size, antialias)
    du = torch.from_numpy(u8).to(DEV)
    df = du.float()
    got_u, got_f = _resize(du, size, antialias), _resize(df, size, antialias)
    assert torch.equal(got_u, got_f), "uint8 and fp32 sources must give identical pixels"
    tag = "%s/%s" % (case, _mode(antialias))
    _parity(tag, "u8", got_u, t32, r64)
    _parity(tag, "f32", got_f, t32, r64)
    if hw == size:
        assert torch.equal(got_f, df) and resize_frames(df, size, antialias=antialias) is df
    else:   # the Python entry point (allocates its own output) gives the same pixels
        assert torch.equal(resize_frames(du, size, antialias=antialias), got_u)
        assert torch.equal(resize_frames(df, size, antialias=antialias), got_u)
    if n > 2:   # sliced launches: the slices' source / destination offsets
        planes_u, planes_got = du.view(-1, hw[0], hw[1]), got_u.view(-1, size[0], size[1])
        ends = (slice(-6, None),) + ((slice(0, 6),) if hw[0] == size[0] else ())
        for sl in ends:
            for src in (planes_u[sl], planes_u[sl].float()):
                alone = _resize(src.reshape(2, 3, hw[0], hw[1]), size, antialias)
                assert torch.equal(alone.view(6, size[0], size[1]), planes_got[sl]), (case, sl, src.dtype)


@pytest.mark.parametrize("hw,size", [((8, 160), (8, 32)), ((8, 129), (8, 32)), ((160, 8), (32, 8))])
def test_ratio_guard_refuses_more_than_eight_taps(hw, size):
    """make_table_aa holds 8 taps per pixel: every ratio up to 4x fits (idy_4x above runs it against fp64), 129 -> 32 and 5x do
    not. The refusal happens before any launch: the output stays as it was."""
    assert max(rr.aa_max_taps(hw[0], size[0]), rr.aa_max_taps(hw[1], size[1])) > rr.MAX_TAPS
    u8 = np.random.RandomState(5).randint(0, 256, size=(2, 3) + hw).astype(np.uint8)
    du = torch.from_numpy(u8).to(DEV)
    for x in (du, du.float()):
        with pytest.raises(RuntimeError, match="more than 4x"):
            resize_frames(x, size, antialias=True)
        rc, buf, _ = _resize_raw(x, size, True)
        torch.cuda.synchronize()
        assert rc != 0 and bool(torch.isnan(buf).all())
    with pytest.raises(RuntimeError, match="more than 4x"):
        FrameIngest(hw, max_frames=2, size=size, antialias=True, device=DEV)
    # two taps per pixel whatever the ratio: plain bilinear has no limit
    r64, t32 = _references(u8, size, False)
    got_u, got_f = _resize(du, size, False), _resize(du.float(), size, False)
    assert torch.equal(got_u, got_f)
    _parity("guard%s->%s/plain" % (hw, size), "u8", got_u, t32, r64)
    ing = FrameIngest(hw, max_frames=2, size=size, antialias=False, device=DEV)
    assert torch.equal(ing(torch.from_numpy(u8).pin_memory()), got_u)


@pytest.mark.parametrize("mode", ["sintel", "kitti"])
@pytest.mark.parametrize("hw", [(1, 1), (8, 8), (7, 9), (161, 515)])
def test_input_padder_against_index_clamping(hw, mode):
    x = torch.from_numpy(np.random.RandomState(hw[0] * 7 + hw[1]).rand(2, 3, hw[0], hw[1]).astype(np.float32))
    padder = transforms.InputPadder(x.shape, mode=mode)
    l, r, t, b = padder._pad
    ref = torch.from_numpy(rr.replicate_pad(x.numpy(), l, r, t, b))
    dx = x.to(DEV)
    got = padder.pad(dx)[0]
    if hw == (8, 8):
        assert got is dx and (l, r, t, b) == (0, 0, 0, 0)
    else:
        assert (l + r, t + b) == ((-hw[1]) % 8, (-hw[0]) % 8)
    assert got.shape == ref.shape and got.shape[-2] % 8 == 0 and got.shape[-1] % 8 == 0
    assert torch.equal(got.cpu(), ref)
    assert torch.equal(_pad(dx, l, r, t, b).cpu(), ref)          # the kernel itself, zero pads included
    assert torch.equal(padder.unpad(got).cpu(), x)


@pytest.mark.parametrize("pad", [(0, 5, 3, 0), (7, 0, 0, 1)])
def test_pad_frames_asymmetric(pad):
    x = torch.from_numpy(np.random.RandomState(sum(pad)).rand(2, 3, 5, 6).astype(np.float32))
    got = _pad(x.to(DEV), *pad).cpu()
    assert torch.equal(got, torch.from_numpy(rr.replicate_pad(x.numpy(), *pad)))
    l, r, t, b = pad
    assert torch.equal(got[..., t:got.shape[-2] - b, l:got.shape[-1] - r], x)


def test_pad_second_trip_of_the_grid_stride_loop():
    """4 x 3 x 376 x 1232 = 5,558,784 output elements > 16,384 blocks x 256 threads."""
    x = torch.from_numpy(np.random.RandomState(12).rand(4, 3, 370, 1226).astype(np.float32))
    padder = transforms.InputPadder(x.shape, mode="sintel")
    l, r, t, b = padder._pad
    ref = torch.from_numpy(rr.replicate_pad(x.numpy(), l, r, t, b))
    assert ref.numel() == 5558784 > 16384 * 256
    dx = x.to(DEV)
    got = _pad(dx, l, r, t, b)
    assert torch.equal(got.cpu(), ref)
    via_padder = padder.pad(dx)[0]
    assert torch.equal(via_padder, got) and torch.equal(padder.unpad(via_padder).cpu(), x)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
def test_ingest_varying_clip_lengths(antialias):
    """Six clips in flight through the two staging slots: each slot is reused three times, with another frame count each time
    (a shorter clip leaves the tail of the longer one before it in the slot)."""
    hw, size = (21, 37), (13, 29)
    ing = FrameIngest(hw, max_frames=4, size=size, antialias=antialias, device=DEV)
    rs = np.random.RandomState(77)
    clips = [torch.from_numpy(rs.randint(0, 256, size=(n, 3) + hw).astype(np.uint8)).pin_memory() for n in (4, 1, 3, 4, 2, 4)]
    outs = [ing(c) for c in clips]
    torch.cuda.synchronize()
    for k, (c, o) in enumerate(zip(clips, outs)):
        assert tuple(o.shape) == (c.shape[0], 3) + size and o.dtype == torch.float32
        assert torch.equal(o, resize_frames(c.to(DEV), size, antialias=antialias)), k
        r64, t32 = _references(c.numpy(), size, antialias)
        _parity("ingest/%s" % _mode(antialias), "clip%d" % k, o, t32, r64)
    with pytest.raises(RuntimeError):
        ing(torch.zeros((5, 3) + hw, dtype=torch.uint8))
