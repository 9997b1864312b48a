"""Forward-backward flow consistency, host form: atdn_flow_consistency_host through the raw C ABI and through
transforms.flow_consistency on CPU tensors, against the NumPy float64 restatement of the rule (tests/flow_consistency_ref.py)
and against cases whose answer is known in closed form. Every comparison is exact — every mask byte and every count: the random
cases are first shown (on the helper alone) to keep every pixel at least 1e-9 away from the threshold, four orders of magnitude
above float64 rounding, so any correct float64 evaluation agrees with the helper everywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flow_consistency_ref import MIN_MARGIN, RANDOM_CASES, flow_consistency_ref, reference_batch, smooth_pair  # noqa: E402


def _raw(fw, bw, alpha1=0.01, alpha2=0.5):
    """The C entry point on numpy arrays [B,2,H,W]; the outputs start out as 0xFF / garbage."""
    fw, bw = np.ascontiguousarray(fw, dtype=np.float32), np.ascontiguousarray(bw, dtype=np.float32)
    B, _, H, W = fw.shape
    mask = np.full((B, 1, H, W), 0xFF, dtype=np.uint8)
    count = np.full((B,), -12345, dtype=np.int32)
    _lib.check(_lib.lib().atdn_flow_consistency_host(C.c_void_p(fw.ctypes.data), C.c_void_p(bw.ctypes.data), B, H, W, alpha1, alpha2,
                                                     C.c_void_p(mask.ctypes.data), C.c_void_p(count.ctypes.data)))
    return mask, count


def _const(H, W, vx, vy):
    f = np.empty((1, 2, H, W), dtype=np.float32)
    f[:, 0], f[:, 1] = vx, vy
    return f


@pytest.mark.parametrize("name, H, W, B, seed, amplitude", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_host_twin_equals_the_helper(name, H, W, B, seed, amplitude):
    """5 x 7; 9 x 33 with B = 3 (H * W = 297 is odd: the planes of b = 1, 2 start at odd offsets); 47 x 154."""
    fw, bw = smooth_pair(H, W, seed, B, amplitude)
    mask, count, margin, inside = reference_batch(fw, bw)
    print("%s: counts %s of %d, inside %.0f %%, smallest margin %.2e" % (name, count.tolist(), H * W, 100 * inside, margin))
    assert margin >= MIN_MARGIN                                  # the condition, on the reference alone
    assert all(0 < c < H * W for c in count) and inside < 1.0    # both outcomes occur, and some pixels leave the image
    got_mask, got_count = _raw(fw, bw)
    assert np.array_equal(got_mask, mask) and np.array_equal(got_count, count)
    m, s = transforms.flow_consistency(torch.from_numpy(fw), torch.from_numpy(bw))
    assert np.array_equal(m.numpy(), mask)
    assert s.dtype == torch.float32 and np.array_equal(s.numpy(), (count.astype(np.float64) / (H * W)).astype(np.float32))


def test_constant_flow_has_a_known_mask():
    """fw = (3, -2), bw = -fw on 9 x 33: consistent exactly where the target stays inside, x <= 29 and y >= 2: 30 * 7 = 210."""
    fw = _const(9, 33, 3.0, -2.0)
    mask, count = _raw(fw, -fw)
    want = np.zeros((9, 33), dtype=np.uint8)
    want[2:, :30] = 1
    assert int(count[0]) == (33 - 3) * (9 - 2) == 210
    assert np.array_equal(mask[0, 0], want)
    assert np.array_equal(mask[0, 0], flow_consistency_ref(fw[0], -fw[0])[0])


def test_zero_flows_and_closed_borders():
    z = np.zeros((2, 2, 9, 33), dtype=np.float32)
    mask, count = _raw(z, z)
    assert mask.min() == 1 and count.tolist() == [297, 297]
    # x1 == W - 1 and y1 == H - 1 exactly count as inside: every pixel is sent to the last column / last row / the corner
    H, W = 9, 33
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for tx, ty in ((W - 1 - x, 0 * y), (0 * x, H - 1 - y), (W - 1 - x, H - 1 - y), (-x, -y)):
        fw = np.stack([tx, ty]).astype(np.float32)[None]
        bw = np.zeros_like(fw)
        # diff = |fw|^2 against 0.01 |fw|^2 + 0.5: consistent only where |fw|^2 <= 0.5 / 0.99, i.e. the pixels that do not move
        mask, count = _raw(fw, bw)
        ref_mask, ref_count, margin = flow_consistency_ref(fw[0], bw[0])
        assert np.isfinite(margin).all()                          # every pixel is inside
        assert np.array_equal(mask[0, 0], ref_mask) and int(count[0]) == ref_count == int(((tx == 0) & (ty == 0)).sum())
    # constant integer flows that end exactly on the border, undone by bw = -fw: the border pixels count
    fw = _const(9, 33, 32.0, 8.0)
    mask, count = _raw(fw, -fw)
    assert int(count[0]) == 1 and mask[0, 0, 0, 0] == 1          # only (0, 0) -> (32, 8) = (W - 1, H - 1) stays inside
    fw = _const(9, 33, -32.0, -8.0)
    mask, count = _raw(fw, -fw)
    assert int(count[0]) == 1 and mask[0, 0, 8, 32] == 1         # only (32, 8) -> (0, 0)
    fw = _const(9, 33, 1.0, 1.0)
    mask, count = _raw(fw, -fw)
    assert int(count[0]) == 32 * 8 and mask[0, 0, 7, 31] == 1 and mask[0, 0, 8, 31] == 0 and mask[0, 0, 7, 32] == 0


def test_contradicting_flows_give_all_zeros():
    """bw = +fw at magnitude 5: where the target is inside, diff = |2 fw|^2 = 100 against 0.01 * 50 + 0.5 = 1."""
    fw = _const(9, 33, 3.0, 4.0)
    mask, count = _raw(fw, fw)
    assert mask.max() == 0 and int(count[0]) == 0


def test_zero_alphas_keep_exact_round_trips_only():
    """alpha1 = alpha2 = 0: only diff == 0 passes. Integer flows with bw = -fw return exactly; half-pixel ones do not once the
    backward flow varies."""
    fw = _const(9, 33, 3.0, -2.0)
    mask, count = _raw(fw, -fw, 0.0, 0.0)
    assert int(count[0]) == 210
    fw2, bw2 = smooth_pair(9, 33, 0, 1, 2.0)
    ref_mask, ref_count, _ = flow_consistency_ref(fw2[0], bw2[0], 0.0, 0.0)
    mask, count = _raw(fw2, bw2, 0.0, 0.0)
    assert ref_count == 0 and int(count[0]) == 0 and np.array_equal(mask[0, 0], ref_mask)
    mixed = fw.copy()
    mixed[0, 0, 4, 10] = 2.5                                      # one pixel with a non-returning flow
    mask, count = _raw(mixed, -fw, 0.0, 0.0)
    assert int(count[0]) == 209 and mask[0, 0, 4, 10] == 0


# (y, x) of a pixel of the 9 x 33 constant field fw = (2.5, 1.5) and its four taps: (x0, y0) = (x + 2, y + 1), weights 1/4 each
_PIX = (3, 10)
_TAPS = [(4, 12), (4, 13), (5, 12), (5, 13)]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values_zero_the_pixels_that_read_them(bad):
    fw = _const(9, 33, 2.5, 1.5)
    bw = -fw
    base_mask, base_count = _raw(fw, bw)
    assert base_mask[0, 0][_PIX] == 1
    # in fw, either channel: that pixel only
    for c in (0, 1):
        f = fw.copy()
        f[0, c][_PIX] = bad
        mask, count = _raw(f, bw)
        diff = np.argwhere(mask[0, 0] != base_mask[0, 0])
        assert diff.tolist() == [list(_PIX)] and mask[0, 0][_PIX] == 0 and int(count[0]) == int(base_count[0]) - 1
        assert np.array_equal(mask[0, 0], flow_consistency_ref(f[0], bw[0])[0])
    # in one of the four taps (weight 1/4 each): the pixel, and nothing but the (up to four) pixels that read that tap
    for tap in _TAPS:
        for c in (0, 1):
            b = bw.copy()
            b[0, c][tap] = bad
            mask, count = _raw(fw, b)
            ref_mask, ref_count, _ = flow_consistency_ref(fw[0], b[0])
            assert np.array_equal(mask[0, 0], ref_mask) and int(count[0]) == ref_count
            assert mask[0, 0][_PIX] == 0
            changed = np.argwhere(mask[0, 0] != base_mask[0, 0])
            readers = {(tap[0] - 1 - dy, tap[1] - 2 - dx) for dy in (0, 1) for dx in (0, 1)}
            assert {tuple(p) for p in changed.tolist()} == readers
    # in a ZERO-weight tap: integer flow (2, 1), ax = ay = 0, taps (x+2, y+1) with weight 1 and three with weight 0
    fw = _const(9, 33, 2.0, 1.0)
    bw = -fw
    base_mask, _ = _raw(fw, bw)
    for tap in ((4, 13), (5, 12), (5, 13)):                       # the zero-weight taps of pixel (3, 10)
        b = bw.copy()
        b[0, 0][tap] = bad
        mask, count = _raw(fw, b)
        ref_mask, ref_count, _ = flow_consistency_ref(fw[0], b[0])
        assert np.array_equal(mask[0, 0], ref_mask) and int(count[0]) == ref_count
        assert mask[0, 0][_PIX] == 0 and base_mask[0, 0][_PIX] == 1


def test_bad_arguments_are_reported():
    L = _lib.lib()
    f = np.zeros((1, 2, 4, 4), dtype=np.float32)
    m = np.zeros((1, 1, 4, 4), dtype=np.uint8)
    c = np.zeros((1,), dtype=np.int32)
    fp, mp, cp = C.c_void_p(f.ctypes.data), C.c_void_p(m.ctypes.data), C.c_void_p(c.ctypes.data)
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, 0.5, mp, cp) == 0
    assert L.atdn_flow_consistency_host(None, fp, 1, 4, 4, 0.01, 0.5, mp, cp) != 0
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, 0.5, None, cp) != 0
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, 0.5, mp, None) != 0
    assert b"null" in L.atdn_last_error()
    assert L.atdn_flow_consistency_host(fp, fp, 1, 0, 4, 0.01, 0.5, mp, cp) != 0
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, -0.01, 0.5, mp, cp) != 0
    assert b"alpha" in L.atdn_last_error()
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, float("nan"), mp, cp) != 0
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, float("inf"), mp, cp) != 0
    assert L.atdn_flow_consistency_host(fp, fp, 1, 4, 4, 0.01, 0.5, fp, cp) != 0          # the mask on top of an input
    assert b"overlap" in L.atdn_last_error()
    with pytest.raises(RuntimeError):
        transforms.flow_consistency(torch.zeros(2, 4, 4), torch.zeros(2, 4, 5))
    with pytest.raises(RuntimeError):
        transforms.flow_consistency(torch.zeros(1, 2, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError):
        transforms.flow_consistency(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="alpha"):
        transforms.flow_consistency(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), alpha1=-1.0)


def test_wrapper_forms_and_score():
    fw, bw = smooth_pair(9, 33, 0, 3, 2.0)
    mask, count, _, _ = reference_batch(fw, bw)
    m4, s4 = transforms.flow_consistency(torch.from_numpy(fw), torch.from_numpy(bw))
    assert m4.dtype == torch.uint8 and tuple(m4.shape) == (3, 1, 9, 33) and s4.dtype == torch.float32 and tuple(s4.shape) == (3,)
    assert np.array_equal(m4.numpy(), mask)
    for b in range(3):
        m3, s3 = transforms.flow_consistency(torch.from_numpy(fw[b]), torch.from_numpy(bw[b]))
        assert m3.dtype == torch.uint8 and tuple(m3.shape) == (1, 9, 33) and s3.dtype == torch.float32 and s3.dim() == 0
        assert np.array_equal(m3.numpy(), mask[b])
        assert float(s3) == float(np.float32(np.float64(count[b]) / 297.0)) == float(s4[b])
    # other thresholds reach the library
    loose, _ = transforms.flow_consistency(torch.from_numpy(fw), torch.from_numpy(bw), alpha1=0.05, alpha2=2.0)
    want = np.stack([flow_consistency_ref(fw[b], bw[b], 0.05, 2.0)[0] for b in range(3)])[:, None]
    assert np.array_equal(loose.numpy(), want) and int(want.sum()) > int(mask.sum())
