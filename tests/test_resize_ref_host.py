"""tests/resize_ref.py (numpy, fp64) against torch's own fp64 path: F.interpolate on a double tensor computes its weights and
sums in double, so the two must agree to rounding (1e-9 on values 0..255) at every geometry the GPU tests use, in both modes.
That pins the reference to the operation the front-end replaces (torchvision's tensor resize = F.interpolate, InputPadder =
F.pad) before tests/test_gpu_frontend_geometry.py measures the HIP kernels against it. No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as rr  # noqa: E402

EXTRA = (("outside_limit_5x", 1, (8, 160), (8, 32)),
         ("outside_limit_129", 1, (8, 129), (8, 32)), ("kitti_crop", 1, (47, 155), (47, 154)))


def _cases():
    return [c for c in rr.CASES] + list(EXTRA)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_numpy_reference_matches_torch_fp64(case, antialias):
    name, n, (h, w), size = case
    x = np.random.RandomState(len(name) + h * w).randint(0, 256, size=(n, 3, h, w)).astype(np.float64)
    got = rr.resize(x, size, antialias)
    want = F.interpolate(torch.from_numpy(x), size=list(size), mode="bilinear", align_corners=False,
                         antialias=antialias).numpy()
    assert got.shape == want.shape == (n, 3) + tuple(size) and got.dtype == np.float64
    err = float(np.abs(got - want).max())
    assert err <= 1e-9, (name, antialias, err)
    if (h, w) == tuple(size):
        assert np.array_equal(got, x)


def test_weights_are_a_partition_of_unity_and_identity_when_sizes_match():
    for n_in, n_out in ((321, 257), (645, 516), (40, 50), (100, 30), (1, 8), (9, 23), (160, 32)):
        for aa in (True, False):
            w = rr.weights(n_in, n_out, aa)
            assert w.shape == (n_out, n_in) and (w >= 0).all()
            assert np.abs(w.sum(axis=1) - 1.0).max() <= 4e-16
            assert int((w > 0).sum(axis=1).max()) <= (rr.aa_max_taps(n_in, n_out) if aa else 2)
    assert np.array_equal(rr.weights(7, 7, True), np.eye(7)) and np.array_equal(rr.weights(7, 7, False), np.eye(7))


def test_antialias_tap_counts_either_side_of_the_library_limit():
    """The library holds MAX_TAPS = 8 weights per output pixel. A window is int(c + s + 0.5) - int(c - s + 0.5) wide, at most
    floor(2s) + 1 and exactly 2s when 2s is an integer and c - s + 0.5 never is (s = 4: fraction 0.5 throughout): every
    down-scaling ratio up to and including 4 fits, 129 -> 32 (4.03) is the first width of this row that does not. By the same
    count 112 -> 32 (s = 3.5) has 7 taps everywhere, not 8: the 8-tap rows of the GPU test are 120 -> 32 and 128 -> 32."""
    assert rr.aa_max_taps(100, 30) == 7 and rr.aa_max_taps(112, 32) == 7
    assert rr.aa_max_taps(120, 32) == 8 and rr.aa_max_taps(128, 32) == 8 and rr.aa_max_taps(4 * 1232, 1232) == 8
    assert rr.aa_max_taps(129, 32) == 9 and rr.aa_max_taps(160, 32) == 10
    for n_out in (3, 32, 257, 1232):
        for n_in in range(n_out + 1, 4 * n_out + 1, max(1, n_out // 7)):
            assert rr.aa_max_taps(n_in, n_out) <= rr.MAX_TAPS, (n_in, n_out)


def test_cases_take_the_dispatch_paths_the_gpu_test_names():
    """The launcher's conditions (frontend.hip launch_resize), evaluated on the cases: a change of a case or of the dispatch
    rule that moves a case to another kernel shows here, not as silently lost coverage."""
    def route(n, hw, size):
        planes = 3 * n
        if hw[0] == size[0] and 4 * hw[1] <= 5 * size[1] and planes <= 65535:
            return "rows", 1
        per = max(1, min(planes, 65535 // size[0]))
        return ("idy" if hw[0] == size[0] else "general"), -(-planes // per)
    want = {"rows_tail_1249": ("rows", 1), "past_boundary": ("idy", 1), "rows_125_span": ("rows", 1), "rows_upscale": ("rows", 1),
            "identity_capi": ("rows", 1), "idy_333x": ("idy", 1), "idy_35x": ("idy", 1), "idy_375x": ("idy", 1), "idy_4x": ("idy", 1),
            "both_down": ("general", 1), "both_up": ("general", 1), "mixed": ("general", 1), "one_pixel": ("general", 1),
            "two_slices": ("general", 2), "planes_65538": ("idy", 5)}
    assert {c[0]: route(c[1], c[2], c[3]) for c in rr.CASES} == want
    assert [rr.aa_max_taps(w, o) for w, o in ((100, 30), (112, 32), (120, 32), (128, 32))] == [7, 7, 8, 8]


PADS = (((1, 1), (3, 4, 3, 4)), ((1, 1), (3, 4, 0, 7)), ((8, 8), (0, 0, 0, 0)), ((7, 9), (3, 4, 0, 1)),
        ((161, 515), (2, 3, 3, 4)), ((161, 515), (2, 3, 0, 7)), ((5, 6), (0, 5, 3, 0)), ((5, 6), (7, 0, 0, 1)))


@pytest.mark.parametrize("hw,pad", PADS)
def test_replicate_pad_equals_torch(hw, pad):
    x = np.random.RandomState(hw[0] * 31 + pad[0]).rand(2, 3, hw[0], hw[1]).astype(np.float32)
    got = rr.replicate_pad(x, *pad)
    want = F.pad(torch.from_numpy(x), list(pad), mode="replicate").numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    l, r, t, b = pad
    assert np.array_equal(got[..., t:got.shape[-2] - b, l:got.shape[-1] - r], x)
