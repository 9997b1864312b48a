"""Forward interpolation of a flow along itself (warm start), host form: atdn_flow_forward_interpolate_host through the raw C
ABI and through transforms.forward_interpolate on CPU tensors, against the recorded outputs of the flow package's own function
(tests/golden/warm_start.npz, written by tests/golden/make_golden_warm.py) and the brute-force float64 helper
(tests/forward_interpolate_ref.py). Everything is compared exactly: the outputs are bit copies of input values."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from forward_interpolate_ref import cases, forward_interpolate_ref  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "warm_start.npz"))
    return [(str(n), g["in_" + str(n)], g["out_" + str(n)]) for n in g["names"]]


def _raw(flow):
    """The C entry point on a numpy array [B,2,h,w]."""
    flow = np.ascontiguousarray(flow, dtype=np.float32)
    out = np.full_like(flow, np.nan)
    B, _, h, w = flow.shape
    _lib.check(_lib.lib().atdn_flow_forward_interpolate_host(C.c_void_p(flow.ctypes.data), B, h, w, C.c_void_p(out.ctypes.data)))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_holds_the_stated_cases(golden):
    """The stored inputs are the seeded flows the helper regenerates: six cases, the shapes and sigmas of the generator."""
    want = cases()
    assert [n for n, _, _ in golden] == [n for n, _, _, _ in want]
    for (_, fin, fout), (_, h, w, flow) in zip(golden, want):
        assert fin.shape == (2, h, w) and fout.shape == (2, h, w) and fin.dtype == np.float32
        assert np.array_equal(_bits(fin), _bits(flow))


def test_host_twin_equals_the_wheel_on_every_stored_case(golden):
    for name, fin, fout in golden:
        got = transforms.forward_interpolate(torch.from_numpy(fin))
        assert got.dtype == torch.float32 and tuple(got.shape) == fin.shape and not got.is_cuda
        assert np.array_equal(_bits(got.numpy()), _bits(fout)), name
        assert np.array_equal(_bits(_raw(fin[None])[0]), _bits(fout)), name


def test_all_invalid_flow_gives_zeros():
    flow = np.full((2, 6, 9), -1000.0, dtype=np.float32)
    assert not _bits(_raw(flow[None])).any()
    assert not _bits(transforms.forward_interpolate(torch.from_numpy(flow)).numpy()).any()


def test_ties_go_to_the_lowest_source_index():
    """Integer-valued flows put every source on a grid point, where equal distances are the rule, not the exception. The helper's
    argmin takes the first minimum, which is the lowest source index; scipy is not consulted (its tie rule is unspecified)."""
    flow = np.empty((2, 6, 9), dtype=np.float32)
    flow[0], flow[1] = 2.0, 1.0                          # constant (2, 1): 35 of 54 sources stay inside the grid
    ref, _, nvalid = forward_interpolate_ref(flow)
    assert nvalid == 35
    assert np.array_equal(_bits(_raw(flow[None])[0]), _bits(ref))
    # a field whose tied nearest sources carry DIFFERENT values, so that the rule shows in the output
    r = np.random.RandomState(5)
    flow = r.randint(-2, 3, size=(2, 6, 9)).astype(np.float32)
    ref, gap, _ = forward_interpolate_ref(flow)
    assert float(gap.min()) == 0.0
    assert np.array_equal(_bits(_raw(flow[None])[0]), _bits(ref))
    assert np.array_equal(_bits(transforms.forward_interpolate(torch.from_numpy(flow)).numpy()), _bits(ref))


def test_batch_of_three_equals_three_single_calls(golden):
    r = np.random.RandomState(7)
    flow = (r.randn(3, 2, 9, 33) * 3).astype(np.float32)
    flow[1] = golden[1][1]                               # the stored 9 x 33 case rides along
    both = transforms.forward_interpolate(torch.from_numpy(flow)).numpy()
    assert both.shape == flow.shape
    for b in range(3):
        one = transforms.forward_interpolate(torch.from_numpy(flow[b])).numpy()
        assert np.array_equal(_bits(both[b]), _bits(one)), b
        assert np.array_equal(_bits(one), _bits(forward_interpolate_ref(flow[b])[0])), b
    assert np.array_equal(_bits(both[1]), _bits(golden[1][2]))
    assert np.array_equal(_bits(_raw(flow)), _bits(both))


def test_outputs_are_bit_copies_of_inputs(golden):
    for name, fin, _ in golden[:4]:
        out = _raw(fin[None])[0]
        pairs_in = set(zip(_bits(fin[0]).ravel().tolist(), _bits(fin[1]).ravel().tolist()))
        pairs_out = set(zip(_bits(out[0]).ravel().tolist(), _bits(out[1]).ravel().tolist()))
        assert pairs_out <= pairs_in, name
    # NaN and infinite flows are invalid sources and never copied
    flow = golden[0][1].copy()
    flow[0, 2, 3], flow[1, 1, 1] = np.nan, np.inf
    out = _raw(flow[None])[0]
    assert np.isfinite(out).all()
    assert np.array_equal(_bits(out), _bits(forward_interpolate_ref(flow)[0]))


def test_bad_arguments_are_reported():
    L = _lib.lib()
    x = np.zeros((1, 2, 4, 4), dtype=np.float32)
    assert L.atdn_flow_forward_interpolate_host(None, 1, 4, 4, C.c_void_p(x.ctypes.data)) != 0
    assert L.atdn_flow_forward_interpolate_host(C.c_void_p(x.ctypes.data), 1, 0, 4, C.c_void_p(x.ctypes.data)) != 0
    assert L.atdn_flow_forward_interpolate_host(C.c_void_p(x.ctypes.data), 1, 4, 4, C.c_void_p(x.ctypes.data)) != 0   # in place
    assert b"overlap" in L.atdn_last_error()
    with pytest.raises(RuntimeError):
        transforms.forward_interpolate(torch.zeros(3, 4, 4))
