"""Which arithmetic a flow handle runs is a property of the handle, on every path it launches by.

The plain-f16 flag is a constructor constant of the handle (GmaNet::fast_) that every launcher of the split-f16 pipeline receives
as an argument. The end-to-end bounds of the f16 mode (0.03 / 0.15 px) would not show a handle that ran the other arithmetic on
one of its paths, or that left its choice behind for the next caller, so this file pins the behaviour on bits:

* order independence: split_f16, f16, split_f16 as three handles in one process on one thread — outputs 1 and 3 identical, the
  f16 output different from them in at least one bit (the flag is live);
* graph against eager: a handle built with ATDN_NO_GRAPH=1 in the environment gives the bits of the graphed handle, for f16 and
  for split_f16_two_pass (the flag reaches the captured and the eager launch path alike);
* nothing leaks into the unit entry: after an f16 forward, atdn_conv2d_nhwc_sf_epi with and without its FAST bit still gives
  what tests/f16_exact_ref.py says (test_gpu_f16_kernels' own check, imported: the FAST kernel fast_ref bit for bit, the
  split-f16 kernel the full product and not fast_ref's bits), on one GEMM-path and one halo-path case;
* predictions: forward(test_mode=False) on an f16 handle — its last prediction is flow_up of the plain forward, bit for bit.

One textured pair at 128 x 136 (the smallest height the network accepts; W / 8 = 17: ragged tiles), B = 1, two iterations, the
synthetic weights of the flow tests. Every comparison is torch.equal on flow_low and flow_up.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from atdn_vslam_amd import synthetic as syn  # noqa: E402
from atdn_vslam_amd.modules import RAFTGMA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, ITERS = 128, 136, 2


@pytest.fixture(scope="module")
def sd():
    return syn.to_torch(syn.make_gma_state(seed=1))


@pytest.fixture(scope="module")
def pair():
    fr = torch.from_numpy(syn.make_frames(2, H, W, seed=4))
    return fr[0:1].to(DEV), fr[1:2].to(DEV)


def _net(sd, precision):
    m = RAFTGMA(max_batch=1, precision=precision)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _forward(sd, pair, precision):
    """A fresh handle's (flow_low, flow_up) on the CPU; the handle is gone on return."""
    net = _net(sd, precision)
    low, up = net(pair[0], pair[1], iters=ITERS, test_mode=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(up).all()), precision
    return low.cpu(), up.cpu()


def test_the_arithmetic_does_not_depend_on_which_handle_ran_before(sd, pair):
    first = _forward(sd, pair, "split_f16")
    f16 = _forward(sd, pair, "f16")
    third = _forward(sd, pair, "split_f16")
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])
    assert not torch.equal(f16[0], first[0]) or not torch.equal(f16[1], first[1]), "the f16 handle returned the split-f16 bits"


@pytest.mark.parametrize("precision", ["f16", "split_f16_two_pass"])
def test_eager_launch_gives_the_bits_of_the_graph(sd, pair, precision, monkeypatch):
    graphed = _forward(sd, pair, precision)
    monkeypatch.setenv("ATDN_NO_GRAPH", "1")   # read when the handle is constructed: inside the first forward
    eager = _forward(sd, pair, precision)
    assert torch.equal(graphed[0], eager[0]) and torch.equal(graphed[1], eager[1])


def test_an_f16_forward_leaves_the_unit_entry_alone(sd, pair):
    import test_gpu_f16_kernels as fk
    _forward(sd, pair, "f16")
    for table in ("stride2", "halo"):   # the GEMM-shaped dispatch and the halo-patch kernels
        p = next(q for q in fk.STORE_CASES if q[0][0] == table and q[1] == 0)
        fk.test_fast_conv_returns_the_hi_product_exactly(p)


def test_the_last_prediction_is_flow_up(sd, pair):
    net = _net(sd, "f16")
    _, up = net(pair[0], pair[1], iters=ITERS, test_mode=True)
    preds = net(pair[0], pair[1], iters=ITERS, test_mode=False)
    torch.cuda.synchronize()
    assert len(preds) == ITERS
    assert torch.equal(preds[-1], up)
