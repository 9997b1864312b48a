"""Warm-started flow on the GPU: the forward-interpolation kernel (atdn_flow_forward_interpolate, csrc/warm_start.hip) against
the recorded outputs of the flow package's own function (tests/golden/warm_start.npz) and the brute-force float64 helper
(tests/forward_interpolate_ref.py) — exactly, every pixel — and the plumbing of `warm_start=True` through
RAFTGMA.forward_consecutive, pipeline.VisualOdometry and slam.NeuralSLAM."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms
from atdn_vslam_amd.modules import RAFTGMA

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from forward_interpolate_ref import forward_interpolate_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _eq(a, b):
    """Bit equality of two float32 arrays / tensors."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                                                 np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "warm_start.npz"))
    return [(str(n), g["in_" + str(n)], g["out_" + str(n)]) for n in g["names"]]


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


# ----------------------------------------------------------------------------- the kernel
def test_kernel_equals_the_wheel_on_every_stored_case(golden):
    """5 x 7 (one workgroup, most lanes idle) to 47 x 154 (227 workgroups, four LDS chunks, a ragged last one): every pixel."""
    for name, fin, fout in golden:
        got = transforms.forward_interpolate(torch.from_numpy(fin).to(DEV))
        assert got.is_cuda and got.dtype == torch.float32
        assert _eq(got, fout), name


def test_kernel_equals_the_helper_on_a_fresh_batch():
    """9 x 33 = 297 points: ten workgroups of 32 queries, the last one ragged; B = 3; the 3-d and the 4-d form."""
    r = np.random.RandomState(77)
    flow = (r.randn(3, 2, 9, 33) * 3).astype(np.float32)
    ref = np.stack([forward_interpolate_ref(flow[b])[0] for b in range(3)])
    got = transforms.forward_interpolate(torch.from_numpy(flow).to(DEV))
    assert tuple(got.shape) == (3, 2, 9, 33) and _eq(got, ref)
    for b in range(3):
        one = transforms.forward_interpolate(torch.from_numpy(flow[b]).to(DEV))
        assert tuple(one.shape) == (2, 9, 33) and _eq(one, ref[b]), b
    # the host form of the same library agrees
    assert _eq(transforms.forward_interpolate(torch.from_numpy(flow)), ref)


def test_kernel_edge_cases_and_streams(golden):
    # no valid source: zeros (the output buffer starts out as NaN)
    none = torch.full((2, 6, 9), -1000.0, device=DEV)
    assert not transforms.forward_interpolate(none).cpu().numpy().view(np.uint32).any()
    # ties: integer-valued fields, lowest source index (the helper's argmin takes the first minimum)
    const = np.empty((2, 6, 9), dtype=np.float32)
    const[0], const[1] = 2.0, 1.0
    assert _eq(transforms.forward_interpolate(torch.from_numpy(const).to(DEV)), forward_interpolate_ref(const)[0])
    ints = np.random.RandomState(5).randint(-2, 3, size=(2, 6, 9)).astype(np.float32)
    ref, gap, _ = forward_interpolate_ref(ints)
    assert float(gap.min()) == 0.0
    assert _eq(transforms.forward_interpolate(torch.from_numpy(ints).to(DEV)), ref)
    # NaN / infinite flows are invalid sources
    bad = golden[1][1].copy()
    bad[0, 2, 3], bad[1, 1, 1] = np.nan, -np.inf
    assert _eq(transforms.forward_interpolate(torch.from_numpy(bad).to(DEV)), forward_interpolate_ref(bad)[0])
    # the same bits on every call
    a = torch.from_numpy(golden[4][1]).to(DEV)
    b = torch.from_numpy(golden[5][1]).to(DEV)
    first = transforms.forward_interpolate(a)
    assert torch.equal(first, transforms.forward_interpolate(a))
    # a side stream next to the main stream, other inputs: each call its own answer (nothing shared between launches)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out_b = transforms.forward_interpolate(b)
    out_a = transforms.forward_interpolate(a)
    torch.cuda.synchronize()
    assert _eq(out_a, golden[4][2]) and _eq(out_b, golden[5][2])


# ----------------------------------------------------------------------------- plumbing
def _net(gsd, low_latency, precision=None):
    n = RAFTGMA(max_batch=1, low_latency=low_latency, precision=precision)
    n.load_state_dict(gsd)
    return n.to(DEV).eval()


@pytest.fixture(scope="module")
def frames3():
    return [f.clone() for f in torch.from_numpy(syn.make_frames(3, 160, 512, seed=3)).to(DEV)]


@pytest.mark.parametrize("low_latency", [False, True])
def test_warm_chain_is_pair_mode_with_the_interpolated_flow(gsd, frames3, low_latency):
    """Synthetic checkpoint, 160 x 512, 8 iterations, three frames."""
    fr = frames3
    warm, ref, cold = _net(gsd, low_latency), _net(gsd, low_latency), _net(gsd, low_latency)
    # a cold chain on a module that never ran warm
    c1 = cold.forward_consecutive(fr[0], fr[1], iters=8)
    c2 = cold.forward_consecutive(fr[1], fr[2], iters=8)
    # call 1 of a warm chain is the cold call
    w1 = warm.forward_consecutive(fr[0], fr[1], iters=8, warm_start=True)
    assert torch.equal(w1[0], c1[0]) and torch.equal(w1[1], c1[1])
    assert warm._warm_low is not None
    # call 2 is pair mode started from the pushed-forward flow of call 1
    w2 = warm.forward_consecutive(fr[1], fr[2], iters=8, warm_start=True)
    init = transforms.forward_interpolate(w1[0][0])[None]
    p2 = ref(fr[1][None], fr[2][None], iters=8, flow_init=init, test_mode=True)
    assert torch.equal(w2[0], p2[0]) and torch.equal(w2[1], p2[1])
    assert not torch.equal(w2[1], c2[1])                 # (and it is not the cold result)
    # a broken chain (any other forward in between) makes the next call cold again
    warm(fr[0][None], fr[1][None], iters=2, test_mode=True)
    assert warm._warm_low is None and warm._stream_tail is None
    w3 = warm.forward_consecutive(fr[1], fr[2], iters=8, warm_start=True)
    assert torch.equal(w3[0], c2[0]) and torch.equal(w3[1], c2[1])
    # a warm_start=False chain after warm chains on the same module: the bits of the module that never ran warm
    d1 = warm.forward_consecutive(fr[0], fr[1], iters=8)
    d2 = warm.forward_consecutive(fr[1], fr[2], iters=8)
    assert warm._warm_low is None
    assert torch.equal(d1[1], c1[1]) and torch.equal(d2[1], c2[1]) and torch.equal(d2[0], c2[0])
    # ... and a warm call that continues a cold one has nothing to start from
    warm.forward_consecutive(fr[0], fr[1], iters=8)
    w4 = warm.forward_consecutive(fr[1], fr[2], iters=8, warm_start=True)
    assert torch.equal(w4[1], c2[1])


def test_warm_chain_in_exact_fp32(gsd, frames3):
    """precision="f32" has no sequence form; the chain still carries the kept flow."""
    fr = frames3
    warm, ref = _net(gsd, False, "f32"), _net(gsd, False, "f32")
    w1 = warm.forward_consecutive(fr[0], fr[1], iters=8, warm_start=True)
    w2 = warm.forward_consecutive(fr[1], fr[2], iters=8, warm_start=True)
    assert torch.equal(w1[1], ref(fr[0][None], fr[1][None], iters=8, test_mode=True)[1])
    init = transforms.forward_interpolate(w1[0][0])[None]
    assert torch.equal(w2[1], ref(fr[1][None], fr[2][None], iters=8, flow_init=init, test_mode=True)[1])
    assert not torch.equal(w2[1], ref(fr[1][None], fr[2][None], iters=8, test_mode=True)[1])


def test_warm_call_matches_the_cpu_oracle(gsd, frames3):
    """Decoupled from the interpolation: the oracle starts from the HELPER's interpolation of the HIP flow_low of call 1 (which
    the kernel test shows equal to the kernel's), so a 1e-5 px difference of that flow cannot flip a nearest neighbour. Bounds:
    those of the C1 flow comparison in tests/test_gpu_parity.py (test_gma_c1_full_flow_matches_golden: flow_low 2e-4, flow_up
    1e-3)."""
    from oracle import gma_ref
    fr = frames3
    warm = _net(gsd, False)
    w1 = warm.forward_consecutive(fr[0], fr[1], iters=8, warm_start=True)
    w2 = warm.forward_consecutive(fr[1], fr[2], iters=8, warm_start=True)
    init = torch.from_numpy(forward_interpolate_ref(w1[0][0].cpu().numpy())[0])[None]
    ref_low, ref_up = gma_ref.gma_forward(gsd, fr[1][None].cpu(), fr[2][None].cpu(), iters=8, flow_init=init)
    e_low = float((w2[0].cpu().double() - ref_low.double()).abs().max())
    e_up = float((w2[1].cpu().double() - ref_up.double()).abs().max())
    print("warm call 2 against the oracle: flow_low %.3e px, flow_up %.3e px" % (e_low, e_up))
    assert e_low < 2e-4 and e_up < 1e-3, (e_low, e_up)


@pytest.fixture(scope="module")
def hsd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def kitti_frames():
    return torch.from_numpy(syn.make_frames(4, 376, 1241, seed=8))


def test_visual_odometry_warm_start(gsd, hsd, kitti_frames):
    from atdn_vslam_amd.pipeline import VisualOdometry
    frames = kitti_frames
    cold = VisualOdometry(gsd, hsd, device=DEV, iters=8)
    warm = VisualOdometry(gsd, hsd, device=DEV, iters=8, warm_start=True)
    assert cold.warm_start is False and warm.warm_start is True
    pc = [cold(f).clone() for f in frames]
    pw = [warm(f).clone() for f in frames]
    assert all(bool(torch.isfinite(p).all()) for p in pw)
    assert torch.equal(pw[0], pc[0]) and torch.equal(pw[1], pc[1])      # identity, then the first pair: cold in both
    assert not torch.equal(pw[2], pc[2])                                # the second pair started from another flow
    assert warm.pipe.flow_net._warm_low is not None and cold.pipe.flow_net._warm_low is None
    warm.reset()                                                         # breaks the chain
    assert warm.pipe.flow_net._warm_low is None and warm.pipe.flow_net._stream_tail is None
    assert torch.equal(warm(frames[0]), torch.eye(4))


def test_neuralslam_warm_start(gsd, hsd, kitti_frames, tmp_path):
    from atdn_vslam_amd.slam import NeuralSLAM

    class Args:
        device = DEV

    poses = {}
    for flag in (False, True):
        args = Args()
        args.keyframes_path = os.path.join(str(tmp_path), "kf%d" % flag)
        slam = NeuralSLAM(args, odometry_weights=hsd, flow_weights=gsd, warm_start=flag)
        slam.start_odometry()
        poses[flag] = [slam(f).clone() for f in kitti_frames[:3]]
        assert (slam._flow_net._warm_low is not None) == flag
    assert all(bool(torch.isfinite(p).all()) for p in poses[True])
    assert torch.equal(poses[True][0], poses[False][0]) and torch.equal(poses[True][1], poses[False][1])
    assert not torch.equal(poses[True][2], poses[False][2])
