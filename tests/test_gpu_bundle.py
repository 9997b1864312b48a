"""Windowed bundle adjustment on the GPU: the kernels of bundle.hip against the host form and the NumPy restatement
(tests/bundle_ref.py) bit for bit at the smallest shapes where they can go wrong, determinism, streams and graphs, fully written
outputs, a workspace that carries nothing, FlowTrack.bundle, and one full-size case against the host form."""
import numpy as np
import pytest
import torch

import bundle_ref as br
from atdn_vslam_amd import depth as depth_mod
from atdn_vslam_amd import transforms as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("poses", "depth", "cost", "counts")


def _t(sc, slots, init, mask, device="cpu"):
    return (torch.from_numpy(sc["acc"]).to(device), torch.from_numpy(sc["alive"]).to(device), torch.from_numpy(sc["poses"]).to(device),
            torch.from_numpy(slots).to(device), sc["calib"], torch.from_numpy(init).to(device),
            None if mask is None else torch.from_numpy(mask).to(device))


def _same(got, want):
    return [n for n, g, w in zip(NAMES, got, want) if not br.same_bits64(g.cpu().numpy(), w if isinstance(w, np.ndarray) else w.cpu().numpy())]


def test_reference_cases_take_every_branch():
    br.check_branches(4)


@pytest.mark.parametrize("iters", [0, 1, 4])
@pytest.mark.parametrize("case", br.CASES, ids=[c[0] for c in br.CASES])
def test_kernel_equals_host_form_and_reference(case, iters):
    """5 x 7, S = 2: one partial chunk. 9 x 33, B = 3, S = 5 with slots -1 and N, stride 1 and 3: W no multiple of 4 or of the
    stride, 192 / S leaves idle threads. 47 x 154, S = 8, stride 1: 15 chunks, the last partial. 33 x 65, S = 16, stride 2: the
    full-width system and the largest staging."""
    sc, slots, init, mask, ref = br.reference(case, iters)
    got = T.bundle_adjust(*_t(sc, slots, init, mask, DEV), iters=iters, **case[8])
    assert all(g.is_cuda for g in got)
    host = T.bundle_adjust(*_t(sc, slots, init, mask), iters=iters, **case[8])
    assert _same(got, ref[:4]) == [] and _same(got, host) == []


@pytest.mark.parametrize("case", br.CASES, ids=[c[0] for c in br.CASES])
def test_terms_equal_reference(case):
    sc, slots, init, mask, ref = br.reference(case, 0)
    sums, counts = T.bundle_terms(*_t(sc, slots, init, mask, DEV), **case[8])
    assert sums.is_cuda and counts.is_cuda
    assert br.same_bits64(sums.cpu().numpy(), np.stack([o["sums0"] for o in ref[4]]))
    assert br.same_bits64(counts.cpu().numpy(), np.stack([o["counts0"] for o in ref[4]]))


def _raw_call(a, kw, iters, poison):
    """atdn_bundle_adjust on buffers of the test's own: outputs and workspace filled with `poison` bytes before the call."""
    import ctypes as C
    from atdn_vslam_amd import _lib
    acc, alive, poses, slots, calib, init, mask = a
    N, _, H, W = acc.shape
    B, S = slots.shape
    L = _lib.lib()
    nbytes = int(L.atdn_bundle_workspace_bytes(B, S, H, W, kw["stride"]))
    assert nbytes > 0
    ws = torch.full((nbytes,), poison, dtype=torch.uint8, device=DEV)
    outs = [torch.full((B * S * 12 * 4,), poison, dtype=torch.uint8, device=DEV), torch.full((B * H * W * 4,), poison, dtype=torch.uint8, device=DEV),
            torch.full((B * 2 * 8,), poison, dtype=torch.uint8, device=DEV), torch.full((B * 4 * 4,), poison, dtype=torch.uint8, device=DEV)]
    fx, fy, cx, cy = (float(v) for v in calib)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.atdn_bundle_adjust(p(acc), p(alive), p(poses), p(slots), p(init), p(mask), N, B, S, H, W, fx, fy, cx, cy, kw["stride"],
                                    iters, 4.0, 2.0, 0.1, 2, *[p(o) for o in outs], p(ws),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return (outs[0].view(torch.float32).reshape(B, S, 12), outs[1].view(torch.float32).reshape(B, 1, H, W),
            outs[2].view(torch.float64).reshape(B, 2), outs[3].view(torch.int32).reshape(B, 4))


def test_outputs_fully_written_and_workspace_carries_nothing():
    """Outputs and workspace poisoned with two different byte patterns: the same bits as the reference both times, so every
    output element is written and nothing of the workspace is read before this call has written it."""
    case = br.CASES[1]
    sc, slots, init, mask, ref = br.reference(case, 4)
    a = _t(sc, slots, init, mask, DEV)
    for poison in (0xFF, 0x7B):
        assert _same(_raw_call(a, case[8], 4, poison), ref[:4]) == []


def test_two_calls_side_stream_and_graph_replay_give_the_same_bits():
    case = br.CASES[3]
    sc, slots, init, mask, ref = br.reference(case, 4)
    a = _t(sc, slots, init, mask, DEV)
    first = T.bundle_adjust(*a, iters=4, **case[8])
    second = T.bundle_adjust(*a, iters=4, **case[8])
    assert _same(first, ref[:4]) == [] and _same(second, ref[:4]) == []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = T.bundle_adjust(*a, iters=4, **case[8])
    side.synchronize()
    assert _same(third, ref[:4]) == []
    graph = torch.cuda.CUDAGraph()                              # one branch: the launches of one solve, in order
    with torch.cuda.graph(graph):
        captured = T.bundle_adjust(*a, iters=4, **case[8])
    for _ in range(2):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(captured, ref[:4]) == []


def test_flow_track_bundle_equals_the_steps_by_hand():
    H, W, K = 24, 40, 4
    sc = br.scene(H, W, 6, 9, noise=0.2)
    track = depth_mod.FlowTrack((H, W), sc["calib"], DEV, history=K)
    with pytest.raises(RuntimeError, match="no step"):
        track.bundle()
    with pytest.raises(RuntimeError, match="history"):
        depth_mod.FlowTrack((H, W), sc["calib"], DEV).bundle()
    track.start()
    prev_pose, prev_acc = np.eye(4), np.zeros((2, H, W), dtype=np.float32)
    for k in range(6):                                           # six steps into a ring of four: slots wrap
        M = np.eye(4)
        M[:3] = sc["poses"][k].reshape(3, 4)
        # the pair flow on the anchor's grid: exact for a chain that resamples nothing where the accumulated flow is smooth
        pair = torch.from_numpy(sc["acc"][k] - prev_acc)[None].to(DEV)
        track.extend(pair, torch.from_numpy(np.linalg.inv(prev_pose) @ M))
        prev_pose, prev_acc = M, sc["acc"][k]
    state = [t.clone() for t in (track.hist_acc, track.hist_alive, track.hist_pose, track.acc, track.alive, track.depth)]
    opts, mv = dict(stride=1, iters=3, min_views=2), dict(max_rel_sigma=1.0)
    got = track.bundle(multiview_options=mv, **opts)
    slots = track.history_slots()
    assert slots.tolist() == [[2, 3, 0, 1]]
    poses, _, cost, counts = T.bundle_adjust(track.hist_acc, track.hist_alive, track.hist_pose, slots.tolist(), sc["calib"], track.depth, **opts)
    refined = track.hist_pose.clone()
    refined[slots.reshape(-1).to(DEV)] = poses.reshape(-1, 12)
    want = T.multiview_depth(track.hist_acc, track.hist_alive, refined, slots.tolist(), sc["calib"], depth_init=track.depth, **mv)
    assert len(got) == 7 and int(counts[0, 0]) > 0 and int(counts[0, 3]) > 0 and not torch.equal(refined, track.hist_pose)
    for g, w in zip(got, (poses,) + tuple(want) + (cost, counts)):
        assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.view(torch.uint8), w.view(torch.uint8))
    for t, s in zip((track.hist_acc, track.hist_alive, track.hist_pose, track.acc, track.alive, track.depth), state):
        assert torch.equal(t.view(torch.uint8), s.view(torch.uint8))


def test_full_size_equals_host_form():
    """376 x 1232, B = 2, S = 16, stride 4, two steps: 57 chunks per problem, the reduced system at full width."""
    name, H, W, B, S, N, seed, opts, kw, skipped, pert = br.FULL_CASE
    sc, slots, init, mask = br.case_inputs(H, W, B, S, N, seed, opts, skipped, pert)
    got = T.bundle_adjust(*_t(sc, slots, init, mask, DEV), iters=2, **kw)
    host = T.bundle_adjust(*_t(sc, slots, init, mask), iters=2, **kw)
    assert int(host[3][0, 0]) > 20000 and int(host[3][0, 3]) >= 1
    assert _same(got, host) == []
