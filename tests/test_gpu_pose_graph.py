"""Pose-graph optimisation on the device: the kernel of atdn_pose_graph_terms / atdn_pose_graph_solve
(transforms.pose_graph_terms and transforms.pose_graph_optimize on device tensors) against the host form and the NumPy float64
restatement of the rule (tests/pose_graph_ref.py) — every bit of the poses, the costs and edge_chi2, and every count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def _cpu(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _optimize(to, args, fixed=None, **opt):
    opt = dict(opt)
    scale = opt.pop("scale", None)
    out = transforms.pose_graph_optimize(*[to(a) for a in args], robust_scale=scale, fixed=to(fixed), **opt)
    assert all(t.is_cuda == (to is _dev) for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _equal_solution(got, ref, tag=""):
    assert _same_bits(got[0].reshape(ref["poses"].shape), ref["poses"]), tag
    assert _same_bits(got[1], ref["cost"]), (tag, got[1], ref["cost"])
    assert _same_bits(got[2], ref["chi2"]), tag
    assert got[3].tolist() == ref["counts"].tolist(), (tag, got[3], ref["counts"])


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("name", list(R.SINGLE_CASES))
def test_kernel_equals_the_helper_and_the_host_form(name):
    """pair: N = 2, E = 1 (one node in the system); ring5: the smallest graph with a loop; robust33: the Geman-McClure edges;
    ring65: crosses a wave; strided: N = E = 257, one above the workgroup's 256 threads and no multiple of 64, with the CG cap;
    rejected: a rejected step (the linearisation is kept)."""
    c = R.check_case(name)
    _equal_solution(_optimize(_dev, c["args"], **c["options"]), c["solve"], name)
    _equal_solution(_optimize(_cpu, c["args"], **c["options"]), c["solve"], name)
    scale = c["options"].get("scale")
    cost, chi2, counts = transforms.pose_graph_terms(*[_dev(a) for a in c["args"]], robust_scale=scale)
    assert cost.is_cuda and chi2.is_cuda and counts.is_cuda
    assert _same_bits(cost.cpu().numpy(), np.float64(c["terms"][0])) and _same_bits(chi2.cpu().numpy(), c["terms"][1])
    assert counts.cpu().tolist() == c["terms"][2].tolist()


@pytest.mark.parametrize("name", list(R.DRIVER_CASES))
def test_kernel_equals_the_helper_and_the_host_form_where_no_step_is_accepted(name):
    """stalled: an exactly zero pivot, the factorisation fails on every step; optimum: an exactly zero right-hand side, the CG
    does not start and the step that changes nothing is rejected. One launch each; the input comes back."""
    c = R.check_driver_case(name)
    got = _optimize(_dev, c["args"], **c["options"])
    _equal_solution(got, c["solve"], name)
    _equal_solution(_optimize(_cpu, c["args"], **c["options"]), c["solve"], name)
    assert _same_bits(got[0], c["scene"]["poses"])
    cost, chi2, counts = transforms.pose_graph_terms(*[_dev(a) for a in c["args"]])
    assert _same_bits(cost.cpu().numpy(), np.float64(c["terms"][0])) and _same_bits(chi2.cpu().numpy(), c["terms"][1])
    assert counts.cpu().tolist() == c["terms"][2].tolist()


def test_three_different_graphs_in_one_call():
    """B = 3: a zero-weight edge, an isolated node, two held nodes, a duplicate edge, a backward edge, a hub of degree 22, a
    missing chain link, a long-range edge, and absent edges (-1, N, i == j), which read nothing out of range."""
    b = R.check_batch()
    s, opt = b["scene"], b["options"]
    want = dict(poses=R.stack(b["solve"], "poses"), cost=R.stack(b["solve"], "cost"), chi2=R.stack(b["solve"], "chi2"),
                counts=R.stack(b["solve"], "counts"))
    args = (s["poses"], s["index"], s["meas"], s["weight"], s["robust"])
    got = _optimize(_dev, args, fixed=s["fixed"], **opt)
    _equal_solution(got, want, "device")
    _equal_solution(_optimize(_cpu, args, fixed=s["fixed"], **opt), want, "host")
    for g in range(3):
        for n in np.flatnonzero(s["fixed"][g]).tolist() + ([25] if g == 1 else []):
            assert _same_bits(got[0][g, n], s["poses"][g, n]), (g, n)
    g, e = 0, 27                                                   # the zero-weight edge equals the list without it
    keep = [k for k in range(s["E"]) if k != e]
    less = _optimize(_dev, (s["poses"][g], s["index"][g][:, keep], s["meas"][g][keep], s["weight"][g][keep], s["robust"][g][keep]),
                     fixed=s["fixed"][g], **opt)
    assert _same_bits(got[0][g], less[0]) and _same_bits(got[1][g], less[1]) and _same_bits(got[2][g][keep], less[2])


def test_outputs_are_fully_written_and_nothing_else():
    """Guard values around every output and a workspace full of NaN bytes: every output is written, nothing else is, and nothing
    is read from the workspace that the call did not write."""
    b = R.check_batch()
    s, opt = b["scene"], b["options"]
    B, N, E = 3, s["N"], s["E"]
    L = _lib.lib()
    ins = [_dev(s[k]) for k in ("poses", "index", "meas", "weight", "robust", "fixed")]
    nws = int(L.atdn_pose_graph_workspace_bytes(B, N, E))
    assert nws % 8 == 0 and nws > 0
    ws = torch.full((nws // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    poses = torch.full((12 * B * N + 2,), -7.0, dtype=torch.float32, device=DEV)
    cost = torch.full((2 * B + 2,), -7.0, dtype=torch.float64, device=DEV)
    chi2 = torch.full((B * E + 2,), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((4 * B + 2,), -7, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.atdn_pose_graph_solve(*[_ptr(t) for t in ins], B, N, E, opt["scale"], opt["iters"], 64, 1e-8, _ptr(poses[1:]),
                                       _ptr(cost[1:]), _ptr(chi2[1:]), _ptr(counts[2:]), _ptr(ws[1:]), stream))
    tcost = torch.full((B + 2,), -7.0, dtype=torch.float64, device=DEV)
    tchi2 = torch.full((B * E + 2,), -7.0, dtype=torch.float64, device=DEV)
    tcounts = torch.full((2 * B + 2,), -7, dtype=torch.int32, device=DEV)
    ws2 = torch.full((nws // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(L.atdn_pose_graph_terms(*[_ptr(t) for t in ins[:5]], B, N, E, opt["scale"], _ptr(tcost[1:]), _ptr(tchi2[1:]),
                                       _ptr(tcounts[2:]), _ptr(ws2[1:]), stream))
    torch.cuda.synchronize()
    p, k, x, n = poses.cpu().numpy(), cost.cpu().numpy(), chi2.cpu().numpy(), counts.cpu().numpy()
    assert p[0] == -7.0 and p[-1] == -7.0 and _same_bits(p[1:-1].reshape(B, N, 12), R.stack(b["solve"], "poses"))
    assert k[0] == -7.0 and k[-1] == -7.0 and _same_bits(k[1:-1].reshape(B, 2), R.stack(b["solve"], "cost"))
    assert x[0] == -7.0 and x[-1] == -7.0 and _same_bits(x[1:-1].reshape(B, E), R.stack(b["solve"], "chi2"))
    assert n[:2].tolist() == [-7, -7] and n[2:].reshape(B, 4).tolist() == R.stack(b["solve"], "counts").tolist()
    want = [R.terms(s["poses"][g], s["index"][g], s["meas"][g], s["weight"][g], s["robust"][g], opt["scale"]) for g in range(B)]
    k, x, n = tcost.cpu().numpy(), tchi2.cpu().numpy(), tcounts.cpu().numpy()
    assert k[0] == -7.0 and k[-1] == -7.0 and _same_bits(k[1:-1], np.array([w[0] for w in want]))
    assert x[0] == -7.0 and x[-1] == -7.0 and _same_bits(x[1:-1].reshape(B, E), np.stack([w[1] for w in want]))
    assert n[:2].tolist() == [-7, -7] and n[2:].reshape(B, 2).tolist() == [w[2].tolist() for w in want]
    for w in (ws, ws2):
        w = w.cpu().numpy()
        assert np.isnan(w[0]) and np.isnan(w[-1])


def test_two_calls_streams_graph_and_batch():
    """ring65: the same bits on a second call, on a side stream, from a captured single-stream graph — a capture fails on any
    host synchronisation, so the replay shows that the call has none — and B = 64 copies in one call equal 64 single calls."""
    c = R.check_case("ring65")
    opt = c["options"]
    d = [_dev(a) for a in c["args"][:4]]
    a1 = transforms.pose_graph_optimize(*d, **opt)
    a2 = transforms.pose_graph_optimize(*d, **opt)
    torch.cuda.synchronize()
    _equal_solution(tuple(t.cpu().numpy() for t in a1), c["solve"])
    assert all(torch.equal(x, y) for x, y in zip(a1, a2))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a3 = transforms.pose_graph_optimize(*d, **opt)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a1, a3))
    B, N, E = 64, 65, c["scene"]["E"]
    batch = [t[None].repeat((B,) + (1,) * t.dim()).contiguous() for t in d]
    many = transforms.pose_graph_optimize(*batch, **opt)
    torch.cuda.synchronize()
    for x, y in zip(a1, many):
        assert y.shape == (B,) + tuple(x.shape) and torch.equal(y, x[None].expand_as(y))
    L = _lib.lib()
    fixed = torch.zeros(N, dtype=torch.uint8, device=DEV)
    fixed[0] = 1
    poses = torch.empty((N, 12), dtype=torch.float32, device=DEV)
    cost = torch.empty((2,), dtype=torch.float64, device=DEV)
    chi2 = torch.empty((E,), dtype=torch.float64, device=DEV)
    counts = torch.empty((4,), dtype=torch.int32, device=DEV)
    ws = torch.empty((int(L.atdn_pose_graph_workspace_bytes(1, N, E)) // 8,), dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(L.atdn_pose_graph_solve(*[_ptr(t) for t in d], None, _ptr(fixed), 1, N, E, 1.0, opt["iters"], 64, 1e-8,
                                           _ptr(poses), _ptr(cost), _ptr(chi2), _ptr(counts), _ptr(ws),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, float("nan")):
        poses.fill_(fill)
        cost.fill_(fill)
        chi2.fill_(fill)
        counts.fill_(123456)
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(poses, a1[0]) and torch.equal(cost, a1[1]) and torch.equal(chi2, a1[2]) and torch.equal(counts, a1[3]), fill


def test_kernel_argument_errors():
    """Every refusal happens before a launch: the calls below hand over pointers that a launch would fault on."""
    c = R.check_case("ring5")
    p, idx, z, w = [_dev(a) for a in c["args"][:4]]
    with pytest.raises(RuntimeError, match="robust_scale"):
        transforms.pose_graph_optimize(p, idx, z, w, robust_scale=-1.0)
    with pytest.raises(RuntimeError, match="iters"):
        transforms.pose_graph_optimize(p, idx, z, w, iters=33)
    with pytest.raises(RuntimeError, match="cg_iters"):
        transforms.pose_graph_optimize(p, idx, z, w, cg_iters=0)
    with pytest.raises(RuntimeError, match="cg_tol"):
        transforms.pose_graph_optimize(p, idx, z, w, cg_tol=float("inf"))
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx.cpu(), z, w)                         # the indices on the host
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx, z, w, fixed=torch.ones(5, dtype=torch.uint8))
    L = _lib.lib()
    out = torch.zeros((5, 12), device=DEV)
    cost = torch.zeros(2, dtype=torch.float64, device=DEV)
    chi2 = torch.zeros(5, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(L.atdn_pose_graph_workspace_bytes(1, 5, 5)) // 8 + 1, dtype=torch.float64, device=DEV)
    ins = [_ptr(t) for t in (p, idx, z, w)] + [None, None]
    outs = [_ptr(t) for t in (out, cost, chi2, cnt, ws)]
    tail = (1.0, 2, 8, 1e-8)
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, *tail, *outs, None) == 0
    assert L.atdn_pose_graph_terms(*ins[:5], 1, 5, 5, 1.0, outs[1], outs[2], outs[3], outs[4], None) == 0
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, *tail, *outs[:4], None, None) != 0 and b"null" in L.atdn_last_error()
    assert L.atdn_pose_graph_terms(*ins[:5], 1, 5, 5, 1.0, outs[1], outs[2], outs[3], None, None) != 0
    assert L.atdn_pose_graph_solve(None, *ins[1:], 1, 5, 5, *tail, *outs, None) != 0
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, *tail, *outs[:4], C.c_void_p(ws.data_ptr() + 4), None) != 0
    assert b"aligned" in L.atdn_last_error()
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, *tail, ins[0], *outs[1:], None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, *tail, *outs[:4], ins[2], None) != 0 and b"overlap" in L.atdn_last_error()
    for B, N, E in ((0, 5, 5), (1025, 5, 5), (1, 1, 5), (1, 2049, 5), (1, 5, 0), (1, 5, 8193)):
        assert L.atdn_pose_graph_solve(*ins, B, N, E, *tail, *outs, None) != 0, (B, N, E)
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, 1.0, 33, 8, 1e-8, *outs, None) != 0
    assert L.atdn_pose_graph_solve(*ins, 1, 5, 5, 1.0, 2, 129, 1e-8, *outs, None) != 0
    torch.cuda.synchronize()
