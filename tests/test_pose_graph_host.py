"""Pose-graph optimisation on the host: atdn_pose_graph_terms_host / atdn_pose_graph_solve_host (transforms.pose_graph_terms
and transforms.pose_graph_optimize on CPU tensors, and the raw ABI) against the NumPy float64 restatement of the rule
(tests/pose_graph_ref.py) — every bit of the poses, the costs and edge_chi2, and every count — the properties the rule promises,
every argument error, and loop_closure's pure host functions. No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, loop_closure, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_ref as R  # noqa: E402


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _optimize(args, fixed=None, **opt):
    opt = dict(opt)
    scale = opt.pop("scale", None)
    p, cost, chi2, counts = transforms.pose_graph_optimize(*[_t(a) for a in args], robust_scale=scale, fixed=_t(fixed), **opt)
    assert p.dtype == torch.float32 and cost.dtype == torch.float64 and chi2.dtype == torch.float64 and counts.dtype == torch.int32
    return p.numpy(), cost.numpy(), chi2.numpy(), counts.numpy()


def _equal_solution(got, ref, tag=""):
    assert _same_bits(got[0].reshape(ref["poses"].shape), ref["poses"]), tag
    assert _same_bits(got[1], ref["cost"]), (tag, got[1], ref["cost"])
    assert _same_bits(got[2], ref["chi2"]), tag
    assert got[3].tolist() == ref["counts"].tolist(), (tag, got[3], ref["counts"])


@pytest.mark.parametrize("name", list(R.SINGLE_CASES))
def test_host_form_equals_the_helper(name):
    """pair: N = 2, E = 1, node 0 held (after the solve T_1 = T_0 Z); ring5: the smallest graph with a loop; robust33; ring65:
    crosses a wave; strided: N = E = 257 with the CG cap; rejected: a rejected step."""
    c = R.check_case(name)
    got = _optimize(c["args"], **c["options"])
    _equal_solution(got, c["solve"], name)
    cost, chi2, counts = transforms.pose_graph_terms(*[_t(a) for a in c["args"]], robust_scale=c["options"].get("scale"))
    assert _same_bits(cost.numpy(), np.float64(c["terms"][0])) and _same_bits(chi2.numpy(), c["terms"][1])
    assert counts.tolist() == c["terms"][2].tolist()
    assert _same_bits(cost.numpy(), c["solve"]["cost"][0])
    # edge_chi2 of a solve is the evaluation at the poses it returns
    again = transforms.pose_graph_terms(_t(got[0]), *[_t(a) for a in c["args"][1:]], robust_scale=c["options"].get("scale"))
    assert _same_bits(again[1].numpy(), got[2])


@pytest.mark.parametrize("name", list(R.DRIVER_CASES))
def test_host_form_equals_the_helper_where_no_step_is_accepted(name):
    """stalled: an exactly zero pivot, the factorisation fails on every step; optimum: an exactly zero right-hand side, the CG
    does not start and the step that changes nothing is rejected. The input comes back."""
    c = R.check_driver_case(name)
    got = _optimize(c["args"], **c["options"])
    _equal_solution(got, c["solve"], name)
    assert _same_bits(got[0], c["scene"]["poses"])
    cost, chi2, counts = transforms.pose_graph_terms(*[_t(a) for a in c["args"]])
    assert _same_bits(cost.numpy(), np.float64(c["terms"][0])) and _same_bits(chi2.numpy(), c["terms"][1])
    assert counts.tolist() == c["terms"][2].tolist() and _same_bits(chi2.numpy(), got[2])


def test_pair_ends_at_the_measurement():
    c = R.check_case("pair")
    s = c["scene"]
    p = c["solve"]["poses"].astype(np.float64).reshape(2, 3, 4)
    T0 = np.vstack([p[0], [0, 0, 0, 1]])
    Z = np.vstack([s["meas"][0].astype(np.float64).reshape(3, 4), [0, 0, 0, 1]])
    assert np.abs((T0 @ Z)[:3] - p[1]).max() < 4 * np.finfo(np.float32).eps * np.abs(p[1]).max()
    assert _same_bits(c["solve"]["poses"][0], s["poses"][0])


def test_batch_through_the_raw_abi_and_transforms():
    """B = 3 different graphs in one call: a zero-weight edge, an isolated node, two held nodes, a duplicate edge, a backward
    edge, a hub of degree 22, a missing chain link, a long-range edge, and absent edges (-1, N, i == j)."""
    b = R.check_batch()
    s, opt = b["scene"], b["options"]
    want = dict(poses=R.stack(b["solve"], "poses"), cost=R.stack(b["solve"], "cost"), chi2=R.stack(b["solve"], "chi2"),
                counts=R.stack(b["solve"], "counts"))
    got = _optimize((s["poses"], s["index"], s["meas"], s["weight"], s["robust"]), fixed=s["fixed"], **opt)
    _equal_solution(got, want, "transforms")
    for g in range(3):                                            # held and isolated nodes: the input bits
        for n in np.flatnonzero(s["fixed"][g]).tolist() + ([25] if g == 1 else []):
            assert _same_bits(got[0][g, n], s["poses"][g, n]), (g, n)
    L = _lib.lib()
    B, N, E = 3, s["N"], s["E"]
    arrays = [np.ascontiguousarray(s[k]) for k in ("poses", "index", "meas", "weight", "robust", "fixed")]
    out = [np.full((B, N, 12), -7, np.float32), np.full((B, 2), -7.0), np.full((B, E), -7.0), np.full((B, 4), -7, np.int32)]
    ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _lib.check(L.atdn_pose_graph_solve_host(*[ptr(a) for a in arrays], B, N, E, opt["scale"], opt["iters"], 64, 1e-8,
                                            *[ptr(a) for a in out]))
    _equal_solution(out, want, "raw ABI")
    for g in range(3):                                            # every graph alone, through the unbatched form
        one = _optimize((s["poses"][g], s["index"][g], s["meas"][g], s["weight"][g], s["robust"][g]), fixed=s["fixed"][g], **opt)
        assert one[0].shape == (N, 12) and one[1].shape == (2,) and one[2].shape == (E,) and one[3].shape == (4,)
        _equal_solution(one, b["solve"][g], g)


def test_a_zero_weight_edge_equals_the_list_without_it():
    s = R.check_batch()["scene"]
    opt = R.check_batch()["options"]
    g, e = 0, 27
    assert (s["weight"][g, e] == 0).all()
    keep = [k for k in range(s["E"]) if k != e]
    full = _optimize((s["poses"][g], s["index"][g], s["meas"][g], s["weight"][g], s["robust"][g]), fixed=s["fixed"][g], **opt)
    less = _optimize((s["poses"][g], s["index"][g][:, keep], s["meas"][g][keep], s["weight"][g][keep], s["robust"][g][keep]),
                     fixed=s["fixed"][g], **opt)
    assert _same_bits(full[0], less[0]) and _same_bits(full[1], less[1]) and _same_bits(full[2][keep], less[2])
    assert full[3].tolist() == [less[3][0] + 1] + less[3][1:].tolist()


def test_iters_zero_returns_the_input():
    c = R.check_case("ring5")
    p, cost, chi2, counts = _optimize(c["args"], iters=0)
    assert _same_bits(p, c["scene"]["poses"]) and _same_bits(cost[0], cost[1]) and _same_bits(cost[0], np.float64(c["terms"][0]))
    assert _same_bits(chi2, c["terms"][1]) and counts.tolist() == [5, 0, 0, 0]


def test_4x4_poses_come_back_4x4():
    c = R.check_case("ring5")
    p44 = np.zeros((5, 4, 4), np.float32)
    p44[:, :3, :] = c["scene"]["poses"].reshape(5, 3, 4)
    p44[:, 3, 3] = 1.0
    m44 = np.zeros((5, 4, 4), np.float32)
    m44[:, :3, :] = c["scene"]["meas"].reshape(5, 3, 4)
    m44[:, 3, 3] = 1.0
    got = _optimize((p44, c["args"][1], m44, c["args"][3], None), **c["options"])
    assert got[0].shape == (5, 4, 4) and (got[0][:, 3] == [0, 0, 0, 1]).all()
    assert _same_bits(got[0][:, :3, :].reshape(5, 12), c["solve"]["poses"])


@pytest.mark.parametrize("name", ["ring5", "ring65"])
def test_consistent_measurements_return_the_truth(name):
    """Exact measurements of a ground truth, a drifted start: the optimum is the truth with cost 0. What remains is the float32
    round-off of the public poses and measurements (pose_graph_ref.TRUTH_ROUNDOFF: measured on the helper; times 4)."""
    c = R.truth_case(name)
    s = c["scene"]
    tol = 4 * R.TRUTH_ROUNDOFF[name]
    start = R.mean_error(s["poses"], s["truth"])
    helper = R.mean_error(c["solve"]["poses"], s["truth"])
    assert start > 1000 * tol and helper <= 1.01 * R.TRUTH_ROUNDOFF[name], (start, helper)      # the helper first
    got = _optimize(c["args"], iters=8)
    _equal_solution(got, c["solve"], name)
    err = R.mean_error(got[0], s["truth"])
    print(name, "start %.4g m, helper %.4g m, host form %.4g m" % (start, helper, err))
    assert err <= tol
    assert got[1][1] < 1e-9 * got[1][0]


@pytest.fixture(scope="module")
def robust_runs():
    """The robust case, on the helper first: N = 33, four true loops and one wrong by (3, -1, 2) m and about 0.1 rad."""
    node0 = R._node0(33)
    s, clean = R.robust_scene(), R.robust_scene(False)
    runs = {}
    for key, scene, robust in (("robust", s, True), ("quadratic", s, False), ("clean", clean, True)):
        args = R._graph_args(scene, robust)
        runs[key] = (scene, args, R.solve(*args, fixed=node0, scale=R.ROBUST_SCALE, iters=8))
    return runs


def test_robust_loss_ignores_a_wrong_loop(robust_runs):
    err = {}
    for key, (scene, args, ref) in robust_runs.items():
        err[key] = R.mean_error(ref["poses"], scene["truth"])
    print("helper: robust %.4f m, without the wrong edge %.4f m, quadratic %.4f m" % (err["robust"], err["clean"], err["quadratic"]))
    assert err["robust"] <= 1.1 * err["clean"] and err["quadratic"] >= 2.0 * err["clean"]      # the helper first
    for key, (scene, args, ref) in robust_runs.items():
        got = _optimize(args, scale=R.ROBUST_SCALE, iters=8)
        _equal_solution(got, ref, key)
        err[key] = R.mean_error(got[0], scene["truth"])
    assert err["robust"] <= 1.1 * err["clean"] and err["quadratic"] >= 2.0 * err["clean"]
    wrong = robust_runs["robust"][2]["chi2"]
    assert wrong[-1] > 100 * wrong[32:-1].max()                   # the wrong loop stands out in edge_chi2


def test_a_scale_sequence_equals_the_solves_chained_by_hand(robust_runs):
    scene, args, _ = robust_runs["robust"]
    seq = _optimize(args, scale=[25.0, 5.0], iters=3)
    first = _optimize(args, scale=25.0, iters=3)
    second = _optimize((first[0],) + tuple(args[1:]), scale=5.0, iters=3)
    assert _same_bits(seq[0], second[0]) and _same_bits(seq[1], second[1]) and _same_bits(seq[2], second[2])
    assert seq[3].tolist() == [37, 0, first[3][2] + second[3][2], first[3][3] + second[3][3]]


def test_argument_errors():
    c = R.check_case("ring5")
    p, idx, z, w = [_t(a) for a in c["args"][:4]]
    with pytest.raises(RuntimeError, match="robust_scale"):
        transforms.pose_graph_optimize(p, idx, z, w, robust_scale=0.0)
    with pytest.raises(RuntimeError, match="robust_scale"):
        transforms.pose_graph_terms(p, idx, z, w, robust_scale=float("nan"))
    with pytest.raises(RuntimeError, match="iters"):
        transforms.pose_graph_optimize(p, idx, z, w, iters=33)
    with pytest.raises(RuntimeError, match="iters"):
        transforms.pose_graph_optimize(p, idx, z, w, iters=-1)
    with pytest.raises(RuntimeError, match="cg_iters"):
        transforms.pose_graph_optimize(p, idx, z, w, cg_iters=0)
    with pytest.raises(RuntimeError, match="cg_iters"):
        transforms.pose_graph_optimize(p, idx, z, w, cg_iters=129)
    with pytest.raises(RuntimeError, match="cg_tol"):
        transforms.pose_graph_optimize(p, idx, z, w, cg_tol=0.0)
    with pytest.raises(RuntimeError, match="N must"):
        transforms.pose_graph_optimize(p[:1], idx, z, w)
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx[:, :4], z, w)                    # four indices, five measurements
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx, z, w[:4])
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx, z, w, fixed=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p[:, :11], idx, z, w)
    with pytest.raises(RuntimeError):
        transforms.pose_graph_optimize(p, idx, z, w, robust_scale=[])
    L = _lib.lib()
    a = [np.ascontiguousarray(x) for x in c["args"][:4]]
    out = [np.zeros((5, 12), np.float32), np.zeros(2), np.zeros(5), np.zeros(4, np.int32)]
    ptr = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    ins = [ptr(x) for x in a] + [None, None]
    outs = [ptr(x) for x in out]
    tail = (1.0, 2, 8, 1e-8)
    assert L.atdn_pose_graph_solve_host(*ins, 1, 5, 5, *tail, *outs) == 0
    assert L.atdn_pose_graph_solve_host(None, *ins[1:], 1, 5, 5, *tail, *outs) != 0 and b"null" in L.atdn_last_error()
    assert L.atdn_pose_graph_solve_host(*ins, 1, 5, 5, *tail, outs[0], None, *outs[2:]) != 0
    assert L.atdn_pose_graph_solve_host(*ins, 1, 5, 5, *tail, ins[0], *outs[1:]) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_pose_graph_solve_host(*ins, 1, 5, 5, *tail, outs[0], outs[1], outs[1], outs[3]) != 0
    for B, N, E in ((0, 5, 5), (1025, 5, 5), (1, 1, 5), (1, 2049, 5), (1, 5, 0), (1, 5, 8193)):
        assert L.atdn_pose_graph_solve_host(*ins, B, N, E, *tail, *outs) != 0, (B, N, E)
        assert L.atdn_pose_graph_workspace_bytes(B, N, E) == 0
    assert L.atdn_pose_graph_workspace_bytes(1, 5, 5) == 8 * (190 * 5 + 122 * 5 + (5 * 5 + 3 * 5 + 1 + 1) // 2)
    assert L.atdn_pose_graph_terms_host(*ins[:5], 1, 5, 5, float("inf"), outs[1], outs[2], outs[3]) != 0


def test_odometry_edges():
    c = R.check_case("ring5")
    idx, meas, w = loop_closure.odometry_edges(_t(c["scene"]["poses"]), sigma=(0.1, 2.0))
    assert idx.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4]] and idx.dtype == torch.int32 and meas.shape == (4, 4, 4)
    assert w.dtype == torch.float64 and torch.allclose(w, torch.tensor([[100.0, 0.25]] * 4, dtype=torch.float64), rtol=1e-15)
    cost, chi2, counts = transforms.pose_graph_terms(_t(c["scene"]["poses"]), idx, meas, w)
    assert float(cost) < 1e-8 and counts.tolist() == [4, 0]         # the edges of a trajectory agree with it
    with pytest.raises(ValueError):
        loop_closure.odometry_edges(torch.eye(4)[None])
    with pytest.raises(ValueError):
        loop_closure.odometry_edges(_t(c["scene"]["poses"]), sigma=(0.0, 1.0))


def test_select_candidates():
    d = torch.tensor([[0.0, 9.0, 9.0, 9.0, 9.0, 9.0],
                      [9.0, 0.0, 9.0, 9.0, 9.0, 9.0],
                      [5.0, 9.0, 0.0, 9.0, 9.0, 9.0],
                      [2.0, 2.0, 0.1, 0.0, 9.0, 9.0],
                      [3.0, 1.0, 4.0, 0.1, 0.0, 9.0],
                      [7.0, 6.0, 6.0, 6.0, 0.1, 0.0]])
    # the band: j - i >= 2, so the 0.1 next to the diagonal never counts; nearest first; ties (row 3: 2.0, 2.0) to the lower index
    assert loop_closure.select_candidates(d, 2, 1) == [(0, 2), (0, 3), (1, 4), (1, 5)]
    assert loop_closure.select_candidates(d, 2, 2) == [(0, 2), (0, 3), (1, 3), (1, 4), (0, 4), (1, 5), (2, 5)]
    # top_k larger than what the band leaves
    assert loop_closure.select_candidates(d, 4, 5) == [(0, 4), (1, 5), (0, 5)]
    assert loop_closure.select_candidates(d, 6, 3) == []
    assert loop_closure.select_candidates(d, 2, 2, max_distance=2.5) == [(0, 3), (1, 3), (1, 4)]
    pairs = loop_closure.select_candidates(d, 1, 16)
    assert len(pairs) == 15 and len(set(pairs)) == 15 and all(i < j for i, j in pairs)      # every unordered pair once
    with pytest.raises(ValueError):
        loop_closure.select_candidates(d[:3], 2, 1)
    with pytest.raises(ValueError):
        loop_closure.select_candidates(d, 0, 1)
