"""Ground plane on the device: the kernels of atdn_ground_terms / atdn_ground_solve / atdn_ground_classify (transforms.ground_terms,
ground_plane and ground_classify on device tensors) against the host form and the NumPy float64 restatement of the rule
(tests/ground_ref.py) — every bit of q, the sums, the residual plane and the flags, and every count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_ref as G  # noqa: E402
from ground_ref import CASES, CASE_MIN_VOTES, CASE_N0, FULL_CASE, OPTS, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVEL = (0.0, 1.0, 0.0)
CLASSIFY = {k: v for k, v in OPTS.items() if k != "scale_rel"}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(DEV)


def _cpu(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _equal(got, want, tag=""):
    for g, w in zip(got, want):
        if w.dtype == np.int32:
            assert np.array_equal(g, w), (tag, g.tolist(), w.tolist())
        else:
            assert same_bits(g, w), tag


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,H,W,rows,seed", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_restatement_and_the_host_form(name, H, W, rows, seed, B):
    """The case table of the host test (5 x 7: one ragged chunk; 9 x 33 with the band (1, 9): off the 16-byte grid; 32 x 32: one
    whole chunk; 33 x 31: 1023 pixels; 47 x 154: 8 chunks), with and without mask, from the vote and from q_init, 0 and 6 steps."""
    depth, mask, calib, q0 = G.case_inputs(H, W, B, seed)
    kw = dict(rows=rows, **OPTS)
    for masked, voted, iters in G.variants():
        m = mask if masked else None
        tag = (name, B, masked, voted, iters)
        want = G.solve_batch(depth, calib, CASE_N0, None if voted else q0, m, iters=iters, min_votes=CASE_MIN_VOTES, **kw)
        got = transforms.ground_plane(_dev(depth), calib, CASE_N0, None if voted else _dev(q0), _dev(m), iters=iters,
                                      min_votes=CASE_MIN_VOTES, **kw)
        assert all(t.is_cuda for t in got) and got[0].dtype == torch.float64 and got[2].dtype == torch.int32
        _equal(_np(got), want, tag)
        host = transforms.ground_plane(_cpu(depth), calib, CASE_N0, None if voted else _cpu(q0), _cpu(m), iters=iters,
                                       min_votes=CASE_MIN_VOTES, **kw)
        _equal(_np(got), _np(host), tag)
        terms = transforms.ground_terms(_dev(depth), got[0], calib, _dev(m), **kw)
        assert terms[0].is_cuda and terms[1].is_cuda
        _equal(_np(terms), G.terms_batch(depth, want[0], calib, m, **kw), tag)
        cls = transforms.ground_classify(_dev(depth), got[0], calib, _dev(m), rows=rows, **CLASSIFY)
        assert cls[0].is_cuda and tuple(cls[0].shape) == (B, 1, H, W) and cls[1].dtype == torch.uint8
        _equal(_np(cls), G.classify_batch(depth, want[0], calib, m, rows=rows, **CLASSIFY), tag)
        _equal(_np(cls), _np(transforms.ground_classify(_cpu(depth), _cpu(want[0]), calib, _cpu(m), rows=rows, **CLASSIFY)), tag)


def test_mask_off_the_dword_grid_and_no_plane():
    """9 x 33, B = 3, all rows: the mask planes of b = 1, 2 start at byte addresses 1 and 2 mod 4 (byte loads), b = 0 reads
    dwords. An all-zero mask leaves no candidate: q = 0, +0.0 sums and zero counts; so does min_votes above every mode."""
    _, H, W, _, seed = CASES[1]
    depth, _, calib, _ = G.case_inputs(H, W, 3, seed)
    mask = (np.random.RandomState(7).uniform(size=(3, H, W)) < 0.7).astype(np.uint8)
    assert (H * W) % 4 == 1
    kw = dict(rows=(0, H), iters=6, min_votes=CASE_MIN_VOTES, **OPTS)
    dm = _dev(mask)
    assert dm.data_ptr() % 4 == 0
    got = transforms.ground_plane(_dev(depth), calib, CASE_N0, mask=dm, **kw)
    _equal(_np(got), G.solve_batch(depth, calib, CASE_N0, None, mask, **kw))
    cls = transforms.ground_classify(_dev(depth), got[0], calib, dm, rows=(0, H), **CLASSIFY)
    _equal(_np(cls), G.classify_batch(depth, got[0].cpu().numpy(), calib, mask, rows=(0, H), **CLASSIFY))
    for none in (transforms.ground_plane(_dev(depth), calib, CASE_N0, mask=torch.zeros_like(dm), **kw),
                 transforms.ground_plane(_dev(depth), calib, CASE_N0, **dict(kw, min_votes=10 ** 6))):
        q, s, c = _np(none)
        assert same_bits(q, np.zeros((3, 3))) and same_bits(s, np.zeros((3, 10))) and not c.any()


def test_outputs_are_fully_written_and_nothing_else():
    """Guard values around every output, the depth at every alignment of its vector grid, a workspace full of NaN bytes: every
    output is written, nothing else is, and nothing is read from the workspace that the call did not write."""
    _, H, W, rows, seed = CASES[1]
    B = 3
    depth, mask, calib, q0 = G.case_inputs(H, W, B, seed)
    n = B * H * W
    kw = dict(rows=rows, **OPTS)
    want = G.solve_batch(depth, calib, CASE_N0, None, mask, iters=6, min_votes=CASE_MIN_VOTES, **kw)
    want_i = G.solve_batch(depth, calib, CASE_N0, q0, mask, iters=6, min_votes=CASE_MIN_VOTES, **kw)
    want_t = G.terms_batch(depth, want[0], calib, mask, **kw)
    want_c = G.classify_batch(depth, want[0], calib, mask, rows=rows, **CLASSIFY)
    L = _lib.lib()
    nws = int(L.atdn_ground_workspace_bytes(B, H, W))
    dq, dq0, dmask = _dev(want[0]), _dev(q0), _dev(mask)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for shift in (0, 1, 2, 3):
        dbuf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        dbuf[shift:shift + n] = _dev(depth).reshape(-1)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        geom = (B, H, W, rows[0], rows[1], *calib)
        opts = (OPTS["scale_rel"], OPTS["inlier_rel"], OPTS["min_z"], OPTS["max_depth"])
        ws = torch.full((nws // 8 + 2,), float("nan"), dtype=torch.float64, device=DEV)
        sums = torch.full((10 * B + 2,), -7.0, dtype=torch.float64, device=DEV)
        cnt3 = torch.full((3 * B + 2,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.atdn_ground_terms(p(dbuf[shift:]), p(dmask), p(dq), *geom, *opts, p(sums[1:]), p(cnt3[1:]), p(ws[1:]), stream))
        for init, ref in ((None, want), (dq0, want_i)):
            ws.fill_(float("nan"))
            q = torch.full((3 * B + 2,), -7.0, dtype=torch.float64, device=DEV)
            ssum = torch.full((10 * B + 2,), -7.0, dtype=torch.float64, device=DEV)
            cnt6 = torch.full((6 * B + 2,), -7, dtype=torch.int32, device=DEV)
            _lib.check(L.atdn_ground_solve(p(dbuf[shift:]), p(dmask), None if init is None else p(init), *geom, *CASE_N0, *opts,
                                           CASE_MIN_VOTES, 6, p(q[1:]), p(ssum[1:]), p(cnt6[1:]), p(ws[1:]), stream))
            torch.cuda.synchronize()
            qq, ss = q.cpu().numpy(), ssum.cpu().numpy()
            assert qq[0] == -7.0 and qq[-1] == -7.0 and same_bits(qq[1:-1].reshape(B, 3), ref[0]), shift
            assert ss[0] == -7.0 and ss[-1] == -7.0 and same_bits(ss[1:-1].reshape(B, 10), ref[1]), shift
            assert cnt6.cpu().tolist() == [-7] + ref[2].reshape(-1).tolist() + [-7], shift
            w = ws.cpu().numpy()
            assert np.isnan(w[0]) and np.isnan(w[-1])
        res = torch.full((n + 2,), -7.0, dtype=torch.float32, device=DEV)
        on = torch.full((n + 8,), 9, dtype=torch.uint8, device=DEV)
        _lib.check(L.atdn_ground_classify(p(dbuf[shift:]), p(dmask), p(dq), *geom, *opts[1:], p(res[1:]), p(on[4:]), stream))
        torch.cuda.synchronize()
        s = sums.cpu().numpy()
        assert s[0] == -7.0 and s[-1] == -7.0 and same_bits(s[1:-1].reshape(B, 10), want_t[0]), shift
        assert cnt3.cpu().tolist() == [-7] + want_t[1].reshape(-1).tolist() + [-7], shift
        r, o = res.cpu().numpy(), on.cpu().numpy()
        assert r[0] == -7.0 and r[-1] == -7.0 and same_bits(r[1:-1].reshape(B, 1, H, W), want_c[0]), shift
        assert (o[:4] == 9).all() and (o[4 + n:] == 9).all() and same_bits(o[4:4 + n].reshape(B, H, W), want_c[1]), shift


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, B = 2 street (scales 1 and 0.8) and its reference (the vote and three steps), computed once."""
    _, H, W, rows, seed = FULL_CASE
    depth, mask, calib, q0 = G.case_inputs(H, W, 2, seed)
    kw = dict(rows=rows, iters=3, min_votes=64, **OPTS)
    return depth, calib, kw, G.solve_batch(depth, calib, LEVEL, None, None, **kw)


def test_full_size_two_calls_streams_and_graph(full_size):
    """376 x 1232, B = 2, the default band (188 rows: 227 chunks and a ragged last one, 32 vote workgroups over them), the vote and
    three steps against the restatement. The same bits on a second call, on a side stream, and from a captured graph replayed
    twice — a capture fails on any host synchronisation, so the replayed chain of 2 + 2 * 4 launches shows the call has none."""
    _, H, W, _, _ = FULL_CASE
    depth, calib, kw, want = full_size
    d = _dev(depth)
    a1 = transforms.ground_plane(d, calib, LEVEL, **kw)
    a2 = transforms.ground_plane(d, calib, LEVEL, **kw)
    torch.cuda.synchronize()
    _equal(_np(a1), want)
    assert (want[2][:, 3] > 0).all() and (want[2][:, 2] > 10000).all()
    assert all(torch.equal(x, y) for x, y in zip(a1, a2))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a3 = transforms.ground_plane(d, calib, LEVEL, **kw)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a1, a3))
    L = _lib.lib()
    B = 2
    q = torch.empty((B, 3), dtype=torch.float64, device=DEV)
    sums = torch.empty((B, 10), dtype=torch.float64, device=DEV)
    counts = torch.empty((B, 6), dtype=torch.int32, device=DEV)
    ws = torch.empty((int(L.atdn_ground_workspace_bytes(B, H, W)) // 8,), dtype=torch.float64, device=DEV)
    y0, y1 = transforms.ground_rows(calib, H)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(L.atdn_ground_solve(C.c_void_p(d.data_ptr()), None, None, B, H, W, y0, y1, *calib, *LEVEL, OPTS["scale_rel"],
                                       OPTS["inlier_rel"], OPTS["min_z"], OPTS["max_depth"], 64, 3, C.c_void_p(q.data_ptr()),
                                       C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, float("nan")):
        q.fill_(fill)
        sums.fill_(fill)
        counts.fill_(123456)
        ws.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(q, a1[0]) and torch.equal(sums, a1[1]) and torch.equal(counts, a1[2]), fill
    cls = transforms.ground_classify(d, a1[0], calib, **CLASSIFY)
    host = transforms.ground_classify(_cpu(depth), _cpu(want[0]), calib, **CLASSIFY)
    _equal(_np(cls), _np(host))
    assert int(cls[1].sum()) == int(want[2][:, 2].sum())


def test_kernel_argument_errors():
    d = torch.ones(1, 4, 4, device=DEV)
    q0 = torch.tensor([[0.0, 0.5, 0.0]], dtype=torch.float64, device=DEV)
    k = (5.0, 5.0, 1.5, 1.5)
    with pytest.raises(RuntimeError, match="scale_rel"):
        transforms.ground_terms(d, q0, k, **dict(OPTS, scale_rel=0.0))
    with pytest.raises(RuntimeError, match="iters"):
        transforms.ground_plane(d, k, iters=-1, min_votes=1, **OPTS)
    with pytest.raises(RuntimeError, match="rows"):
        transforms.ground_plane(d, k, rows=(2, 2), min_votes=1, **OPTS)
    with pytest.raises(RuntimeError, match="normal"):
        transforms.ground_plane(d, k, normal_prior=(0.0, 0.0, 0.0), min_votes=1, **OPTS)
    with pytest.raises(RuntimeError):
        transforms.ground_plane(d, k, q_init=q0.cpu(), min_votes=1, **OPTS)          # q_init on the host
    with pytest.raises(RuntimeError):
        transforms.ground_classify(d, q0, k, mask=torch.ones(1, 4, 4, dtype=torch.uint8), **CLASSIFY)
    L = _lib.lib()
    q = torch.zeros(3, dtype=torch.float64, device=DEV)
    sums = torch.zeros(10, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(6, dtype=torch.int32, device=DEV)
    res = torch.zeros(16, device=DEV)
    on = torch.zeros(16, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(int(L.atdn_ground_workspace_bytes(1, 4, 4)) // 8 + 1, dtype=torch.float64, device=DEV)
    dp, ip, qp, sp, cp, rp, op, wp = (C.c_void_p(t.data_ptr()) for t in (d, q0, q, sums, cnt, res, on, ws))
    geom = (1, 4, 4, 2, 4, 5.0, 5.0, 1.5, 1.5)
    opts = (0.05, 0.05, 0.1, 80.0)
    solve = (*geom, 0.0, 1.0, 0.0, *opts, 1)
    assert L.atdn_ground_workspace_bytes(1, 4, 4) > 0 and L.atdn_ground_workspace_bytes(1, 4097, 4097) == 0
    assert L.atdn_ground_terms(dp, None, ip, *geom, *opts, sp, cp, wp, None) == 0
    assert L.atdn_ground_solve(dp, None, None, *solve, 2, qp, sp, cp, wp, None) == 0
    assert L.atdn_ground_solve(dp, None, ip, *solve, 2, qp, sp, cp, wp, None) == 0
    assert L.atdn_ground_classify(dp, None, ip, *geom, *opts[1:], rp, op, None) == 0
    assert L.atdn_ground_terms(dp, None, ip, *geom, *opts, sp, cp, None, None) != 0 and b"null" in L.atdn_last_error()
    assert L.atdn_ground_terms(dp, None, None, *geom, *opts, sp, cp, wp, None) != 0 and b"null" in L.atdn_last_error()
    assert L.atdn_ground_solve(dp, None, None, *solve, 2, qp, sp, cp, None, None) != 0
    assert L.atdn_ground_solve(None, None, None, *solve, 2, qp, sp, cp, wp, None) != 0
    assert L.atdn_ground_classify(dp, None, None, *geom, *opts[1:], rp, op, None) != 0
    assert L.atdn_ground_classify(dp, None, ip, *geom, *opts[1:], None, op, None) != 0
    assert L.atdn_ground_terms(dp, None, ip, *geom, *opts, sp, cp, C.c_void_p(ws.data_ptr() + 4), None) != 0
    assert b"aligned" in L.atdn_last_error()
    assert L.atdn_ground_solve(dp, None, C.c_void_p(q0.data_ptr() + 4), *solve, 2, qp, sp, cp, wp, None) != 0
    assert b"aligned" in L.atdn_last_error()
    assert L.atdn_ground_solve(dp, None, ip, *solve, 2, ip, sp, cp, wp, None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_ground_solve(dp, None, None, *solve, 2, qp, sp, cp, dp, None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_ground_classify(dp, None, ip, *geom, *opts[1:], dp, op, None) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_ground_solve(dp, None, None, *solve, 65, qp, sp, cp, wp, None) != 0
    assert L.atdn_ground_solve(dp, None, None, *solve[:-1], 0, 2, qp, sp, cp, wp, None) != 0                  # min_votes
    assert L.atdn_ground_solve(dp, None, None, 65536, *solve[1:], 2, qp, sp, cp, wp, None) != 0
    assert L.atdn_ground_solve(dp, None, None, 1, 4, 4, 3, 3, *solve[5:], 2, qp, sp, cp, wp, None) != 0      # y0 = y1
    assert L.atdn_ground_solve(dp, None, None, 1, 4, 4, 0, 5, *solve[5:], 2, qp, sp, cp, wp, None) != 0      # y1 > H
    torch.cuda.synchronize()
