"""Multi-view keyframe depth on the GPU: the kernel (atdn_multiview_depth, csrc/multiview_depth.hip) against the library's host
form and the NumPy float64 restatement of the rule (tests/multiview_ref.py) — every depth and information bit, every views byte
and every count, exactly —, and depth.FlowTrack(history=K), whose ring feeds it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.depth import FlowTrack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiview_ref as R  # noqa: E402
from flow_track_ref import pose_mats  # noqa: E402
from two_view_ref import scene as pair_scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gpu(sc, slots, init, **kw):
    out = transforms.multiview_depth(_dev(sc["acc"]), _dev(sc["alive"]), _dev(sc["poses"]), _dev(slots), sc["calib"],
                                     depth_init=None if init is None else _dev(init), **kw)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in out) and [t.dtype for t in out] == [torch.float32, torch.float32, torch.uint8, torch.int32]
    return tuple(t.cpu().numpy() for t in out)


def _host(sc, slots, init, **kw):
    out = transforms.multiview_depth(torch.from_numpy(sc["acc"]), torch.from_numpy(sc["alive"]), torch.from_numpy(sc["poses"]),
                                     torch.from_numpy(np.ascontiguousarray(slots)), sc["calib"],
                                     depth_init=None if init is None else torch.from_numpy(init), **kw)
    return tuple(t.numpy() for t in out)


CASE_ITERS = [(c, it) for c in R.CASES for it in ((0, 1, 4) if c[0].startswith("47x154") else (4,))]


@pytest.mark.parametrize("case, iters", CASE_ITERS, ids=["%s_it%d" % (c[0], it) for c, it in CASE_ITERS])
def test_kernel_equals_the_host_form_and_the_reference(case, iters):
    """The cases of the host tests (5 x 7: one ragged workgroup; 9 x 33, B = 3: odd planes, skipped slots; 47 x 154: 29
    workgroups, the last one ragged), with the initial depth and without (NULL)."""
    sc, slots, init, want, _ = R.reference(case, iters)
    got = _gpu(sc, slots, init, iters=iters, **case[8])
    assert R.same_outputs(got, want) and R.same_outputs(got, _host(sc, slots, init, iters=iters, **case[8]))
    none = _gpu(sc, slots, None, iters=iters, **case[8])
    assert R.same_outputs(none, _host(sc, slots, None, iters=iters, **case[8]))
    assert (none[3][:, 0] == got[3][:, 0]).all() and (none[3][:, 1] <= got[3][:, 1]).all()   # the same candidates, no more solved


@pytest.fixture(scope="module")
def full_size():
    """376 x 1232, B = 2, S = 16 over a bank of 16 views, and the host form's outputs, computed once."""
    name, H, W, B, S, N, seed, opts, kw, skipped = R.FULL_CASE
    sc, slots, init = R.case_inputs(H, W, B, S, N, seed, opts)
    return sc, slots, init, _host(sc, slots, init)


def test_kernel_at_full_size_streams_and_graph(full_size):
    """1810 workgroups per problem. The host form's bits, on a second call, on a side stream, and from a captured graph (one
    linear chain: the memset of the counts, then the kernel) replayed twice over pre-filled outputs."""
    sc, slots, init, want = full_size
    _, H, W, B, S, N = R.FULL_CASE[:6]
    assert 0 < want[3][0, 2] < want[3][0, 1] < want[3][0, 0] < H * W
    dacc, dalive, dposes, dslots, dinit = _dev(sc["acc"]), _dev(sc["alive"]), _dev(sc["poses"]), _dev(slots), _dev(init)
    one = transforms.multiview_depth(dacc, dalive, dposes, dslots, sc["calib"], depth_init=dinit)
    two = transforms.multiview_depth(dacc, dalive, dposes, dslots, sc["calib"], depth_init=dinit)
    torch.cuda.synchronize()
    assert R.same_outputs(tuple(t.cpu().numpy() for t in one), want)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        three = transforms.multiview_depth(dacc, dalive, dposes, dslots, sc["calib"], depth_init=dinit)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(one, three))
    d = torch.empty((B, 1, H, W), dtype=torch.float32, device=DEV)
    i = torch.empty((B, 1, H, W), dtype=torch.float32, device=DEV)
    v = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    c = torch.empty((B, 3), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_lib.lib().atdn_multiview_depth(_ptr(dacc), _ptr(dalive), _ptr(dposes), _ptr(dslots), _ptr(dinit), N, B, S, H, W,
                                                   *sc["calib"], 4.0, 2.0, 0.1, 2, 0.25, 80.0, 4, _ptr(d), _ptr(i), _ptr(v), _ptr(c),
                                                   _stream()))
    for fill in (-3.0, 1e30):
        d.fill_(fill)
        i.fill_(fill)
        v.fill_(77)
        c.fill_(123456)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(d, one[0]) and torch.equal(i, one[1]) and torch.equal(v, one[2]) and torch.equal(c, one[3]), fill


def test_kernel_outputs_are_fully_written():
    """Pre-filled outputs with guard values around them through the raw entry point: `views` at the four offsets of a dword,
    `depth` (and `info`, and the input planes) one float off the 16-byte grid; 9 x 33 with B = 3 (odd planes) and 47 x 154.
    Everything is written, nothing else is, and the counts are reset."""
    L = _lib.lib()
    for case in (R.CASES[1], R.CASES[2]):
        name, H, W, B, S, N, seed, opts, kw, skipped = case
        sc, slots, init, want, _ = R.reference(case)
        n = H * W
        dposes, dslots = _dev(sc["poses"]), _dev(slots)
        for sv, sf in ((0, 0), (1, 0), (2, 1), (3, 1)):
            abuf = torch.zeros(N * 2 * n + 8, dtype=torch.float32, device=DEV)
            abuf[sf:sf + N * 2 * n] = _dev(sc["acc"]).reshape(-1)
            lbuf = torch.zeros(N * n + 8, dtype=torch.uint8, device=DEV)
            lbuf[sv:sv + N * n] = _dev(sc["alive"]).reshape(-1)
            zbuf = torch.zeros(B * n + 8, dtype=torch.float32, device=DEV)
            zbuf[sf:sf + B * n] = _dev(init).reshape(-1)
            dbuf = torch.full((B * n + 32,), -7.0, dtype=torch.float32, device=DEV)
            ibuf = torch.full((B * n + 32,), -9.0, dtype=torch.float32, device=DEV)
            vbuf = torch.full((B * n + 32,), 99, dtype=torch.uint8, device=DEV)
            cnt = torch.full((3 * B + 2,), -7, dtype=torch.int32, device=DEV)
            _lib.check(L.atdn_multiview_depth(_ptr(abuf[sf:]), _ptr(lbuf[sv:]), _ptr(dposes), _ptr(dslots), _ptr(zbuf[sf:]), N, B, S, H,
                                              W, *sc["calib"], 4.0, 2.0, 0.1, 2, 0.25, 80.0, 4, _ptr(dbuf[16 + sf:]),
                                              _ptr(ibuf[16 + 3 * sf:]), _ptr(vbuf[16 + sv:]), _ptr(cnt[1:]), _stream()))
            torch.cuda.synchronize()
            tag = (name, sv, sf)
            for buf, fill, off, ref in ((dbuf, -7.0, 16 + sf, want[0]), (ibuf, -9.0, 16 + 3 * sf, want[1]), (vbuf, 99, 16 + sv, want[2])):
                h = buf.cpu().numpy()
                assert (h[:off] == fill).all() and (h[off + B * n:] == fill).all(), tag
                assert R.same_bits(h[off:off + B * n].reshape(ref.shape), ref), tag
            assert cnt.cpu().tolist() == [-7] + want[3].reshape(-1).tolist() + [-7], tag


def test_kernel_argument_errors():
    """On the device path the null, range and overlap cases return non-zero without launching; mixed devices raise."""
    L = _lib.lib()
    N, B, S, H, W = 3, 2, 2, 4, 4
    acc = torch.zeros(N, 2, H, W, device=DEV)
    alive = torch.ones(N, H, W, dtype=torch.uint8, device=DEV)
    poses = torch.eye(4, device=DEV)[:3].reshape(1, 12).repeat(N, 1).contiguous()
    slots = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32, device=DEV)
    init = torch.zeros(B, 1, H, W, device=DEV)
    d, i = torch.zeros(B, 1, H, W, device=DEV), torch.zeros(B, 1, H, W, device=DEV)
    v = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    c = torch.zeros(B, 3, dtype=torch.int32, device=DEV)
    good = dict(acc=_ptr(acc), alive=_ptr(alive), poses=_ptr(poses), slots=_ptr(slots), init=_ptr(init), depth=_ptr(d), info=_ptr(i),
                views=_ptr(v), counts=_ptr(c))

    def call(S=S, B=B, min_views=2, iters=4, **kw):
        a = dict(good, **kw)
        return L.atdn_multiview_depth(a["acc"], a["alive"], a["poses"], a["slots"], a["init"], N, B, S, H, W, 5.0, 5.0, 1.5, 1.5, 4.0,
                                      2.0, 0.1, min_views, 0.25, 80.0, iters, a["depth"], a["info"], a["views"], a["counts"], None)

    assert call() == 0 and call(init=None) == 0
    for name in good:
        if name != "init":
            assert call(**{name: None}) != 0 and b"null" in L.atdn_last_error(), name
    assert call(depth=_ptr(acc)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(info=_ptr(init)) != 0 and call(views=_ptr(alive)) != 0 and call(counts=_ptr(slots)) != 0 and call(counts=_ptr(poses)) != 0
    assert call(info=_ptr(d)) != 0 and b"two outputs overlap" in L.atdn_last_error()
    assert call(views=_ptr(d)) != 0 and call(counts=_ptr(i)) != 0
    assert call(B=65536) != 0 and call(S=0) != 0 and call(S=17) != 0 and call(min_views=3) != 0 and call(iters=17) != 0
    torch.cuda.synchronize()
    k = (5.0, 5.0, 1.5, 1.5)
    with pytest.raises(RuntimeError):
        transforms.multiview_depth(acc, alive.cpu(), poses, slots, k)
    with pytest.raises(RuntimeError):
        transforms.multiview_depth(acc, alive, poses.cpu(), slots, k)
    with pytest.raises(RuntimeError):
        transforms.multiview_depth(acc, alive, poses, slots.cpu(), k)
    with pytest.raises(RuntimeError):
        transforms.multiview_depth(acc, alive, poses, slots, k, depth_init=init.cpu())
    with pytest.raises(RuntimeError, match="max_rel_sigma"):
        transforms.multiview_depth(acc, alive, poses, slots, k, max_rel_sigma=0.0)


# ------------------------------------------------------------------ FlowTrack(history=K)
def _pairs(H, W, B, steps, seed):
    """Seeded pair flows [steps,B,2,H,W] float32 and relative poses [steps,B,4,4] float64 (two_view_ref.scene per step)."""
    flows, rels = [], []
    for k in range(steps):
        flow, rel, calib, _ = pair_scene(H, W, seed + 17 * k, B, 0.5)
        flows.append(flow)
        rels.append(pose_mats(rel))
    return np.stack(flows), np.stack(rels), calib


@pytest.mark.parametrize("K", [1, 3])
def test_flow_track_history_ring(K):
    """K + 3 extend calls at 47 x 154, B = 2: the ring wraps. multiview() equals transforms.multiview_depth on banks assembled by
    hand from the acc, alive and pose rows recorded after each of the last K steps; a track with history=0 fed the same calls has
    the same acc, alive, depth and counts, bit for bit; before the ring is full multiview() uses the steps there are; start()
    empties it."""
    H, W, B = 47, 154, 2
    flows, rels, calib = _pairs(H, W, B, K + 3, 21)
    ring, plain = FlowTrack((H, W), calib, DEV, batch=B, history=K), FlowTrack((H, W), calib, DEV, batch=B)
    assert plain.hist_acc is None and plain.history == 0 and tuple(ring.hist_acc.shape) == (K * B, 2, H, W)
    with pytest.raises(RuntimeError, match="history"):
        plain.multiview()
    with pytest.raises(RuntimeError, match="no step"):
        ring.multiview()
    options = dict(min_views=1, max_rel_sigma=4.0)
    rec = []
    for k in range(K + 3):
        for t in (ring, plain):
            t.extend(_dev(flows[k]), torch.from_numpy(rels[k]))
        for name in ("acc", "alive", "depth", "counts"):
            assert torch.equal(getattr(ring, name), getattr(plain, name)), (k, name)
        rec.append((ring.acc.clone(), ring.alive.clone(), ring.pose[:, :3, :].reshape(B, 12).float().to(DEV)))
        last = rec[-K:]
        S = len(last)
        by_hand = transforms.multiview_depth(torch.cat([r[0] for r in last]), torch.cat([r[1] for r in last]),
                                             torch.cat([r[2] for r in last]), [[s * B + b for s in range(S)] for b in range(B)], calib,
                                             depth_init=ring.depth, **options)
        got = ring.multiview(**options)
        assert all(torch.equal(a, b) for a, b in zip(got, by_hand)), k
        assert ring.history_slots().shape == (B, S)
    assert int(got[3][:, 2].min()) > 0                                  # and it is not an empty statement
    ring.start()
    assert ring.steps == 0
    with pytest.raises(RuntimeError, match="no step"):
        ring.multiview()
    ring.extend(_dev(flows[0]), torch.from_numpy(rels[0]))
    assert tuple(ring.history_slots().shape) == (B, 1) and ring.history_slots()[:, 0].tolist() == [0, 1]
    with pytest.raises(ValueError):
        FlowTrack((H, W), calib, DEV, history=17)
