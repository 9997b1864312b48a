"""Keyframe depth fusion on the GPU: the kernel (atdn_depth_fuse, csrc/depth_fusion.hip) against the NumPy float64 restatement of
the rule (tests/depth_fusion_ref.py) and against the library's host form — every fused bit, every views byte and every count,
exactly (the scenes keep every decision at least 1e-9 from its threshold, asserted on the helper alone)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_fusion_ref import CASES, FULL_CASE, all_sources, check_case, check_reference, scene  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _gpu(bank, poses, targets, sources, calib, **kw):
    f, v, c = transforms.fuse_depths(_dev(bank), _dev(poses), targets, sources, calib, **kw)
    torch.cuda.synchronize()
    assert f.is_cuda and v.is_cuda and c.is_cuda and f.dtype == torch.float32 and v.dtype == torch.uint8 and c.dtype == torch.int32
    return f.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()


def _host(bank, poses, targets, sources, calib, **kw):
    f, v, c = transforms.fuse_depths(torch.from_numpy(np.ascontiguousarray(bank)), torch.from_numpy(np.ascontiguousarray(poses)),
                                     targets, sources, calib, **kw)
    return f.numpy(), v.numpy(), c.numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same(got, want):
    return _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def _check(bank, poses, targets, sources, calib, want, tag="", **kw):
    """Kernel == helper == host form; returns the kernel's outputs."""
    got = _gpu(bank, poses, targets, sources, calib, **kw)
    assert _same(got, want), tag
    assert _same(got, _host(bank, poses, targets, sources, calib, **kw)), tag
    return got


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, N = 5 scene, targets 1 and 3 with all other views as sources, and its reference, computed once."""
    _, H, W, N, seed, mv = FULL_CASE
    bank, poses, calib, _ = scene(H, W, N, seed)
    targets, sources = all_sources(N)
    targets, sources = targets[[1, 3]], sources[[1, 3]]
    return (bank, poses, calib, targets, sources) + check_reference(bank, poses, targets, sources, calib, min_views=mv)


@pytest.mark.parametrize("average", [True, False], ids=["average", "plain"])
@pytest.mark.parametrize("name, H, W, N, seed, min_views", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_helper_and_the_host_form(name, H, W, N, seed, min_views, average):
    """All N targets in one launch. 5 x 7 (one ragged workgroup); 9 x 33 (H * W = 297 is odd: the planes of b >= 1 sit off the
    vector grids of fused and of views, so the anchor offset and the scalar paths differ per b); 8 x 16 (everything aligned, no
    tail); 47 x 154 (8 workgroups, H * W = 2 mod 4)."""
    bank, poses, calib, _, targets, sources, fused, views, counts = check_case(H, W, N, seed, min_views, average)
    _check(bank, poses, targets, sources, calib, (fused, views, counts), tag=name, min_views=min_views, average=average)
    for b in (0, N - 1):                                           # a target alone; index tensors on the device
        f, v, c = transforms.fuse_depths(_dev(bank), _dev(poses).view(N, 3, 4), _dev(targets[b:b + 1]), _dev(sources[b:b + 1]), calib,
                                         min_views=min_views, average=average)
        assert _same((f.cpu().numpy(), v.cpu().numpy(), c.cpu().numpy()), (fused[b:b + 1], views[b:b + 1], counts[b:b + 1]))


@pytest.mark.parametrize("S", [0, 1, 3, 8, 20])
def test_source_counts(S):
    """S = 0 (no pass), 1, 3, 8 and S = 20 with repeated sources and empty slots: more than one chunk of the source loop, the
    second one partly filled. 9 x 33, N = 4; the lists cycle through the other views."""
    name, H, W, N, seed, mv = CASES[1]
    bank, poses, calib, _ = scene(H, W, N, seed)
    targets = np.arange(N, dtype=np.int32)
    sources = np.array([[(i + 1 + s % (N - 1)) % N for s in range(S)] for i in range(N)], dtype=np.int32).reshape(N, S)
    if S == 20:
        sources[:, 5], sources[:, 17], sources[1, 16] = -1, N + 2, 1
    strict = S >= 3
    want = check_reference(bank, poses, targets, sources, calib, strict=strict, min_views=min(mv, max(S, 1)))
    got = _check(bank, poses, targets, sources, calib, want, tag=str(S), min_views=min(mv, max(S, 1)))
    if S == 0:
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2][:, 1:] == 0).all() and (got[2][:, 0] > 0).all()
    if S == 20:
        assert got[1].max() > 8


def test_target_outside_the_bank():
    name, H, W, N, seed, mv = CASES[1]
    bank, poses, calib, _ = scene(H, W, N, seed)
    targets, sources = [N, 1, -1], [[0, 1, 2], [0, 2, 3], [0, 1, 2]]
    want = check_reference(bank, poses, targets, sources, calib, strict=False)
    got = _check(bank, poses, targets, sources, calib, want)
    assert (got[0][[0, 2]] == 0).all() and (got[1][[0, 2]] == 0).all() and (got[2][[0, 2]] == 0).all() and got[2][1, 2] > 0


def test_kernel_outputs_are_fully_written():
    """Pre-filled outputs with guard values around them; bank, fused and views each at every offset 0..3 of its vector grid
    (the others at 0) through the raw entry point: everything is written, nothing else is, and the counts are reset. 8 x 16
    (aligned planes: the shifts alone decide) and 9 x 33 (odd planes)."""
    L = _lib.lib()
    for name, H, W, N, seed, mv in (CASES[2], CASES[1]):
        bank, poses, calib, _, targets, sources, fused, views, counts = check_case(H, W, N, seed, mv)
        n, B, S = H * W, N, sources.shape[1]
        dposes, dt, ds = _dev(poses), _dev(targets), _dev(sources)
        for which in ("bank", "fused", "views"):
            for shift in (0, 1, 2, 3):
                sb, sf, sv = (shift if which == w else 0 for w in ("bank", "fused", "views"))
                bbuf = torch.zeros(N * n + 8, dtype=torch.float32, device=DEV)
                bbuf[sb:sb + N * n] = _dev(bank).reshape(-1)
                fbuf = torch.full((B * n + 32,), -7.0, dtype=torch.float32, device=DEV)
                vbuf = torch.full((B * n + 32,), 99, dtype=torch.uint8, device=DEV)
                cnt = torch.full((3 * B + 2,), -7, dtype=torch.int32, device=DEV)
                _lib.check(L.atdn_depth_fuse(_ptr(bbuf[sb:]), _ptr(dposes), _ptr(dt), _ptr(ds), N, B, S, H, W, *calib, 1.0, 0.01, mv,
                                             0.1, 1, _ptr(fbuf[16 + sf:]), _ptr(vbuf[16 + sv:]), _ptr(cnt[1:]),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
                torch.cuda.synchronize()
                tag = (name, which, shift)
                f, v = fbuf.cpu().numpy(), vbuf.cpu().numpy()
                assert (f[:16 + sf] == -7.0).all() and (f[16 + sf + B * n:] == -7.0).all(), tag
                assert _same_bits(f[16 + sf:16 + sf + B * n].reshape(B, 1, H, W), fused), tag
                assert (v[:16 + sv] == 99).all() and (v[16 + sv + B * n:] == 99).all(), tag
                assert np.array_equal(v[16 + sv:16 + sv + B * n].reshape(B, H, W), views), tag
                assert cnt.cpu().tolist() == [-7] + counts.reshape(-1).tolist() + [-7], tag


def test_kernel_at_full_size_streams_and_graph(full_size):
    """376 x 1232, N = 5, B = 2: 453 workgroups per target. The same bits as the helper and the host form, on a second call, on a
    side stream, and from a captured graph (one linear chain: the memset of the counts, then the kernel) replayed twice over
    pre-filled outputs."""
    bank, poses, calib, targets, sources, fused, views, counts = full_size
    _, H, W, N, _, mv = FULL_CASE
    dbank, dposes, dt, ds = _dev(bank), _dev(poses), _dev(targets), _dev(sources)
    f1, v1, c1 = transforms.fuse_depths(dbank, dposes, dt, ds, calib, min_views=mv)
    f2, v2, c2 = transforms.fuse_depths(dbank, dposes, dt, ds, calib, min_views=mv)
    torch.cuda.synchronize()
    assert _same((f1.cpu().numpy(), v1.cpu().numpy(), c1.cpu().numpy()), (fused, views, counts))
    assert torch.equal(f1, f2) and torch.equal(v1, v2) and torch.equal(c1, c2)
    assert _same(_host(bank, poses, targets, sources, calib, min_views=mv), (fused, views, counts))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f3, v3, c3 = transforms.fuse_depths(dbank, dposes, dt, ds, calib, min_views=mv)
    side.synchronize()
    assert torch.equal(f3, f1) and torch.equal(v3, v1) and torch.equal(c3, c1)
    # captured: static output buffers, pre-filled before every replay so that unwritten values and un-reset counts would show
    f = torch.empty((2, 1, H, W), dtype=torch.float32, device=DEV)
    v = torch.empty((2, H, W), dtype=torch.uint8, device=DEV)
    c = torch.empty((2, 3), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_lib.lib().atdn_depth_fuse(_ptr(dbank), _ptr(dposes), _ptr(dt), _ptr(ds), N, 2, sources.shape[1], H, W, *calib,
                                              1.0, 0.01, mv, 0.1, 1, _ptr(f), _ptr(v), _ptr(c),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (-3.0, 1e30):
        f.fill_(fill)
        v.fill_(77)
        c.fill_(123456)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(f, f1) and torch.equal(v, v1) and torch.equal(c, c1), fill


def test_kernel_argument_errors():
    """On the device path the overlap and null cases return non-zero without launching; mixed devices raise."""
    L = _lib.lib()
    N, B, S, H, W = 3, 2, 2, 4, 4
    bank = torch.ones(N, H, W, device=DEV)
    poses = torch.eye(4, device=DEV)[:3].reshape(1, 12).repeat(N, 1).contiguous()
    t = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    s = torch.tensor([[1, 2], [0, 2]], dtype=torch.int32, device=DEV)
    f = torch.zeros(B, 1, H, W, device=DEV)
    v = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    c = torch.zeros(B, 3, dtype=torch.int32, device=DEV)
    good = dict(bank=_ptr(bank), poses=_ptr(poses), targets=_ptr(t), sources=_ptr(s), fused=_ptr(f), views=_ptr(v), counts=_ptr(c))

    def call(S=S, B=B, **kw):
        a = dict(good, **kw)
        return L.atdn_depth_fuse(a["bank"], a["poses"], a["targets"], a["sources"], N, B, S, H, W, 5.0, 5.0, 1.5, 1.5, 1.0, 0.01, 1,
                                 0.1, 1, a["fused"], a["views"], a["counts"], None)

    assert call() == 0
    for name in good:
        assert call(**{name: None}) != 0, name
        assert b"null" in L.atdn_last_error()
    assert call(sources=None, S=0) == 0
    assert call(fused=_ptr(bank)) != 0 and b"overlap" in L.atdn_last_error()          # in place into the bank
    assert call(fused=C.c_void_p(bank.data_ptr() + 4 * H * W * (N - 1)), B=1) != 0 and b"overlap" in L.atdn_last_error()
    assert call(views=_ptr(bank)) != 0 and call(counts=_ptr(poses)) != 0 and call(counts=_ptr(t)) != 0
    assert call(views=_ptr(f)) != 0 and call(counts=_ptr(f)) != 0 and b"overlap" in L.atdn_last_error()
    assert call(B=65536) != 0 and call(S=256) != 0
    torch.cuda.synchronize()
    k = (5.0, 5.0, 1.5, 1.5)
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(bank, poses.cpu(), [0], [[1]], k)                       # the poses on the host
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(bank, poses, t.cpu(), s, k)                             # the targets on the host
    with pytest.raises(RuntimeError):
        transforms.fuse_depths(bank.cpu(), poses.cpu(), [0, 1], s, k)                  # the sources on the device
    with pytest.raises(RuntimeError, match="min_z"):
        transforms.fuse_depths(bank, poses, t, s, k, min_z=0.0)
