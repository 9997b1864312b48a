"""Voxel map on the device: the kernels of atdn_voxel_clear / integrate / rehash / extract (voxel_map.VoxelMap and
transforms.voxel_map on device tensors, and the raw entry points) against the host form and the NumPy restatement of the rule
(tests/voxel_map_ref.py) — every bit of keys, points, colours, counts and counters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_map_ref as V  # noqa: E402
from voxel_map_ref import CASES, FULL_CASE, same_cloud  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = (0.25, 0.0, 0.0, 0.0, 0.5, 40.0)         # voxel, origin, min_z, max_z of the raw calls


def _t(a, dev=DEV):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


def _np(cloud):
    return tuple(None if t is None else t.cpu().numpy() for t in cloud)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(dev, s, images=None, mask=None, indices=None, stride=1, min_count=1, capacity=64, **grid):
    m = VoxelMap(dev, capacity=capacity, **grid)
    counts = m.integrate(_t(s["depth"], dev), _t(s["poses"], dev), s["calib"], images=_t(images, dev), mask=_t(mask, dev),
                         indices=indices, stride=stride)
    cloud = m.extract(min_count)
    assert all(t is None or t.device.type == torch.device(dev).type for t in cloud)
    return _np(cloud), counts, m


@pytest.mark.parametrize("name,H,W,K,seed", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_the_restatement_and_the_host_form(name, H, W, K, seed):
    """The case table of the host test (5 x 7 and 9 x 33: H W no multiple of 4 or 64; 47 x 154: 57 waves), every variant of
    stride, images and mask, min_count 1 and 3, the special depths in every frame."""
    s = V.scene(H, W, K, seed)
    for stride, colored, masked in V.variants():
        im, mk = (s["images"] if colored else None), (s["mask"] if masked else None)
        for min_count in (1, 3):
            tag = (name, stride, colored, masked, min_count)
            want, wc = V.reference(s["depth"], s["poses"], s["calib"], im, mk, stride=stride, min_count=min_count)
            got, gc, _ = _run(DEV, s, im, mk, stride=stride, min_count=min_count)
            assert gc == wc, (tag, gc, wc)
            assert same_cloud(got, want), tag
            host, hc, _ = _run("cpu", s, im, mk, stride=stride, min_count=min_count)
            assert hc == gc and same_cloud(got, host), tag


def _lane_scene(kind):
    """9 x 33 under the identity pose and a calibration with a long focal length, so the whole frame spans a metre at 30 m."""
    H, W = 9, 33
    calib = (1000.0, 1000.0, 16.0, 4.0)
    depth = np.full((1, H, W), 5.0, dtype=np.float32)
    if kind == "two":
        depth.reshape(-1)[1::2] = 30.0
    s = dict(depth=depth, poses=V.IDENTITY[None].copy(), calib=calib)
    grid = dict(voxel=16.0, origin=(-8.0, -8.0, 0.0)) if kind != "own" else dict(voxel=0.004, origin=(0.0, 0.0, 0.0))
    return s, grid


@pytest.mark.parametrize("kind,voxels", [("one", 1), ("two", 2), ("own", 297)])
def test_one_voxel_two_alternating_keys_and_a_voxel_per_pixel(kind, voxels):
    """Every lane of every wave with the same key (one round of the aggregation); two keys that alternate lane by lane; every
    pixel in a voxel of its own (64 rounds, every lane a leader)."""
    s, grid = _lane_scene(kind)
    im = np.random.RandomState(1).randint(0, 256, size=(1, 3, 9, 33)).astype(np.uint8)
    want, wc = V.reference(s["depth"], s["poses"], s["calib"], im, **grid)
    assert wc["voxels"] == voxels and wc["inserted"] == 297
    got, gc, _ = _run(DEV, s, im, capacity=1024, **grid)
    assert gc == wc and same_cloud(got, want)
    host, hc, _ = _run("cpu", s, im, capacity=1024, **grid)
    assert hc == gc and same_cloud(got, host)


def test_probing_wraps_around_the_end_of_the_table():
    """Capacity 64 and 30 voxels whose home slots are the last eight: the probe runs over the end of the table and on from
    slot 0. No growth (2 * 30 <= 64), so this is the table the kernel filled."""
    s = V.clustered_scene()
    want, wc = V.reference(s["depth"], s["poses"], s["calib"])
    got, gc, m = _run(DEV, s, capacity=64)
    assert m.capacity == 64 and gc == wc and gc["voxels"] == 30 and same_cloud(got, want)
    table = m.table.cpu().numpy()
    keys = table[8::8]
    used = np.flatnonzero(keys != -1)
    assert len(used) == 30 and len(set(keys[used].tolist())) == 30
    assert (used >= 56).sum() >= 1 and (used < 30).sum() >= 22         # at most 8 fit at the end: the others wrapped
    host, hc, _ = _run("cpu", s, capacity=64)
    assert hc == gc and same_cloud(got, host)


def test_growth_equals_a_table_that_was_large_from_the_start():
    s = V.scene(47, 154, 2, 11)
    a, ac, ma = _run(DEV, s, s["images"], capacity=1 << 16)
    assert ma.capacity == 1 << 16
    b, bc, mb = _run(DEV, s, s["images"], capacity=64)
    assert mb.capacity > 64 and ac == bc and same_cloud(a, b)
    # keyframe by keyframe into a small table: one rehash per call
    m = VoxelMap(DEV, capacity=64)
    for k in (1, 0):
        m.integrate(_t(s["depth"]), _t(s["poses"]), s["calib"], images=_t(s["images"]), indices=[k])
    assert m.counts == ac and same_cloud(_np(m.extract()), a)


def _raw(s, images=True):
    L = _lib.lib()
    K, H, W = s["depth"].shape
    d, P, im = _t(s["depth"]), _t(s["poses"]), (_t(s["images"]) if images else None)

    def table(cap):
        t = torch.empty(int(L.atdn_voxel_table_bytes(cap)) // 8, dtype=torch.int64, device=DEV)
        _lib.check(L.atdn_voxel_clear(_p(t), cap, _stream()))
        return t

    def integrate(t, cap, mask, retry, pending):
        _lib.check(L.atdn_voxel_integrate(_p(d), _p(P), _p(im), _p(mask), None, K, K, H, W, *s["calib"], 1, *GRID, retry, _p(t), cap,
                                          _p(pending), _stream()))

    def extract(t, cap, max_out, min_count=1):
        out = (torch.full((max_out + 1, 3), -7.0, device=DEV), torch.full((max_out + 1, 3), 7, dtype=torch.uint8, device=DEV),
               torch.full((max_out + 1,), -7, dtype=torch.int32, device=DEV), torch.full((max_out + 1,), -7, dtype=torch.int64, device=DEV))
        found = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        _lib.check(L.atdn_voxel_extract(_p(t), cap, min_count, *GRID[:4], max_out, _p(out[0]), _p(out[1] if images else None),
                                        _p(out[2]), _p(out[3]), _p(found), _stream()))
        return out, int(found.item())

    return L, table, integrate, extract


def _sorted(out, n):
    keys, order = torch.sort(out[3][:n])
    return (out[0][:n][order].cpu().numpy(), out[1][:n][order].cpu().numpy(), out[2][:n][order].cpu().numpy(), keys.cpu().numpy())


def test_undersized_table_pending_and_max_out():
    """Through the raw entry points. A table of 16 slots for hundreds of voxels: the call returns with candidates == inserted +
    outside + dropped, every key at most once in the table, n summing to `inserted`, and `pending` marking exactly the dropped
    pixels; rehashing into a large table and integrating `pending` with retry gives the large table's counters and cloud.
    max_out below the number of voxels: the number is reported, max_out entries are written — all of them real voxels — and
    nothing behind them."""
    s = V.scene(47, 154, 2, 12)
    K, H, W = s["depth"].shape
    L, table, integrate, extract = _raw(s)
    want, wc = V.reference(s["depth"], s["poses"], s["calib"], s["images"])
    small, pending = table(16), torch.full((K, H, W), 7, dtype=torch.uint8, device=DEV)
    integrate(small, 16, None, 0, pending)
    host = small.cpu().numpy()
    cnt = host[:5].tolist()
    print("undersized: counters", cnt)
    assert cnt[0] == cnt[1] + cnt[2] + cnt[3] and cnt[0] == wc["candidates"] and cnt[2] == wc["outside"]
    assert cnt[3] > 0 and cnt[4] == 16 and cnt[1] > 0
    keys = host[8::8]
    assert len(set(keys.tolist())) == 16 and -1 not in keys.tolist() and set(keys.tolist()) <= set(want[3].tolist())
    assert int(host[9::8].sum()) == cnt[1]
    pend = pending.cpu().numpy()
    assert set(np.unique(pend).tolist()) <= {0, 1} and int(pend.sum()) == cnt[3]
    big = table(1 << 14)
    _lib.check(L.atdn_voxel_rehash(_p(small), 16, _p(big), 1 << 14, _stream()))
    again = torch.full((K, H, W), 7, dtype=torch.uint8, device=DEV)
    integrate(big, 1 << 14, pending, 1, again)
    assert not again.any()
    assert big[:5].cpu().tolist() == [wc[c] for c in V.COUNTERS]
    n = wc["voxels"]
    out, found = extract(big, 1 << 14, n)
    assert found == n and same_cloud(_sorted(out, n), want)
    assert (out[0][n] == -7).all() and (out[1][n] == 7).all() and out[2][n] == -7 and out[3][n] == -7
    few, found = extract(big, 1 << 14, 5)
    assert found == n
    got = _sorted(few, 5)
    at = np.searchsorted(want[3], got[3])
    assert np.array_equal(want[3][at], got[3]) and len(set(got[3].tolist())) == 5
    assert same_cloud(got, tuple(w[at] for w in want))
    assert (few[0][5] == -7).all() and (few[1][5] == 7).all() and few[2][5] == -7 and few[3][5] == -7
    three, found3 = extract(big, 1 << 14, n, min_count=3)
    want3, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], min_count=3)
    assert found3 == len(want3[3]) and same_cloud(_sorted(three, found3), want3)


def test_guards_around_every_output_at_every_alignment():
    """Every input and output one element off its natural vector alignment (depth, poses, images, mask, indices, pending, points,
    colours, counts, keys), guard values around pending and the extraction's outputs, the table followed by guard words."""
    s = V.scene(9, 33, 3, 13)
    K, H, W = s["depth"].shape
    n = K * H * W
    L = _lib.lib()
    idx = [2, 0, 1]
    want, wc = V.reference(s["depth"], s["poses"], s["calib"], s["images"], s["mask"], indices=idx)

    def shifted(a, dtype, fill):
        flat = torch.full((a.size + 2,), fill, dtype=dtype, device=DEV)
        flat[1:1 + a.size] = _t(a).reshape(-1)
        return flat, flat[1:]

    _, d = shifted(s["depth"], torch.float32, 1.0)
    _, P = shifted(s["poses"], torch.float32, 1.0)
    _, im = shifted(s["images"], torch.uint8, 9)
    _, mk = shifted(s["mask"], torch.uint8, 1)
    _, ix = shifted(np.array(idx, dtype=np.int32), torch.int32, 0)
    cap = 1 << 12
    words = int(L.atdn_voxel_table_bytes(cap)) // 8
    tbuf = torch.full((words + 4,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
    pend = torch.full((n + 2,), 7, dtype=torch.uint8, device=DEV)
    _lib.check(L.atdn_voxel_clear(_p(tbuf[2:]), cap, _stream()))
    _lib.check(L.atdn_voxel_integrate(_p(d), _p(P), _p(im), _p(mk), _p(ix), K, K, H, W, *s["calib"], 1, *GRID, 0, _p(tbuf[2:]), cap,
                                      _p(pend[1:]), _stream()))
    assert tbuf[:2].tolist() == [0x5A5A5A5A] * 2 and tbuf[-2:].tolist() == [0x5A5A5A5A] * 2
    assert pend[0] == 7 and pend[-1] == 7 and not pend[1:-1].any()
    assert tbuf[2:7].tolist() == [wc[c] for c in V.COUNTERS]
    M = wc["voxels"]
    pts = torch.full((3 * M + 2,), -7.0, device=DEV)
    col = torch.full((3 * M + 2,), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.full((M + 2,), -7, dtype=torch.int32, device=DEV)
    keys = torch.full((M + 2,), -7, dtype=torch.int64, device=DEV)
    found = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    _lib.check(L.atdn_voxel_extract(_p(tbuf[2:]), cap, 1, *GRID[:4], M, _p(pts[1:]), _p(col[1:]), _p(cnt[1:]), _p(keys[1:]),
                                    _p(found[1:]), _stream()))
    assert found.tolist() == [-7, M, -7]
    for buf, g in ((pts, -7.0), (col, 7), (cnt, -7), (keys, -7)):
        assert buf[0] == g and buf[-1] == g
    out = (pts[1:-1].view(M, 3), col[1:-1].view(M, 3), cnt[1:-1], keys[1:-1])
    assert same_cloud(_sorted(out, M), want)
    # the guard refuses overlapping and misaligned buffers before anything is launched
    assert L.atdn_voxel_integrate(_p(d), _p(P), _p(im), _p(mk), _p(ix), K, K, H, W, *s["calib"], 1, *GRID, 0, _p(tbuf[2:]), cap,
                                  _p(mk), _stream()) != 0 and b"overlaps" in L.atdn_last_error()
    assert L.atdn_voxel_clear(C.c_void_p(tbuf.data_ptr() + 4), cap, _stream()) != 0 and b"aligned" in L.atdn_last_error()
    assert L.atdn_voxel_rehash(_p(tbuf[2:]), cap, _p(tbuf[2:]), cap, _stream()) != 0 and b"overlap" in L.atdn_last_error()


@pytest.fixture(scope="module")
def full_size():
    _, H, W, K, seed = FULL_CASE
    s = V.scene(H, W, K, seed)
    host, hc, _ = _run("cpu", s, s["images"], capacity=1 << 21)
    return s, host, hc


def test_full_size_two_calls_streams_and_graph(full_size):
    """376 x 1232, K = 2 against the host form: 3619 workgroup chunks over 2048 workgroups (two trips of the loop, a ragged
    last one). The same bits on a second call, on a side stream, and from a captured graph of clear, integrate and extract
    replayed twice — a capture fails on any host synchronisation, so the replay shows the three calls have none."""
    s, host, hc = full_size
    a, ac, m = _run(DEV, s, s["images"], capacity=1 << 21)
    assert m.capacity == 1 << 21 and ac == hc and same_cloud(a, host)
    assert ac["voxels"] > 10000 and ac["dropped"] == 0
    b, bc, _ = _run(DEV, s, s["images"], capacity=1 << 21)
    assert bc == ac and same_cloud(a, b)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c, cc, _ = _run(DEV, s, s["images"], capacity=1 << 21)
    side.synchronize()
    assert cc == ac and same_cloud(a, c)
    L = _lib.lib()
    K, H, W = s["depth"].shape
    d, P, im = _t(s["depth"]), _t(s["poses"]), _t(s["images"])
    cap, M = 1 << 21, ac["voxels"]
    table = torch.empty(int(L.atdn_voxel_table_bytes(cap)) // 8, dtype=torch.int64, device=DEV)
    out = (torch.empty((M, 3), device=DEV), torch.empty((M, 3), dtype=torch.uint8, device=DEV),
           torch.empty((M,), dtype=torch.int32, device=DEV), torch.empty((M,), dtype=torch.int64, device=DEV))
    found = torch.empty((1,), dtype=torch.int64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(L.atdn_voxel_clear(_p(table), cap, _stream()))
        _lib.check(L.atdn_voxel_integrate(_p(d), _p(P), _p(im), None, None, K, K, H, W, *s["calib"], 1, *GRID, 0, _p(table), cap, None,
                                          _stream()))
        _lib.check(L.atdn_voxel_extract(_p(table), cap, 1, *GRID[:4], M, *(_p(o) for o in out), _p(found), _stream()))
    for fill in (0, -1):
        table.fill_(fill)
        found.fill_(fill)
        for o in out:
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert int(found.item()) == M and table[:5].tolist() == [ac[c] for c in V.COUNTERS], fill
        assert same_cloud(_sorted(out, M), a), fill
