"""Voxel map, host form (no GPU): atdn_voxel_*_host through voxel_map.VoxelMap and transforms.voxel_map on CPU tensors against
the NumPy restatement of the rule (tests/voxel_map_ref.py) — every bit of keys, points, colours, counts and counters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_map_ref as V  # noqa: E402
from voxel_map_ref import CASES, same_cloud  # noqa: E402


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _np(cloud):
    return tuple(None if t is None else t.cpu().numpy() for t in cloud)


def _host(s, images=None, mask=None, indices=None, stride=1, min_count=1, capacity=64, **grid):
    m = VoxelMap("cpu", capacity=capacity, **grid)
    counts = m.integrate(_t(s["depth"]), _t(s["poses"]), s["calib"], images=_t(images), mask=_t(mask), indices=indices, stride=stride)
    return _np(m.extract(min_count)), counts, m


@pytest.mark.parametrize("name,H,W,K,seed", CASES, ids=[c[0] for c in CASES])
def test_host_form_equals_the_restatement(name, H, W, K, seed):
    """5 x 7 with K = 1, 9 x 33 with K = 3, 47 x 154 with K = 2; stride 1, 2, 3, with and without images and mask; the cameras
    stand at negative world coordinates (the floor below zero); NaN, +-inf, 0, negative depths and min_z and max_z hit exactly
    in every frame; min_count 1 and 3."""
    s = V.scene(H, W, K, seed)
    assert (s["poses"][:, [3, 7, 11]] < 0).any()
    for stride, colored, masked in V.variants():
        im, mk = (s["images"] if colored else None), (s["mask"] if masked else None)
        for min_count in (1, 3):
            want, wc = V.reference(s["depth"], s["poses"], s["calib"], im, mk, stride=stride, min_count=min_count)
            got, gc, m = _host(s, im, mk, stride=stride, min_count=min_count)
            tag = (name, stride, colored, masked, min_count)
            assert gc == wc, (tag, gc, wc)
            assert same_cloud(got, want), tag
            assert gc["candidates"] == gc["inserted"] + gc["outside"] + gc["dropped"] and gc["dropped"] == 0
            assert (got[1] is None) == (not colored)
        assert (got[3][:-1] < got[3][1:]).all()                        # ascending keys
    # the exact min_z and max_z pixels are candidates, the specials are not
    one, _ = V.reference(s["depth"][:1, :1, :min(W, 7)], s["poses"][:1], s["calib"])
    assert one[2].sum() == min(W, 7) - 5


def test_voxel_faces_and_the_ends_of_the_key_range():
    """Points exactly on voxel faces (g an integer, also a negative one: q = 0 in the voxel above), at g = -2^20 (inside) and
    just below 2^20 (inside), at 2^20 and just below -2^20 (outside); a tiny negative g whose fraction rounds to 1 (q = 65536)."""
    gx = [0.0, 1.0, -1.0, -3.0, 2.5, -2.5, -1048576.0, 1048575.875, 1048576.0, -1048576.125, 7.0, -1e-30]
    gz = [0.0, -2.0, 5.0, -1048576.0, 1048575.875, 3.0, 1.0, 2.0, 0.0, 0.0, 1048576.0, 4.0]
    s = V.axis_scene(gx, gz=gz)
    grid = dict(min_z=0.5, max_z=40.0)
    want, wc = V.reference(s["depth"], s["poses"], s["calib"], **grid)
    got, gc, _ = _host(s, **grid)
    assert gc == wc and same_cloud(got, want)
    assert gc["outside"] == 3 and gc["inserted"] == 9 and gc["voxels"] == 9
    kx = (got[3] >> 42) - 1048576
    assert sorted(kx.tolist()) == [-1048576, -3, -3, -1, -1, 0, 1, 2, 1048575]
    ref = V.RefMap(**dict(V.DEFAULTS, **grid))
    ref.integrate(s["depth"], s["poses"], s["calib"])
    assert max(e[1] for e in ref.table.values()) == 65536              # the -1e-30 point
    assert sum(1 for e in ref.table.values() if e[1] == 0 and e[3] == 0) >= 3


def test_probing_wraps_around_the_end_of_the_table():
    """Capacity 64 and 30 voxels whose home slots are the last eight: the probe runs over the end of the table and on from
    slot 0 (no growth: 2 * 30 <= 64)."""
    s = V.clustered_scene()
    want, wc = V.reference(s["depth"], s["poses"], s["calib"])
    got, gc, m = _host(s, capacity=64)
    assert m.capacity == 64 and gc == wc and gc["voxels"] == 30 and same_cloud(got, want)
    used = np.flatnonzero(m.table.numpy()[8::8] != -1)
    assert len(used) == 30 and (used >= 56).sum() >= 1 and (used < 30).sum() >= 22


def test_nan_and_infinity_in_one_pose_leave_the_other_keyframes_alone():
    s = V.scene(9, 33, 3, 5)
    clean, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], indices=[0, 2])
    poses = s["poses"].copy()
    poses[1, 3] = np.nan
    poses[1, 5] = np.inf
    bad = dict(s, poses=poses)
    want, wc = V.reference(s["depth"], poses, s["calib"], s["images"])
    got, gc, _ = _host(bad, s["images"])
    assert gc == wc and same_cloud(got, want) and same_cloud(got, clean)
    assert gc["outside"] > 0 and gc["candidates"] == gc["inserted"] + gc["outside"]


def test_indices_with_a_repeat_and_outside_the_bank():
    s = V.scene(9, 33, 3, 6)
    idx = [2, 0, 2, 7, -1]
    mask = (np.random.RandomState(3).uniform(size=(5, 9, 33)) < 0.8).astype(np.uint8)
    want, wc = V.reference(s["depth"], s["poses"], s["calib"], s["images"], mask, indices=idx)
    got, gc, _ = _host(s, s["images"], mask, indices=idx)
    assert gc == wc and same_cloud(got, want)
    twice, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], indices=[2, 2])
    once, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], indices=[2])
    assert np.array_equal(twice[2], 2 * once[2]) and same_cloud((twice[0], twice[1], once[2], twice[3]), once)


def test_split_invariance_and_growth():
    """K keyframes in one call equal one call per keyframe in any order; a table that starts with 2 slots and grows by rehash
    equals one that was large from the start, counters included."""
    s = V.scene(9, 33, 3, 7)
    whole, wc, _ = _host(s, s["images"], capacity=1 << 12)
    assert same_cloud(whole, V.reference(s["depth"], s["poses"], s["calib"], s["images"])[0])
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        m = VoxelMap("cpu", capacity=2)
        for k in order:
            m.integrate(_t(s["depth"]), _t(s["poses"]), s["calib"], images=_t(s["images"]), indices=[k])
        assert m.counts == wc and same_cloud(_np(m.extract()), whole), order
        assert m.capacity >= 2 * m.counts["voxels"]


def test_raw_entry_points_undersized_table_and_max_out():
    """Through the C ABI: a table of 8 slots for more voxels drops points, counts them, marks exactly them in `pending`, and holds
    every key once; re-integrating `pending` into a grown table gives the large table's bits. max_out below the number of
    voxels: the number is reported and nothing is written past max_out."""
    L = _lib.lib()
    s = V.scene(9, 33, 2, 8)
    K, H, W = s["depth"].shape
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    grid = (0.25, 0.0, 0.0, 0.0, 0.5, 40.0)

    def table(cap):
        t = np.zeros(int(L.atdn_voxel_table_bytes(cap)) // 8, dtype=np.uint64)
        _lib.check(L.atdn_voxel_clear_host(p(t), cap))
        return t

    def integrate(t, cap, mask, retry, pending):
        _lib.check(L.atdn_voxel_integrate_host(p(s["depth"]), p(s["poses"]), p(s["images"]), None if mask is None else p(mask), None,
                                               K, K, H, W, *s["calib"], 1, *grid, retry, p(t), cap, p(pending)))

    small, pending = table(8), np.full((K, H, W), 7, dtype=np.uint8)
    integrate(small, 8, None, 0, pending)
    cnt = small[:5].astype(np.int64).tolist()
    assert cnt[0] == cnt[1] + cnt[2] + cnt[3] and cnt[3] > 0 and cnt[4] == 8
    assert int(pending.sum()) == cnt[3] and set(np.unique(pending)) <= {0, 1}
    keys = small[8::8]
    assert len(set(keys.tolist())) == 8 and int(small[9::8].sum()) == cnt[1]
    big = table(1 << 10)
    _lib.check(L.atdn_voxel_rehash_host(p(small), 8, p(big), 1 << 10))
    again = np.full((K, H, W), 7, dtype=np.uint8)
    integrate(big, 1 << 10, pending, 1, again)
    assert not again.any()
    direct = table(1 << 10)
    integrate(direct, 1 << 10, None, 0, again)
    assert big[:8].tolist() == direct[:8].tolist()

    def extract(t, cap, max_out):
        out = (np.full((max_out + 1, 3), -7, np.float32), np.full((max_out + 1, 3), 7, np.uint8), np.full(max_out + 1, -7, np.int32),
               np.full(max_out + 1, -7, np.int64))
        found = np.zeros(1, dtype=np.int64)
        _lib.check(L.atdn_voxel_extract_host(p(t), cap, 1, 0.25, 0.0, 0.0, 0.0, max_out, *(p(o) for o in out), p(found)))
        return out, int(found[0])

    n = int(direct[4])
    a, fa = extract(big, 1 << 10, n)
    b, fb = extract(direct, 1 << 10, n)
    assert fa == fb == n and all(np.array_equal(x, y) for x, y in zip(a, b))
    want, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"])
    assert same_cloud(tuple(x[:n] for x in a), want)
    c, fc = extract(direct, 1 << 10, 5)
    assert fc == n and all(np.array_equal(x[:5], y[:5]) for x, y in zip(c, b))
    assert (c[0][5] == -7).all() and (c[1][5] == 7).all() and c[2][5] == -7 and c[3][5] == -7


def test_closed_form_wall_and_ground():
    """A fronto-parallel wall at z = 10.1 and a ground plane at y = 1.65 seen from three level cameras with exact depths: a
    point's coordinate along the normal is o + (k + (mean q + 0.5)/65536) voxel with every q within one step of the plane's own
    fraction, so it lies within voxel/65536 of the plane — inside the issue's bound voxel/2 + voxel/65536. The float32 depth of a
    ground pixel carries a relative error of 2^-24, far below voxel/65536. The number of voxels equals the restatement's."""
    H, W, voxel = 24, 64, 0.25
    fx, fy, cx, cy = calib = (60.0, 60.0, 31.5, 8.0)
    ys = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    with np.errstate(all="ignore"):
        ground = np.where(ys - cy > 0, 1.65 * fy / (ys - cy), np.inf)
    poses = np.tile(V.IDENTITY, (3, 1))
    depth = np.zeros((3, H, W), dtype=np.float32)
    for k in range(3):
        poses[k, 3], poses[k, 11] = 0.5 * k - 0.7, 1.25 * k
        depth[k] = np.minimum(ground, 10.1 - 1.25 * k)
    is_wall = ground[None] > (10.1 - 1.25 * np.arange(3, dtype=np.float64))[:, None, None]
    for part, axis, level in ((is_wall, 2, 10.1), (~is_wall, 1, 1.65)):
        s = dict(depth=depth, poses=poses, calib=calib)
        got, gc, _ = _host(s, mask=part.astype(np.uint8), voxel=voxel)
        want, wc = V.reference(depth, poses, calib, mask=part.astype(np.uint8), voxel=voxel)
        assert gc["voxels"] == wc["voxels"] == len(got[0]) > 10 and same_cloud(got, want)
        err = np.abs(got[0][:, axis].astype(np.float64) - level)
        print("closed form: axis %d, %d voxels, max |error| %.3e, bound %.3e" % (axis, len(err), err.max(), voxel / 2 + voxel / 65536))
        assert err.max() <= voxel / 2 + voxel / 65536
        assert err.max() <= 2 * voxel / 65536                          # what the argument above gives for an axis-aligned plane


def test_save_ply_load_ply_round_trip(tmp_path):
    s = V.scene(9, 33, 3, 9)
    for colored in (True, False):
        m = VoxelMap("cpu", capacity=64)
        m.integrate(_t(s["depth"]), _t(s["poses"]), s["calib"], images=_t(s["images"]) if colored else None)
        path = str(tmp_path / ("c%d.ply" % colored))
        for min_count in (1, 3):
            n = m.save_ply(path, min_count=min_count)
            points, colors, counts, _ = m.extract(min_count)
            lp, lc, ln = VoxelMap.load_ply(path)
            assert n == len(lp) and torch.equal(lp.view(torch.int32), points.view(torch.int32)) and torch.equal(ln, counts)
            assert (lc is None and colors is None) if not colored else torch.equal(lc, colors)
        head = open(path, "rb").read(400).split(b"end_header\n")[0].decode().split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"]
        props = [h for h in head if h.startswith("property")]
        assert props == ["property float x", "property float y", "property float z"] + \
            (["property uchar red", "property uchar green", "property uchar blue"] if colored else []) + ["property int count"]
        assert os.path.getsize(path) == len(open(path, "rb").read().split(b"end_header\n")[0]) + 11 + n * (19 if colored else 16)


def test_functional_form_and_argument_errors():
    s = V.scene(9, 33, 2, 10)
    d, P, im = _t(s["depth"]), _t(s["poses"]), _t(s["images"])
    got = _np(transforms.voxel_map(d, P, s["calib"], images=im, stride=2, min_count=2, voxel=0.5, origin=(0.1, -0.2, 0.3)))
    want, _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], stride=2, min_count=2, voxel=0.5, origin=(0.1, -0.2, 0.3))
    assert same_cloud(got, want)
    for kw in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(capacity=48), dict(capacity=1), dict(origin=(0, 0))):
        with pytest.raises(ValueError):
            VoxelMap("cpu", **kw)
    m = VoxelMap("cpu", capacity=64)
    with pytest.raises(RuntimeError):
        m.integrate(d[0], P, s["calib"])                               # not a bank
    with pytest.raises(RuntimeError):
        m.integrate(d, P[:1], s["calib"])                              # one pose for two keyframes
    with pytest.raises(RuntimeError):
        m.integrate(d, P, s["calib"], images=im.float())               # colours must be uint8
    with pytest.raises(RuntimeError):
        m.integrate(d, P, s["calib"], mask=torch.ones(2, 9, 32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        m.integrate(d, P, s["calib"], stride=0)
    with pytest.raises(ValueError):
        m.extract(min_count=0)
    m.integrate(d, P, s["calib"], images=im)
    with pytest.raises(RuntimeError, match="coloured"):
        m.integrate(d, P, s["calib"])
    big = VoxelMap("cpu", capacity=64)
    big._points_bound = 2 ** 31 - 1 - 100
    with pytest.raises(RuntimeError, match="2\\^31"):
        big.integrate(d, P, s["calib"])
    # the C ABI's own guard
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = np.zeros(8 + 8 * 64, dtype=np.uint64)
    assert L.atdn_voxel_table_bytes(64) == 64 + 64 * 64 and L.atdn_voxel_table_bytes(48) == 0 and L.atdn_voxel_table_bytes(1) == 0
    assert L.atdn_voxel_clear_host(p(t), 48) != 0 and b"power of two" in L.atdn_last_error()
    assert L.atdn_voxel_clear_host(None, 64) != 0
    geom = (2, 2, 9, 33, *s["calib"])

    def call(depth=s["depth"], voxel=0.25, stride=1, table=t, cap=64, pending=None, geom=geom):
        return L.atdn_voxel_integrate_host(p(depth), p(s["poses"]), None, None, None, *geom, stride, voxel, 0.0, 0.0, 0.0, 0.5, 40.0, 0,
                                           p(table), cap, None if pending is None else p(pending))

    _lib.check(L.atdn_voxel_clear_host(p(t), 64))
    assert call() == 0
    assert call(voxel=0.0) != 0 and b"voxel" in L.atdn_last_error()
    assert call(stride=0) != 0 and b"stride" in L.atdn_last_error()
    assert call(cap=32 + 1) != 0
    assert call(geom=(2, 3, 9, 33, *s["calib"])) != 0 and b"K <= N" in L.atdn_last_error()
    assert call(pending=s["depth"].view(np.uint8).reshape(-1)) != 0 and b"overlaps" in L.atdn_last_error()
    assert call(table=t.view(np.uint8)[4:-4].view(np.uint64), cap=32) != 0 and b"aligned" in L.atdn_last_error()
    assert L.atdn_voxel_rehash_host(p(t), 64, p(t), 64) != 0 and b"overlap" in L.atdn_last_error()
    t2 = np.zeros(8 + 8 * 32, dtype=np.uint64)
    assert L.atdn_voxel_rehash_host(p(t), 64, p(t2), 32) != 0 and b"smaller" in L.atdn_last_error()
