"""Visibility votes and carving on the device: the kernels of atdn_voxel_votes and atdn_voxel_remove (transforms.visibility_votes,
VoxelMap.votes / remove / carve, KeyframeMap.carve and the raw entry points) against the NumPy restatement of the rule
(tests/carve_ref.py) and the host form — every bit. The shared checks are in tests/carve_cases.py; test_carve_host.py runs them
on the host form and shows the properties' inputs on the CPU first."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.keyframe_map import KeyframeMap
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carve_cases as X  # noqa: E402
import carve_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HAND = R.hand_cases()


def _t(a, dev=DEV):
    return X.t(a, dev)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- 1. the shared checks
@pytest.mark.parametrize("name,H,W,K,seed", R.CASES, ids=[c[0] for c in R.CASES])
def test_kernel_equals_the_restatement(name, H, W, K, seed):
    print("votes (in view, support, free) summed over radii and index lists:", X.check_house_case(DEV, H, W, K, seed).tolist())


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_placed_points(case):
    X.check_hand_case(DEV, case)


def test_nan_and_infinity_in_a_point_a_pose_and_a_depth_pixel():
    X.check_nan_and_infinity(DEV)


def test_index_list_with_a_repeat_and_entries_outside_the_bank():
    X.check_index_lists(DEV)


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65])
def test_point_counts_around_a_wave(M):
    X.check_point_counts(DEV, M)


def test_keyframe_counts_around_the_camera_chunk():
    X.check_camera_chunks(DEV)


def test_split_invariance():
    X.check_split_invariance(DEV)


def test_removal_on_a_table_whose_probe_chains_wrap():
    X.check_removal(DEV)


def test_carve_report_equals_the_restatement():
    X.check_carve_report(DEV)


def test_wall_and_floater():
    X.check_wall(DEV)


def test_ground_plane_at_a_grazing_angle_never_carves_itself():
    X.check_ground(DEV)


# ---------------------------------------------------------------------------------------------------- 2. guards
def _raw_votes(L, d, s, shape, votes, accumulate=0, thresholds=(0.5, 40.0, 0.05, 0.25, 1)):
    N, K, H, W = shape
    return L.atdn_voxel_votes(_p(d["points"]), d["M"], _p(d["depth"]), _p(d["poses"]), _p(d.get("indices")), N, K, H, W, *s["calib"],
                              *thresholds, accumulate, _p(votes), _stream())


def test_guards_around_the_votes_with_every_buffer_off_its_grid():
    """Every input one element off its allocation's start, votes at an odd int32, guard values before and behind it; then the
    refusals: overlapping and misaligned buffers, before anything is launched."""
    s = R.cloud_scene(9, 33, 3, 13)
    N, (H, W) = 3, s["depth"].shape[1:]
    M = len(s["points"])
    L = _lib.lib()
    ix = [2, 0, 1, 1]
    want = R.votes(s["points"], s["depth"], s["poses"], s["calib"], ix)

    def shifted(a, dtype, fill):
        flat = torch.full((a.size + 2,), fill, dtype=dtype, device=DEV)
        flat[1:1 + a.size] = _t(a).reshape(-1)
        return flat[1:]

    d = dict(points=shifted(s["points"], torch.float32, 1.0), depth=shifted(s["depth"], torch.float32, 3.0),
             poses=shifted(s["poses"], torch.float32, 1.0), indices=shifted(np.array(ix, dtype=np.int32), torch.int32, 0), M=M)
    buf = torch.full((3 * M + 2,), -7, dtype=torch.int32, device=DEV)
    out = buf[1:1 + 3 * M]
    for fill in (0, -1):                                                 # a second call into the same buffer
        out.fill_(fill)
        _lib.check(_raw_votes(L, d, s, (N, len(ix), H, W), out))
        assert buf[0] == -7 and buf[-1] == -7 and np.array_equal(out.view(M, 3).cpu().numpy(), want), fill
    _lib.check(_raw_votes(L, d, s, (N, len(ix), H, W), out, accumulate=1))
    assert buf[0] == -7 and buf[-1] == -7 and np.array_equal(out.view(M, 3).cpu().numpy(), 2 * want)
    assert _raw_votes(L, d, s, (N, len(ix), H, W), d["points"].view(torch.int32)) != 0 and b"overlaps" in L.atdn_last_error()
    assert _raw_votes(L, d, s, (N, len(ix), H, W), d["depth"].view(torch.int32)[5:]) != 0 and b"overlaps" in L.atdn_last_error()
    odd = C.c_void_p(out.data_ptr() + 2)
    assert L.atdn_voxel_votes(_p(d["points"]), M, _p(d["depth"]), _p(d["poses"]), None, N, N, H, W, *s["calib"], 0.5, 40.0, 0.05,
                              0.25, 1, 0, odd, _stream()) != 0 and b"aligned" in L.atdn_last_error()
    assert _raw_votes(L, d, s, (N, len(ix), H, W), out, thresholds=(0.5, 40.0, 0.05, 0.25, 9)) != 0
    assert b"radius" in L.atdn_last_error()
    torch.cuda.synchronize()
    assert buf[0] == -7 and buf[-1] == -7


def test_guards_around_the_removal():
    m, ref, _ = X.clustered_maps(DEV)
    L = _lib.lib()
    keys = ref.extract()[3]
    kbuf = torch.full((len(keys) + 2,), -1, dtype=torch.int64, device=DEV)
    kbuf[1:-1] = _t(keys)
    flags = torch.zeros(len(keys) + 9, dtype=torch.uint8, device=DEV)
    f = flags[3:3 + len(keys)]                                           # a byte plane off every vector alignment
    f[[1, 5, 29]] = torch.tensor([1, 255, 7], dtype=torch.uint8, device=DEV)
    flags[2], flags[3 + len(keys)] = 1, 1                                # flags next to the plane: not read
    rbuf = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    table_before = m.table.clone()
    _lib.check(L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kbuf[1:]), _p(f), len(keys), _p(rbuf[1:]), _stream()))
    assert rbuf.tolist() == [-7, 3, 3, 0, -7] == [-7] + R.remove(ref, keys, f.cpu().numpy()).tolist() + [-7]
    assert V.same_cloud(X._np(m.extract()), ref.extract())
    changed = (m.table != table_before).nonzero().reshape(-1).tolist()
    # three slots lost their n (their sums were 0: the points sit on voxel corners); no key word and no header word changed
    assert len(changed) == 3 and all(w >= 8 and (w - 8) % 8 == 1 for w in changed)
    _lib.check(L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kbuf[1:]), None, len(keys), _p(rbuf[1:]), _stream()))
    assert rbuf.tolist() == [-7, 27, 27, 3, -7] and len(m.extract()[3]) == 0
    _lib.check(L.atdn_voxel_remove(_p(m.table), m.capacity, None, None, 0, _p(rbuf[1:]), _stream()))
    assert rbuf.tolist() == [-7, 0, 0, 0, -7]
    assert L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kbuf[1:]), None, 3, _p(kbuf[2:]), _stream()) != 0
    assert b"overlap" in L.atdn_last_error()
    assert L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kbuf[1:]), None, 3, _p(m.table[3:]), _stream()) != 0
    assert b"overlap" in L.atdn_last_error()
    assert L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kbuf[1:]), None, 3, C.c_void_p(rbuf.data_ptr() + 4), _stream()) != 0
    assert b"aligned" in L.atdn_last_error()


# ---------------------------------------------------------------------------------------------------- 3. execution variants
@pytest.fixture(scope="module")
def full_size():
    _, H, W, K, seed = R.FULL_CASE
    s = V.scene(H, W, K, seed)
    m = VoxelMap("cpu", capacity=1 << 21)
    m.integrate(X.t(s["depth"], "cpu"), X.t(s["poses"], "cpu"), s["calib"], stride=2)
    pts, _, _, keys = m.extract()
    host = transforms.visibility_votes(pts, X.t(s["depth"], "cpu"), X.t(s["poses"], "cpu"), s["calib"]).numpy()
    return s, m, pts.numpy(), keys.numpy(), host


def test_full_size_two_calls_a_side_stream_and_a_graph(full_size):
    """376 x 1232, K = 2 against the host form; the same bits on a side stream; then a captured graph of votes + remove +
    extract (a linear chain of five launches) replayed twice over a table restored in between — a capture fails on any host
    synchronisation, so the replay shows the calls have none."""
    s, host_map, pts, keys, host = full_size
    K, H, W = s["depth"].shape
    args = (_t(pts), _t(s["depth"]), _t(s["poses"]), s["calib"])
    a = transforms.visibility_votes(*args).cpu().numpy()
    assert np.array_equal(a, host) and a[:, 1].sum() > len(pts) // 2
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = transforms.visibility_votes(*args)
    side.synchronize()
    assert np.array_equal(b.cpu().numpy(), host)
    # the graph: votes of the cloud, removal of a fixed set of keys, extraction
    L = _lib.lib()
    m = VoxelMap(DEV, capacity=host_map.capacity)
    m.table.copy_(host_map.table)
    pristine = m.table.clone()
    M = len(pts)
    d = dict(points=args[0], depth=args[1], poses=args[2], M=M)
    votes = torch.empty((M, 3), dtype=torch.int32, device=DEV)
    flags = _t((np.arange(M) % 5 == 0).astype(np.uint8))
    kd = _t(keys)
    removed = torch.empty((3,), dtype=torch.int64, device=DEV)
    out = (torch.empty((M, 3), device=DEV), torch.empty((M,), dtype=torch.int32, device=DEV),
           torch.empty((M,), dtype=torch.int64, device=DEV), torch.empty((1,), dtype=torch.int64, device=DEV))

    def chain():
        _lib.check(_raw_votes(L, d, s, (K, K, H, W), votes))
        _lib.check(L.atdn_voxel_remove(_p(m.table), m.capacity, _p(kd), _p(flags), M, _p(removed), _stream()))
        _lib.check(L.atdn_voxel_extract(_p(m.table), m.capacity, 1, m.voxel, *m.origin, M, _p(out[0]), None, _p(out[1]), _p(out[2]),
                                        _p(out[3]), _stream()))

    gone = int(flags.sum())
    removed_host = torch.empty((3,), dtype=torch.int64)
    keys_host, flags_host = kd.cpu(), flags.cpu()                       # (the fixture's map is this test's alone)
    host_map._call("atdn_voxel_remove", _lib.ptr(host_map.table), host_map.capacity, _lib.ptr(keys_host), _lib.ptr(flags_host), M,
                   _lib.ptr(removed_host))
    want_cloud = X._np(host_map.extract())
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        chain()
    for fill in (0, -1):
        m.table.copy_(pristine)
        for o in out + (votes, removed):
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(votes.cpu().numpy(), host) and removed.tolist() == removed_host.tolist() == [gone, removed.tolist()[1], 0]
        n = int(out[3].item())
        assert n == M - gone
        order = torch.argsort(out[2][:n])
        got = (out[0][:n][order].cpu().numpy(), None, out[1][:n][order].cpu().numpy(), out[2][:n][order].cpu().numpy())
        assert V.same_cloud(got, want_cloud), fill


# ---------------------------------------------------------------------------------------------------- 4. the keyframe map
def test_keyframe_map_carve_reads_the_bank_and_fused_depths():
    H, W, N = 16, 48, 4
    s = V.scene(H, W, N, 21, special=False)
    km = KeyframeMap(DEV, hw=(H, W), capacity=2)
    P = torch.cat([torch.from_numpy(s["poses"]).view(N, 3, 4), torch.tensor([0.0, 0, 0, 1]).view(1, 1, 4).repeat(N, 1, 1)], dim=1)
    for k in range(N):
        km.append(torch.from_numpy(s["images"][k]), P[k])
        km.set_depth(k, torch.from_numpy(s["depth"][k]))
    options = dict(min_free=1, ratio=0.0, radius=0)
    for fused in (None, s["depth"][::-1].copy()):
        depth = s["depth"] if fused is None else fused
        vm = km.voxel_map(s["calib"], capacity=1 << 12)
        ref = V.RefMap(**V.DEFAULTS)
        ref.integrate(s["depth"], s["poses"], s["calib"], s["images"])
        want, _ = R.carve(ref, depth, s["poses"], s["calib"], **options)
        got = km.carve(vm, s["calib"], fused=None if fused is None else _t(fused), batch=3, **options)
        assert got == want, (got, want)
        assert V.same_cloud(X._np(vm.extract()), ref.extract())
    assert want["removed_voxels"] > 0                                    # depths of the wrong keyframes carve
    with pytest.raises(ValueError, match="fused"):
        km.carve(vm, s["calib"], fused=_t(s["depth"][:2]))
