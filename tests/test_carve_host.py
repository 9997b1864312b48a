"""Visibility votes and carving through the library's host form (CPU tensors: atdn_voxel_votes_host, atdn_voxel_remove_host)
against the NumPy restatement of the rule (tests/carve_ref.py) — every bit. The same checks run on the kernels in
test_gpu_carve.py; the properties are first shown here, on the CPU, with the restatement alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carve_cases as X  # noqa: E402
import carve_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402

DEV = "cpu"
HAND = R.hand_cases()


@pytest.mark.parametrize("name,H,W,K,seed", R.CASES, ids=[c[0] for c in R.CASES])
def test_host_form_equals_the_restatement(name, H, W, K, seed):
    print("votes (in view, support, free) summed over radii and index lists:", X.check_house_case(DEV, H, W, K, seed).tolist())


def test_hand_placed_points_sit_where_their_names_say():
    X.check_hand_preconditions()


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


def test_flags_select_the_keys_and_null_means_all():
    m, ref, _ = X.clustered_maps(DEV)
    keys = torch.from_numpy(ref.extract()[3].copy())
    flags = torch.zeros(len(keys), dtype=torch.uint8)
    flags[[1, 5, 29]] = torch.tensor([1, 255, 7], dtype=torch.uint8)
    removed = torch.full((4,), -7, dtype=torch.int64)
    p = _lib.ptr
    _lib.call("atdn_voxel_remove", m.device, p(m.table), m.capacity, p(keys), p(flags), len(keys), p(removed))
    assert removed.tolist() == R.remove(ref, keys.numpy(), flags.numpy()).tolist() + [-7] == [3, 3, 0, -7]
    assert V.same_cloud(X._np(m.extract()), ref.extract())
    _lib.call("atdn_voxel_remove", m.device, p(m.table), m.capacity, p(keys), None, len(keys), p(removed))
    assert removed.tolist() == R.remove(ref, keys.numpy()).tolist() + [-7] == [27, 27, 3, -7]
    assert len(m.extract()[3]) == 0 and m._read_counts()["voxels"] == 30
    _lib.call("atdn_voxel_remove", m.device, p(m.table), m.capacity, None, None, 0, p(removed))
    assert removed.tolist() == [0, 0, 0, -7]


def test_carve_report_equals_the_restatement():
    X.check_carve_report(DEV)


def test_wall_and_floater():
    X.check_wall(DEV)


def test_ground_plane_at_a_grazing_angle_never_carves_itself():
    X.check_ground(DEV)


def test_argument_rules():
    L = _lib.lib()
    s = R.cloud_scene(5, 7, 1, 1)
    pts, d, P = (torch.from_numpy(np.ascontiguousarray(s[k])) for k in ("points", "depth", "poses"))
    M = len(pts)
    votes = torch.zeros((M, 3), dtype=torch.int32)
    p = _lib.ptr

    def call(points=pts, M=M, K=1, near=0.5, far=40.0, rel=0.05, tol=0.25, radius=1, accumulate=0, out=votes, indices=None):
        return L.atdn_voxel_votes_host(p(points), M, p(d), p(P), p(indices), 1, K, 5, 7, *s["calib"], near, far, rel, tol, radius,
                                       accumulate, p(out))

    assert call() == 0
    for kw, word in ((dict(near=0.0), b"near"), (dict(near=2.0, far=1.0), b"near"), (dict(far=float("inf")), b"far"),
                     (dict(rel=-1.0), b"rel"), (dict(tol=float("nan")), b"rel"), (dict(radius=9), b"radius"),
                     (dict(radius=-1), b"radius"), (dict(accumulate=2), b"accumulate"), (dict(K=2), b"K <= N"), (dict(M=-1), b"M"),
                     (dict(out=pts.view(torch.int32)), b"overlaps"), (dict(out=d.view(torch.int32)), b"overlaps")):
        assert call(**kw) != 0 and word in L.atdn_last_error(), kw
    odd = C.c_void_p(votes.data_ptr() + 2)
    assert L.atdn_voxel_votes_host(p(pts), M, p(d), p(P), None, 1, 1, 5, 7, *s["calib"], 0.5, 40.0, 0.05, 0.25, 1, 0, odd) != 0
    assert b"aligned" in L.atdn_last_error()
    assert call(points=None, M=0, out=None) == 0                         # M == 0 is a no-op that succeeds
    m = VoxelMap("cpu", capacity=64)
    keys = torch.zeros(4, dtype=torch.int64)
    removed = torch.zeros(3, dtype=torch.int64)
    assert L.atdn_voxel_remove_host(p(m.table), 64, p(keys), None, 4, p(removed)) == 0 and removed.tolist() == [0, 0, 4]
    assert L.atdn_voxel_remove_host(p(m.table), 63, p(keys), None, 4, p(removed)) != 0 and b"capacity" in L.atdn_last_error()
    assert L.atdn_voxel_remove_host(p(m.table), 64, p(keys), None, -1, p(removed)) != 0
    assert L.atdn_voxel_remove_host(p(m.table), 64, p(keys), None, 3, p(keys[1:])) != 0 and b"overlap" in L.atdn_last_error()
    assert L.atdn_voxel_remove_host(p(m.table), 64, p(m.table[8:]), None, 4, p(removed)) != 0 and b"overlap" in L.atdn_last_error()
    with pytest.raises(RuntimeError):
        transforms.visibility_votes(pts, d, P, s["calib"], out=torch.zeros((M, 3), dtype=torch.int64))
