"""The checks that test_carve_host.py (the library's host form, CPU tensors) and test_gpu_carve.py (the kernels) share: every
function takes the device and compares transforms.visibility_votes / VoxelMap with the NumPy restatement (tests/carve_ref.py)
bit for bit. Helper, not a test module."""
import os
import sys

import numpy as np
import torch

from atdn_vslam_amd import transforms
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carve_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402


def t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


def votes(dev, points, depth, poses, calib, indices=None, out=None, **thresholds):
    got = transforms.visibility_votes(t(points, dev), t(depth, dev), t(poses, dev), calib, indices=indices,
                                      out=None if out is None else t(out, dev), **thresholds)
    return got.cpu().numpy()


def same(dev, points, depth, poses, calib, indices=None, **thresholds):
    """The device's votes == the restatement's, every bit; returns them."""
    want = R.votes(points, depth, poses, calib, indices, **thresholds)
    got = votes(dev, points, depth, poses, calib, indices, **thresholds)
    assert V.same_bits(got, want), (thresholds, indices, np.flatnonzero((got != want).any(axis=1))[:8])
    return got


# ---------------------------------------------------------------------------------------------------- votes
def check_house_case(dev, H, W, K, seed):
    s = R.cloud_scene(H, W, K, seed)
    lists = [None, [K - 1] + list(range(K))]
    hits = np.zeros(3, dtype=np.int64)
    for radius in R.RADII:
        for ix in lists:
            hits += same(dev, s["points"], s["depth"], s["poses"], s["calib"], ix, radius=radius).sum(axis=0)
    assert hits[0] > 0 and hits[1] > 0, hits                         # the cases are not vacuous
    return hits


def check_hand_case(dev, case):
    name, pts, depth, poses, thresholds, want = case
    got = same(dev, pts, depth, poses, R.HAND_CAL, **thresholds)
    assert got.tolist() == want.tolist(), (name, got.tolist(), want.tolist())


def check_hand_preconditions():
    """The boundary cases sit where their names say: computed with the rule's own operations."""
    cases = {c[0]: c for c in R.hand_cases()}
    for r in (1, 2):
        for name, axis, A in (("left", 1, float(r)), ("top", 2, float(r)), ("right", 1, 11.0 - r), ("bottom", 2, 9.0 - r)):
            on = R.project(cases["%s_r%d" % (name, r)][1], cases["%s_r%d" % (name, r)][3], R.HAND_CAL)[axis][0]
            below = R.project(cases["%s_below_r%d" % (name, r)][1], cases["%s_below_r%d" % (name, r)][3], R.HAND_CAL)[axis][0]
            assert on == A and below == np.nextafter(A, 0.0), (name, r, on, below)
    assert R.project(cases["left_r0"][1], cases["left_r0"][3], R.HAND_CAL)[1][0] == 0.0
    assert R.project(cases["left_below_r0"][1], cases["left_below_r0"][3], R.HAND_CAL)[1][0] == -2.0 ** -53
    assert R.project(cases["right_r0"][1], cases["right_r0"][3], R.HAND_CAL)[1][0] == 11.0
    assert R.project(cases["right_below_r0"][1], cases["right_below_r0"][3], R.HAND_CAL)[1][0] == np.nextafter(11.0, 0.0)
    z = R.project(cases["z_below_near"][1], cases["z_below_near"][3], R.HAND_CAL)[0]
    assert z[0] == np.nextafter(0.5, 0.0) and z[1] == 40.0
    z = R.project(cases["z_above_far"][1], cases["z_above_far"][3], R.HAND_CAL)[0]
    assert z[1] == np.nextafter(40.0, 50.0) and z[0] > 0.5
    z = R.project(cases["z_near_far"][1], cases["z_near_far"][3], R.HAND_CAL)[0]
    assert z.tolist() == [0.5, 40.0]


def check_nan_and_infinity(dev):
    """NaN and +-inf in one point, in one pose of three and in one depth pixel: the other points and cameras vote as before."""
    s = R.cloud_scene(9, 33, 3, 2)
    args = (s["calib"],)
    clean = same(dev, s["points"], s["depth"], s["poses"], *args)
    two = same(dev, s["points"], s["depth"], s["poses"], *args, indices=[0, 2])
    i = int(np.argmax(clean[:, 0]))
    for bad in (np.nan, np.inf, -np.inf):
        pts = s["points"].copy()
        pts[i, 1] = bad
        got = same(dev, pts, s["depth"], s["poses"], *args)
        keep = np.arange(len(pts)) != i
        assert np.array_equal(got[keep], clean[keep]) and got[i].tolist() == [0, 0, 0]
        for slot in (3, 0, 10):                                          # t_x, r_00, r_22
            poses = s["poses"].copy()
            poses[1, slot] = bad
            assert np.array_equal(same(dev, s["points"], s["depth"], poses, *args), two)
        depth = s["depth"].copy()
        depth[1, 4, 16] = bad
        got = same(dev, s["points"], depth, s["poses"], *args)
        assert np.array_equal(got[:, 0], clean[:, 0]) and (got[:, 1:] <= clean[:, 1:]).all()


def check_index_lists(dev):
    s = R.cloud_scene(9, 33, 3, 5)
    args = (s["points"], s["depth"], s["poses"], s["calib"])
    one = [same(dev, *args, indices=[k]) for k in range(3)]
    got = same(dev, *args, indices=[1, 1, -1, 3, 0, 2 ** 31 - 1])
    assert np.array_equal(got, 2 * one[1] + one[0]) and one[1].any()
    assert not same(dev, *args, indices=[-1, 3, 7]).any()
    assert not votes(dev, *args, indices=[]).any()


def check_point_counts(dev, M):
    s = R.cloud_scene(9, 33, 3, 2)
    pick = np.random.RandomState(M).permutation(len(s["points"]))[:M]
    got = same(dev, s["points"][pick], s["depth"], s["poses"], s["calib"])
    assert got.shape == (M, 3)


def check_camera_chunks(dev):
    """K one less than, equal to and one more than the kernel's camera chunk, and two chunks and one more."""
    N = 2 * R.CHUNK + 1
    s = V.scene(9, 33, N, 7)
    (pts, _, _, _), _ = V.reference(s["depth"], s["poses"], s["calib"])
    for K in (R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK, N):
        same(dev, pts, s["depth"][:K], s["poses"][:K], s["calib"])
        same(dev, pts, s["depth"], s["poses"], s["calib"], indices=list(range(N - 1, N - 1 - K, -1)))


def check_split_invariance(dev):
    """K keyframes in one call == the same keyframes over three calls with accumulation, in two orders."""
    s = R.cloud_scene(9, 33, 3, 9)
    s7 = V.scene(9, 33, 7, 9)
    args = (s["points"], s7["depth"], s7["poses"], s7["calib"])
    whole = same(dev, *args)
    assert whole[:, 1].any()
    for parts in ([[0, 1], [2, 3, 4, 5], [6]], [[6, 3], [5], [1, 0, 4, 2]]):
        acc = None
        for ix in parts:
            acc = votes(dev, *args, indices=ix, out=acc)
        assert V.same_bits(acc, whole), parts
    # out= is added to, whatever it holds
    base = np.arange(3 * len(s["points"]), dtype=np.int32).reshape(-1, 3)
    assert V.same_bits(votes(dev, *args, out=base), base + whole)


# ---------------------------------------------------------------------------------------------------- removal
def _np(out):
    return tuple(None if x is None else x.cpu().numpy() for x in out)


def clustered_maps(dev, capacity=64):
    """A table of `capacity` slots with 30 keys whose home slots are its last 8: the probe chains wrap around the table's end.
    Returns (VoxelMap, RefMap, scene)."""
    s = V.clustered_scene(capacity=capacity, n=30, first=capacity - 8)
    m = VoxelMap(dev, capacity=capacity)
    m.integrate(t(s["depth"], dev), t(s["poses"], dev), s["calib"])
    assert m.capacity == capacity and m.counts["voxels"] == 30
    ref = V.RefMap(**V.DEFAULTS)
    ref.integrate(s["depth"], s["poses"], s["calib"])
    assert V.same_cloud(_np(m.extract()), ref.extract())
    return m, ref, s


def check_removal(dev):
    m, ref, s = clustered_maps(dev)
    keys = ref.extract()[3]
    before = m.counts
    absent = int(keys.max()) + 12345
    # every third key, one of them twice, and a key that is absent
    ask = np.concatenate([keys[::3], keys[3:4], [absent]]).astype(np.int64)
    want = R.remove(ref, ask)
    assert want.tolist() == [10, 10, 2]
    assert list(m.remove(t(ask, dev))) == want.tolist() and m.removed == dict(voxels=10, points=10)
    assert m.counts == before and m._read_counts() == before             # the five counters are not touched
    assert V.same_cloud(_np(m.extract()), ref.extract()) and len(ref.extract()[3]) == 20
    assert list(m.remove(ask)) == [0, 0, 12]                             # already empty: nothing, from a host sequence too
    assert list(m.remove(np.zeros(0, dtype=np.int64))) == [0, 0, 0]      # R = 0
    # rehash into a larger table carries the emptied voxels along: the same cloud, the same counters
    m._grow(256)
    assert V.same_cloud(_np(m.extract()), ref.extract()) and m._read_counts() == before
    # integrate refills an emptied voxel like any other
    again = m.integrate(t(s["depth"], dev), t(s["poses"], dev), s["calib"], indices=[0, 3, 4])
    ref.integrate(s["depth"], s["poses"], s["calib"], indices=[0, 3, 4])
    assert V.same_cloud(_np(m.extract()), ref.extract()) and again["voxels"] == 30
    got = dict(zip(ref.extract()[3].tolist(), ref.extract()[2].tolist()))
    assert got[int(keys[0])] == 1 and got[int(keys[3])] == 1 and got[int(keys[4])] == 2


def check_carve_report(dev):
    """VoxelMap.carve == the restatement: report, votes and the cloud afterwards."""
    s = V.scene(9, 33, 3, 4)
    m = VoxelMap(dev, capacity=1 << 12)
    m.integrate(t(s["depth"], dev), t(s["poses"], dev), s["calib"], images=t(s["images"], dev))
    ref = V.RefMap(**V.DEFAULTS)
    ref.integrate(s["depth"], s["poses"], s["calib"], s["images"])
    options = dict(min_free=1, ratio=0.5, min_support=1, radius=0)
    keys, v = m.votes(t(s["depth"], dev), t(s["poses"], dev), s["calib"], batch=2, radius=0)
    assert np.array_equal(keys.cpu().numpy(), ref.extract(1)[3])
    want, want_votes = R.carve(ref, s["depth"], s["poses"], s["calib"], **options)
    assert V.same_bits(v.cpu().numpy(), want_votes)
    got = m.carve(t(s["depth"], dev), t(s["poses"], dev), s["calib"], batch=2, **options)
    assert got == want and 0 < got["removed_voxels"] < got["voxels"], (got, want)
    assert V.same_cloud(_np(m.extract()), ref.extract())
    assert m.removed == dict(voxels=got["removed_voxels"], points=got["removed_points"])
    # an emptied voxel starts again from zero sums, position and colour alike
    m.integrate(t(s["depth"], dev), t(s["poses"], dev), s["calib"], images=t(s["images"], dev), indices=[0])
    ref.integrate(s["depth"], s["poses"], s["calib"], s["images"], indices=[0])
    assert V.same_cloud(_np(m.extract()), ref.extract())


# ---------------------------------------------------------------------------------------------------- properties
def wall_maps(dev, with_floater):
    w = R.wall_scene()
    m = VoxelMap(dev, voxel=w["voxel"], capacity=1 << 12)
    m.integrate(t(w["depth"], dev), t(w["poses"], dev), w["calib"], indices=[0, 1, 2, 3] if with_floater else [0, 1, 2])
    return w, m


def check_wall_inputs():
    """On the CPU, with the restatement alone: the wall scene behaves as the property test states."""
    w = R.wall_scene()
    ref = V.RefMap(voxel=w["voxel"])
    ref.integrate(w["depth"], w["poses"], w["calib"])
    pts, _, cnt, keys = ref.extract()
    floater = pts[:, 2] < 3.0
    assert floater.sum() == 1 and cnt[floater].tolist() == [1]
    v = R.votes(pts, w["depth"], w["poses"], w["calib"], indices=[0, 1, 2], rel=0.0, abs_tol=w["voxel"], radius=1)
    assert v[floater].tolist() == [[3, 0, 3]]
    wall = ~floater
    assert (v[wall, 2] == 0).all() and np.array_equal(v[wall, 1], v[wall, 0]) and v[wall, 0].max() == 3 and (v[wall, 0] >= 1).any()
    behind = pts[wall].copy()
    behind[:, 2] += 2.0
    b = R.votes(behind, w["depth"], w["poses"], w["calib"], indices=[0, 1, 2], rel=0.0, abs_tol=w["voxel"], radius=1)
    assert b[:, 0].max() == 3 and not b[:, 1:].any()
    return pts, keys, floater, v


def check_wall(dev):
    """A fronto-parallel wall at z = 4 from three cameras and one floater voxel at z = 2 from a fourth image. Against the three
    wall depths (rel 0, abs_tol one voxel, radius 1): every wall voxel has free 0 and support == in view (every pixel of the
    wall images is measured, and the wall's depth lies inside the band of a voxel whose mean is within voxel / 65536 of 4);
    the floater, whose window lies inside all three images and whose hi = 2.25 < 4, has free 3. carve(min_free=2) then leaves,
    bit for bit, the map that never integrated the floater. The wall moved 2 m back is occluded: lo = 5.75 > 4, no vote."""
    pts, keys, floater, want = check_wall_inputs()
    w, m = wall_maps(dev, True)
    d, P = t(w["depth"], dev), t(w["poses"], dev)
    options = dict(indices=[0, 1, 2], rel=0.0, abs_tol=w["voxel"], radius=1)
    k, v = m.votes(d, P, w["calib"], **options)
    assert np.array_equal(k.cpu().numpy(), keys) and np.array_equal(v.cpu().numpy(), want)
    report = m.carve(d, P, w["calib"], min_free=2, **options)
    assert report["removed_voxels"] == 1 and report["removed_points"] == 1 and report["voxels"] == len(keys)
    assert report["free_hist"] == [len(keys) - 1, 0, 0, 1, 0, 0, 0, 0, 0] and m.removed == dict(voxels=1, points=1)
    _, clean = wall_maps(dev, False)
    assert V.same_cloud(_np(m.extract()), _np(clean.extract()))
    behind = pts[~floater].copy()
    behind[:, 2] += 2.0
    b = votes(dev, behind, w["depth"], w["poses"], w["calib"], **options)
    assert b[:, 0].max() == 3 and not b[:, 1:].any()


def check_ground(dev):
    """A ground plane seen at a grazing angle from two cameras, defaults (rel 0.05, abs_tol one voxel, radius 1): free is 0
    everywhere. A voxel's mean lies on the plane; seen at row coordinate v it has z = h fy / (v - cy), and the window's row
    y + 1 > v holds the plane's depth at a lower row, which is smaller than z: that pixel is never beyond hi."""
    g = R.ground_scene()
    ref = V.RefMap(**V.DEFAULTS)
    ref.integrate(g["depth"], g["poses"], g["calib"])
    pts = ref.extract()[0]
    want = R.votes(pts, g["depth"], g["poses"], g["calib"], near=0.5, far=40.0, abs_tol=0.25)
    assert (want[:, 2] == 0).all() and want[:, 1].sum() > len(pts) // 2
    # the window is what does it: with radius 0 the far rows, a metre of depth apart and more, do carve themselves
    assert R.votes(pts, g["depth"], g["poses"], g["calib"], near=0.5, far=40.0, abs_tol=0.25, radius=0)[:, 2].any()
    got = votes(dev, pts, g["depth"], g["poses"], g["calib"], near=0.5, far=40.0, abs_tol=0.25)
    assert np.array_equal(got, want)
