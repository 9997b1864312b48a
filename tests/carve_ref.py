"""NumPy restatement of the visibility votes and the removal (include/atdn_hip.h, atdn_voxel_votes and atdn_voxel_remove) and the
scene builders of their tests: helper of test_carve_host.py, test_gpu_carve.py and test_gpu_carve_slam.py, not a test module.
One IEEE float64 operation per element in the rule's order; the window is a loop over its (2 radius + 1)^2 offsets. Clouds and
tables come from voxel_map_ref (imported, not edited)."""
import numpy as np

import voxel_map_ref as V

CHUNK = 4                  # list positions per workgroup of the kernel (carve.hip: CARVE_CHUNK)
DEFAULTS = dict(near=0.5, far=40.0, rel=0.05, abs_tol=0.25, radius=1)


def vote(points, depth, pose, calib, near=0.5, far=40.0, rel=0.05, abs_tol=0.25, radius=1):
    """One keyframe: points [M,3] float32, depth [H,W] float32, pose [12] float32 -> (view, support, free) [M] bool."""
    fx, fy, cx, cy = (np.float64(v) for v in calib)
    H, W = depth.shape
    P = np.asarray(pose, dtype=np.float32).reshape(12).astype(np.float64)
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    D = depth.astype(np.float64)
    near, far, rel, abs_tol = np.float64(near), np.float64(far), np.float64(rel), np.float64(abs_tol)
    with np.errstate(all="ignore"):
        d = [p[:, 0] - P[3], p[:, 1] - P[7], p[:, 2] - P[11]]
        c = [(P[a] * d[0] + P[4 + a] * d[1]) + P[8 + a] * d[2] for a in range(3)]
        z = c[2]
        inr = (near <= z) & (z <= far)
        u = (c[0] / z) * fx + cx
        v = (c[1] / z) * fy + cy
        a = u + 0.5
        b = v + 0.5
        view = inr & (a >= radius) & (a < W - radius) & (b >= radius) & (b < H - radius)
        x = np.where(view, a, radius).astype(np.int64)            # truncation of a non-negative number
        y = np.where(view, b, radius).astype(np.int64)
        x, y = np.clip(x, radius, max(W - 1 - radius, radius)), np.clip(y, radius, max(H - 1 - radius, radius))
        if not view.any():
            return view, view.copy(), view.copy()
        band = rel * z + abs_tol
        lo = z - band
        hi = z + band
        m = D[np.minimum(y, H - 1), np.minimum(x, W - 1)]
        measured = (near <= m) & (m <= far)
        support = view & measured & (lo <= m) & (m <= hi)
        free = view.copy()
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                w = D[np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, W - 1)]
                free &= (near <= w) & (w <= far) & (w > hi)
    return view, support, free


def votes(points, depth, poses, calib, indices=None, out=None, **thresholds):
    """votes [M,3] int32 = (in view, support, free) over the list positions; `out` is added to (a copy)."""
    N = depth.shape[0]
    poses = np.asarray(poses, dtype=np.float32).reshape(N, 12)
    M = len(np.asarray(points).reshape(-1, 3))
    total = np.zeros((M, 3), dtype=np.int32) if out is None else np.array(out, dtype=np.int32)
    for kf in (range(N) if indices is None else [int(i) for i in indices]):
        if not 0 <= kf < N:
            continue
        for a, bits in enumerate(vote(points, depth[kf], poses[kf], calib, **dict(DEFAULTS, **thresholds))):
            total[:, a] += bits.astype(np.int32)
    return total


def remove(ref_map, keys, flags=None):
    """The removal on a voxel_map_ref.RefMap: the flagged keys' rows become zeros and stay in the table. Returns removed [3] int64 =
    voxels emptied, points they held, flagged keys not found or already empty."""
    out = np.zeros(3, dtype=np.int64)
    for r, key in enumerate(int(k) for k in keys):
        if flags is not None and not flags[r]:
            continue
        e = ref_map.table.get(key)
        if e is None or e[0] == 0:
            out[2] += 1
            continue
        out[0] += 1
        out[1] += e[0]
        e[:] = [0] * 7
    return out


def decide(v, min_free=2, ratio=1.0, min_support=0):
    """The decision of VoxelMap.carve on votes [M,3]."""
    support, free = v[:, 1].astype(np.int64), v[:, 2].astype(np.int64)
    return ((free >= min_free) & (free.astype(np.float64) > np.float64(ratio) * support.astype(np.float64))) | (support < min_support)


def hist(x):
    return np.bincount(np.minimum(x, 8), minlength=9).tolist()


def carve(ref_map, depth, poses, calib, indices=None, min_free=2, ratio=1.0, min_support=0, **thresholds):
    """VoxelMap.carve on a RefMap: the report; thresholds default as VoxelMap's (near = min_z, far = max_z, abs_tol = voxel)."""
    pts, _, _, keys = ref_map.extract(1)
    t = dict(near=ref_map.min_z, far=ref_map.max_z, abs_tol=ref_map.voxel)
    t.update(thresholds)
    v = votes(pts, depth, poses, calib, indices, **t)
    removed = remove(ref_map, keys[decide(v, min_free, ratio, min_support)])
    return dict(voxels=len(keys), removed_voxels=int(removed[0]), removed_points=int(removed[1]), free_hist=hist(v[:, 2]),
                support_hist=hist(v[:, 1])), v


# ---------------------------------------------------------------------------------------------------- scenes
CASES = V.CASES                                       # 5 x 7 K = 1, 9 x 33 K = 3, 47 x 154 K = 2
FULL_CASE = V.FULL_CASE
RADII = (0, 1, 2)
# the small hand camera: 9 x 11, fx = fy = 4, principal point (0, 0): a point at (u / 4 * z, v / 4 * z, z) is seen at pixel
# coordinates (u, v), so a = u + 0.5 and b = v + 0.5, all exact in binary for the values used
HAND_HW, HAND_CAL = (9, 11), (4.0, 4.0, 0.0, 0.0)
EYE = V.IDENTITY[None].copy()


def at(u, v, z=2.0):
    return [u / HAND_CAL[0] * z, v / HAND_CAL[1] * z, z]


def hand_depth(value=8.0, K=1):
    return np.full((K,) + HAND_HW, value, dtype=np.float32)


def project(points, pose, calib):
    """(z, a, b) [M] float64 of the rule, for tests that place a point on a boundary and say so."""
    fx, fy, cx, cy = (np.float64(v) for v in calib)
    P = np.asarray(pose, dtype=np.float32).reshape(12).astype(np.float64)
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        d = [p[:, 0] - P[3], p[:, 1] - P[7], p[:, 2] - P[11]]
        c = [(P[a] * d[0] + P[4 + a] * d[1]) + P[8 + a] * d[2] for a in range(3)]
        return c[2], ((c[0] / c[2]) * fx + cx) + 0.5, ((c[1] / c[2]) * fy + cy) + 0.5


def shifted(axis, t):
    """The identity pose with translation component `axis` (0, 1, 2) set to t."""
    pose = EYE.copy()
    pose[0, 4 * axis + 3] = t
    return pose


def up32(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down32(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def hand_cases():
    """Hand-placed cases: (name, points, depth [K,9,11], poses [K,12], thresholds, wanted votes [M,3]). The wanted votes are
    derived by hand in the comments; every case is also compared with the restatement by the tests. z = 2, rel = 0.25 and
    abs_tol = 0.5 give band = 1, lo = 1, hi = 3 exactly."""
    T = dict(rel=0.25, abs_tol=0.5, radius=1)
    mid = [at(5.0, 4.0)]
    cases = []

    def add(name, pts, depth, poses, t, want):
        cases.append((name, np.asarray(pts, dtype=np.float32).reshape(-1, 3), np.asarray(depth, dtype=np.float32),
                      np.asarray(poses, dtype=np.float32).reshape(-1, 12), t, np.asarray(want, dtype=np.int32).reshape(-1, 3)))

    # the view's borders: a = radius is in, the next double below is out; a just below W - radius is in, W - radius is out
    for r in (1, 2):
        t = dict(T, radius=r)
        step_lo = (r - np.nextafter(np.float64(r), 0.0)) / 2                      # t = (the step of a) * z / fx
        step_x, step_y = (11 - r - np.nextafter(11.0 - r, 0.0)) / 2, (9 - r - np.nextafter(9.0 - r, 0.0)) / 2
        add("left_r%d" % r, [at(r - 0.5, 4.0)], hand_depth(), EYE, t, [[1, 0, 1]])
        add("left_below_r%d" % r, [at(r - 0.5, 4.0)], hand_depth(), shifted(0, step_lo), t, [[0, 0, 0]])
        add("top_r%d" % r, [at(5.0, r - 0.5)], hand_depth(), EYE, t, [[1, 0, 1]])
        add("top_below_r%d" % r, [at(5.0, r - 0.5)], hand_depth(), shifted(1, step_lo), t, [[0, 0, 0]])
        add("right_r%d" % r, [at(10.5 - r, 4.0)], hand_depth(), EYE, t, [[0, 0, 0]])
        add("right_below_r%d" % r, [at(10.5 - r, 4.0)], hand_depth(), shifted(0, step_x), t, [[1, 0, 1]])
        add("bottom_r%d" % r, [at(5.0, 8.5 - r)], hand_depth(), EYE, t, [[0, 0, 0]])
        add("bottom_below_r%d" % r, [at(5.0, 8.5 - r)], hand_depth(), shifted(1, step_y), t, [[1, 0, 1]])
    # radius 0: a = 0 is in; the nearest a below that the sum u + 0.5 can give is -2^-53 (u = -0.5 - 2^-53, the next double below
    # -0.5), which is out
    t0 = dict(T, radius=0)
    add("left_r0", [at(-0.5, 4.0)], hand_depth(), EYE, t0, [[1, 0, 1]])
    add("left_below_r0", [at(-0.5, 4.0)], hand_depth(), shifted(0, 2.0 ** -54), t0, [[0, 0, 0]])
    add("right_r0", [at(10.5, 4.0)], hand_depth(), EYE, t0, [[0, 0, 0]])
    add("right_below_r0", [at(10.5, 4.0)], hand_depth(), shifted(0, 2.0 ** -50), t0, [[1, 0, 1]])
    # the band's ends
    add("m_eq_hi", mid, hand_depth(3.0), EYE, T, [[1, 1, 0]])
    add("m_above_hi", mid, hand_depth(up32(3.0)), EYE, T, [[1, 0, 1]])
    add("m_eq_lo", mid, hand_depth(1.0), EYE, T, [[1, 1, 0]])
    add("m_below_lo", mid, hand_depth(down32(1.0)), EYE, T, [[1, 0, 0]])
    # the window: pixel (y, x) = (4, 5) is the centre
    for name, value in (("zero", 0.0), ("nan", np.nan), ("inf", np.inf), ("neg", -8.0), ("eq_hi", 3.0)):
        d = hand_depth()
        d[0, 3, 4] = value
        add("corner_" + name, mid, d, EYE, T, [[1, 0, 0]])
        add("corner_" + name + "_r0", mid, d, EYE, t0, [[1, 0, 1]])                # outside a radius-0 window
    d = hand_depth()
    d[0, 4, 5] = 0.0
    add("centre_unmeasured", mid, d, EYE, T, [[1, 0, 0]])
    # near and far, on z (R = I: z = (double)p_z - (double)t_z exactly) and on m
    ends = [at(5.0, 4.0, 0.5), at(5.0, 4.0, 40.0)]
    add("z_near_far", ends, hand_depth(0.0), EYE, T, [[1, 0, 0], [1, 0, 0]])
    add("z_below_near", ends, hand_depth(0.0), shifted(2, 2.0 ** -54), T, [[0, 0, 0], [1, 0, 0]])
    add("z_above_far", ends, hand_depth(0.0), shifted(2, -2.0 ** -47), T, [[1, 0, 0], [0, 0, 0]])
    add("m_eq_far", mid, hand_depth(40.0), EYE, T, [[1, 0, 1]])
    add("m_above_far", mid, hand_depth(up32(40.0)), EYE, T, [[1, 0, 0]])
    exact = dict(rel=0.0, abs_tol=0.0, radius=1)
    add("m_eq_near", [at(5.0, 4.0, 0.5)], hand_depth(0.5), EYE, exact, [[1, 1, 0]])
    add("m_below_near", [at(5.0, 4.0, 0.5)], hand_depth(down32(0.5)), EYE, exact, [[1, 0, 0]])
    add("behind", [at(5.0, 4.0, -2.0), [0.0, 0.0, 0.0]], hand_depth(), EYE, T, [[0, 0, 0], [0, 0, 0]])
    return cases


def cloud_scene(H, W, K, seed):
    """The street of voxel_map_ref.scene seen from K cameras: its restated cloud plus floaters halfway to the camera, and the
    scene itself: dict(points, depth, poses, calib)."""
    s = V.scene(H, W, K, seed)
    (pts, _, _, _), _ = V.reference(s["depth"], s["poses"], s["calib"])
    rs = np.random.RandomState(seed + 100)
    t = s["poses"][0].reshape(3, 4)[:, 3]
    pick = pts[rs.permutation(len(pts))[:max(1, len(pts) // 4)]]
    floaters = (t + (pick - t) * rs.uniform(0.3, 0.9, (len(pick), 1))).astype(np.float32)
    return dict(points=np.concatenate([pts, floaters]), depth=s["depth"], poses=s["poses"], calib=s["calib"])


def wall_scene(voxel=0.25):
    """A fronto-parallel wall at z = 4 seen by three cameras translated sideways, and a fourth depth image that holds one
    floater pixel at z = 2: dict(depth [4,H,W], poses [4,12], calib, hw, voxel). Cameras 0..2 see the wall alone."""
    H, W = 16, 64
    calib = (32.0, 32.0, 31.5, 7.5)
    depth = np.full((4, H, W), 4.0, dtype=np.float32)
    depth[3] = 0.0
    depth[3, 8, 30] = 2.0
    poses = np.tile(V.IDENTITY, (4, 1))
    poses[:, 3] = [0.0, 0.25, -0.25, 0.0]
    return dict(depth=depth, poses=poses, calib=calib, hw=(H, W), voxel=voxel)


def ground_scene():
    """A ground plane 1.65 below two cameras one metre apart, seen at a grazing angle: depth [2,H,W] (0 above the horizon),
    poses, calib."""
    H, W = 24, 48
    calib = (40.0, 40.0, 23.5, 4.5)
    ys = np.arange(H, dtype=np.float64)[:, None] * np.ones((1, W))
    with np.errstate(all="ignore"):
        g = np.where(ys - calib[3] > 0, 1.65 * calib[1] / (ys - calib[3]), 0.0)
    depth = np.stack([g, g]).astype(np.float32)
    poses = np.tile(V.IDENTITY, (2, 1))
    poses[1, 11] = 1.0
    return dict(depth=depth, poses=poses, calib=calib, hw=(H, W))
