"""NumPy restatement of the voxel-map rule (include/atdn_hip.h, atdn_voxel_integrate and atdn_voxel_extract) and the scene
builder of its tests: helper of test_voxel_map_host.py, test_gpu_voxel_map.py and test_gpu_voxel_map_slam.py, not a test module.
One IEEE float64 operation per element in the rule's order, np.floor for the floor, np.unique for the table."""
import numpy as np

LIM = 1048576.0            # 2^20
COUNTERS = ("candidates", "inserted", "outside", "dropped", "voxels")
DEFAULTS = dict(voxel=0.25, origin=(0.0, 0.0, 0.0), min_z=0.5, max_z=40.0)
GOLDEN = 0x9E3779B97F4A7C15


def home(key, capacity):
    """The home slot of a key in a table of `capacity` slots (the table's layout, include/atdn_hip.h)."""
    return ((((int(key) * GOLDEN) & (2 ** 64 - 1)) >> 32) * capacity) >> 32


def pixel_keys(depth, pose, calib, voxel, origin, min_z, max_z):
    """One keyframe: depth [H,W] float32, pose [12] float32 -> (candidate [H,W] bool, inside [H,W] bool, key [H,W] int64,
    q [3,H,W] int64); key and q are meaningful where `inside`."""
    fx, fy, cx, cy = (np.float64(v) for v in calib)
    H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    P = pose.astype(np.float64)
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64)
        cand = (np.float64(min_z) <= z) & (z <= np.float64(max_z))
        xn = (xs - cx) / fx
        yn = (ys - cy) / fy
        c = (xn * z, yn * z, z)
        inside = cand.copy()
        key = np.zeros((H, W), dtype=np.int64)
        q = np.zeros((3, H, W), dtype=np.int64)
        for a in range(3):
            p = ((P[4 * a] * c[0] + P[4 * a + 1] * c[1]) + P[4 * a + 2] * c[2]) + P[4 * a + 3]
            g = (p - np.float64(origin[a])) / np.float64(voxel)
            ok = (-LIM <= g) & (g < LIM)
            inside &= ok
            g = np.where(ok, g, 0.0)
            k = np.floor(g)
            f = g - k
            q[a] = (f * 65536.0).astype(np.int64)
            key = (key << 21) | (k.astype(np.int64) + 1048576)
    return cand, inside, key, q


class RefMap:
    """The table as a dict: key -> [n, S_x, S_y, S_z, C_r, C_g, C_b] (Python ints)."""

    def __init__(self, voxel=0.25, origin=(0.0, 0.0, 0.0), min_z=0.5, max_z=40.0):
        self.voxel, self.origin, self.min_z, self.max_z = voxel, tuple(origin), min_z, max_z
        self.table = {}
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.colored = None

    def integrate(self, depth, poses, calib, images=None, mask=None, indices=None, stride=1):
        N, H, W = depth.shape
        poses = np.asarray(poses, dtype=np.float32).reshape(N, 12)
        idx = list(range(N)) if indices is None else [int(i) for i in indices]
        self.colored = images is not None
        part = np.zeros((H, W), dtype=bool)
        part[::stride, ::stride] = True
        for j, kf in enumerate(idx):
            if not 0 <= kf < N:
                continue
            cand, inside, key, q = pixel_keys(depth[kf], poses[kf], calib, self.voxel, self.origin, self.min_z, self.max_z)
            take = part if mask is None else part & (mask[j] != 0)
            cand, inside = cand & take, inside & take
            self.counts["candidates"] += int(cand.sum())
            self.counts["outside"] += int((cand & ~inside).sum())
            self.counts["inserted"] += int(inside.sum())
            keys, inv = np.unique(key[inside], return_inverse=True)
            rows = np.zeros((len(keys), 7), dtype=np.int64)
            np.add.at(rows[:, 0], inv, 1)
            for a in range(3):
                np.add.at(rows[:, 1 + a], inv, q[a][inside])
                if images is not None:
                    np.add.at(rows[:, 4 + a], inv, images[kf, a][inside].astype(np.int64))
            for k, r in zip(keys.tolist(), rows.tolist()):
                e = self.table.setdefault(k, [0] * 7)
                for i in range(7):
                    e[i] += r[i]
        self.counts["voxels"] = len(self.table)
        return dict(self.counts)

    def extract(self, min_count=1):
        """(points [M,3] float32, colors [M,3] uint8 or None, counts [M] int32, keys [M] int64), ascending keys."""
        keys = sorted(k for k, e in self.table.items() if e[0] >= min_count)
        rows = np.array([self.table[k] for k in keys], dtype=np.int64).reshape(len(keys), 7)
        ks = np.array(keys, dtype=np.int64)
        n = rows[:, 0].astype(np.float64)
        pts = np.zeros((len(keys), 3), dtype=np.float32)
        for a in range(3):
            ka = ((ks >> (21 * (2 - a))) & 0x1FFFFF) - 1048576
            m = rows[:, 1 + a].astype(np.float64) / n
            fr = (m + 0.5) / 65536.0
            pts[:, a] = (np.float64(self.origin[a]) + (ka.astype(np.float64) + fr) * np.float64(self.voxel)).astype(np.float32)
        colors = None
        if self.colored:
            colors = ((rows[:, 4:7] + rows[:, 0:1] // 2) // rows[:, 0:1]).astype(np.uint8)
        return pts, colors, rows[:, 0].astype(np.int32), ks


def reference(depth, poses, calib, images=None, mask=None, indices=None, stride=1, min_count=1, **grid):
    m = RefMap(**dict(DEFAULTS, **grid))
    counts = m.integrate(depth, poses, calib, images, mask, indices, stride)
    return m.extract(min_count), counts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_cloud(got, want):
    """Two extract() tuples (NumPy): equal in every bit."""
    if len(got) != 4 or len(want) != 4:
        return False
    for g, w in zip(got, want):
        if (g is None) != (w is None) or (g is not None and not same_bits(g, w)):
            return False
    return True


# ---------------------------------------------------------------------------------------------------- scenes
def scene_calib(H, W):
    return 718.856 * W / 1241.0, 718.856 * W / 1241.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2


def euler(a):
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def scene(H, W, K, seed, start=(-3.0, -0.4, -2.0), step=1.0, far=45.0, special=True):
    """A street seen from K cameras `step` metres apart that start at `start` (negative world coordinates: the floor below zero):
    the depth of every frame is the nearer of a ground plane 1.65 m below the camera and a smooth wall between 3 m and `far`
    (beyond the default max_z in places), float32. With `special` the first pixels of every frame are NaN, +inf, -inf, 0, -1 and
    exactly min_z and max_z of the defaults (as far as the frame has that many pixels).
    Returns dict(depth [K,H,W] float32, poses [K,12] float32, images [K,3,H,W] uint8, mask [K,H,W] uint8, calib)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = calib = scene_calib(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((K, H, W), dtype=np.float32)
    poses = np.zeros((K, 12), dtype=np.float32)
    for k in range(K):
        wall = 3.0 + (far - 3.0) * (0.5 + 0.5 * np.cos(2 * np.pi * (xs / W + 0.13 * seed + 0.05 * k))) * \
            (0.35 + 0.65 * (0.5 + 0.5 * np.cos(np.pi * ys / H)))
        with np.errstate(all="ignore"):
            ground = np.where(ys - cy > 0, 1.65 * fy / (ys - cy), np.inf)
        depth[k] = np.minimum(wall, ground)
        R = euler(rs.uniform(-0.03, 0.03, 3))
        t = np.array(start) + np.array([0.1 * rs.randn(), 0.02 * rs.randn(), step * k])
        poses[k] = np.concatenate([R, t[:, None]], axis=1).reshape(12)
        if special:
            values = [np.nan, np.inf, -np.inf, 0.0, -1.0, DEFAULTS["min_z"], DEFAULTS["max_z"]]
            flat = depth[k].reshape(-1)
            flat[:min(len(values), flat.size)] = values[:flat.size]
    images = rs.randint(0, 256, size=(K, 3, H, W)).astype(np.uint8)
    mask = (rs.uniform(size=(K, H, W)) < 0.7).astype(np.uint8)
    return dict(depth=depth, poses=poses, images=images, mask=mask, calib=calib)


IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)
CASES = [("5x7_k1", 5, 7, 1, 1), ("9x33_k3", 9, 33, 3, 2), ("47x154_k2", 47, 154, 2, 3)]
FULL_CASE = ("376x1232_k2", 376, 1232, 2, 4)


def variants():
    """(stride, with images, with mask)"""
    return [(1, True, True), (1, False, False), (2, True, False), (2, False, True), (3, True, True), (3, False, False)]


def axis_scene(gx, gy=None, gz=None, voxel=0.25):
    """len(gx) keyframes of one pixel each whose point lands at the grid coordinate (gx[i], gy[i], gz[i]) exactly (origin 0,
    g * voxel representable in float32): the identity rotation, calib (1, 1, 0, 0) and depth 1 make the camera point (0, 0, 1),
    and the pose's translation places it."""
    gx = np.asarray(gx, dtype=np.float64)
    gy = np.zeros_like(gx) if gy is None else np.asarray(gy, dtype=np.float64)
    gz = np.zeros_like(gx) if gz is None else np.asarray(gz, dtype=np.float64)
    K = len(gx)
    depth = np.ones((K, 1, 1), dtype=np.float32)
    poses = np.tile(IDENTITY, (K, 1))
    # pixel (0, 0) with calib (1, 1, 0, 0) and depth 1 is the camera point (0, 0, 1): p = t + (0, 0, 1)
    poses[:, 3] = (gx * voxel).astype(np.float32)
    poses[:, 7] = (gy * voxel).astype(np.float32)
    poses[:, 11] = (gz * voxel - 1.0).astype(np.float32)
    return dict(depth=depth, poses=poses, calib=(1.0, 1.0, 0.0, 0.0))


def clustered_scene(capacity=64, n=30, first=56):
    """n points one or more voxels apart along x whose keys' home slots are the last capacity - first slots of the table."""
    gx = [float(g) for g in range(100000) if home(((g + 1048576) << 42) | (1048576 << 21) | 1048576, capacity) >= first][:n]
    assert len(gx) == n
    return axis_scene(gx)
