"""The map as one coloured point cloud: every keyframe's depth accumulated into a voxel-hashed table (libatdn_hip's
atdn_voxel_* entry points; the rule, the table's layout and the counters are stated in full in include/atdn_hip.h).

A pixel's point falls into a cubic voxel; per voxel the table keeps the number of points and the integer sums of their sub-voxel
positions and colour bytes. Integer sums commute, so the cloud does not depend on thread order, on how the keyframes are split
over calls or on the table's size: the same bits on the device, in the library's host form (CPU tensors) and in the NumPy
restatement of the tests.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr
from .transforms import _byte_plane, _index_tensor, _pose_rows

COUNTERS = ("candidates", "inserted", "outside", "dropped", "voxels")
MAX_POINTS = 2 ** 31 - 1
_HEADER_WORDS = 8
_GROW_ROUNDS = 8            # doublings tried for the pixels an integrate dropped before the call gives up


class VoxelMap:
    """A voxel-hashed point cloud on `device` (a CUDA device: the HIP kernels; "cpu": the library's host form, same bits).
    `voxel` is the edge of a voxel and `origin` the corner of voxel (0, 0, 0), in the units of the poses; a depth outside
    [min_z, max_z] is no point (0 = no depth among them). `capacity` (a power of two) is the table's first size: it grows by
    itself, and growing gives the same bits as starting large."""

    def __init__(self, device, voxel=0.25, origin=(0.0, 0.0, 0.0), min_z=0.5, max_z=40.0, capacity=1 << 20):
        self.device = torch.device(device)
        self.voxel = float(voxel)
        if not (np.isfinite(self.voxel) and self.voxel > 0.0):
            raise ValueError("voxel must be finite and > 0, got %r" % (voxel,))
        self.origin = tuple(float(v) for v in origin)
        if len(self.origin) != 3 or not all(np.isfinite(v) for v in self.origin):
            raise ValueError("origin must be three finite numbers, got %r" % (origin,))
        self.min_z, self.max_z = float(min_z), float(max_z)
        if np.isnan(self.min_z) or np.isnan(self.max_z):
            raise ValueError("min_z and max_z must not be NaN")
        capacity = int(capacity)
        if capacity < 2 or capacity > 2 ** 31 or capacity & (capacity - 1):
            raise ValueError("capacity must be a power of two in [2, 2^31], got %d" % capacity)
        self.capacity = capacity
        self.has_colors = None              # set by the first integrate: every call gives images, or none does
        self._points_bound = 0              # host-side upper bound of the points in the table
        self._counts = dict.fromkeys(COUNTERS, 0)
        self._extraction = None             # extract(1) as render() last saw it; dropped by integrate, _grow and remove
        self.removed = dict(voxels=0, points=0)   # what remove() took out so far (host side; the table's counters do not change)
        self.table = self._new_table(capacity)

    # ------------------------------------------------------------------ the table
    def _call(self, name, *args):
        _lib.call(name, self.device, *args)

    def _new_table(self, capacity):
        words = int(_lib.lib().atdn_voxel_table_bytes(capacity)) // 8
        if words <= 0:
            raise ValueError("capacity must be a power of two in [2, 2^31], got %d" % capacity)
        table = torch.empty((words,), dtype=torch.int64, device=self.device)
        self._call("atdn_voxel_clear", _ptr(table), capacity)
        return table

    def _grow(self, capacity):
        """Rehash into a cleared table of `capacity` slots."""
        self._extraction = None
        table = self._new_table(capacity)
        self._call("atdn_voxel_rehash", _ptr(self.table), self.capacity, _ptr(table), capacity)
        self.table, self.capacity = table, capacity

    def _read_counts(self):
        head = self.table[:5].cpu().tolist()       # the one synchronisation of an integrate
        self._counts = dict(zip(COUNTERS, (int(v) for v in head)))
        return self._counts

    @property
    def counts(self):
        """The five counters (host ints): candidates == inserted + outside + dropped; voxels = occupied slots."""
        return dict(self._counts)

    # ------------------------------------------------------------------ filling
    def integrate(self, depth, poses, calib, images=None, mask=None, indices=None, stride=1):
        """Add keyframes to the cloud. `depth` [N,H,W] float32 and `poses` ([N,12], [N,3,4] or [N,4,4]; rows of [R|t], world <-
        camera) are banks of N keyframes, `images` [N,3,H,W] uint8 (red, green, blue) their colours or None, `calib` is
        (fx, fy, cx, cy) or a calibration matrix without skew. `indices` (integers, host or on the device) lists the keyframes
        to add — the whole bank by default; an index outside the bank adds nothing, a repeat adds its keyframe again — and
        `mask` [K,H,W] (by list position; zero = skip) and `stride` (every stride-th pixel of every stride-th row) thin the
        pixels. The table grows first to twice (voxels so far + pixels of this call); pixels that still find no slot are
        integrated again into a larger table, so no point is lost silently: `counts["dropped"]` ends at 0 or the call raises.
        Returns the counters."""
        from .depth import intrinsics
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise RuntimeError("expected a depth bank [N,H,W], got %s" % (tuple(getattr(depth, "shape", ())),))
        if depth.device != self.device:
            raise RuntimeError("the voxel map is on %s but the depth on %s" % (self.device, depth.device))
        if depth.dtype != torch.float32 or not depth.is_contiguous():
            depth = depth.detach().float().contiguous()
        N, H, W = (int(v) for v in depth.shape)
        if isinstance(poses, torch.Tensor) and poses.device != self.device:
            raise RuntimeError("the voxel map is on %s but the poses on %s" % (self.device, poses.device))
        p = _pose_rows(poses, N, self.device)
        if images is not None:
            if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or tuple(images.shape) != (N, 3, H, W):
                raise RuntimeError("expected images [%d,3,%d,%d] uint8, got %s %s" %
                                   (N, H, W, tuple(getattr(images, "shape", ())), getattr(images, "dtype", None)))
            if images.device != self.device:
                raise RuntimeError("the voxel map is on %s but the images on %s" % (self.device, images.device))
            images = images.detach().contiguous()
        if self.has_colors is not None and self.has_colors != (images is not None):
            raise RuntimeError("a voxel map is coloured by every integrate or by none")
        ix = None if indices is None else _index_tensor(indices, "indices", self.device).reshape(-1)
        K = N if ix is None else int(ix.shape[0])
        if K < 1:
            raise RuntimeError("integrate: no keyframe")
        if mask is not None:
            if mask.device != self.device:
                raise RuntimeError("the voxel map is on %s but the mask on %s" % (self.device, mask.device))
            mask = _byte_plane(mask, "a mask", K, H, W)
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1, got %d" % stride)
        pixels = K * ((H + stride - 1) // stride) * ((W + stride - 1) // stride)
        if self._points_bound + pixels > MAX_POINTS:
            raise RuntimeError("the voxel map could pass 2^31 - 1 points (%d so far, %d in this call): its sums are sized for fewer"
                               % (self._points_bound, pixels))
        fx, fy, cx, cy = intrinsics(calib)
        need = 2 * (self._counts["voxels"] + pixels)
        capacity = self.capacity
        while capacity < need:
            capacity *= 2
        if capacity > 2 ** 31:
            raise RuntimeError("the voxel map would need more than 2^31 slots")
        if capacity != self.capacity:
            self._grow(capacity)
        self.has_colors = images is not None
        self._extraction = None
        self._points_bound += pixels
        pending = torch.empty((K, H, W), dtype=torch.uint8, device=self.device)

        def run(mask_, retry, pending_):
            self._call("atdn_voxel_integrate", _ptr(depth), _ptr(p), _ptr(images), _ptr(mask_), _ptr(ix), N, K, H, W, fx, fy, cx, cy,
                       stride, self.voxel, self.origin[0], self.origin[1], self.origin[2], self.min_z, self.max_z, retry,
                       _ptr(self.table), self.capacity, _ptr(pending_))

        run(mask, 0, pending)
        counts = self._read_counts()
        for _ in range(_GROW_ROUNDS):
            if counts["dropped"] == 0:
                break
            if self.capacity >= 2 ** 31:
                break
            self._grow(self.capacity * 2)
            again = torch.empty_like(pending)
            run(pending, 1, again)
            pending = again
            counts = self._read_counts()
        if counts["dropped"] != 0:
            raise RuntimeError("the voxel map dropped %d points after growing to %d slots" % (counts["dropped"], self.capacity))
        return self.counts

    # ------------------------------------------------------------------ reading
    def extract(self, min_count=1):
        """The voxels with at least `min_count` points, in ascending key order, on the map's device: `(points [M,3] float32,
        colors [M,3] uint8 or None, counts [M] int32, keys [M] int64)`."""
        min_count = int(min_count)
        if min_count < 1:
            raise ValueError("min_count must be >= 1, got %d" % min_count)
        max_out = max(1, self._counts["voxels"])
        points = torch.empty((max_out, 3), dtype=torch.float32, device=self.device)
        colors = torch.empty((max_out, 3), dtype=torch.uint8, device=self.device) if self.has_colors else None
        counts = torch.empty((max_out,), dtype=torch.int32, device=self.device)
        keys = torch.empty((max_out,), dtype=torch.int64, device=self.device)
        found = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._call("atdn_voxel_extract", _ptr(self.table), self.capacity, min_count, self.voxel, self.origin[0], self.origin[1],
                   self.origin[2], max_out, _ptr(points), _ptr(colors), _ptr(counts), _ptr(keys), _ptr(found))
        M = min(int(found.item()), max_out)
        points, counts, keys = points[:M], counts[:M], keys[:M]
        colors = None if colors is None else colors[:M]
        if self.device.type == "cuda":                      # the kernel emits in table order
            keys, order = torch.sort(keys)
            points, counts = points[order], counts[order]
            colors = None if colors is None else colors[order]
        return points, colors, counts, keys

    def render(self, poses, calib, hw, min_count=1, splat=1.0, max_splat=64, near=None, far=None):
        """The cloud seen from the cameras `poses` ([B,12], [B,3,4] or [B,4,4]; rows of [R|t], world <- camera) under `calib` at
        `hw` = (H, W): `transforms.render_points` of the extraction, with this map's `voxel` as the splat's unit and, by default,
        its `min_z` and `max_z` as `near` and `far`. Returns `(depth [B,H,W] float32, colors [B,3,H,W] uint8 or None, support
        [B,H,W] uint8, counts [B,3] int64)` on the map's device. The extraction (every voxel; `min_count` is applied by the
        render) is kept until the next `integrate`, so repeated renders do not extract again."""
        from .transforms import render_points
        if self._extraction is None:
            self._extraction = self.extract(1)[:3]
        points, colors, counts = self._extraction
        return render_points(points, colors, counts, poses, calib, hw, self.voxel, splat=splat, max_splat=max_splat,
                             near=self.min_z if near is None else near, far=self.max_z if far is None else far,
                             min_count=min_count)

    # ------------------------------------------------------------------ carving
    def votes(self, depth, poses, calib, indices=None, batch=8, **thresholds):
        """Visibility votes of every voxel of the map (`extract(1)`) against the keyframes `indices` (a host sequence or a tensor;
        the whole bank by default) of the banks `depth` [N,H,W] and `poses`: `transforms.visibility_votes`, where the rule and the
        `thresholds` near, far, rel, abs_tol, radius are described; `near` and `far` default to this map's `min_z` and `max_z`,
        `abs_tol` to its `voxel`. The keyframes go `batch` at a time through the index list, accumulated on the device. Returns
        `(keys [M] int64, votes [M,3] int32 = in view, support, free)` on the map's device, in ascending key order."""
        from .transforms import visibility_votes
        points, _, _, keys = self.extract(1)
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise RuntimeError("expected a depth bank [N,H,W], got %s" % (tuple(getattr(depth, "shape", ())),))
        if depth.device != self.device:
            raise RuntimeError("the voxel map is on %s but the depth on %s" % (self.device, depth.device))
        if depth.dtype != torch.float32 or not depth.is_contiguous():
            depth = depth.detach().float().contiguous()
        N = int(depth.shape[0])
        if isinstance(poses, torch.Tensor) and poses.device != self.device:
            raise RuntimeError("the voxel map is on %s but the poses on %s" % (self.device, poses.device))
        p = _pose_rows(poses, N, self.device)
        ix = _index_tensor(np.arange(N) if indices is None else indices, "indices", self.device).reshape(-1)
        options = dict(near=self.min_z, far=self.max_z, abs_tol=self.voxel)
        options.update(thresholds)
        batch = max(1, int(batch))
        votes = torch.zeros((int(points.shape[0]), 3), dtype=torch.int32, device=self.device)
        for a in range(0, int(ix.shape[0]), batch):
            visibility_votes(points, depth, p, calib, indices=ix[a:a + batch], out=votes, **options)
        return keys, votes

    def remove(self, keys):
        """Empty the voxels `keys` (int64, a tensor on the map's device or a host sequence): their counts and sums become 0, their
        slots stay (atdn_voxel_remove in include/atdn_hip.h), so `extract` no longer returns them and a later `integrate` refills
        them like any voxel. `counts` is unchanged: `inserted` keeps meaning points ever inserted and `voxels` occupied slots.
        What was removed is added to the host-side `removed` dict (voxels, points). Returns (voxels emptied, points they held,
        keys not found or already empty) as host ints."""
        if isinstance(keys, torch.Tensor):
            if keys.device != self.device:
                raise RuntimeError("the voxel map is on %s but the keys on %s" % (self.device, keys.device))
            k = keys.detach().reshape(-1)
            if k.dtype != torch.int64:
                raise RuntimeError("keys must be int64, got %s" % k.dtype)
            k = k.contiguous()
        else:
            k = torch.from_numpy(np.asarray(keys, dtype=np.int64).reshape(-1)).to(self.device)
        R = int(k.shape[0])
        removed = torch.empty((3,), dtype=torch.int64, device=self.device)
        self._extraction = None
        self._call("atdn_voxel_remove", _ptr(self.table), self.capacity, _ptr(k) if R else None, None, R, _ptr(removed))
        voxels, points, missing = (int(v) for v in removed.cpu().tolist())
        self.removed["voxels"] += voxels
        self.removed["points"] += points
        return voxels, points, missing

    def carve(self, depth, poses, calib, indices=None, min_free=2, ratio=1.0, min_support=0, batch=8, **thresholds):
        """Free-space carving: vote (`votes`, with its `thresholds`), decide, remove. A voxel goes iff
        `(free >= min_free) & (free > ratio * support) | (support < min_support)`: at least `min_free` keyframes see straight
        through it and more than `ratio` times as many as confirm it, or fewer than `min_support` confirm it (0: never). Returns a
        report (dict): `voxels` before, `removed_voxels`, `removed_points`, and `free_hist` / `support_hist`, the numbers of
        voxels with 0, 1, .. 7 and 8 or more free / support votes."""
        keys, votes = self.votes(depth, poses, calib, indices=indices, batch=batch, **thresholds)
        support, free = votes[:, 1], votes[:, 2]
        go = ((free >= int(min_free)) & (free.double() > float(ratio) * support.double())) | (support < int(min_support))
        voxels, points, _ = self.remove(keys[go])
        hist = [torch.bincount(v.clamp(max=8).long(), minlength=9).cpu().tolist() for v in (free, support)]
        return dict(voxels=int(keys.shape[0]), removed_voxels=voxels, removed_points=points, free_hist=hist[0], support_hist=hist[1])

    def save_ply(self, path, min_count=1):
        """Write the cloud as a binary little-endian PLY: x y z float, red green blue uchar (a coloured map only), count int.
        Returns the number of points."""
        points, colors, counts, _ = self.extract(min_count)
        write_ply(path, points.cpu().numpy(), None if colors is None else colors.cpu().numpy(), counts.cpu().numpy())
        return int(points.shape[0])

    @staticmethod
    def load_ply(path):
        """What `save_ply` wrote, as host tensors `(points [M,3] float32, colors [M,3] uint8 or None, counts [M] int32)`."""
        points, colors, counts = read_ply(path)
        return (torch.from_numpy(points), None if colors is None else torch.from_numpy(colors), torch.from_numpy(counts))


def _ply_dtype(colored):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if colored:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields + [("count", "<i4")])


def write_ply(path, points, colors, counts):
    dt = _ply_dtype(colors is not None)
    rows = np.empty((points.shape[0],), dtype=dt)
    for a, name in enumerate(("x", "y", "z")):
        rows[name] = points[:, a]
    if colors is not None:
        for a, name in enumerate(("red", "green", "blue")):
            rows[name] = colors[:, a]
    rows["count"] = counts
    names = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<i4": "int"}
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % rows.shape[0]]
    head += ["property %s %s" % (names[dt[name].str], name) for name in dt.names]
    head.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(rows.tobytes())


def read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if head[0] != "ply" or head[1] != "format binary_little_endian 1.0":
        raise ValueError("%s is not a binary little-endian PLY" % path)
    n = int([h for h in head if h.startswith("element vertex ")][0].split()[2])
    props = [h.split()[2] for h in head if h.startswith("property ")]
    colored = "red" in props
    dt = _ply_dtype(colored)
    if props != list(dt.names):
        raise ValueError("%s: unexpected properties %s" % (path, props))
    rows = np.frombuffer(data, dtype=dt, count=n, offset=end)
    points = np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)
    colors = np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).astype(np.uint8) if colored else None
    return points, colors, rows["count"].astype(np.int32)
