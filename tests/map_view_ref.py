"""NumPy restatement of the map-view rule (include/atdn_hip.h, atdn_view_render) and the cloud builders of its tests: helper
of test_map_view_host.py and test_gpu_map_view.py, not a test module. One IEEE float64 operation per element in the rule's
order, np.ceil for the ceil, np.minimum.at on uint64 for the z-buffer. Clouds come from voxel_map_ref (imported, not edited)."""
import numpy as np

import voxel_map_ref as V

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULTS = dict(splat=1.0, max_splat=64, near=0.5, far=40.0, min_count=1)


def _span(centre, half, size):
    """Per point: (ok, lo, hi) of the pixels that [centre - half, centre + half) covers on an axis of `size` pixels."""
    with np.errstate(all="ignore"):
        a = centre - half
        e = centre + half
        last = np.float64(size - 1)
        ok = (a <= last) & (e > 0.0)
        lo = np.where(ok & (a >= 0.0), np.ceil(np.where(ok, a, 0.0)), 0.0)
        hi = np.where(ok & (e <= last), np.ceil(np.where(ok, e, 1.0)) - 1.0, last)
    lo, hi = lo.astype(np.int64), hi.astype(np.int64)
    return ok & (lo <= hi), lo, hi


def words(points, colors, counts, pose, calib, hw, size, splat=1.0, max_splat=64, near=0.5, far=40.0, min_count=1):
    """One camera: (candidate [M] bool, visible [M] bool, x0, x1, y0, y1 [M] int64, word [M] uint64)."""
    fx, fy, cx, cy = (np.float64(v) for v in calib)
    H, W = hw
    P = np.asarray(pose, dtype=np.float32).reshape(12).astype(np.float64)
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    n = np.asarray(counts, dtype=np.int32).reshape(-1).astype(np.int64)
    cand = n >= min_count
    with np.errstate(all="ignore"):
        d = [p[:, 0] - P[3], p[:, 1] - P[7], p[:, 2] - P[11]]
        c = [(P[a] * d[0] + P[4 + a] * d[1]) + P[8 + a] * d[2] for a in range(3)]
        z = c[2]
        inr = (np.float64(near) <= z) & (z <= np.float64(far))
        u = (c[0] / z) * fx + cx
        v = (c[1] / z) * fy + cy
        s = (np.float64(0.5) * np.float64(splat)) * np.float64(size)
        hmax = np.float64(0.5) * np.float64(max_splat)
        hx = (s * fx) / z
        hy = (s * fy) / z
        hx = np.where(hx < 0.5, 0.5, np.where(hx > hmax, hmax, hx))
        hy = np.where(hy < 0.5, 0.5, np.where(hy > hmax, hmax, hy))
        okx, x0, x1 = _span(u, hx, W)
        oky, y0, y1 = _span(v, hy, H)
        vis = cand & inr & okx & oky
        zbits = np.where(vis, z, 1.0).astype(np.float32).view(np.uint32).astype(np.uint64)
    low = (np.uint64(255) - np.minimum(n, 255).astype(np.uint64)) << np.uint64(24)
    if colors is not None:
        col = np.asarray(colors, dtype=np.uint8).reshape(-1, 3).astype(np.uint64)
        low = low | (col[:, 0] << np.uint64(16)) | (col[:, 1] << np.uint64(8)) | col[:, 2]
    return cand, vis, x0, x1, y0, y1, (zbits << np.uint64(32)) | low


def render(points, colors, counts, poses, calib, hw, size, **options):
    """(depth [B,H,W] float32, colors [B,3,H,W] uint8 or None, support [B,H,W] uint8, counts [B,3] int64)."""
    H, W = hw
    poses = np.asarray(poses, dtype=np.float32).reshape(-1, 12)
    B = poses.shape[0]
    depth = np.zeros((B, H, W), dtype=np.float32)
    out_colors = None if colors is None else np.zeros((B, 3, H, W), dtype=np.uint8)
    support = np.zeros((B, H, W), dtype=np.uint8)
    out_counts = np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        cand, vis, x0, x1, y0, y1, word = words(points, colors, counts, poses[b], calib, hw, size, **dict(DEFAULTS, **options))
        zbuf = np.full(H * W, EMPTY, dtype=np.uint64)
        for i in np.flatnonzero(vis):
            ys, xs = np.meshgrid(np.arange(y0[i], y1[i] + 1), np.arange(x0[i], x1[i] + 1), indexing="ij")
            np.minimum.at(zbuf, (ys * W + xs).reshape(-1), word[i])
        covered = zbuf != EMPTY
        w = np.where(covered, zbuf, np.uint64(0xFF000000))
        depth[b] = (w >> np.uint64(32)).astype(np.uint32).view(np.float32).reshape(H, W)
        support[b] = (255 - ((w >> np.uint64(24)) & np.uint64(255)).astype(np.int64)).astype(np.uint8).reshape(H, W)
        if out_colors is not None:
            for a in range(3):
                out_colors[b, a] = ((w >> np.uint64(16 - 8 * a)) & np.uint64(255)).astype(np.uint8).reshape(H, W)
        out_counts[b] = (int(cand.sum()), int(vis.sum()), int(covered.sum()))
    return depth, out_colors, support, out_counts


def same_images(got, want):
    """Two render() tuples (NumPy): equal in every bit."""
    if len(got) != 4 or len(want) != 4:
        return False
    for g, w in zip(got, want):
        if (g is None) != (w is None) or (g is not None and not V.same_bits(g, w)):
            return False
    return True


# ---------------------------------------------------------------------------------------------------- clouds and cases
CASES = V.CASES                                       # 5 x 7 B = 1, 9 x 33 B = 3, 47 x 154 B = 2
FULL_CASE = V.FULL_CASE
VOXEL = 0.25


def cloud(H, W, K, seed, colored=True):
    """The street of voxel_map_ref.scene seen from K cameras, as its restated cloud, and those K poses plus a NaN-free set of
    view poses: dict(points, colors, counts, poses [K,12], calib, hw)."""
    s = V.scene(H, W, K, seed)
    (pts, col, cnt, _), _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"] if colored else None)
    return dict(points=pts, colors=col, counts=cnt, poses=s["poses"].copy(), calib=s["calib"], hw=(H, W))


def variants():
    """(with colours, min_count, splat)"""
    return [(True, 1, 1.0), (False, 1, 0.5), (True, 3, 2.0), (False, 3, 1.0), (True, 1, 0.5), (False, 1, 2.0)]


def hand(xyz, n=None, rgb=None):
    """Hand-placed points: (points [M,3] float32, colors [M,3] uint8 or None, counts [M] int32)."""
    pts = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    cnt = np.ones(len(pts), dtype=np.int32) if n is None else np.asarray(n, dtype=np.int32).reshape(-1)
    col = None if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    return pts, col, cnt
