"""NumPy float64 restatement of the pose-from-depth rule (include/atdn_hip.h, atdn_pnp_terms and atdn_pnp_solve) and the scene
generator of its tests: helper of the PnP tests, not a test, and not a call into the library.

Every array operation below is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the
rule states. The rule has only + - * / and comparisons, all correctly rounded, and it fixes the order of every sum — four pixels
per thread, a binary tree over the 256 threads of a chunk (`reshape` and pairwise adds of neighbours), the chunks in order
(`cumsum`, which adds sequentially) — so every correct evaluation gives the same bits, unless a decision quantity sits on its
threshold. `margin` is the smallest relative distance of Z from min_z (over the candidates) and of e2 from inlier_px^2 (over the
used pixels), at every pose that was evaluated; with 1e-9 — six orders of magnitude above float64 rounding of these expressions —
the tests compare exactly. (x2 and y2 are exact sums; the scenes keep them off the image border by construction of the flow.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from two_view_ref import euler_yxz, scene  # noqa: E402

MIN_MARGIN = 1e-9
FLT_MAX = float(np.finfo(np.float32).max)
DEFAULTS = dict(scale_px=4.0, inlier_px=2.0, min_z=0.1)
CHUNK = 1024


def internal_pose(pose12):
    """12 float32 (rows of [R|t], X1 = R X2 + t) -> (Rc [3,3], tc [3]) float64 with X2 = Rc X1 + tc."""
    M = np.asarray(pose12, dtype=np.float32).astype(np.float64).reshape(3, 4)
    r, t = M[:, :3], M[:, 3]
    Rc = r.T.copy()
    tc = np.array([-((r[0, i] * t[0] + r[1, i] * t[1]) + r[2, i] * t[2]) for i in range(3)])
    return Rc, tc


def public_pose(Rc, tc):
    out = np.zeros((3, 4), dtype=np.float32)
    out[:, :3] = Rc.T.astype(np.float32)
    for i in range(3):
        out[i, 3] = np.float32(-((Rc[0, i] * tc[0] + Rc[1, i] * tc[1]) + Rc[2, i] * tc[2]))
    return out.reshape(12)


def plane_sum(t):
    """t [..., n] float64 per-pixel values in flat-index order -> the plane sum in the rule's order."""
    n = t.shape[-1]
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(t.shape[:-1] + (chunks * CHUNK,), dtype=t.dtype)
    pad[..., :n] = t
    q = pad.reshape(t.shape[:-1] + (chunks, 256, 4))
    v = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return np.cumsum(v[..., 0], axis=-1)[..., -1]


def terms_ref(depth, flow, Rc, tc, calib, mask=None, scale_px=4.0, inlier_px=2.0, min_z=0.1):
    """depth [H,W] float32, flow [2,H,W] float32, internal pose, calib (fx, fy, cx, cy), mask [H,W] or None ->
    (sums [28] float64, counts [3] int32, margin)."""
    d, f = np.asarray(depth), np.asarray(flow)
    assert d.dtype == np.float32 and f.dtype == np.float32 and f.ndim == 3 and f.shape[0] == 2
    fx, fy, cx, cy = (float(v) for v in calib)
    _, H, W = f.shape
    d = d.reshape(H, W)
    c2, thr = scale_px * scale_px, inlier_px * inlier_px
    eb = float(H + W)
    e2b = eb * eb
    rho_behind = (0.5 * e2b) / (1.0 + e2b / c2)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z, u, v = d.astype(np.float64), f[0].astype(np.float64), f[1].astype(np.float64)
    keep = np.ones((H, W), dtype=bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    with np.errstate(all="ignore"):
        x2, y2 = xs + u, ys + v
        cand = keep & (z > 0) & (z <= FLT_MAX) & (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1)
        X1, Y1 = (z * (xs - cx)) / fx, (z * (ys - cy)) / fy
        X, Y, Z = [((Rc[i, 0] * X1 + Rc[i, 1] * Y1) + Rc[i, 2] * z) + tc[i] for i in range(3)]
        used = cand & (Z >= min_z)
        iz = 1.0 / Z
        px, py = (fx * X) * iz, (fy * Y) * iz
        rx, ry = (px + cx) - x2, (py + cy) - y2
        e2 = rx * rx + ry * ry
        s = 1.0 + e2 / c2
        w = 1.0 / (s * s)
        rho = (0.5 * e2) / s
        inlier = used & (e2 <= thr)
        a, k = fx * iz, fy * iz
        b, dd = -(px * iz), -(py * iz)
        zero = np.zeros_like(a)
        Jx = [b * Y, a * Z - b * X, -(a * Y), a, zero, b]
        Jy = [dd * Y - k * Z, -(dd * X), k * X, zero, k, dd]
        t = []
        for i in range(6):
            for j in range(i, 6):
                t.append((w * Jx[i]) * Jx[j] + (w * Jy[i]) * Jy[j])
        for i in range(6):
            t.append((w * Jx[i]) * rx + (w * Jy[i]) * ry)
        t.append(rho)
        t = np.stack(t)
        t = np.where(used[None], t, 0.0)
        t[27] = np.where(cand & ~used, rho_behind, t[27])
        sums = plane_sum(t.reshape(28, H * W))

        def rel(q, thr_, where):
            dist = np.abs(q - thr_) / abs(thr_)
            dist = np.where(where & np.isfinite(dist), dist, np.inf)
            return float(dist.min()) if dist.size else np.inf

        margin = min(rel(Z, min_z, cand), rel(e2, thr, used))
    counts = np.array([cand.sum(), used.sum(), inlier.sum()], dtype=np.int32)
    return sums, counts, margin


def lm_step(H21, g, lam, Rc, tc):
    """The damped step of the rule from the accepted point: (Rc', tc'), or (Rc, tc) again where the factorisation fails."""
    A = np.zeros((6, 6))
    n = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = H21[n]
            n += 1
    for i in range(6):
        A[i, i] = A[i, i] + lam * A[i, i]
    L, D = np.zeros((6, 6)), np.zeros(6)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j, j]
            for k in range(j):
                dj = dj - L[j, k] * (L[j, k] * D[k])
            ok = ok and bool(dj > 0.0)
            D[j] = dj
            for i in range(j + 1, 6):
                l = A[i, j]
                for k in range(j):
                    l = l - L[i, k] * (L[j, k] * D[k])
                L[i, j] = l / dj
        dl = np.zeros(6)
        for i in range(6):
            y = -g[i]
            for k in range(i):
                y = y - L[i, k] * dl[k]
            dl[i] = y
        for i in range(6):
            dl[i] = dl[i] / D[i]
        for i in range(5, -1, -1):
            y = dl[i]
            for k in range(i + 1, 6):
                y = y - L[k, i] * dl[k]
            dl[i] = y
        ok = ok and bool(np.all(np.abs(dl) <= np.finfo(np.float64).max))
        if not ok:
            return Rc.copy(), tc.copy()
        h = 0.5 * dl[:3]
        n2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
        f = 2.0 / (1.0 + n2)
        K = np.array([[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]])
        E = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                hh = h[i] * h[j]
                E[i, j] = 1.0 + f * (hh - n2) if i == j else f * (K[i, j] + hh)
        R2, t2 = np.zeros((3, 3)), np.zeros(3)
        for i in range(3):
            for j in range(3):
                R2[i, j] = (E[i, 0] * Rc[0, j] + E[i, 1] * Rc[1, j]) + E[i, 2] * Rc[2, j]
            t2[i] = ((E[i, 0] * tc[0] + E[i, 1] * tc[1]) + E[i, 2] * tc[2]) + dl[3 + i]
    return R2, t2


def solve_ref(depth, flow, pose12, calib, mask=None, iters=16, **kw):
    """One problem: (pose_out [12] float32, cost float64, counts [4] int32, margin)."""
    pose12 = np.asarray(pose12, dtype=np.float32).reshape(12)
    Rt, tt = internal_pose(pose12)
    margin = np.inf
    lam, accepted = 1e-3, 0
    for k in range(iters + 1):
        sums, counts, m = terms_ref(depth, flow, Rt, tt, calib, mask, **kw)
        margin = min(margin, m)
        if k == 0 or sums[27] < acc_sums[27]:
            Ra, ta, acc_sums, acc_counts = Rt, tt, sums, counts
            if k > 0:
                lam = max(lam / 3.0, 1e-9)
                accepted += 1
        else:
            lam = min(4.0 * lam, 1e6)
        if k < iters:
            Rt, tt = lm_step(acc_sums[:21], acc_sums[21:27], lam, Ra, ta)
    out = pose12.copy() if accepted == 0 else public_pose(Ra, ta)
    return out, np.float64(acc_sums[27]), np.concatenate([acc_counts, [accepted]]).astype(np.int32), margin


def terms_batch(depth, flow, pose, calib, mask=None, **kw):
    """(sums [B,28], counts [B,3], smallest margin) at the public poses [B,12]."""
    out = [terms_ref(depth[b], flow[b], *internal_pose(pose[b]), calib, None if mask is None else mask[b], **kw)
           for b in range(flow.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), min(o[2] for o in out)


def solve_batch(depth, flow, pose, calib, mask=None, iters=16, **kw):
    """(pose [B,12] float32, cost [B] float64, counts [B,4] int32, smallest margin)."""
    out = [solve_ref(depth[b], flow[b], pose[b], calib, None if mask is None else mask[b], iters, **kw)
           for b in range(flow.shape[0])]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.float64), np.stack([o[2] for o in out]),
            min(o[3] for o in out))


def pnp_scene(H, W, seed, B=1, noise_free=False):
    """A synthetic PnP scene from two_view_ref.scene's smooth depth (disturbance 0) with its own, larger motion: rotations up to
    0.08 rad, t = (U(+-0.3), U(+-0.15), U(1, 3)). Returns (depth [B,H,W] float32, flow [B,2,H,W] float32, pose_true [B,12]
    float32, pose_start [B,12] float32, calib). The flow is that of the float32 depth and the float32 true pose. Unless
    `noise_free`: 20 % of the depths are holes (0), 10 % of the flows are off by +-25 px (+-0.45 of the image's width and
    height where that is less, so that some outliers stay inside a small image), and a patch holds depths below t_z, so
    that its points lie behind camera 2 at the true pose and at the start; the start is the true pose turned by 0.03 rad and
    moved by 0.4 m."""
    rs = np.random.RandomState(1000 + seed)
    _, _, calib, Z = scene(H, W, seed, B, 0.0)
    fx, fy, cx, cy = calib
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((B, H, W), dtype=np.float32)
    flow = np.zeros((B, 2, H, W), dtype=np.float32)
    true = np.zeros((B, 12), dtype=np.float32)
    start = np.zeros((B, 12), dtype=np.float32)
    for b in range(B):
        R = euler_yxz(rs.uniform(-0.08, 0.08, 3))
        t = np.array([rs.uniform(-0.3, 0.3), rs.uniform(-0.15, 0.15), rs.uniform(1.0, 3.0)])
        P = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
        z = Z[b].astype(np.float32)
        if not noise_free:
            ph, pw = max(1, H // 4), max(2, W // 5)
            y0, x0 = H // 3, W // 2
            z[y0:y0 + ph, x0:x0 + pw] = np.float32(0.45 * float(P[2, 3])) * (1.0 + 0.1 * rs.uniform(size=z[y0:y0 + ph, x0:x0 + pw].shape)).astype(np.float32)
        zd = z.astype(np.float64)
        R32, t32 = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
        X1 = np.stack([zd * (xs - cx) / fx, zd * (ys - cy) / fy, zd])
        X2 = np.einsum("ji,jhw->ihw", R32, X1 - t32[:, None, None])
        with np.errstate(all="ignore"):
            u = fx * X2[0] / X2[2] + cx - xs
            v = fy * X2[1] / X2[2] + cy - ys
        behind = X2[2] < 0.2
        # points behind camera 2 have no image: give them a small flow, so that they stay candidates
        u = np.where(behind, 0.5, u)
        v = np.where(behind, -0.25, v)
        if not noise_free:
            out = rs.uniform(size=(H, W)) < 0.10
            ou, ov = min(25.0, 0.45 * W), min(25.0, 0.45 * H)
            u = np.where(out, u + rs.choice([-ou, ou], size=(H, W)), u)
            v = np.where(out, v + rs.choice([-ov, ov], size=(H, W)), v)
            z = np.where(rs.uniform(size=(H, W)) < 0.20, np.float32(0.0), z)
        dR = euler_yxz(0.03 * np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62]))
        dt = 0.4 * np.array([0.5, -0.3, 0.81]) / np.linalg.norm([0.5, -0.3, 0.81])
        S = np.concatenate([dR @ R, (t + dt)[:, None]], axis=1).astype(np.float32)
        depth[b], flow[b, 0], flow[b, 1] = z, u.astype(np.float32), v.astype(np.float32)
        true[b], start[b] = P.reshape(12), S.reshape(12)
    return depth, flow, true, start, calib


# (name, H, W, B, seed): the cases shared by the host and the GPU tests. 47x154 has 8 chunks: the chunk order matters.
# The seeds are the first for which the helper alone meets the conditions of check_case.
CASES = [("5x7", 5, 7, 1, 8), ("9x33_b3", 9, 33, 3, 1), ("8x16_b2", 8, 16, 2, 2), ("47x154_b2", 47, 154, 2, 3)]
RECOVERY_CASE = ("47x154_b2", 47, 154, 2, 5)
FULL_CASE = ("376x1232_b2", 376, 1232, 2, 6)
_cache = {}


def check_case(H, W, B, seed, iters=16, start_inliers=True):
    """The scene of a case with its references (computed once per process), after asserting on the helper alone that the case
    decides nothing by a tie and takes every branch at the start pose: margin >= 1e-9 at every evaluated pose and
    0 < inliers < used < candidates < H * W in every image (`start_inliers=False` drops `0 < inliers`: at 376 x 1232 the focal
    length is 714 px and a start 0.03 rad off is 20 px off, so no pixel is an inlier there before the first step). Returns a dict: depth, flow, true, start, calib, terms = (sums,
    counts) at the start pose, solve = (pose, cost, counts) after `iters` steps."""
    key = (H, W, B, seed, iters)
    if key not in _cache:
        depth, flow, true, start, calib = pnp_scene(H, W, seed, B)
        sums, counts, m0 = terms_batch(depth, flow, start, calib)
        pose, cost, counts4, m1 = solve_batch(depth, flow, start, calib, iters=iters)
        assert min(m0, m1) >= MIN_MARGIN, (H, W, B, seed, m0, m1)
        for c in counts:
            assert (0 < c[2] or not start_inliers) and c[2] < c[1] < c[0] < H * W, (H, W, B, seed, counts.tolist())
        for a in (depth, flow, true, start, sums, counts, pose, cost, counts4):
            a.setflags(write=False)
        _cache[key] = dict(depth=depth, flow=flow, true=true, start=start, calib=calib, terms=(sums, counts),
                           solve=(pose, cost, counts4))
    return _cache[key]
