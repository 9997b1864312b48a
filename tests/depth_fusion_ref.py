"""NumPy float64 restatement of the depth-fusion rule (include/atdn_hip.h, atdn_depth_fuse) and the scene generator of its tests:
helper of the depth-fusion tests, not a test, and not a call into the library.

Every array operation below is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the
rule states; see `fuse_ref`. The rule has only + - * /, floor, |.| and comparisons, all correctly rounded in IEEE arithmetic, so
every correct float64 evaluation gives the same bits — unless a decision quantity sits on its threshold. `margin` is the smallest
relative distance of any decision quantity from its threshold over the pixels where that decision is taken: Xs_2 and Yt_2 from
min_z, u from 0 and W-1 and v from 0 and H-1 (relative to W-1, H-1), e2 from max_reproj^2, rd from max_rel_depth. MIN_MARGIN and
its reasoning are those of tests/two_view_ref.py: 1e-9 is six orders of magnitude above float64 rounding of these expressions, so
the tests compare exactly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from two_view_ref import MIN_MARGIN, euler_yxz, scene_calib  # noqa: E402,F401


def relative_pose(Pi, Pj):
    """(R [3,3], t [3]) float64 with X_j = R X_i + t, from two float32 rows of [R|t] (world <- camera)."""
    A, B = np.asarray(Pi), np.asarray(Pj)
    assert A.dtype == np.float32 and B.dtype == np.float32 and A.shape == (12,) and B.shape == (12,)
    A, B = A.astype(np.float64).reshape(3, 4), B.astype(np.float64).reshape(3, 4)
    ri, ti, rj, tj = A[:, :3], A[:, 3], B[:, :3], B[:, 3]
    d = ti - tj
    R, t = np.zeros((3, 3)), np.zeros(3)
    with np.errstate(all="ignore"):
        for k in range(3):
            for l in range(3):
                R[k, l] = (rj[0, k] * ri[0, l] + rj[1, k] * ri[1, l]) + rj[2, k] * ri[2, l]
            t[k] = (rj[0, k] * d[0] + rj[1, k] * d[1]) + rj[2, k] * d[2]
    return R, t


def _rel(q, thr, where):
    d = np.abs(q - thr) / (abs(thr) if thr != 0 else 1.0)
    d = np.where(where & np.isfinite(d), d, np.inf)
    return float(d.min()) if d.size else np.inf


def fuse_ref(bank, poses, target, sources, calib, max_reproj=1.0, max_rel_depth=0.01, min_views=2, min_z=0.1, average=True):
    """bank [N,H,W] float32, poses [N,12] float32, one target, its source list -> dict(fused [H,W] float32, views [H,W] uint8,
    counts [3] int32, margin, ok [S,H,W] bool, consistent [S,H,W] bool); the last two are False in skipped slots."""
    bank, poses = np.asarray(bank), np.asarray(poses)
    assert bank.dtype == np.float32 and bank.ndim == 3 and poses.dtype == np.float32 and poses.shape == (bank.shape[0], 12)
    N, H, W = bank.shape
    S = len(sources)
    fx, fy, cx, cy = (float(v) for v in calib)
    oks, cons = np.zeros((S, H, W), dtype=bool), np.zeros((S, H, W), dtype=bool)
    i = int(target)
    if i < 0 or i >= N:
        return dict(fused=np.zeros((H, W), np.float32), views=np.zeros((H, W), np.uint8), counts=np.zeros(3, np.int32),
                    margin=np.inf, ok=oks, consistent=cons)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    zf = bank[i]
    margin = np.inf
    with np.errstate(all="ignore"):
        has = zf > 0
        z = zf.astype(np.float64)
        a0, a1 = (xs - cx) / fx, (ys - cy) / fy
        X0, X1, X2 = z * a0, z * a1, z
        n = np.zeros((H, W), dtype=np.int64)
        zsum = z.copy()
        seen = np.zeros((H, W), dtype=bool)
        thr = max_reproj * max_reproj
        for s, j in enumerate(int(v) for v in sources):
            if j < 0 or j >= N or j == i:
                continue
            R, t = relative_pose(poses[i], poses[j])
            Xs = [((R[k, 0] * X0 + R[k, 1] * X1) + R[k, 2] * X2) + t[k] for k in range(3)]
            front = has & (Xs[2] >= min_z)
            u = fx * (Xs[0] / Xs[2]) + cx
            v = fy * (Xs[1] / Xs[2]) + cy
            inside = front & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            us, vs = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
            xf, yf = np.floor(us), np.floor(vs)
            ax, ay = us - xf, vs - yf
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            xn, yn = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            wx, wy = 1.0 - ax, 1.0 - ay
            D = bank[j]
            f00, f10, f01, f11 = D[y0, x0], D[y0, xn], D[yn, x0], D[yn, xn]
            t00, t10, t01, t11 = (f.astype(np.float64) for f in (f00, f10, f01, f11))
            top = t00 * wx + t10 * ax
            bot = t01 * wx + t11 * ax
            ds = top * wy + bot * ay
            ok = inside & (f00 > 0) & (f10 > 0) & (f01 > 0) & (f11 > 0)
            q0, q1 = (u - cx) / fx, (v - cy) / fy
            Y0, Y1, Y2 = ds * q0 - t[0], ds * q1 - t[1], ds - t[2]
            Yt = [(R[0, k] * Y0 + R[1, k] * Y1) + R[2, k] * Y2 for k in range(3)]
            back = ok & (Yt[2] >= min_z)
            xr = fx * (Yt[0] / Yt[2]) + cx
            yr = fy * (Yt[1] / Yt[2]) + cy
            ex, ey = xr - xs, yr - ys
            e2 = ex * ex + ey * ey
            rd = np.abs(Yt[2] - z) / z
            consistent = back & (e2 <= thr) & (rd <= max_rel_depth)
            n = n + consistent
            zsum = np.where(consistent, zsum + Yt[2], zsum)
            seen |= ok
            oks[s], cons[s] = ok, consistent
            fin = front & np.isfinite(u) & np.isfinite(v)
            margin = min(margin, _rel(Xs[2], min_z, has), _rel(Yt[2], min_z, ok), _rel(e2, thr, back), _rel(rd, max_rel_depth, back),
                         _rel(u / max(W - 1, 1), 0.0, fin), _rel(u / max(W - 1, 1), 1.0 if W > 1 else 0.0, fin),
                         _rel(v / max(H - 1, 1), 0.0, fin), _rel(v / max(H - 1, 1), 1.0 if H > 1 else 0.0, fin))
        kept = has & (n >= min_views)
        value = zsum / (n + 1).astype(np.float64) if average else z
        fused = np.where(kept, value, 0.0).astype(np.float32)
    counts = np.array([has.sum(), (has & seen).sum(), kept.sum()], dtype=np.int32)
    return dict(fused=fused, views=n.astype(np.uint8), counts=counts, margin=margin, ok=oks, consistent=cons)


def reference_batch(bank, poses, targets, sources, calib, **kw):
    """The helper over a batch: (fused [B,1,H,W] float32, views [B,H,W] uint8, counts [B,3] int32, smallest margin)."""
    out = [fuse_ref(bank, poses, t, list(np.asarray(sources).reshape(len(targets), -1)[b]), calib, **kw)
           for b, t in enumerate(targets)]
    return (np.stack([o["fused"] for o in out])[:, None], np.stack([o["views"] for o in out]),
            np.stack([o["counts"] for o in out]), min(o["margin"] for o in out))


GROUND, LEFT, RIGHT, FRONT = 1.65, -5.0, 6.0, 60.0


def analytic_depth(P12, calib, H, W):
    """The depth of every pixel of a camera with pose P12 (float32 rows of [R|t], world <- camera) in the scene of planes: the
    ground Y = 1.65, walls X = -5 and X = 6, a front wall Z = 60, by closed-form ray intersection (the nearest hit). float64."""
    fx, fy, cx, cy = calib
    M = np.asarray(P12, dtype=np.float32).astype(np.float64).reshape(3, 4)
    R, t = M[:, :3], M[:, 3]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)])
    d = np.einsum("ij,jhw->ihw", R, a)                      # the ray in world axes; the camera-frame depth is the ray parameter
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for axis, level in ((1, GROUND), (0, LEFT), (0, RIGHT), (2, FRONT)):
            s = (level - t[axis]) / d[axis]
            best = np.where((s > 0) & np.isfinite(s) & (s < best), s, best)
    assert np.isfinite(best).all()
    return best


def scene(H, W, N, seed, holes=0.1, disturbance=0.002, outlier_view=1, outlier=1.3, step=0.8):
    """A synthetic keyframe map: (bank [N,H,W] float32, poses [N,12] float32, calib, Z [N,H,W] float64 the analytic depth). The
    camera drives forward (`step` per keyframe, small random rotations and side steps); the poses are rounded to float32 BEFORE
    the depths are generated, so the analytic depth is that of the poses the rule sees. Then per view a smooth multiplicative
    disturbance of relative size `disturbance`, a block of view `outlier_view` scaled by `outlier`, and a share `holes` of pixels
    without a depth."""
    rs = np.random.RandomState(seed)
    calib = scene_calib(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    poses = np.zeros((N, 12), dtype=np.float32)
    Z = np.zeros((N, H, W))
    bank = np.zeros((N, H, W))
    for k in range(N):
        R = euler_yxz(rs.uniform(-0.02, 0.02, 3))
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.03, 0.03), step * k + rs.uniform(-0.1, 0.1)])
        poses[k] = np.concatenate([R, t[:, None]], axis=1).astype(np.float32).reshape(12)
        Z[k] = analytic_depth(poses[k], calib, H, W)
        d = Z[k] * (1.0 + disturbance * np.sin(2 * np.pi * (1.3 * xs / W + 0.7 * ys / H) + 0.9 * k + 0.37 * seed))
        if k == outlier_view and outlier != 1.0:
            y0, x0 = H // 4, W // 3
            y1, x1 = max(y0 + 1, H // 2), max(x0 + 1, W // 2)
            d[y0:y1, x0:x1] *= outlier
        d[rs.uniform(size=(H, W)) < holes] = 0.0
        bank[k] = d
    return bank.astype(np.float32), poses, calib, Z


def all_sources(N):
    """targets 0 .. N-1, each with every other view as a source, in order: (targets [N], sources [N, N-1]) int32."""
    return (np.arange(N, dtype=np.int32),
            np.array([[j for j in range(N) if j != i] for i in range(N)], dtype=np.int32).reshape(N, max(N - 1, 0)))


# (name, H, W, N, seed, min_views) of the random cases shared by the host and the GPU tests; thresholds 1 px / 1 % / min_z 0.1
CASES = [("5x7", 5, 7, 3, 2, 1), ("9x33", 9, 33, 4, 1, 2), ("8x16", 8, 16, 3, 1, 1), ("47x154", 47, 154, 6, 1, 2)]
FULL_CASE = ("376x1232", 376, 1232, 5, 1, 2)


def check_reference(bank, poses, targets, sources, calib, strict=True, **kw):
    """The reference of a call, after asserting on the helper alone that it decides nothing by a tie (margin >= 1e-9) and, with
    `strict`, that every outcome occurs: 0 < kept < seen < has < H * W per target and at least three distinct `views` values."""
    fused, views, counts, margin = reference_batch(bank, poses, targets, sources, calib, **kw)
    assert margin >= MIN_MARGIN, margin
    if strict:
        n = bank.shape[1] * bank.shape[2]
        for c in counts:
            assert 0 < c[2] < c[1] < c[0] < n, counts.tolist()
        assert len(np.unique(views)) >= 3, np.unique(views)
    return fused, views, counts


def check_case(H, W, N, seed, min_views, average=True, **scene_kw):
    """The scene of a case, all targets with all other views as sources, and its checked reference."""
    bank, poses, calib, Z = scene(H, W, N, seed, **scene_kw)
    targets, sources = all_sources(N)
    fused, views, counts = check_reference(bank, poses, targets, sources, calib, min_views=min_views, average=average)
    return bank, poses, calib, Z, targets, sources, fused, views, counts
