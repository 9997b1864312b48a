"""NumPy float64 restatement of the pose-from-flow rule (include/atdn_hip.h, atdn_epipolar_terms and atdn_epipolar_solve) and the
scene generator of its tests: helper of the epipolar tests, not a test, and not a call into the library.

Every array operation below is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the
rule states; the plane sum is `pnp_ref.plane_sum` (the rule's tree). The rule has only + - * / and comparisons, so every correct
evaluation gives the same bits unless a decision sits on its threshold. `margin` is the smallest relative distance of every
comparison the rule takes, at every pose that was evaluated: x2 from 0 and W-1, y2 from 0 and H-1 (`inside`; relative to W-1, H-1),
epi2 from inlier_px^2 (`inlier`), and the trial cost from the accepted cost (accept / reject; a trial that IS the accepted pose
again — a failed step — is no decision). With pnp_ref's floor of 1e-9 the tests compare exactly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pnp_ref import MIN_MARGIN, plane_sum  # noqa: E402
from two_view_ref import euler_yxz  # noqa: E402

DBL_MAX = float(np.finfo(np.float64).max)
DEFAULTS = dict(scale_px=2.0, inlier_px=1.0)


def load_pose(pose12):
    """12 float32 (rows of [R|t], X1 = R X2 + t) -> (R [3,3], t [3]) float64."""
    M = np.asarray(pose12, dtype=np.float32).astype(np.float64).reshape(3, 4)
    return M[:, :3].copy(), M[:, 3].copy()


def store_pose(R, t):
    out = np.zeros((3, 4), dtype=np.float32)
    out[:, :3] = R.astype(np.float32)
    out[:, 3] = t.astype(np.float32)
    return out.reshape(12)


def _rel(q, thr, where):
    d = np.abs(q - thr) / (abs(thr) if thr != 0 else 1.0)
    d = np.where(where & np.isfinite(d), d, np.inf)
    return float(d.min()) if d.size else np.inf


def terms_ref(flow, r, t, calib, mask=None, scale_px=2.0, inlier_px=1.0):
    """flow [2,H,W] float32, pose (r [3,3], t [3]) float64, calib (fx, fy, cx, cy), mask [H,W] or None ->
    (sums [28] float64, counts [3] int32, margin)."""
    f = np.asarray(flow)
    assert f.dtype == np.float32 and f.ndim == 3 and f.shape[0] == 2
    fx, fy, cx, cy = (float(v) for v in calib)
    _, H, W = f.shape
    c2, thr = scale_px * scale_px, inlier_px * inlier_px
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = f[0].astype(np.float64), f[1].astype(np.float64)
    keep = np.ones((H, W), dtype=bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    with np.errstate(all="ignore"):
        x2, y2 = xs + u, ys + v
        inside = (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1)
        a0, a1 = (xs - cx) / fx, (ys - cy) / fy
        q0, q1 = (x2 - cx) / fx, (y2 - cy) / fy
        b = [(r[i, 0] * q0 + r[i, 1] * q1) + r[i, 2] for i in range(3)]
        n = [t[1] - t[2] * a1, t[2] * a0 - t[0], t[0] * a1 - t[1] * a0]
        res = (n[0] * b[0] + n[1] * b[1]) + n[2] * b[2]
        m = [(r[0, j] * n[0] + r[1, j] * n[1]) + r[2, j] * n[2] for j in range(2)]
        l0, l1 = m[0] / fx, m[1] / fy
        ll = l0 * l0 + l1 * l1
        epi2 = (res * res) / ll
        cand = keep & inside
        used = cand & (ll > 0) & (epi2 <= DBL_MAX)
        inlier = used & (epi2 <= thr)
        s = 1.0 + epi2 / c2
        w = 1.0 / (s * s)
        rho = (0.5 * epi2) / s
        jr = [b[1] * n[2] - b[2] * n[1], b[2] * n[0] - b[0] * n[2], b[0] * n[1] - b[1] * n[0]]
        k = [a1 * b[2] - b[1], b[0] - a0 * b[2], a0 * b[1] - a1 * b[0]]
        jr += [t[1] * k[2] - t[2] * k[1], t[2] * k[0] - t[0] * k[2], t[0] * k[1] - t[1] * k[0]]
        at = (a0 * t[0] + a1 * t[1]) + t[2]
        e0, e1 = l0 / fx, l1 / fy
        dm = []
        for j in range(2):
            r0, r1, r2 = r[0, j], r[1, j], r[2, j]
            rt = (r0 * t[0] + r1 * t[1]) + r2 * t[2]
            dm.append([r1 * n[2] - r2 * n[1], r2 * n[0] - r0 * n[2], r0 * n[1] - r1 * n[0],
                       rt * a0 - at * r0, rt * a1 - at * r1, rt - at * r2])
        kk = res / (2.0 * ll)
        ww = w / ll
        jd = [jr[i] - kk * (2.0 * (e0 * dm[0][i] + e1 * dm[1][i])) for i in range(6)]
        terms = []
        for i in range(6):
            for j in range(i, 6):
                terms.append((ww * jd[i]) * jd[j])
        for i in range(6):
            terms.append((ww * jd[i]) * res)
        terms.append(rho)
        terms = np.where(used[None], np.stack(terms), 0.0)
        sums = plane_sum(terms.reshape(28, H * W))
        kept = keep & np.isfinite(x2) & np.isfinite(y2)
        margin = min(_rel(epi2, thr, used),
                     _rel(x2 / max(W - 1, 1), 0.0, kept), _rel(x2 / max(W - 1, 1), 1.0 if W > 1 else 0.0, kept),
                     _rel(y2 / max(H - 1, 1), 0.0, kept), _rel(y2 / max(H - 1, 1), 1.0 if H > 1 else 0.0, kept))
    counts = np.array([cand.sum(), used.sum(), inlier.sum()], dtype=np.int32)
    return sums, counts, margin


def cayley(d):
    h = 0.5 * np.asarray(d, dtype=np.float64)
    n2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
    f = 2.0 / (1.0 + n2)
    K = np.array([[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]])
    E = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            hh = h[i] * h[j]
            E[i, j] = 1.0 + f * (hh - n2) if i == j else f * (K[i, j] + hh)
    return E


def retract(r, t, dl):
    """(C(dw) R, C(dth) t) in the rule's order."""
    E, G = cayley(dl[:3]), cayley(dl[3:])
    r2, t2 = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            r2[i, j] = (E[i, 0] * r[0, j] + E[i, 1] * r[1, j]) + E[i, 2] * r[2, j]
        t2[i] = (G[i, 0] * t[0] + G[i, 1] * t[1]) + G[i, 2] * t[2]
    return r2, t2


def lm_step(H21, g, lam, r, t):
    """The damped step of the rule from the accepted point: (R', t', True), or (R, t, False) where it fails."""
    A = np.zeros((6, 6))
    n = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = H21[n]
            n += 1
    with np.errstate(all="ignore"):
        tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
        gamma = ((A[3, 3] + A[4, 4]) + A[5, 5]) / tt
        for i in range(3):
            for j in range(3):
                A[3 + i, 3 + j] = A[3 + i, 3 + j] + (gamma * t[i]) * t[j]
        for i in range(6):
            A[i, i] = A[i, i] + lam * A[i, i]
        L, D = np.zeros((6, 6)), np.zeros(6)
        ok = True
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
        ok = ok and bool(np.all(np.abs(dl) <= DBL_MAX))
        if not ok:
            return r.copy(), t.copy(), False
        r2, t2 = retract(r, t, dl)
    return r2, t2, True


def solve_ref(flow, pose12, calib, mask=None, iters=16, **kw):
    """One problem: (pose_out [12] float32, cost float64, counts [4] int32, margin)."""
    pose12 = np.asarray(pose12, dtype=np.float32).reshape(12)
    rt, tt = load_pose(pose12)
    margin = np.inf
    lam, accepted, stepped = 1e-3, 0, False
    for k in range(iters + 1):
        sums, counts, m = terms_ref(flow, rt, tt, calib, mask, **kw)
        margin = min(margin, m)
        if k > 0 and stepped and acc_sums[27] > 0:
            margin = min(margin, abs(sums[27] - acc_sums[27]) / acc_sums[27])
        if k == 0 or sums[27] < acc_sums[27]:
            ra, ta, acc_sums, acc_counts = rt, tt, sums, counts
            if k > 0:
                lam = max(lam / 3.0, 1e-9)
                accepted += 1
        else:
            lam = min(4.0 * lam, 1e6)
        if k < iters:
            rt, tt, stepped = lm_step(acc_sums[:21], acc_sums[21:27], lam, ra, ta)
    out = pose12.copy() if accepted == 0 else store_pose(ra, ta)
    return out, np.float64(acc_sums[27]), np.concatenate([acc_counts, [accepted]]).astype(np.int32), margin


def terms_batch(flow, pose, calib, mask=None, **kw):
    """(sums [B,28], counts [B,3], smallest margin) at the public poses [B,12]."""
    out = [terms_ref(flow[b], *load_pose(pose[b]), calib, None if mask is None else mask[b], **kw) for b in range(flow.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), min(o[2] for o in out)


def solve_batch(flow, pose, calib, mask=None, iters=16, **kw):
    """(pose [B,12] float32, cost [B] float64, counts [B,4] int32, smallest margin)."""
    out = [solve_ref(flow[b], pose[b], calib, None if mask is None else mask[b], iters, **kw) for b in range(flow.shape[0])]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.float64), np.stack([o[2] for o in out]),
            min(o[3] for o in out))


def gradient_check(flow, pose12, calib, mask=None, h=1e-6, **kw):
    """(g [6] = terms 21..26, central differences of the summed cost over the step (dw, dth) at the pose) — both taken here."""
    r, t = load_pose(pose12)
    g = terms_ref(flow, r, t, calib, mask, **kw)[0][21:27]
    num = np.zeros(6)
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        cp = terms_ref(flow, *retract(r, t, d), calib, mask, **kw)[0][27]
        cm = terms_ref(flow, *retract(r, t, -d), calib, mask, **kw)[0][27]
        num[i] = (cp - cm) / (2.0 * h)
    return g, num


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def pose_errors_deg(pose, true):
    """(rotation error, error of the direction of t) in degrees of poses [B,12] against the generating poses [B,12]."""
    P, T = (np.asarray(a, dtype=np.float64).reshape(-1, 3, 4) for a in (pose, true))
    rot, dirn = [], []
    for p, q in zip(P, T):
        D = p[:, :3] @ q[:, :3].T
        v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
        rot.append(np.degrees(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0))))
        dirn.append(np.degrees(np.arctan2(np.linalg.norm(np.cross(p[:, 3], q[:, 3])), float(p[:, 3] @ q[:, 3]))))
    return np.array(rot), np.array(dirn)


def epipolar_scene(H, W, seed, B=1, noise_px=0.0, outliers=0.0):
    """A synthetic rigid scene of a camera that drives forward: f = 0.58 W, a smooth depth of 5 .. 35 |t|, a rotation of Euler
    angles uniform in +-0.02, t = (U(+-0.1), U(+-0.05), 1) scaled to |t| = U(0.6, 1.4). Returns (flow [B,2,H,W] float32, pose_true
    [B,12] float32, pose_start [B,12] float32, calib): the flow is that of the float32 true pose, rounded to float32, plus Gaussian
    noise of `noise_px` and, for a share `outliers` of the pixels, a uniform +-0.3 of the image's width and height instead; the
    start is the true pose turned by 1 degree with t turned by 8 degrees."""
    rs = np.random.RandomState(2000 + seed)
    fx = fy = 0.58 * W
    cx, cy = (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.zeros((B, 2, H, W), dtype=np.float32)
    true = np.zeros((B, 12), dtype=np.float32)
    start = np.zeros((B, 12), dtype=np.float32)
    for b in range(B):
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.05, 0.05), 1.0])
        t = t / np.linalg.norm(t) * rs.uniform(0.6, 1.4)
        R = euler_yxz(rs.uniform(-0.02, 0.02, 3))
        P = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
        R32, t32 = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
        Z = np.linalg.norm(t32) * (5.0 + 30.0 * (0.5 + 0.5 * np.cos(2 * np.pi * (xs / W * (1 + b) + 0.13 * seed))) *
                                   (0.5 + 0.5 * np.cos(np.pi * ys / H + 0.4 * b)))
        X1 = np.stack([Z * (xs - cx) / fx, Z * (ys - cy) / fy, Z])
        X2 = np.einsum("ji,jhw->ihw", R32, X1 - t32[:, None, None])
        u = fx * X2[0] / X2[2] + cx - xs
        v = fy * X2[1] / X2[2] + cy - ys
        if noise_px > 0.0:
            u = u + noise_px * rs.standard_normal((H, W))
            v = v + noise_px * rs.standard_normal((H, W))
        if outliers > 0.0:
            out = rs.uniform(size=(H, W)) < outliers
            u = np.where(out, rs.uniform(-0.3 * W, 0.3 * W, (H, W)), u)
            v = np.where(out, rs.uniform(-0.3 * H, 0.3 * H, (H, W)), v)
        axis_r = np.array([0.6, -0.5, 0.62])
        axis_t = np.cross(t, [0.3, 1.0, 0.1])
        S = np.concatenate([rodrigues(axis_r, np.radians(1.0)) @ R, (rodrigues(axis_t, np.radians(8.0)) @ t)[:, None]], axis=1)
        flow[b, 0], flow[b, 1] = u.astype(np.float32), v.astype(np.float32)
        true[b], start[b] = P.reshape(12), S.astype(np.float32).reshape(12)
    return flow, true, start, (fx, fy, cx, cy)


# (name, H, W, B, seed): the noise-free cases shared by the host and the GPU tests. 47x154 has 8 chunks: the chunk order matters.
# The seeds are the first for which the helper alone keeps every margin of the tests' calls above the floor: near convergence the
# trial cost comes within rounding of the accepted one, and which side it falls on is then no property of a correct evaluation.
CASES = [("5x7", 5, 7, 1, 1), ("9x33_b3", 9, 33, 3, 9), ("8x16_b2", 8, 16, 2, 15), ("47x154_b2", 47, 154, 2, 18)]
NOISY_CASE = ("94x308", 94, 308, 1, 1)
FULL_CASE = ("376x1232_b2", 376, 1232, 2, 1)
_cache = {}


def check_case(H, W, B, seed, iters=16, noise_px=0.0, outliers=0.0):
    """The scene of a case with its references (computed once per process), after asserting on the helper alone that the case
    decides nothing by a tie: margin >= 1e-9 at every evaluated pose. Returns a dict: flow, true, start, calib, terms = (sums,
    counts) at the start pose, solve = (pose, cost, counts) after `iters` steps."""
    key = (H, W, B, seed, iters, noise_px, outliers)
    if key not in _cache:
        flow, true, start, calib = epipolar_scene(H, W, seed, B, noise_px, outliers)
        sums, counts, m0 = terms_batch(flow, start, calib)
        pose, cost, counts4, m1 = solve_batch(flow, start, calib, iters=iters)
        assert min(m0, m1) >= MIN_MARGIN, (H, W, B, seed, m0, m1)
        for a in (flow, true, start, sums, counts, pose, cost, counts4):
            a.setflags(write=False)
        _cache[key] = dict(flow=flow, true=true, start=start, calib=calib, terms=(sums, counts), solve=(pose, cost, counts4))
    return _cache[key]
