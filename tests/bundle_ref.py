"""NumPy float64 restatement of the windowed bundle adjustment (include/atdn_hip.h, atdn_bundle_adjust) and the cases of its
tests: helper of the bundle tests, not a test, and not a call into the library.

Every array operation is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the rule
states. The candidates of a chunk are an array axis; a sum over them is the last row of a cumulative sum along that axis behind a
row of +0.0, which NumPy forms one addition after the other in ascending order; the views and the chunks are Python loops, the
n x n factorisation is written in Python floats (IEEE float64 too). The rule has only + - * / and comparisons, all correctly
rounded, so every correct evaluation gives the same bits — unless a decision quantity that depends on the inputs alone sits on its
threshold. `margin` is the smallest relative distance of such a quantity from its threshold where the decision is taken: x2 from
0 and W-1, y2 from 0 and H-1 (observed), P_2 from min_z*rho (front), e2 from inlier_px^2 (inlier), the two largest |tc_j| of the
gauge view from each other. The accept comparison, the pivot signs, c > 0 and the sign of a trial rho compare bit-defined values
and need none."""
import numpy as np

from multiview_ref import scene, euler_yxz, same_bits, MIN_MARGIN, DBL_MAX, FLT_MAX, _rel   # noqa: F401

CHUNK = 512
DEFAULTS = dict(stride=2, iters=8, scale_px=4.0, inlier_px=2.0, min_z=0.1, min_views=2)


def n_sums(S):
    n = 6 * S
    return n * (n + 1) // 2 + n + 27 * S + 1


def internal_pose(row):
    M = np.asarray(row, dtype=np.float32).astype(np.float64).reshape(3, 4)
    r, t = M[:, :3], M[:, 3]
    tc = np.array([-((r[0, i] * t[0] + r[1, i] * t[1]) + r[2, i] * t[2]) for i in range(3)])
    return np.ascontiguousarray(r.T), tc


def public_pose(rc, tc):
    out = np.zeros((3, 4), dtype=np.float32)
    for i in range(3):
        for j in range(3):
            out[i, j] = np.float32(rc[j, i])
        out[i, 3] = np.float32(-((rc[0, i] * tc[0] + rc[1, i] * tc[1]) + rc[2, i] * tc[2]))
    return out.reshape(12)


def cayley(w):
    h = [0.5 * float(w[0]), 0.5 * float(w[1]), 0.5 * float(w[2])]
    n2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
    f = 2.0 / (1.0 + n2)
    K = [[0.0, -h[2], h[1]], [h[2], 0.0, -h[0]], [-h[1], h[0], 0.0]]
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            hh = h[i] * h[j]
            C[i, j] = 1.0 + f * (hh - n2) if i == j else f * (K[i][j] + hh)
    return C


def _fold(rows):
    """The sum of the rows [K, E] in ascending order from +0.0, one addition after the other."""
    z = np.zeros((1,) + rows.shape[1:])
    return np.cumsum(np.concatenate([z, rows], axis=0), axis=0)[-1]


class _Problem:
    def __init__(self, acc_bank, alive_bank, poses, slots, calib, depth_init, mask, stride, scale_px, inlier_px, min_z, min_views):
        N, _, H, W = acc_bank.shape
        self.H, self.W, self.S, self.stride = H, W, len(slots), int(stride)
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in calib)
        self.c2, self.thr, self.min_z = scale_px * scale_px, inlier_px * inlier_px, float(min_z)
        e = float(H + W)
        self.rho_behind = (0.5 * (e * e)) / (1.0 + (e * e) / self.c2)
        self.slot = [int(k) if 0 <= int(k) < N else -1 for k in slots]
        self.poses32 = poses
        self.pose0 = [internal_pose(poses[k]) if k >= 0 else None for k in self.slot]
        ys, xs = np.meshgrid(np.arange(0, H, stride, dtype=np.float64), np.arange(0, W, stride, dtype=np.float64), indexing="ij")
        self.Hs, self.Ws = ys.shape
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        yi, xi = ys.astype(np.int64), xs.astype(np.int64)
        self.pix = yi * W + xi
        self.margin = np.inf
        obs, x2s, y2s = [], [], []
        with np.errstate(all="ignore"):
            for k in self.slot:
                if k < 0:
                    obs.append(np.zeros(xs.shape, dtype=bool)), x2s.append(xs), y2s.append(ys)
                    continue
                u, v = acc_bank[k, 0][yi, xi].astype(np.float64), acc_bank[k, 1][yi, xi].astype(np.float64)
                x2, y2 = xs + u, ys + v
                live = alive_bank[k][yi, xi] != 0
                obs.append(live & (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1))
                kept = live & np.isfinite(x2) & np.isfinite(y2)
                self.margin = min(self.margin, _rel(x2 / max(W - 1, 1), 0.0, kept), _rel(x2 / max(W - 1, 1), 1.0 if W > 1 else 0.0, kept),
                                  _rel(y2 / max(H - 1, 1), 0.0, kept), _rel(y2 / max(H - 1, 1), 1.0 if H > 1 else 0.0, kept))
                x2s.append(x2), y2s.append(y2)
        z0 = np.asarray(depth_init, dtype=np.float32).reshape(H, W)[yi, xi].astype(np.float64)
        allowed = np.ones(xs.shape, dtype=bool) if mask is None else np.asarray(mask).reshape(H, W)[yi, xi] != 0
        n_obs = np.sum(np.stack(obs), axis=0)
        self.cand = allowed & (z0 > 0) & (z0 <= FLT_MAX) & (n_obs >= min_views)
        self.q = np.nonzero(self.cand)[0]                       # the candidates' positions, ascending
        sel = self.q
        self.obs = [o[sel] for o in obs]
        self.x2, self.y2 = [a[sel] for a in x2s], [a[sel] for a in y2s]
        self.a0, self.a1 = (xs[sel] - self.cx) / self.fx, (ys[sel] - self.cy) / self.fy
        with np.errstate(all="ignore"):
            self.rho0 = 1.0 / z0[sel]
        self.npos = xs.shape[0]
        # the gauge
        self.held = -1
        g = max([s for s, k in enumerate(self.slot) if k >= 0], default=-1)
        if g >= 0:
            a = np.abs(self.pose0[g][1])
            j = int(np.argmax(a))                               # the first of equal maxima
            if a[j] > 0:
                self.held = 6 * g + 3 + j
                others = np.delete(a, j)
                self.margin = min(self.margin, float(np.min(np.abs(a[j] - others) / a[j])))
        self.behind_seen = False

    def view(self, s, pose, rho):
        """The terms of view s over all candidates: t [K,27], E [K,6], cs, bs, cost [K], front, inlier [K] bool."""
        rc, tc = pose
        K = rho.shape[0]
        obs = self.obs[s]
        with np.errstate(all="ignore"):
            m = [(rc[i, 0] * self.a0 + rc[i, 1] * self.a1) + rc[i, 2] for i in range(3)]
            P = [m[i] + rho * tc[i] for i in range(3)]
            zlim = self.min_z * rho
            front = P[2] >= zlim
            self.margin = min(self.margin, _rel(P[2], zlim, obs))
            iz = 1.0 / P[2]
            px, py = (self.fx * P[0]) * iz, (self.fy * P[1]) * iz
            rx, ry = (px + self.cx) - self.x2[s], (py + self.cy) - self.y2[s]
            e2 = rx * rx + ry * ry
            sc = 1.0 + e2 / self.c2
            w = 1.0 / (sc * sc)
            cost = (0.5 * e2) / sc
            ax, ay = self.fx * iz, self.fy * iz
            bx, by = -(px * iz), -(py * iz)
            zero = np.zeros(K)
            Jx = [bx * m[1], ax * m[2] - bx * m[0], -(ax * m[1]), rho * ax, zero, rho * bx]
            Jy = [by * m[1] - ay * m[2], -(by * m[0]), ay * m[0], zero, rho * ay, rho * by]
            jrx, jry = ax * tc[0] + bx * tc[2], ay * tc[1] + by * tc[2]
            t = np.zeros((K, 27))
            E = np.zeros((K, 6))
            n = 0
            for i in range(6):
                wx, wy = w * Jx[i], w * Jy[i]
                for j in range(i, 6):
                    t[:, n] = wx * Jx[j] + wy * Jy[j]
                    n += 1
                t[:, 21 + i] = wx * rx + wy * ry
                E[:, i] = wx * jrx + wy * jry
            cs = (w * jrx) * jrx + (w * jry) * jry
            bs = (w * jrx) * rx + (w * jry) * ry
        use = obs & front
        self.margin = min(self.margin, _rel(e2, self.thr, use))
        self.behind_seen = self.behind_seen or bool((obs & ~front).any())
        t = np.where(use[:, None], t, 0.0)
        E = np.where(use[:, None], E, 0.0)
        cs, bs = np.where(use, cs, 0.0), np.where(use, bs, 0.0)
        cost = np.where(use, cost, np.where(obs, self.rho_behind, 0.0))
        return t, E, cs, bs, cost, use, use & (e2 <= self.thr)

    def depth_step(self, poses, rho, dxi, lam):
        """rho' of every candidate from the accepted state; also how many trials were refused."""
        K = rho.shape[0]
        c, b, e = np.zeros(K), np.zeros(K), np.zeros(K)
        for s in range(self.S):
            if self.slot[s] < 0:
                continue
            _, E, cs, bs, _, _, _ = self.view(s, poses[s], rho)
            d = dxi[6 * s:6 * s + 6]
            ev = E[:, 0] * d[0]
            for i in range(1, 6):
                ev = ev + E[:, i] * d[i]
            o = self.obs[s]
            c, b, e = np.where(o, c + cs, c), np.where(o, b + bs, b), np.where(o, e + ev, e)
        with np.errstate(all="ignore"):
            rt = rho - (b + e) / (c * (1.0 + lam))
        ok = (c > 0) & (rt > 0) & (rt <= DBL_MAX)
        return np.where(ok, rt, rho), int(((c > 0) & ~ok).sum())

    def evaluate(self, poses, rho):
        """All sums [n_sums] and counts (candidates, front, inliers) at (poses, rho)."""
        S, n = self.S, 6 * self.S
        K = rho.shape[0]
        T = [np.zeros((K, 27)) for _ in range(S)]
        E = np.zeros((K, n))
        c, b, cost = np.zeros(K), np.zeros(K), np.zeros(K)
        n_front = n_in = 0
        for s in range(S):
            if self.slot[s] < 0:
                continue
            t, Es, cs, bs, co, front, inl = self.view(s, poses[s], rho)
            o = self.obs[s]
            T[s], E[:, 6 * s:6 * s + 6] = t, Es
            c, b, cost = np.where(o, c + cs, c), np.where(o, b + bs, b), np.where(o, cost + co, cost)
            n_front += int(front.sum())
            n_in += int(inl.sum())
        valid = c > 0
        with np.errstate(all="ignore"):
            ic = np.where(valid, 1.0 / c, 0.0)
        bc = np.where(valid, b * ic, 0.0)
        E = np.where(valid[:, None], E, 0.0)
        T = [np.where(valid[:, None], t, 0.0) for t in T]
        iu, ju = np.triu_indices(n)
        sums = np.zeros(n_sums(S))
        chunk_of = self.q // CHUNK
        for ch in range((self.npos + CHUNK - 1) // CHUNK):
            r = np.nonzero(chunk_of == ch)[0]
            if r.size == 0:
                continue
            Ec = E[r]
            F = Ec * ic[r, None]
            rows = np.concatenate([F[:, iu] * Ec[:, ju], Ec * bc[r, None]] + [t[r] for t in T] + [cost[r, None]], axis=1)
            sums = sums + _fold(rows)
        return sums, np.array([K, n_front, n_in], dtype=np.int32)

    def is_held(self, i):
        return self.slot[i // 6] < 0 or i == self.held

    def step(self, sums, lam):
        """dxi [n] or None (no step) from the accepted sums."""
        S, n = self.S, 6 * self.S
        if self.held < 0:
            return None
        tri = n * (n + 1) // 2
        ut = lambda i, j: i * n - i * (i - 1) // 2 + (j - i)
        ut6 = lambda i, j: i * 6 - i * (i - 1) // 2 + (j - i)
        opl = 1.0 + lam
        sm = [float(v) for v in sums]
        A = [[0.0] * n for _ in range(n)]                       # A[i][j], j <= i: the lower triangle
        x = [0.0] * n
        for i in range(n):
            hi = self.is_held(i)
            vi = i // 6
            x[i] = 0.0 if hi else -(sm[tri + n + 27 * vi + 21 + (i - 6 * vi)] - sm[tri + i] / opl)
            for j in range(i, n):
                if hi or self.is_held(j):
                    a = 1.0 if i == j else 0.0
                else:
                    h = sm[tri + n + 27 * vi + ut6(i - 6 * vi, j - 6 * vi)] if j // 6 == vi else 0.0
                    d = sm[ut(i, j)] / opl
                    a = (h + lam * h) - d if i == j else h - d
                A[j][i] = a
        L = [[0.0] * n for _ in range(n)]
        D = [0.0] * n
        ok = True
        with np.errstate(all="ignore"):
            for j in range(n):
                Lj = L[j]
                ld = [Lj[k] * D[k] for k in range(j)]
                dj = A[j][j]
                for k in range(j):
                    dj = dj - Lj[k] * ld[k]
                D[j] = dj
                ok = ok and dj > 0.0
                for i in range(j + 1, n):
                    Li = L[i]
                    a = A[i][j]
                    for k in range(j):
                        a = a - Li[k] * ld[k]
                    Li[j] = _div(a, dj)
            for i in range(n):
                v = x[i]
                for k in range(i):
                    v = v - L[i][k] * x[k]
                x[i] = v
            for i in range(n):
                x[i] = _div(x[i], D[i])
            for i in range(n - 1, -1, -1):
                v = x[i]
                for k in range(i + 1, n):
                    v = v - L[k][i] * x[k]
                x[i] = v
        x = np.array(x)
        if not (ok and np.all(np.isfinite(x))):
            return None
        return x


def _div(a, b):
    return float(np.float64(a) / np.float64(b))                 # IEEE: a zero divisor gives an infinity or a NaN, no exception


def bundle_ref(acc_bank, alive_bank, poses, slots, calib, depth_init, mask=None, stride=2, iters=8, scale_px=4.0, inlier_px=2.0,
               min_z=0.1, min_views=2):
    """One problem. acc_bank [N,2,H,W] float32, alive_bank [N,H,W] uint8, poses [N,12] float32, slots [S], depth_init [H,W]
    float32, mask [H,W] or None -> dict: poses [S,12] float32, depth [H,W] float32, cost [2] float64, counts [4] int32, sums0 (the
    sums of evaluation 0: what atdn_bundle_terms returns) and counts0 [3], margin, costs (the accepted cost after every
    evaluation), accepted / rejected (steps), refused (trial depths kept back), behind (a view was behind at some evaluation),
    held, empty (an empty slot)."""
    acc_bank, alive_bank, poses = np.asarray(acc_bank), np.asarray(alive_bank), np.asarray(poses)
    assert acc_bank.dtype == np.float32 and poses.dtype == np.float32 and alive_bank.dtype == np.uint8
    pr = _Problem(acc_bank, alive_bank, poses, slots, calib, depth_init, mask, stride, scale_px, inlier_px, min_z, min_views)
    S, H, W = pr.S, pr.H, pr.W
    zero_pose = (np.zeros((3, 3)), np.zeros(3))
    acc_p = [p if p is not None else zero_pose for p in pr.pose0]
    trial_p, rho_a, rho_t = list(acc_p), pr.rho0, pr.rho0
    lam, cost_a, sums_a, counts_a = 1e-3, None, None, None
    accepted = rejected = refused = 0
    costs = []
    sums0 = counts0 = None
    for k in range(int(iters) + 1):
        sums, cnt = pr.evaluate(trial_p, rho_t)
        if k == 0:
            sums0, counts0, cost0 = sums, cnt, sums[-1]
        accept = k == 0 or bool(sums[-1] < cost_a)
        if accept:
            acc_p, rho_a, cost_a, sums_a, counts_a = list(trial_p), rho_t, sums[-1], sums, cnt
        if k > 0:
            lam = max(lam / 3.0, 1e-9) if accept else min(4.0 * lam, 1e6)
            accepted += accept
            rejected += not accept
        costs.append(float(cost_a))
        if k < iters:
            dxi = pr.step(sums_a, lam)
            if dxi is None:
                trial_p, rho_t = list(acc_p), rho_a
            else:
                trial_p = []
                for s in range(S):
                    rc, tc = acc_p[s]
                    if pr.slot[s] < 0:
                        trial_p.append((rc, tc))
                        continue
                    C = cayley(dxi[6 * s:6 * s + 3])
                    rn = np.array([[(C[i, 0] * rc[0, j] + C[i, 1] * rc[1, j]) + C[i, 2] * rc[2, j] for j in range(3)] for i in range(3)])
                    trial_p.append((rn, tc + dxi[6 * s + 3:6 * s + 6]))
                rho_t, nref = pr.depth_step(acc_p, rho_a, dxi, lam)
                refused += nref
    out_poses = np.zeros((S, 12), dtype=np.float32)
    for s in range(S):
        if pr.slot[s] >= 0:
            out_poses[s] = poses[pr.slot[s]] if accepted == 0 else public_pose(*acc_p[s])
    depth = np.zeros(H * W, dtype=np.float32)
    with np.errstate(all="ignore"):
        depth[pr.pix[pr.q]] = (1.0 / rho_a).astype(np.float32)
    return dict(poses=out_poses, depth=depth.reshape(H, W), cost=np.array([cost0, cost_a]),
                counts=np.array(list(counts_a[:3]) + [accepted], dtype=np.int32), sums0=sums0, counts0=counts0, margin=pr.margin,
                costs=costs, accepted=int(accepted), rejected=int(rejected), refused=refused, behind=pr.behind_seen, held=pr.held,
                empty=any(k < 0 for k in pr.slot))


def reference_batch(acc_bank, alive_bank, poses, slots, calib, depth_init, mask=None, **kw):
    """(poses [B,S,12], depth [B,1,H,W], cost [B,2], counts [B,4], per-problem dicts)"""
    slots = np.asarray(slots)
    out = [bundle_ref(acc_bank, alive_bank, poses, slots[b], calib, depth_init[b, 0], None if mask is None else mask[b], **kw)
           for b in range(slots.shape[0])]
    return (np.stack([o["poses"] for o in out]), np.stack([o["depth"] for o in out])[:, None], np.stack([o["cost"] for o in out]),
            np.stack([o["counts"] for o in out]), out)


# ------------------------------------------------------------------ cases
def perturb(poses, seed, rot=0.004, scale=0.03, shift=0.03, offset=(0.0, 0.0, 0.0)):
    """Deterministic pose errors: a rotation of up to `rot` rad per axis, a scale error of up to `scale` and a shift of up to
    `shift` metres per axis on every row of poses [N,12] float32, plus the fixed `offset` (which makes another coordinate of the
    translation the largest: another gauge coordinate); rounded to float32."""
    rs = np.random.RandomState(1000 + seed)
    out = np.zeros_like(poses)
    for k in range(poses.shape[0]):
        M = poses[k].astype(np.float64).reshape(3, 4)
        R = euler_yxz(rs.uniform(-rot, rot, 3)) @ M[:, :3]
        t = M[:, 3] * (1.0 + rs.uniform(-scale, scale)) + rs.uniform(-shift, shift, 3) + np.asarray(offset, dtype=np.float64)
        out[k] = np.concatenate([R, t[:, None]], axis=1).astype(np.float32).reshape(12)
    return out


def pose_errors(got, true, held_view, held_axis):
    """Per listed view the rotation error (rad) and the translation error (m) of poses `got` [S,12] against `true` [S,12], after
    scaling `got` so that the held coordinate of the held view's internal translation agrees (the held gauge)."""
    gi = [internal_pose(p) for p in got]
    ti = [internal_pose(p) for p in true]
    k = ti[held_view][1][held_axis] / gi[held_view][1][held_axis]
    rot, tr = [], []
    for (rg, tg), (rt, tt) in zip(gi, ti):
        c = (np.trace(rg.T @ rt) - 1.0) / 2.0
        rot.append(float(np.arccos(np.clip(c, -1.0, 1.0))) if c < 1.0 - 1e-12 else float(np.linalg.norm(rg.T @ rt - np.eye(3)) / np.sqrt(2.0)))
        tr.append(float(np.linalg.norm(tg * k - tt)))
    return np.array(rot), np.array(tr)


def _views(N, S, b):
    return [(b + s * (1 + b % 2)) % N for s in range(S)]


NOISY = dict(noise=0.3, outliers=0.1, dead=0.15, wrong=0.1, reversed_patch=True)
# (name, H, W, B, S, N, seed, scene options, solver options, skipped slots, pose perturbation options)
CASES = [("5x7_s2", 5, 7, 1, 2, 2, 39, dict(NOISY, noise=0.1, wrong=0.3, far=12.0, calib=(6.0, 6.0, 3.3, 1.8)), dict(stride=1), False,
          dict(offset=(0.0, 2.5, 0.0))),
         ("9x33_b3_s5_st1", 9, 33, 3, 5, 6, 3, NOISY, dict(stride=1), True, {}),
         ("9x33_b3_s5_st3", 9, 33, 3, 5, 6, 3, NOISY, dict(stride=3), True, dict(offset=(8.0, 0.0, 0.0))),
         ("47x154_s8", 47, 154, 1, 8, 8, 5, NOISY, dict(stride=1), False, {}),
         ("33x65_s16", 33, 65, 1, 16, 16, 7, dict(NOISY, step=0.5), dict(stride=2), False, {})]
FULL_CASE = ("376x1232_b2_s16", 376, 1232, 2, 16, 16, 6, dict(NOISY, step=0.5), dict(stride=4), False, {})


def case_inputs(H, W, B, S, N, seed, opts, skipped=False, pert=None):
    """(scene dict with the perturbed poses under "poses" and the true ones under "true_poses", slots [B,S] int32, depth_init
    [B,1,H,W] float32 without holes: where the scene has none — its reversed patch among them — the true depth stands, mask
    [B,H,W] uint8 that forbids a band of rows in every second problem)."""
    sc = scene(H, W, N, seed, **opts)
    sc["true_poses"] = sc["poses"]
    sc["poses"] = perturb(sc["poses"], seed, **(pert or {}))
    slots = np.array([_views(N, S, b) for b in range(B)], dtype=np.int32)
    if skipped:
        slots[0, 1], slots[B - 1, S - 1] = -1, N
    base = np.where(sc["depth_init"] > 0, sc["depth_init"], sc["Z"].astype(np.float32)[None, None])
    init = np.concatenate([np.roll(base, b, axis=3) for b in range(B)], axis=0)
    mask = np.ones((B, H, W), dtype=np.uint8)
    mask[1::2, : max(H // 8, 1)] = 0
    return sc, slots, np.ascontiguousarray(init), mask


_REFERENCES = {}


def reference(case, iters=4):
    """The inputs of a case and its reference with `iters` steps, computed once per process and shared; nobody writes into it.
    Asserts on the helper alone that the case decides nothing by a tie."""
    name, H, W, B, S, N, seed, opts, kw, skipped, pert = case
    if (name, iters) not in _REFERENCES:
        sc, slots, init, mask = case_inputs(H, W, B, S, N, seed, opts, skipped, pert)
        ref = reference_batch(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], init, mask, iters=iters, **kw)
        for o in ref[4]:
            assert o["margin"] >= MIN_MARGIN, (name, o["margin"])
        _REFERENCES[name, iters] = (sc, slots, init, mask, ref)
    return _REFERENCES[name, iters]


def check_branches(iters=4):
    """Asserts on the helper alone that the cases take every branch of the rule. In every problem of every case: an accepted
    step, a view behind its camera and a candidate whose trial depth is refused. Across the cases (the well-conditioned ones
    accept every step, and only the case the issue gives empty slots has some): a rejected step, an empty slot, and a held gauge
    coordinate of each index j = 0, 1, 2."""
    rejected = empty = False
    held = set()
    for case in CASES:
        for o in reference(case, iters)[4][4]:
            assert o["accepted"] >= 1 and o["behind"] and o["refused"] >= 1, (case[0], o["accepted"], o["behind"], o["refused"])
            assert o["counts"][0] >= 1 and o["held"] >= 0, case[0]
            rejected, empty = rejected or o["rejected"] >= 1, empty or o["empty"]
            held.add(o["held"] % 6 - 3)
    assert rejected and empty and held == {0, 1, 2}, (rejected, empty, held)


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = {8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(v), b.view(v)))
