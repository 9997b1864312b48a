"""NumPy float64 restatement of the multi-view depth rule (include/atdn_hip.h, atdn_multiview_depth) and the scene generator of
its tests: helper of the multi-view tests, not a test, and not a call into the library.

Every array operation of `multiview_ref` is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in
the order the rule states; the pixels are the array axes, the views a Python loop. The rule has only + - * / and comparisons, all
correctly rounded, so every correct evaluation gives the same bits — unless a decision quantity sits on its threshold. `margin` is
the smallest relative distance of any decision quantity from its threshold over the pixels and evaluations where that decision is
taken: x2 from 0 and W-1, y2 from 0 and H-1 (inside), P_2 from min_z*rho (front), e2 from inlier_px^2 (inlier), ri from
min_rel_info, z from FLT_MIN and from max_depth (validity), and the two costs of the choice between the two starts from each
other. The accept comparison of a step needs none: both of its sides are bit-defined. The tests assert margin >= 1e-9 on the
helper alone before anything is compared."""
import numpy as np

MIN_MARGIN = 1e-9
DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
DEFAULTS = dict(iters=4, scale_px=4.0, inlier_px=2.0, min_z=0.1, min_views=2, max_rel_sigma=0.25, max_depth=80.0)


def _rel(q, thr, where):
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), q.shape)
    d = np.abs(q - thr) / np.where(thr != 0, np.abs(thr), 1.0)
    d = np.where(where & np.isfinite(d), d, np.inf)
    return float(d.min()) if d.size else np.inf


class _Problem:
    """One problem (one anchor image and its listed views): the per-view terms that do not depend on rho, and E(rho)."""

    def __init__(self, acc_bank, alive_bank, poses, slots, calib, scale_px, inlier_px, min_z):
        N, _, H, W = acc_bank.shape
        self.H, self.W = H, W
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in calib)
        self.c2 = scale_px * scale_px
        self.thr = inlier_px * inlier_px
        self.min_z = float(min_z)
        e = float(H + W)
        self.rho_behind = (0.5 * (e * e)) / (1.0 + (e * e) / self.c2)
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        self.a0, self.a1 = (xs - self.cx) / self.fx, (ys - self.cy) / self.fy
        self.views = []
        self.margin = np.inf
        with np.errstate(all="ignore"):
            for k in (int(k) for k in slots):
                if k < 0 or k >= N:
                    continue
                M = poses[k].astype(np.float64).reshape(3, 4)
                r, t = M[:, :3], M[:, 3]
                rc = r.T
                tc = [-((r[0, i] * t[0] + r[1, i] * t[1]) + r[2, i] * t[2]) for i in range(3)]
                u, v = acc_bank[k, 0].astype(np.float64), acc_bank[k, 1].astype(np.float64)
                x2, y2 = xs + u, ys + v
                live = alive_bank[k] != 0
                obs = live & (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1)
                kept = live & np.isfinite(x2) & np.isfinite(y2)
                self.margin = min(self.margin, _rel(x2 / max(W - 1, 1), 0.0, kept), _rel(x2 / max(W - 1, 1), 1.0 if W > 1 else 0.0, kept),
                                  _rel(y2 / max(H - 1, 1), 0.0, kept), _rel(y2 / max(H - 1, 1), 1.0 if H > 1 else 0.0, kept))
                m = [(rc[i, 0] * self.a0 + rc[i, 1] * self.a1) + rc[i, 2] for i in range(3)]
                kx = self.fx * (tc[0] * m[2] - m[0] * tc[2])
                ky = self.fy * (tc[1] * m[2] - m[1] * tc[2])
                self.views.append(dict(obs=obs, m=m, tc=tc, kx=kx, ky=ky, x2=x2, y2=y2, xt=x2 - self.cx, yt=y2 - self.cy))

    def linear(self):
        """(num, den, n_obs)"""
        shape = (self.H, self.W)
        num, den, n_obs = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
        with np.errstate(all="ignore"):
            for w in self.views:
                m, tc = w["m"], w["tc"]
                Ax = self.fx * tc[0] - w["xt"] * tc[2]
                Bx = w["xt"] * m[2] - self.fx * m[0]
                Ay = self.fy * tc[1] - w["yt"] * tc[2]
                By = w["yt"] * m[2] - self.fy * m[1]
                num = np.where(w["obs"], num + (Ax * Bx + Ay * By), num)
                den = np.where(w["obs"], den + (Ax * Ax + Ay * Ay), den)
                n_obs = n_obs + w["obs"]
        return num, den, n_obs

    def evaluate(self, rho, active=None):
        """E(rho) -> (g, h, cost, n_in). `active`: where the rule takes this evaluation (for the margins only)."""
        shape = (self.H, self.W)
        g, h, cost, n_in = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
        act = np.ones(shape, dtype=bool) if active is None else active
        with np.errstate(all="ignore"):
            zlim = self.min_z * rho
            for w in self.views:
                m, tc, obs = w["m"], w["tc"], w["obs"]
                P = [m[i] + rho * tc[i] for i in range(3)]
                front = P[2] >= zlim
                self.margin = min(self.margin, _rel(P[2], zlim, obs & act))
                iz = 1.0 / P[2]
                px, py = (self.fx * P[0]) * iz, (self.fy * P[1]) * iz
                rx, ry = (px + self.cx) - w["x2"], (py + self.cy) - w["y2"]
                e2 = rx * rx + ry * ry
                s = 1.0 + e2 / self.c2
                wt = 1.0 / (s * s)
                r = (0.5 * e2) / s
                Jx, Jy = (w["kx"] * iz) * iz, (w["ky"] * iz) * iz
                use = obs & front
                self.margin = min(self.margin, _rel(e2, self.thr, use & act))
                g = np.where(use, g + ((wt * Jx) * rx + (wt * Jy) * ry), g)
                h = np.where(use, h + ((wt * Jx) * Jx + (wt * Jy) * Jy), h)
                cost = np.where(use, cost + r, np.where(obs, cost + self.rho_behind, cost))
                n_in = n_in + (use & (e2 <= self.thr))
        return g, h, cost, n_in


def multiview_ref(acc_bank, alive_bank, poses, slots, calib, depth_init=None, iters=4, scale_px=4.0, inlier_px=2.0, min_z=0.1,
                  min_views=2, max_rel_sigma=0.25, max_depth=80.0):
    """One problem. acc_bank [N,2,H,W] float32, alive_bank [N,H,W] uint8, poses [N,12] float32, slots [S] integers, depth_init
    [H,W] float32 or None -> dict: depth, info [H,W] float32, views [H,W] uint8, counts [3] int32, margin, and for the tests'
    branch assertions rho [H,W] float64 (NaN where not solved), cand, solved, valid, from_init, from_linear [H,W] bool,
    has_lin, has_init [H,W] bool (which starts existed), rejected (the number of rejected steps over all pixels), problem (the
    _Problem, whose evaluate(rho)[2] is the cost function)."""
    acc_bank, alive_bank, poses = np.asarray(acc_bank), np.asarray(alive_bank), np.asarray(poses)
    assert acc_bank.dtype == np.float32 and poses.dtype == np.float32 and alive_bank.dtype == np.uint8
    pr = _Problem(acc_bank, alive_bank, poses, slots, calib, scale_px, inlier_px, min_z)
    H, W = pr.H, pr.W
    min_rel_info = 1.0 / (max_rel_sigma * max_rel_sigma)
    with np.errstate(all="ignore"):
        num, den, n_obs = pr.linear()
        cand = n_obs >= min_views
        rho_lin = num / den
        lin_ok = cand & (rho_lin > 0) & (rho_lin <= DBL_MAX)
        z0 = np.zeros((H, W)) if depth_init is None else np.asarray(depth_init, dtype=np.float32).reshape(H, W).astype(np.float64)
        init_ok = cand & (z0 > 0) & (z0 <= FLT_MAX)
        rho_0 = 1.0 / z0
        gl, hl, cl, nl = pr.evaluate(np.where(lin_ok, rho_lin, 1.0), lin_ok)
        gi, hi, ci, ni = pr.evaluate(np.where(init_ok, rho_0, 1.0), init_ok)
        both = lin_ok & init_ok
        from_init = init_ok & (~lin_ok | (ci < cl))
        from_linear = lin_ok & ~from_init
        margin_start = _rel(ci, cl, both)
        solved = lin_ok | init_ok
        rho = np.where(from_init, rho_0, np.where(from_linear, rho_lin, np.nan))
        g, h = np.where(from_init, gi, gl), np.where(from_init, hi, hl)
        cost, n_in = np.where(from_init, ci, cl), np.where(from_init, ni, nl)
        lam = np.full((H, W), 1e-3)
        rejected = 0
        for _ in range(int(iters)):
            r_t = rho - g / (h + lam * h)
            ok = solved & (r_t > 0) & (r_t <= DBL_MAX)
            gt, ht, ct, nt = pr.evaluate(np.where(ok, r_t, 1.0), ok)
            accept = ok & (ct < cost)
            rejected += int((solved & ~accept).sum())
            rho, g, h = np.where(accept, r_t, rho), np.where(accept, gt, g), np.where(accept, ht, h)
            cost, n_in = np.where(accept, ct, cost), np.where(accept, nt, n_in)
            lam = np.where(accept, np.maximum(lam / 3.0, 1e-9), np.minimum(4.0 * lam, 1e6))
        z = 1.0 / rho
        ri = (h * rho) * rho
        enough = solved & (n_in >= min_views)
        valid = enough & (ri >= min_rel_info) & (z >= FLT_MIN) & (z <= max_depth)
        margin = min(pr.margin, margin_start, _rel(ri, min_rel_info, enough), _rel(z, FLT_MIN, enough), _rel(z, max_depth, enough))
        depth = np.where(valid, z, 0.0).astype(np.float32)
        info = np.where(valid, np.minimum(ri, FLT_MAX), 0.0).astype(np.float32)
        views = np.where(solved, n_in, 0).astype(np.uint8)
    counts = np.array([cand.sum(), solved.sum(), valid.sum()], dtype=np.int32)
    return dict(depth=depth, info=info, views=views, counts=counts, margin=margin, rho=rho, cand=cand, solved=solved, valid=valid,
                from_init=from_init, from_linear=from_linear, has_lin=lin_ok, has_init=init_ok, rejected=rejected, problem=pr)


def reference_batch(acc_bank, alive_bank, poses, slots, calib, depth_init=None, **kw):
    """The helper over the problems of slots [B,S]: (depth, info [B,1,H,W], views [B,H,W], counts [B,3], smallest margin, the
    list of the per-problem dicts)."""
    slots = np.asarray(slots)
    out = [multiview_ref(acc_bank, alive_bank, poses, slots[b], calib, None if depth_init is None else depth_init[b, 0], **kw)
           for b in range(slots.shape[0])]
    return (np.stack([o["depth"] for o in out])[:, None], np.stack([o["info"] for o in out])[:, None],
            np.stack([o["views"] for o in out]), np.stack([o["counts"] for o in out]), min(o["margin"] for o in out), out)


# ------------------------------------------------------------------ scenes
def euler_yxz(angles):
    a, b, c = (float(v) for v in angles)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return ry @ rx @ rz


def scene_calib(H, W):
    return 718.856 * W / 1241.0, 718.856 * W / 1241.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2


def scene(H, W, N, seed, noise=0.0, outliers=0.0, dead=0.0, holes=0.0, wrong=0.0, reversed_patch=False, step=1.0, far=120.0,
          calib=None):
    """A street-like scene seen from an anchor camera and N later frames `step` metres apart. The anchor's depth is the nearer of a
    ground plane 1.65 m below the camera and a smooth wall between 6 m and `far`, rounded to float32; frame k stands (k + 1) steps
    ahead with small side steps and rotations (Euler angles within +-0.01), its pose anchor <- frame k rounded to float32; the
    flow of slot k is the exact projection of the float32 depth under the float32 pose minus the pixel, plus Gaussian noise of
    `noise` pixels, rounded to float32. A point that comes closer than 0.5 m to a frame is dead there (a real track has died
    before); a point that leaves the image stays alive (the rule's own `inside` test meets it).
    `outliers`: that share of the pixels of every second view is moved by 3 .. 12 pixels. `dead`: that share of the pixels is dead
    in a random set of views, in a left band of the image in ALL views. `reversed_patch`: in a patch of the image every view's flow
    is negated (an object moving against the scene: the linear solution is negative). depth_init is the true depth times
    (1 + 2 % Gaussian), 0 in `holes` of the pixels and in the reversed patch, and far too near (x 0.15) in `wrong` of them.
    Returns dict(acc [N,2,H,W] float32, alive [N,H,W] uint8, poses [N,12] float32, calib, Z [H,W] float64 (of the float32 depth),
    depth_init [1,1,H,W] float32)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = calib = scene_calib(H, W) if calib is None else calib
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    wall = 6.0 + (far - 6.0) * (0.5 + 0.5 * np.cos(2 * np.pi * (xs / W + 0.13 * seed))) * (0.35 + 0.65 * (0.5 + 0.5 * np.cos(np.pi * ys / H)))
    with np.errstate(all="ignore"):
        ground = np.where(ys - cy > 0, 1.65 * fy / (ys - cy), np.inf)
    Z = np.minimum(wall, ground).astype(np.float32).astype(np.float64)
    X1 = np.stack([Z * (xs - cx) / fx, Z * (ys - cy) / fy, Z])
    acc = np.zeros((N, 2, H, W), dtype=np.float32)
    alive = np.ones((N, H, W), dtype=np.uint8)
    poses = np.zeros((N, 12), dtype=np.float32)
    patch = np.zeros((H, W), dtype=bool)
    if reversed_patch:
        patch[H // 5:H // 5 + max(H // 6, 1), (3 * W) // 5:(3 * W) // 5 + max(W // 8, 2)] = True
    band = xs < max(1, int(round(0.06 * W))) if dead > 0 else np.zeros((H, W), dtype=bool)
    for k in range(N):
        R = euler_yxz(rs.uniform(-0.01, 0.01, 3))
        t = np.array([rs.uniform(-0.05, 0.05), rs.uniform(-0.02, 0.02), step * (k + 1) + rs.uniform(-0.1, 0.1)])
        P = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
        R32, t32 = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
        X2 = np.einsum("ji,jhw->ihw", R32, X1 - t32[:, None, None])          # R^T (X1 - t)
        near = X2[2] < 0.5
        zz = np.where(near, 1.0, X2[2])
        u, v = fx * X2[0] / zz + cx - xs, fy * X2[1] / zz + cy - ys
        u, v = u + noise * rs.standard_normal((H, W)), v + noise * rs.standard_normal((H, W))
        if outliers > 0 and k % 2 == 1:
            out = rs.uniform(size=(H, W)) < outliers
            ang, mag = rs.uniform(0, 2 * np.pi, (H, W)), rs.uniform(3.0, 12.0, (H, W))
            u, v = np.where(out, u + mag * np.cos(ang), u), np.where(out, v + mag * np.sin(ang), v)
        u, v = np.where(patch, -u, u), np.where(patch, -v, v)
        acc[k, 0], acc[k, 1] = u, v
        gone = near | band | (rs.uniform(size=(H, W)) < dead)
        alive[k][gone] = 0
        poses[k] = P.reshape(12)
    init = Z * (1.0 + 0.02 * rs.standard_normal((H, W)))
    pick = rs.uniform(size=(H, W))
    init = np.where(pick < wrong, 0.15 * Z, init)
    init = np.where((pick > 1.0 - holes) | patch, 0.0, init)
    return dict(acc=acc, alive=alive, poses=poses, calib=calib, Z=Z, depth_init=init.astype(np.float32)[None, None])


def _views(N, S, b, B):
    """The view list of problem b: S slots out of N, a different set and order per problem."""
    return [(b + s * (1 + b % 2)) % N for s in range(S)]


# (name, H, W, B, S, N, seed, scene options, solver options, skipped slots): the cases shared by the host and the GPU tests. B
# problems share one bank of N views; problem b has its own depth_init (the scene's, shifted by b columns: other holes, other
# wrong starts). 5 x 7: a camera of 6 pixels focal length sees disparities of a pixel, so the case asks for sigma_z / z <= 2
# only — with the default 0.25 none of its 35 pixels is valid and the `valid` branch would not be taken.
NOISY = dict(noise=0.3, outliers=0.1, dead=0.15, holes=0.3, wrong=0.1, reversed_patch=True)
CASES = [("5x7_s2", 5, 7, 1, 2, 2, 39, dict(NOISY, noise=0.1, outliers=0.15, dead=0.2, wrong=0.15, far=12.0, calib=(6.0, 6.0, 3.3, 1.8)),
          dict(max_rel_sigma=2.0), False),
         ("9x33_b3_s5", 9, 33, 3, 5, 6, 3, NOISY, {}, True),
         ("47x154_s8", 47, 154, 1, 8, 8, 5, NOISY, {}, False)]
FULL_CASE = ("376x1232_b2_s16", 376, 1232, 2, 16, 16, 6, dict(NOISY, step=0.5), {}, False)
STAT_CASE = dict(H=48, W=160, N=8, seed=11, noise=0.3, dead=0.05, holes=0.2)


def case_inputs(H, W, B, S, N, seed, opts, skipped=False):
    """(scene dict, slots [B,S] int32, depth_init [B,1,H,W] float32). `skipped`: slots -1 and N among the lists."""
    sc = scene(H, W, N, seed, **opts)
    slots = np.array([_views(N, S, b, B) for b in range(B)], dtype=np.int32)
    if skipped:
        slots[0, 1], slots[B - 1, S - 1] = -1, N
    init = np.concatenate([np.roll(sc["depth_init"], b, axis=3) for b in range(B)], axis=0)
    return sc, slots, np.ascontiguousarray(init)


def check_case(H, W, B, S, N, seed, opts, skipped=False, strict=True, **kw):
    """The inputs of a case with their reference, after asserting on the helper alone that the case decides nothing by a tie and
    (strict) takes every branch in every problem: margin >= 1e-9, 0 < valid < solved < candidates < H * W, a pixel started from
    depth_init and one from the linear start, and — with at least one step — a rejected step."""
    sc, slots, init = case_inputs(H, W, B, S, N, seed, opts, skipped)
    depth, info, views, counts, margin, per = reference_batch(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], init, **kw)
    assert margin >= MIN_MARGIN, (H, W, B, S, seed, margin)
    if strict:
        for o in per:
            c = o["counts"]
            assert 0 < c[2] < c[1] < c[0] < H * W, (H, W, seed, c.tolist())
            assert o["from_init"].any() and o["from_linear"].any(), (H, W, seed)
            assert kw.get("iters", DEFAULTS["iters"]) == 0 or o["rejected"] > 0, (H, W, seed)
    return sc, slots, init, (depth, info, views, counts), per


_REFERENCES = {}


def reference(case, iters=DEFAULTS["iters"]):
    """check_case of an entry of CASES (or FULL_CASE is NOT meant: its reference is the host form) with `iters` steps, computed
    once per process and shared by the tests that need it; nobody writes into it."""
    name, H, W, B, S, N, seed, opts, kw, skipped = case
    if (name, iters) not in _REFERENCES:
        _REFERENCES[name, iters] = check_case(H, W, B, S, N, seed, opts, skipped=skipped, iters=iters, **kw)
    return _REFERENCES[name, iters]


def last_valid_two_view(acc, alive, poses, calib):
    """The depth the flow track's own rule leaves for these views: flow_track_ref over the views in order with a zero pair flow
    (the chain adds nothing: acc_out = acc), so at every pixel the two-view triangulation of the last view where it is valid."""
    from flow_track_ref import flow_track_ref
    N, _, H, W = acc.shape
    depth = np.zeros((H, W), dtype=np.float32)
    zero = np.zeros((2, H, W), dtype=np.float32)
    for k in range(N):
        _, _, depth, _, _ = flow_track_ref(zero, None, acc[k], alive[k], poses[k], calib, depth)
    return depth


def same_bits(a, b):
    """Equal dtype, shape and bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = {4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(v), b.view(v)))


def same_outputs(got, want):
    return len(got) == len(want) == 4 and all(same_bits(g, w) for g, w in zip(got, want))
