"""NumPy float64 restatement of the flow-track rule (include/atdn_hip.h, atdn_flow_track_step) and the scene generators of its
tests: helper of the flow-track tests, not a test, and not a call into the library.

For pixel (x, y) of an anchor frame with state (acc [2, H, W] float32, alive [H, W] uint8) and the flow [2, H, W] of the pair
frame k -> k+1, every array operation of `flow_track_ref` is one IEEE float64 operation per element (NumPy never fuses a multiply
with an add), in the order the rule states. The rule has only + - * /, floor, comparisons and one float64 -> float32 rounding, all
correctly rounded in IEEE arithmetic, so every correct evaluation gives the same bits. The depth part is `two_view_ref` of
tests/two_view_ref.py on the new acc with the new alive as its mask; its `margin` is handed through."""
import numpy as np

from two_view_ref import DEFAULTS, MIN_MARGIN, euler_yxz, min_sin2_of, scene, scene_calib, two_view_ref  # noqa: F401

DBL_MAX = float(np.finfo(np.float64).max)


def flow_track_ref(flow, mask, acc, alive, pose12=None, calib=None, depth=None, max_epipolar=1.0, min_sin2=None, max_depth=80.0):
    """One image. flow [2,H,W] float32, mask [H,W] uint8 or None, acc [2,H,W] float32, alive [H,W] uint8; pose12 [12] float32 or
    None, with it calib (fx, fy, cx, cy) and depth [H,W] float32 -> (acc_out [2,H,W] float32, alive_out [H,W] uint8 of 0 / 1,
    depth_out [H,W] float32 or None, counts [4] int32, margin of the two-view part or inf)."""
    f, a = np.asarray(flow), np.asarray(acc)
    assert f.dtype == np.float32 and a.dtype == np.float32 and f.shape == a.shape and f.ndim == 3 and f.shape[0] == 2
    _, H, W = f.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    live = np.asarray(alive).reshape(H, W) != 0
    ux, uy = a[0].astype(np.float64), a[1].astype(np.float64)
    with np.errstate(all="ignore"):
        x1, y1 = xs + ux, ys + uy
        inside = live & (x1 >= 0) & (x1 <= W - 1) & (y1 >= 0) & (y1 <= H - 1)
        # the pixels that are not inside read nothing: give them a harmless position, their results are dropped below
        x1, y1 = np.where(inside, x1, 0.0), np.where(inside, y1, 0.0)
        xf, yf = np.floor(x1), np.floor(y1)
        ax, ay = x1 - xf, y1 - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        xn, yn = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        wx, wy = 1.0 - ax, 1.0 - ay
        s = []
        for c in range(2):
            p = f[c].astype(np.float64)
            t00, t10, t01, t11 = p[y0, x0], p[y0, xn], p[yn, x0], p[yn, xn]
            top = t00 * wx + t10 * ax
            bot = t01 * wx + t11 * ax
            s.append(top * wy + bot * ay)
        nx, ny = ux + s[0], uy + s[1]
        finite = (np.abs(nx) <= DBL_MAX) & (np.abs(ny) <= DBL_MAX)
        if mask is None:
            trusted = np.ones((H, W), dtype=bool)
        else:
            xm, ym = np.floor(x1 + 0.5).astype(np.int64), np.floor(y1 + 0.5).astype(np.int64)
            trusted = np.asarray(mask).reshape(H, W)[ym, xm] != 0
        ox, oy = nx.astype(np.float32), ny.astype(np.float32)
        alive_out = inside & finite & trusted & ~np.isinf(ox) & ~np.isinf(oy)
    acc_out = a.copy()                                   # a dead pixel keeps its bits
    acc_out[0][alive_out] = ox[alive_out]
    acc_out[1][alive_out] = oy[alive_out]
    counts = np.zeros(4, dtype=np.int32)
    counts[0] = alive_out.sum()
    if pose12 is None:
        return acc_out, alive_out.astype(np.uint8), None, counts, np.inf
    if min_sin2 is None:
        min_sin2 = min_sin2_of(DEFAULTS["min_parallax_deg"])
    d2, c2, margin = two_view_ref(acc_out, np.asarray(pose12), calib, alive_out.astype(np.uint8), max_epipolar, min_sin2, max_depth)
    depth_out = np.asarray(depth, dtype=np.float32).reshape(H, W).copy()
    depth_out[d2 != 0] = d2[d2 != 0]                     # a valid depth is a normal positive float32: never 0
    counts[1:] = c2
    return acc_out, alive_out.astype(np.uint8), depth_out, counts, margin


def reference_step(flow, mask, acc, alive, pose=None, calib=None, depth=None, **kw):
    """The helper over a batch: flow, acc [B,2,H,W], mask, alive [B,H,W], pose [B,12], depth [B,1,H,W] ->
    (acc_out, alive_out, depth_out [B,1,H,W] or None, counts [B,4], smallest margin)."""
    B = flow.shape[0]
    out = [flow_track_ref(flow[b], None if mask is None else mask[b], acc[b], alive[b], None if pose is None else pose[b], calib,
                          None if depth is None else depth[b, 0], **kw) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            None if pose is None else np.stack([o[2] for o in out])[:, None], np.stack([o[3] for o in out]), min(o[4] for o in out))


def pose_rows(mats):
    """[B,4,4] float64 -> [B,12] float32, the rows of [R|t]."""
    return np.ascontiguousarray(np.asarray(mats)[:, :3, :].reshape(len(mats), 12)).astype(np.float32)


def pose_mats(rows):
    """[B,12] float32 -> [B,4,4] float64."""
    m = np.tile(np.eye(4), (len(rows), 1, 1))
    m[:, :3, :] = np.asarray(rows, dtype=np.float64).reshape(len(rows), 3, 4)
    return m


# (name, H, W, B, seed) of the random sequences shared by the host and the GPU tests: those of the two-view tests
CASES = [("5x7", 5, 7, 1, 2), ("9x33_b3", 9, 33, 3, 3), ("8x16_b2", 8, 16, 2, 4), ("47x154_b2", 47, 154, 2, 5)]
FULL_CASE = ("376x1232_b2", 376, 1232, 2, 6)
STEPS = 4


def sequence(H, W, B, seed, steps=STEPS, noise=0.05):
    """A random sequence: per step the flow of a synthetic two-view scene (two_view_ref.scene: a camera that drives forward over a
    smooth depth map, plus a smooth 1.5-pixel disturbance — large enough that tracks leave the image) plus Gaussian noise of
    `noise` pixels, and the accumulated pose anchor <- frame k+1 (the float64 product of the steps' float32 poses, rounded).
    Returns (flows [steps,B,2,H,W] float32, poses [steps,B,12] float32, masks [steps,B,H,W] uint8 with ~12 % zeros, calib)."""
    rs = np.random.RandomState(1000 + seed)
    flows, poses, masks = [], [], []
    P = np.tile(np.eye(4), (B, 1, 1))
    calib = scene_calib(H, W)
    for k in range(steps):
        flow, rel, _, _ = scene(H, W, seed + 17 * k, B, 1.5)
        flow = (flow.astype(np.float64) + noise * rs.standard_normal(flow.shape)).astype(np.float32)
        P = P @ pose_mats(rel)
        flows.append(flow)
        poses.append(pose_rows(P))
        masks.append((rs.uniform(size=(B, H, W)) > 0.12).astype(np.uint8))
    return np.stack(flows), np.stack(poses), np.stack(masks), calib


def reference_sequence(flows, poses, masks, calib, **kw):
    """The helper along a sequence from a fresh track (acc 0, all alive, depth 0): a list, per step, of
    (acc, alive, depth, counts), and the smallest two-view margin. `poses` None: the chain-only form; `masks` None: no mask."""
    steps, B, _, H, W = flows.shape
    acc = np.zeros((B, 2, H, W), dtype=np.float32)
    alive = np.ones((B, H, W), dtype=np.uint8)
    depth = None if poses is None else np.zeros((B, 1, H, W), dtype=np.float32)
    out, margin = [], np.inf
    for k in range(steps):
        acc, alive, depth, counts, m = reference_step(flows[k], None if masks is None else masks[k], acc, alive,
                                                      None if poses is None else poses[k], calib, depth, **kw)
        margin = min(margin, m)
        out.append((acc, alive, depth, counts))
    return out, margin


# ------------------------------------------------------------------ the drive: what the feature is for
DRIVE = dict(H=47, W=154, steps=8, noise=0.3, seed=11)


def drive(H=47, W=154, steps=8, noise=0.3, seed=11):
    """A camera 1.65 m above a ground plane (Y = 1.65, y down) drives `steps` steps of about 1 m towards a slanted wall
    (Z + 0.4 X = 40 in the first camera's frame), with small random rotations and side steps. Every pixel of every frame sees the
    nearer of the two planes. Returns (flows [steps,1,2,H,W] float32 — the true flow of pair k -> k+1 on frame k's grid plus
    Gaussian noise of `noise` pixels —, rel [steps,4,4] float64 — the pairs' relative poses, X_k = R X_k+1 + t, float32 values
    —, calib, Z0 [H,W] float64 the true depth of the first frame)."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = calib = scene_calib(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))])         # camera frame, a2 = 1: the scale IS the depth
    planes = [(np.array([0.0, 1.0, 0.0]), 1.65), (np.array([0.4, 0.0, 1.0]), 40.0)]   # n . X = d in the world (= first camera)
    T = np.eye(4)                                                              # world <- camera k
    flows, rels, Z0 = [], [], None
    for k in range(steps):
        R = euler_yxz(rs.uniform(-0.005, 0.005, 3))
        t = np.array([rs.uniform(-0.05, 0.05), rs.uniform(-0.02, 0.02), rs.uniform(0.9, 1.1)])
        rel = np.eye(4)
        rel[:3, :] = np.concatenate([R, t[:, None]], axis=1).astype(np.float32).astype(np.float64)
        o, d = T[:3, 3], np.einsum("ij,jhw->ihw", T[:3, :3], rays)
        Z = np.full((H, W), np.inf)
        for nrm, dist in planes:
            with np.errstate(all="ignore"):
                sc = (dist - nrm @ o) / np.einsum("i,ihw->hw", nrm, d)
            Z = np.where((sc > 0) & (sc < Z), sc, Z)
        assert np.isfinite(Z).all()
        if k == 0:
            Z0 = Z
        X2 = np.einsum("ji,jhw->ihw", rel[:3, :3], Z * rays - rel[:3, 3][:, None, None])   # R^T (X_k - t)
        flow = np.stack([fx * X2[0] / X2[2] + cx - xs, fy * X2[1] / X2[2] + cy - ys])
        flows.append((flow + noise * rs.standard_normal(flow.shape)).astype(np.float32)[None])
        rels.append(rel)
        T = T @ rel
    return np.stack(flows), np.stack(rels), calib, Z0


def drive_errors(depths, Z0):
    """Per depth map [H,W]: (median of |depth - Z0| / Z0 over the pixels with a depth, their number)."""
    out = []
    for d in depths:
        have = d > 0
        out.append((float(np.median(np.abs(d[have].astype(np.float64) - Z0[have]) / Z0[have])), int(have.sum())))
    return out


# ------------------------------------------------------------------ small sequences with a known answer, shared by the host and GPU tests
def _const_flow(B, H, W, u, v):
    f = np.empty((B, 2, H, W), dtype=np.float32)
    f[:, 0], f[:, 1] = u, v
    return f


def _rows(t, B=1):
    P = np.concatenate([np.eye(3), np.asarray(t, dtype=np.float64)[:, None]], axis=1)
    return np.repeat(P.reshape(1, 12), B, axis=0).astype(np.float32)


PLANE_CALIB = (64.0, 64.0, 5.0, 2.0)
AFFINE = dict(A=np.array([[0.03, -0.02], [0.015, 0.025]]), b=np.array([0.4, -0.3]), N=6, H=24, W=40)


def affine_flow(H, W):
    """flow(p) = A p + b on the grid, float32 (AFFINE)."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    A, b = AFFINE["A"], AFFINE["b"]
    return np.stack([A[0, 0] * xs + A[0, 1] * ys + b[0], A[1, 0] * xs + A[1, 1] * ys + b[1]]).astype(np.float32)[None]


def special_sequences():
    """name -> dict(flows [S,B,2,H,W], poses [S,B,12] or None, masks [S,B,H,W] or None, calib, init = (acc, alive, depth) or None):
    closed forms and non-finite inputs. Each is run from `init` (None: a fresh track) by the tests' own step loop."""
    out = {}
    H, W = 6, 12
    side = np.stack([_rows((0.25 * (k + 1), 0.0, 0.0), 2) for k in range(3)])
    out["zero"] = dict(flows=np.zeros((3, 2, 2, H, W), dtype=np.float32), poses=side, masks=None, calib=PLANE_CALIB, init=None)
    out["const"] = dict(flows=np.stack([_const_flow(2, H, W, 0.75, -0.5)] * 5), poses=None, masks=None, calib=None, init=None)
    out["plane"] = dict(flows=np.stack([_const_flow(2, H, W, -2.0, 0.0)] * 3), poses=side, masks=None, calib=PLANE_CALIB, init=None)
    out["affine"] = dict(flows=np.stack([affine_flow(AFFINE["H"], AFFINE["W"])] * AFFINE["N"]), poses=None, masks=None, calib=None,
                         init=None)
    # dead pixels (one with a NaN payload, one with an infinity in acc) under a flow that would carry them back inside
    acc = np.zeros((1, 2, H, W), dtype=np.float32)
    alive = np.ones((1, H, W), dtype=np.uint8)
    acc[0, 0, 2, 3], alive[0, 2, 3] = -5.0, 0                       # x1 = -2: outside; the flow +4 would bring it back
    acc[0, :, 1, 1] = np.array([0x7FC12345, 0xFFC00001], dtype=np.uint32).view(np.float32)
    alive[0, 1, 1] = 0
    acc[0, 0, 4, 4], alive[0, 4, 4] = 1.0, 0                        # dead although its position is inside
    acc[0, 0, 3, 0] = -1.5                                           # alive on entry, outside: dies now, keeps -1.5
    out["dead"] = dict(flows=np.stack([_const_flow(1, H, W, 4.0, 0.0)] * 2), poses=side[:2, :1], masks=None, calib=PLANE_CALIB,
                       init=(acc, alive, np.full((1, 1, H, W), 3.0, dtype=np.float32)))
    # the mask is read at the nearest pixel of where the track stands: x1 = k + 0.5 reads k + 1, x1 = W - 1 reads W - 1
    acc = np.zeros((1, 2, H, W), dtype=np.float32)
    acc[0, 0, 0, 2], acc[0, 0, 1, 2], acc[0, 0, 2, 2], acc[0, 0, 3, 5] = 0.5, 0.49, 0.5, 6.0
    acc[0, 1, 4, 7], acc[0, 1, 5, 7] = 0.5, -0.5                     # y1 = 4.5 reads row 5, y1 = 4.5 from below reads row 5 too
    mask = np.ones((1, 1, H, W), dtype=np.uint8)
    mask[0, 0, 0, 3], mask[0, 0, 1, 3], mask[0, 0, 2, 2], mask[0, 0, 3, W - 1], mask[0, 0, 5, 7] = 0, 0, 0, 0, 0
    out["mask"] = dict(flows=np.zeros((1, 1, 2, H, W), dtype=np.float32), poses=None, masks=mask, calib=None,
                       init=(acc, np.full((1, H, W), 1, dtype=np.uint8), None))
    out["1x1"] = dict(flows=np.zeros((2, 1, 2, 1, 1), dtype=np.float32), poses=np.stack([_rows((0.5, 0.0, 0.0))] * 2), masks=None,
                      calib=(5.0, 5.0, 0.0, 0.0), init=None)
    # alive bytes other than 0 and 1 are alive; the output is 0 / 1
    alive = np.array([0, 1, 2, 7, 128, 255, 0, 3, 0, 0, 64, 1], dtype=np.uint8).reshape(1, 1, W).repeat(H, axis=1)
    out["alive_bytes"] = dict(flows=np.stack([_const_flow(1, H, W, 0.25, 0.25)]), poses=None, masks=None, calib=None,
                              init=(np.zeros((1, 2, H, W), dtype=np.float32), alive, None))
    # the largest float32 in a tap: the sum FLT_MAX + 3 rounds to FLT_MAX and the track lives (a sum of an acc inside the image
    # and a bilinear mean of float32 taps stays below 2^128 - 2^103, so no finite input reaches the rule's float32-infinity clause)
    flow = np.zeros((1, 1, 2, H, W), dtype=np.float32)
    flow[0, 0, 0, 2, 3] = np.finfo(np.float32).max
    flow[0, 0, 1, 2, 3] = -np.finfo(np.float32).max
    acc = np.zeros((1, 2, H, W), dtype=np.float32)
    acc[0, 0, 2, 0], acc[0, 1, 2, 0] = 3.0, 0.0                      # (0, 2) stands on (3, 2)
    out["float_max"] = dict(flows=np.concatenate([flow, flow]), poses=side[:2, :1], masks=None, calib=PLANE_CALIB,
                            init=(acc, np.ones((1, H, W), dtype=np.uint8), np.zeros((1, 1, H, W), dtype=np.float32)))
    # non-finite values: in acc_in, in each of the four taps of pixel (4, 2) standing at (4.25, 2.5) or — zero weights — at (4, 2)
    for name, bad in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        flows, poses, masks, calib = sequence(9, 33, 1, 3, steps=2)
        acc = np.zeros((1, 2, 9, 33), dtype=np.float32)
        acc[0, 0, 5, 7] = bad
        acc[0, 1, 6, 8] = bad
        out["acc_" + name] = dict(flows=flows, poses=poses, masks=None, calib=calib,
                                  init=(acc, np.ones((1, 9, 33), dtype=np.uint8), np.zeros((1, 1, 9, 33), dtype=np.float32)))
        for frac in (True, False):
            for t, (ty, tx) in enumerate(((2, 4), (2, 5), (3, 4), (3, 5))):
                for c in (0, 1):
                    f = flows.copy()
                    f[0, 0, c, ty, tx] = bad
                    acc = np.zeros((1, 2, 9, 33), dtype=np.float32)
                    if frac:
                        acc[0, 0, 2, 4], acc[0, 1, 2, 4] = 0.25, 0.5
                    out["tap%d%d_%s_%s" % (t, c, "frac" if frac else "int", name)] = dict(
                        flows=f, poses=poses, masks=None, calib=calib,
                        init=(acc, np.ones((1, 9, 33), dtype=np.uint8), np.zeros((1, 1, 9, 33), dtype=np.float32)))
        for j in (0, 5, 11):
            p = poses.copy()
            p[:, 0, j] = bad
            out["pose%d_%s" % (j, name)] = dict(flows=flows, poses=p, masks=None, calib=calib, init=None)
    return out


def run_sequence(step, seq, **kw):
    """Run a sequence of `special_sequences` (or dict(flows, poses, masks, calib, init)) with `step(flow, mask, acc, alive, pose,
    calib, depth, **kw) -> (acc, alive, depth, counts)` on NumPy arrays; returns the per-step list of those four."""
    flows, poses, masks, calib, init = seq["flows"], seq["poses"], seq["masks"], seq["calib"], seq["init"]
    S, B, _, H, W = flows.shape
    if init is None:
        acc, alive = np.zeros((B, 2, H, W), dtype=np.float32), np.ones((B, H, W), dtype=np.uint8)
        depth = None if poses is None else np.zeros((B, 1, H, W), dtype=np.float32)
    else:
        acc, alive, depth = init
    out = []
    for k in range(S):
        acc, alive, depth, counts = step(flows[k], None if masks is None else masks[min(k, len(masks) - 1)], acc, alive,
                                         None if poses is None else poses[k], calib, depth, **kw)
        out.append((acc, alive, depth, counts))
    return out


def helper_step(flow, mask, acc, alive, pose, calib, depth, **kw):
    return reference_step(flow, mask, acc, alive, pose, calib, depth, **kw)[:4]


def same_bits(a, b):
    """Equal dtype, shape and bits (NaN payloads included)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    v = {4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(v), b.view(v)))


def same_steps(got, want):
    return len(got) == len(want) and all(all(same_bits(g, w) for g, w in zip(gs, ws)) for gs, ws in zip(got, want))
