"""NumPy float64 restatement of the two-view rule (include/atdn_hip.h, atdn_flow_two_view_depth) and the scene generator of its
tests: helper of the two-view tests, not a test, and not a call into the library.

For pixel (x, y) of a flow [2, H, W] (channel 0 = x) and a pose of 12 values (rows of [R|t], X1 = R X2 + t), every array operation
below is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the rule states; see
`two_view_ref`. The rule has only + - * / and comparisons, all correctly rounded in IEEE arithmetic, so every correct float64
evaluation gives the same bits — unless a decision quantity sits on its threshold, where nothing may be assumed of an
implementation that is merely correct to the last bit. `margin` is the smallest relative distance of any decision quantity from
its threshold over the pixels where that decision is taken: epi2 from max_epipolar^2, sin2 from min_sin2, z1 from max_depth (each
relative to the threshold), x2 from 0 and W-1, y2 from 0 and H-1 (relative to W-1, H-1; x2 and y2 are exact sums, the margin only
shows that no pixel is decided by a tie). With 1e-9 — six orders of magnitude above float64 rounding of these ~100-operation
expressions — the tests compare exactly."""
import numpy as np

MIN_MARGIN = 1e-9
FLT_MIN = float(np.finfo(np.float32).tiny)          # 2^-126
DEFAULTS = dict(max_epipolar=1.0, min_parallax_deg=0.05, max_depth=80.0)


def min_sin2_of(min_parallax_deg):
    import math
    return math.sin(math.radians(float(min_parallax_deg))) ** 2


def two_view_ref(flow, pose12, calib, mask=None, max_epipolar=1.0, min_sin2=None, max_depth=80.0):
    """flow [2,H,W] float32, pose12 [12] float32, calib (fx, fy, cx, cy), mask [H,W] uint8 or None ->
    (depth [H,W] float32, counts [3] int32, margin float)."""
    f, P = np.asarray(flow), np.asarray(pose12)
    assert f.dtype == np.float32 and f.ndim == 3 and f.shape[0] == 2 and P.dtype == np.float32 and P.shape == (12,)
    if min_sin2 is None:
        min_sin2 = min_sin2_of(DEFAULTS["min_parallax_deg"])
    fx, fy, cx, cy = (float(v) for v in calib)
    _, H, W = f.shape
    M = P.astype(np.float64).reshape(3, 4)
    r, t = M[:, :3], M[:, 3]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = f[0].astype(np.float64), f[1].astype(np.float64)
    keep = np.ones((H, W), dtype=bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    with np.errstate(all="ignore"):
        x2, y2 = xs + u, ys + v
        inside = keep & (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1)
        a0, a1 = (xs - cx) / fx, (ys - cy) / fy
        q0, q1 = (x2 - cx) / fx, (y2 - cy) / fy
        b = [(r[i, 0] * q0 + r[i, 1] * q1) + r[i, 2] for i in range(3)]
        n0, n1, n2 = t[1] - t[2] * a1, t[2] * a0 - t[0], t[0] * a1 - t[1] * a0
        res = (n0 * b[0] + n1 * b[1]) + n2 * b[2]
        m0 = (r[0, 0] * n0 + r[1, 0] * n1) + r[2, 0] * n2
        m1 = (r[0, 1] * n0 + r[1, 1] * n1) + r[2, 1] * n2
        l0, l1 = m0 / fx, m1 / fy
        epi2 = (res * res) / (l0 * l0 + l1 * l1)
        thr = max_epipolar * max_epipolar
        inlier = inside & (epi2 <= thr)
        aa = (a0 * a0 + a1 * a1) + 1.0
        bb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
        ab = (a0 * b[0] + a1 * b[1]) + b[2]
        at = (a0 * t[0] + a1 * t[1]) + t[2]
        bt = (b[0] * t[0] + b[1] * t[1]) + b[2] * t[2]
        p = aa * bb
        det = p - ab * ab
        sin2 = det / p
        z1 = (bb * at - ab * bt) / det
        z2 = (ab * at - aa * bt) / det
        valid = inlier & (sin2 >= min_sin2) & (z1 >= FLT_MIN) & (z2 > 0) & (z1 <= max_depth)
        depth = np.where(valid, z1, 0.0).astype(np.float32)

        def rel(q, thr_, where):
            d = np.abs(q - thr_) / (abs(thr_) if thr_ != 0 else 1.0)
            d = np.where(where & np.isfinite(d), d, np.inf)
            return float(d.min()) if d.size else np.inf

        kept = keep & np.isfinite(x2) & np.isfinite(y2)
        margin = min(rel(epi2, thr, inside), rel(sin2, min_sin2, inlier), rel(z1, max_depth, inlier),
                     rel(x2 / max(W - 1, 1), 0.0, kept), rel(x2 / max(W - 1, 1), 1.0 if W > 1 else 0.0, kept),
                     rel(y2 / max(H - 1, 1), 0.0, kept), rel(y2 / max(H - 1, 1), 1.0 if H > 1 else 0.0, kept))
    counts = np.array([inside.sum(), inlier.sum(), valid.sum()], dtype=np.int32)
    return depth, counts, margin


def reference_batch(flow, pose, calib, mask=None, **kw):
    """The helper over a batch: (depth [B,1,H,W] float32, counts [B,3] int32, smallest margin)."""
    B = flow.shape[0]
    out = [two_view_ref(flow[b], pose[b], calib, None if mask is None else mask[b], **kw) for b in range(B)]
    return np.stack([o[0] for o in out])[:, None], np.stack([o[1] for o in out]), min(o[2] for o in out)


def euler_yxz(angles):
    """Rotation matrix of yxz Euler angles (a about y, b about x, c about z): Ry(a) Rx(b) Rz(c), float64."""
    a, b, c = (float(v) for v in angles)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return ry @ rx @ rz


def scene_calib(H, W):
    return 718.856 * W / 1241.0, 718.856 * W / 1241.0, (W - 1) / 2.0 + 0.3, (H - 1) / 2.0 - 0.2


def scene(H, W, seed, B=1, disturbance=1.5, zero_translation=False):
    """A synthetic two-view scene: (flow [B,2,H,W] float32, pose [B,12] float32, calib, Z [B,H,W] float64 the true depth).
    Per image a smooth depth Z = 4 + 116 * (1/2 + 1/2 cos(2 pi (x/W (1+b) + 0.13 seed))) * (1/2 + 1/2 cos(pi y/H)), a rotation of
    Euler angles uniform in +-0.02 (yxz), t = (U(+-0.1), U(+-0.05), U(0.6, 1.4)) — the camera drives forward —,
    flow = project(R^T (X1 - t)) - pixel, plus a smooth sinusoidal disturbance of `disturbance` pixels. Flow and pose are rounded to
    float32, so the true depth is met only up to that rounding."""
    rs = np.random.RandomState(seed)
    fx, fy, cx, cy = scene_calib(H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.zeros((B, 2, H, W))
    pose = np.zeros((B, 12))
    depth = np.zeros((B, H, W))
    for b in range(B):
        Z = 4.0 + 116.0 * (0.5 + 0.5 * np.cos(2 * np.pi * (xs / W * (1 + b) + 0.13 * seed))) * (0.5 + 0.5 * np.cos(np.pi * ys / H))
        R = euler_yxz(rs.uniform(-0.02, 0.02, 3))
        t = np.array([rs.uniform(-0.1, 0.1), rs.uniform(-0.05, 0.05), rs.uniform(0.6, 1.4)])
        if zero_translation:
            t = np.zeros(3)
        # the pose as float32 is what the rule sees: generate the flow from the rounded pose
        P = np.concatenate([R, t[:, None]], axis=1).astype(np.float32)
        R32, t32 = P[:, :3].astype(np.float64), P[:, 3].astype(np.float64)
        X1 = np.stack([Z * (xs - cx) / fx, Z * (ys - cy) / fy, Z])
        X2 = np.einsum("ji,jhw->ihw", R32, X1 - t32[:, None, None])          # R^T (X1 - t)
        x2 = fx * X2[0] / X2[2] + cx
        y2 = fy * X2[1] / X2[2] + cy
        ph = 0.7 * seed + 1.3 * b
        du = disturbance * np.sin(2 * np.pi * (1.7 * xs / W + 0.9 * ys / H) + ph)
        dv = disturbance * np.cos(2 * np.pi * (0.8 * xs / W + 2.3 * ys / H) + 0.5 * ph)
        flow[b, 0], flow[b, 1] = x2 - xs + du, y2 - ys + dv
        pose[b] = P.reshape(12)
        depth[b] = Z
    return flow.astype(np.float32), pose.astype(np.float32), (fx, fy, cx, cy), depth


# (name, H, W, B, seed) of the random cases shared by the host and the GPU tests; disturbance 1.5 px, default thresholds
CASES = [("5x7", 5, 7, 1, 2), ("9x33_b3", 9, 33, 3, 3), ("8x16_b2", 8, 16, 2, 4), ("47x154_b2", 47, 154, 2, 5)]
FULL_CASE = ("376x1232_b2", 376, 1232, 2, 6)


def check_case(H, W, B, seed, disturbance=1.5, mask=None):
    """The scene of a case with its reference, after asserting on the helper alone that the case decides nothing by a tie and
    exercises every outcome: margin >= 1e-9 and 0 < valid < inliers < inside < H * W in every image."""
    flow, pose, calib, Z = scene(H, W, seed, B, disturbance)
    depth, counts, margin = reference_batch(flow, pose, calib, mask, min_sin2=min_sin2_of(DEFAULTS["min_parallax_deg"]))
    assert margin >= MIN_MARGIN, (H, W, B, seed, margin)
    if mask is None:
        for c in counts:
            assert 0 < c[2] < c[1] < c[0] < H * W, (H, W, B, seed, counts.tolist())
    return flow, pose, calib, Z, depth, counts
