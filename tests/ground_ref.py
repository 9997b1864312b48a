"""NumPy float64 restatement of the ground-plane rule (include/atdn_hip.h, atdn_ground_terms, atdn_ground_solve and
atdn_ground_classify), the scenes and the case table of its tests: helper of the ground tests, not a test, and not a call into the
library.

Every array operation below is one IEEE float64 operation per element (NumPy never fuses a multiply with an add), in the order the
rule states; the rule has only + - * /, comparisons and integer operations and fixes the order of every sum — four pixels per
thread, a binary tree over the 256 threads of a chunk, the chunks in order (`cumsum`, which adds sequentially) —, so every correct
evaluation gives the same bits. The vote's bin is written here with `frexp` (mantissa and exponent as numbers), not with the bit
pattern the header states it with: two statements of one integer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multiview_ref import scene as street, scene_calib  # noqa: E402

CHUNK = 1024
BINS = 320
DBL_MAX = float(np.finfo(np.float64).max)
# what the tests pass, always explicitly (the library's defaults are the maintainer's choice)
OPTS = dict(scale_rel=0.05, inlier_rel=0.05, min_z=0.1, max_depth=80.0)
H_TRUE = 1.65


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


def default_rows(calib, H):
    return max(int(np.floor(calib[3])) + 1, 0), H


def _band(depth, calib, mask, rows, min_z, max_depth):
    """The band's pixels in flat order: (z, ax, ay, cand, used), each [(y1 - y0) * W]."""
    d = np.asarray(depth)
    assert d.dtype == np.float32 and d.ndim == 2
    H, W = d.shape
    fx, fy, cx, cy = (float(v) for v in calib)
    y0, y1 = default_rows(calib, H) if rows is None else rows
    ys, xs = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = d[y0:y1].astype(np.float64)
    cand = np.ones(z.shape, dtype=bool) if mask is None else (np.asarray(mask).reshape(H, W)[y0:y1] != 0)
    with np.errstate(all="ignore"):
        used = cand & (z >= min_z) & (z <= max_depth)
    ax, ay = (xs - cx) / fx, (ys - cy) / fy
    return z.ravel(), ax.ravel(), ay.ravel(), cand.ravel(), used.ravel()


def terms_ref(depth, q, calib, mask=None, rows=None, scale_rel=None, inlier_rel=None, min_z=None, max_depth=None):
    """One plane: depth [H,W] float32, q [3] float64 -> (sums [10] float64, counts [3] int32)."""
    z, ax, ay, cand, used = _band(depth, calib, mask, rows, min_z, max_depth)
    q = np.asarray(q, dtype=np.float64)
    c2, thr = scale_rel * scale_rel, inlier_rel * inlier_rel
    with np.errstate(all="ignore"):
        e = z * ((q[0] * ax + q[1] * ay) + q[2] * 1.0) - 1.0
        e2 = e * e
        s = 1.0 + e2 / c2
        w = 1.0 / (s * s)
        rho = (0.5 * e2) / s
        J = [z * ax, z * ay, z]
        t = [(w * J[i]) * J[j] for i in range(3) for j in range(i, 3)] + [(w * J[i]) * e for i in range(3)] + [rho]
        t = np.where(used[None], np.stack(t), 0.0)
        inlier = used & (e2 <= thr)
    return plane_sum(t), np.array([cand.sum(), used.sum(), inlier.sum()], dtype=np.int32)


def vote_bins(depth, calib, n0, mask=None, rows=None, min_z=None, max_depth=None, **_):
    """The histogram [320] of the start vote of one plane."""
    z, ax, ay, _, used = _band(depth, calib, mask, rows, min_z, max_depth)
    with np.errstate(all="ignore"):
        h = z * ((n0[0] * ax + n0[1] * ay) + n0[2] * 1.0)
        ok = used & (h >= 2.0 ** -4) & (h < 2.0 ** 6)
    m, ex = np.frexp(np.where(ok, h, 1.0))                        # h = m 2^ex, 0.5 <= m < 1
    k = (ex - 1 + 4) * 32 + np.floor((2.0 * m - 1.0) * 32.0).astype(np.int64)
    return np.bincount(k[ok], minlength=BINS).astype(np.int64)


def bin_centre(k):
    return 2.0 ** (k // 32 - 4) * (1.0 + ((k % 32) + 0.5) / 32.0)


def vote_mode(hist):
    sm = hist.copy()
    sm[1:] += hist[:-1]
    sm[:-1] += hist[1:]
    # the largest smoothed count; among equals the largest own count; among those the first: the lowest bin
    k = int(np.argmax(sm * (int(hist.sum()) + 1) + hist))
    return k, int(sm[k])


def lm_step(sums, lam, q):
    """The damped 3 x 3 step of the rule from the accepted point, or q again where the factorisation fails."""
    A = np.zeros((3, 3))
    n = 0
    for i in range(3):
        for j in range(i, 3):
            A[i, j] = A[j, i] = sums[n]
            n += 1
    g = sums[6:9]
    for i in range(3):
        A[i, i] = A[i, i] + lam * A[i, i]
    L, D = np.zeros((3, 3)), np.zeros(3)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(3):
            dj = A[j, j]
            for k in range(j):
                dj = dj - L[j, k] * (L[j, k] * D[k])
            ok = ok and bool(dj > 0.0)
            D[j] = dj
            for i in range(j + 1, 3):
                l = A[i, j]
                for k in range(j):
                    l = l - L[i, k] * (L[j, k] * D[k])
                L[i, j] = l / dj
        dl = np.zeros(3)
        for i in range(3):
            y = -g[i]
            for k in range(i):
                y = y - L[i, k] * dl[k]
            dl[i] = y
        for i in range(3):
            dl[i] = dl[i] / D[i]
        for i in range(2, -1, -1):
            y = dl[i]
            for k in range(i + 1, 3):
                y = y - L[k, i] * dl[k]
            dl[i] = y
        ok = ok and bool(np.all(np.abs(dl) <= DBL_MAX))
        return q + dl if ok else q.copy()


def solve_ref(depth, calib, n0=(0.0, 1.0, 0.0), q_init=None, mask=None, rows=None, iters=8, min_votes=None, **opts):
    """One plane: (q [3] float64, sums [10] float64, counts [6] int32)."""
    n0 = np.asarray(n0, dtype=np.float64)
    if q_init is None:
        k, votes = vote_mode(vote_bins(depth, calib, n0, mask, rows, **opts))
        if votes < min_votes:
            return np.zeros(3), np.zeros(10), np.zeros(6, dtype=np.int32)
        qt = n0 / bin_centre(k)
    else:
        k, votes, qt = -1, 0, np.asarray(q_init, dtype=np.float64).copy()
    lam, accepted = 1e-3, 0
    for it in range(iters + 1):
        sums, counts = terms_ref(depth, qt, calib, mask, rows, **opts)
        if it == 0 or sums[9] < acc_sums[9]:
            qa, acc_sums, acc_counts = qt, sums, counts
            if it > 0:
                lam = max(lam / 3.0, 1e-9)
                accepted += 1
        else:
            lam = min(4.0 * lam, 1e6)
        if it < iters:
            qt = lm_step(acc_sums, lam, qa)
    return qa, acc_sums, np.concatenate([acc_counts, [accepted, votes, k]]).astype(np.int32)


def classify_ref(depth, q, calib, mask=None, rows=None, inlier_rel=None, min_z=None, max_depth=None, **_):
    """One plane: (residual [H,W] float32, on_ground [H,W] uint8)."""
    H, W = depth.shape
    y0, y1 = default_rows(calib, H) if rows is None else rows
    z, ax, ay, _, used = _band(depth, calib, mask, rows, min_z, max_depth)
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = z * ((q[0] * ax + q[1] * ay) + q[2] * 1.0) - 1.0
        inl = used & (e * e <= inlier_rel * inlier_rel)
        e32 = np.where(used, e, 0.0).astype(np.float32)
    res, on = np.zeros((H, W), dtype=np.float32), np.zeros((H, W), dtype=np.uint8)
    res[y0:y1], on[y0:y1] = e32.reshape(y1 - y0, W), inl.reshape(y1 - y0, W)
    return res, on


def terms_batch(depth, q, calib, mask=None, **kw):
    out = [terms_ref(depth[b], q[b], calib, None if mask is None else mask[b], **kw) for b in range(depth.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def solve_batch(depth, calib, n0, q_init=None, mask=None, **kw):
    out = [solve_ref(depth[b], calib, n0, None if q_init is None else q_init[b], None if mask is None else mask[b], **kw)
           for b in range(depth.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def classify_batch(depth, q, calib, mask=None, **kw):
    out = [classify_ref(depth[b], q[b], calib, None if mask is None else mask[b], **kw) for b in range(depth.shape[0])]
    return np.stack([o[0] for o in out])[:, None], np.stack([o[1] for o in out])


def height_of(q):
    n = np.sqrt((np.asarray(q) ** 2).sum(-1))
    return 1.0 / n


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ scenes
def tilt_normal(pitch_deg, roll_deg):
    """The road's normal in the camera frame (y down) of a camera pitched and rolled against it."""
    p, r = np.radians(pitch_deg), np.radians(roll_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    return rz @ rx @ np.array([0.0, 1.0, 0.0])


def plane_depth(H, W, normal, height, calib=None):
    """The noise-free float32 depth of the plane normal . X = height (0 where the ray does not meet it in front of the camera)."""
    fx, fy, cx, cy = calib = scene_calib(H, W) if calib is None else calib
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    na = normal[0] * (xs - cx) / fx + normal[1] * (ys - cy) / fy + normal[2]
    with np.errstate(all="ignore"):
        z = np.where(na > 1e-9, height / na, 0.0)
    return z.astype(np.float32), calib


def street_depth(H, W, seed, scale=1.0, noise=0.02, holes=0.2, outliers=0.05, far=40.0):
    """The anchor depth of multiview_ref.scene (the nearer of the road 1.65 m below the camera and a smooth wall between 6 m and
    `far`), times `scale`, with Gaussian noise of `noise` (relative), `holes` of the pixels 0 and `outliers` of them multiplied by
    U(0.3, 3). Returns (depth [H,W] float32, calib)."""
    sc = street(H, W, 1, seed, far=far)
    rs = np.random.RandomState(5000 + seed)
    z = scale * sc["Z"] * (1.0 + noise * rs.standard_normal((H, W)))
    pick = rs.uniform(size=(H, W))
    z = np.where(pick < outliers, z * rs.uniform(0.3, 3.0, (H, W)), z)
    z = np.where(pick > 1.0 - holes, 0.0, z)
    return z.astype(np.float32), sc["calib"]


# (name, H, W, rows or None, seed): the cases shared by the host and the GPU tests. 5x7: one ragged chunk; 9x33 with the band (1, 9):
# the band starts off the 16-byte grid; 32x32 with all rows: exactly one chunk; 33x31: 1023 pixels; 47x154: 8 chunks in all rows.
CASES = [("5x7", 5, 7, None, 1), ("9x33_band1", 9, 33, (1, 9), 2), ("32x32", 32, 32, (0, 32), 3), ("33x31", 33, 31, (0, 33), 4),
         ("47x154", 47, 154, (0, 47), 5)]
FULL_CASE = ("376x1232_b2", 376, 1232, None, 6)
CASE_N0 = (0.0, 0.9993908270190958, 0.03489949670250097)        # the level normal pitched by 2 degrees
CASE_MIN_VOTES = 3
_cache = {}


def case_inputs(H, W, B, seed):
    """depth [B,H,W] float32 (plane b at scale 1, 0.8, 1.25; with a NaN, an infinity, a negative and a far depth in the last row),
    mask [B,H,W] uint8 with ~12 % zeros, calib, q_init [B,3] (the true plane at 1.1 of its height, slightly turned)."""
    key = (H, W, B, seed)
    if key not in _cache:
        rs = np.random.RandomState(7000 + seed)
        depth, q0 = np.zeros((B, H, W), dtype=np.float32), np.zeros((B, 3))
        for b in range(B):
            s = (1.0, 0.8, 1.25)[b % 3]
            depth[b], calib = street_depth(H, W, seed + 10 * b, scale=s, far=12.0 if H < 32 else 40.0)
            depth[b, H - 1, :4] = (np.nan, np.inf, -1.0, 200.0)
            q0[b] = np.array([0.01, 1.0, -0.02]) / (1.1 * s * H_TRUE)
        mask = (rs.uniform(size=(B, H, W)) > 0.12).astype(np.uint8)
        for a in (depth, mask, q0):
            a.setflags(write=False)
        _cache[key] = (depth, mask, calib, q0)
    return _cache[key]


def variants():
    """(masked, voted, iters) of the case table."""
    return [(m, v, it) for m in (False, True) for v in (True, False) for it in (0, 6)]
