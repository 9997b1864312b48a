"""NumPy float64 restatement of the forward-backward consistency rule (include/atdn_hip.h, atdn_flow_consistency): helper of
the flow-consistency tests, not a test, and not a call into the library.

For pixel (x, y) of flows [2, H, W] (channel 0 = x), every array operation below is one IEEE float64 operation per element
(NumPy never fuses a multiply with an add), in the order the rule states:
  x1 = x + fw_x, y1 = y + fw_y;  inside = 0 <= x1 <= W-1 and 0 <= y1 <= H-1 (closed, NaN fails);  not inside: 0
  x0 = floor(x1), ax = x1 - x0 (same for y);  four taps of flow_bw at x0 / min(x0+1, W-1), y0 / min(y0+1, H-1)
  top = t00*(1-ax) + t10*ax, bot = t01*(1-ax) + t11*ax, b = top*(1-ay) + bot*ay        (per channel)
  diff = (fw_x + b_x)^2 + (fw_y + b_y)^2;  mag = (fw_x^2 + fw_y^2) + (b_x^2 + b_y^2);  thr = alpha1*mag + alpha2
  mask = inside and diff <= thr and diff is not +inf
`margin` = |diff - thr| over the inside pixels (inf elsewhere): how far a pixel is from changing sides. With a smallest margin
of 1e-9 — four orders of magnitude above float64 rounding at these magnitudes (flows of a few pixels: diff, thr ~ 1..100,
ulp ~ 1e-14; ~20 roundings) — every correct float64 evaluation agrees on every pixel, so the tests compare exactly."""
import numpy as np

MIN_MARGIN = 1e-9


def flow_consistency_ref(flow_fw, flow_bw, alpha1=0.01, alpha2=0.5):
    """flow_fw, flow_bw [2, H, W] float32 -> (mask [H, W] uint8, count int, margin [H, W] float64)."""
    fw, bw = np.asarray(flow_fw), np.asarray(flow_bw)
    assert fw.dtype == np.float32 and bw.dtype == np.float32 and fw.shape == bw.shape and fw.ndim == 3 and fw.shape[0] == 2
    _, H, W = fw.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fx, fy = fw[0].astype(np.float64), fw[1].astype(np.float64)
    with np.errstate(all="ignore"):
        x1, y1 = xs + fx, ys + fy
        inside = (x1 >= 0) & (x1 <= W - 1) & (y1 >= 0) & (y1 <= H - 1)
        xs1 = np.where(inside, x1, 0.0)                  # (outside pixels: any in-range tap, the result is discarded)
        ys1 = np.where(inside, y1, 0.0)
        xf, yf = np.floor(xs1), np.floor(ys1)
        ax, ay = xs1 - xf, ys1 - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        xn, yn = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        wx, wy = 1.0 - ax, 1.0 - ay
        b = []
        for c in range(2):
            p = bw[c].astype(np.float64)
            top = p[y0, x0] * wx + p[y0, xn] * ax
            bot = p[yn, x0] * wx + p[yn, xn] * ax
            b.append(top * wy + bot * ay)
        sx, sy = fx + b[0], fy + b[1]
        diff = sx * sx + sy * sy
        mag = (fx * fx + fy * fy) + (b[0] * b[0] + b[1] * b[1])
        thr = alpha1 * mag + alpha2
        mask = inside & (diff <= thr) & (diff != np.inf)
        margin = np.where(inside, np.abs(diff - thr), np.inf)
    return mask.astype(np.uint8), int(mask.sum()), margin


def smooth_pair(H, W, seed, B=1, amplitude=2.0, noise=0.45):
    """(fw, bw) [B, 2, H, W] float32: fw a sum of three low-frequency sinusoids per channel (amplitude ~`amplitude` px),
    bw = -fw + noise * randn — neither all consistent nor all inconsistent."""
    r = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.zeros((B, 2, H, W))
    for b in range(B):
        for c in range(2):
            for _ in range(3):
                kx, ky = r.uniform(0.5, 3.0, 2) * 2 * np.pi / np.array([W, H], dtype=np.float64)
                fw[b, c] += amplitude / 1.5 * r.uniform(0.3, 1.0) * np.sin(kx * x + ky * y + r.uniform(0, 2 * np.pi))
    fw = fw.astype(np.float32)
    bw = (-fw.astype(np.float64) + noise * r.randn(B, 2, H, W)).astype(np.float32)
    return fw, bw


def reference_batch(fw, bw, alpha1=0.01, alpha2=0.5):
    """The helper over a batch: (mask [B,1,H,W] uint8, count [B] int32, smallest margin, share of inside pixels)."""
    out = [flow_consistency_ref(fw[b], bw[b], alpha1, alpha2) for b in range(fw.shape[0])]
    mask = np.stack([m for m, _, _ in out])[:, None]
    count = np.array([c for _, c, _ in out], dtype=np.int32)
    margin = np.stack([g for _, _, g in out])
    return mask, count, float(margin.min()), float(np.isfinite(margin).mean())


# (name, H, W, B, seed, amplitude) of the random cases shared by the host and the GPU test
RANDOM_CASES = [("5x7", 5, 7, 1, 2, 1.0), ("9x33_b3", 9, 33, 3, 0, 2.0), ("47x154", 47, 154, 1, 0, 2.0)]
