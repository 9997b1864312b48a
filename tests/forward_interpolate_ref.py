"""Brute-force float64 restatement of forward interpolation (helper of the warm-start tests, not a test): the oracle where
neither scipy nor the flow package is at hand.

Source i = y * w + x of a flow [2, h, w] sits at (x + dx_i, y + dy_i) in float64 and is valid when 0 < x1 < w and 0 < y1 < h
(strict). Every grid point takes (dx_j, dy_j) of the valid source with the smallest (qx - x1)^2 + (qy - y1)^2; np.argmin
returns the first minimum, so equal distances go to the lowest source index. No valid source: zeros."""
import numpy as np


def cases():
    """(name, h, w, flow) of the stored cases of tests/golden/warm_start.npz, regenerated from their seeds."""
    out = []
    for k, (h, w, sigma) in enumerate([(5, 7, 1.5), (9, 33, 3.0), (20, 64, 3.0), (20, 64, 30.0), (47, 154, 3.0)]):
        r = np.random.RandomState(100 + k)
        out.append(("randn_%dx%d_s%g" % (h, w, sigma), h, w, (r.randn(2, h, w) * sigma).astype(np.float32)))
    h, w = 47, 154
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    zoom = np.stack([0.08 * (x - w / 2) + 0.013, 0.05 * (y - h / 2) + 0.007]).astype(np.float32)
    out.append(("zoom_47x154", h, w, zoom))
    return out


def forward_interpolate_ref(flow, block=256):
    """flow [2, h, w] float32 -> (out [2, h, w] float32, gap [h, w] float64, valid count). `gap` is the second-smallest minus
    the smallest squared distance of every grid point (inf with fewer than two valid sources)."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[0] == 2
    _, h, w = flow.shape
    n = h * w
    y0, x0 = np.divmod(np.arange(n), w)
    dx, dy = flow[0].reshape(-1), flow[1].reshape(-1)
    x1 = x0 + dx                     # int64 + float32 -> float64
    y1 = y0 + dy
    assert x1.dtype == np.float64
    valid = np.nonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))[0]   # ascending source indices
    out = np.zeros((2, n), dtype=np.float32)
    gap = np.full(n, np.inf)
    if valid.size:
        sx, sy = x1[valid], y1[valid]
        qx, qy = x0.astype(np.float64), y0.astype(np.float64)
        for s in range(0, n, block):
            d = (qx[s:s + block, None] - sx[None, :]) ** 2 + (qy[s:s + block, None] - sy[None, :]) ** 2
            j = np.argmin(d, axis=1)     # first minimum = lowest source index
            out[0, s:s + block] = dx[valid[j]]
            out[1, s:s + block] = dy[valid[j]]
            if valid.size > 1:
                two = np.partition(d, 1, axis=1)[:, :2]
                gap[s:s + block] = two[:, 1] - two[:, 0]
    return out.reshape(2, h, w), gap.reshape(h, w), int(valid.size)
