"""fp64 reference of the frame front-end (atdn_vslam_amd/csrc/frontend.hip): bilinear resize with and without antialiasing,
align_corners=False, and replicate padding. numpy only — no torch op is used, so it shares no code and no rounding habit with
either the HIP kernels or ATen. tests/test_resize_ref_host.py pins it to F.interpolate / F.pad in fp64.

Resizing is separable: out = Wy @ x @ Wx^T per plane, with one dense fp64 weight matrix per axis.

CASES lists the geometries both test files use (tests/test_gpu_frontend_geometry.py says which kernel each one reaches)."""
import numpy as np

MAX_TAPS = 8   # RESIZE_TAPS of atdn_vslam_amd/csrc/frontend.h: the widest antialias row a weight table holds

# (name, frames, (Hin, Win), (Hout, Wout)); every frame has three planes
CASES = (
    ("rows_tail_1249", 2, (13, 321), (13, 257)),
    ("past_boundary", 2, (13, 322), (13, 257)),
    ("rows_125_span", 2, (9, 645), (9, 516)),
    ("rows_upscale", 2, (8, 40), (8, 50)),
    ("identity_capi", 2, (5, 300), (5, 300)),
    ("idy_333x", 2, (8, 100), (8, 30)),      # 6- and 7-tap rows
    ("idy_35x", 2, (8, 112), (8, 32)),       # 7 taps everywhere
    ("idy_375x", 2, (8, 120), (8, 32)),      # 7- and 8-tap rows
    ("idy_4x", 2, (8, 128), (8, 32)),        # 8 taps everywhere but the borders: the largest ratio every width supports
    ("both_down", 2, (21, 37), (13, 29)),
    ("both_up", 2, (7, 9), (19, 23)),
    ("mixed", 2, (30, 20), (9, 40)),
    ("one_pixel", 2, (1, 1), (8, 8)),
    ("two_slices", 911, (16, 12), (24, 10)),
    ("planes_65538", 21846, (4, 10), (4, 9)),
)
CASE = {c[0]: c for c in CASES}


def aa_window(n_in, n_out):
    """Antialias tap windows [lo, hi) per output index, the support and the centres (all fp64)."""
    s = n_in / n_out
    sup = max(s, 1.0)
    c = s * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum((c - sup + 0.5).astype(np.int64), 0)     # int(): truncation; negative values clamp to 0 either way
    hi = np.minimum((c + sup + 0.5).astype(np.int64), n_in)
    return lo, hi, sup, c


def aa_max_taps(n_in, n_out):
    """Widest antialias window of the axis: the quantity the library's ratio guard bounds by MAX_TAPS."""
    if n_in == n_out:
        return 1
    lo, hi, _, _ = aa_window(n_in, n_out)
    return int((hi - lo).max())


def weights(n_in, n_out, antialias):
    """[n_out, n_in] fp64 interpolation matrix of one axis."""
    w = np.zeros((n_out, n_in), dtype=np.float64)
    if n_in == n_out:
        w[np.arange(n_out), np.arange(n_out)] = 1.0
        return w
    if antialias:
        lo, hi, sup, c = aa_window(n_in, n_out)
        for i in range(n_out):
            j = np.arange(lo[i], hi[i], dtype=np.float64)
            t = np.maximum(0.0, 1.0 - np.abs((j - c[i] + 0.5) / sup))
            w[i, lo[i]:hi[i]] = t / t.sum()
        return w
    s = n_in / n_out
    src = np.maximum(s * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    x0 = np.minimum(src.astype(np.int64), n_in - 1)
    x1 = np.minimum(x0 + 1, n_in - 1)
    lam = src - x0
    np.add.at(w, (np.arange(n_out), x0), 1.0 - lam)
    np.add.at(w, (np.arange(n_out), x1), lam)
    return w


def resize(x, size, antialias):
    """x [..., Hin, Win] (any real dtype) -> [..., Hout, Wout] float64."""
    x = np.asarray(x, dtype=np.float64)
    wy = weights(x.shape[-2], size[0], antialias)
    wx = weights(x.shape[-1], size[1], antialias)
    return np.matmul(wy, np.matmul(x, wx.T))


def replicate_pad(x, l, r, t, b):
    """F.pad(x, [l, r, t, b], mode="replicate") on the last two axes by index clamping; keeps the dtype."""
    x = np.asarray(x)
    h, w = x.shape[-2:]
    ys = np.clip(np.arange(-t, h + b), 0, h - 1)
    xs = np.clip(np.arange(-l, w + r), 0, w - 1)
    return np.ascontiguousarray(x[..., ys[:, None], xs[None, :]])


def noise_u8(case, seed=0):
    """The uint8 noise frames [frames, 3, Hin, Win] of a case: full local contrast, the worst input for weight rounding."""
    name, n, (h, w), _ = CASE[case]
    k = [c[0] for c in CASES].index(name)
    return np.random.RandomState(1000 + 17 * k + seed).randint(0, 256, size=(n, 3, h, w)).astype(np.uint8)
