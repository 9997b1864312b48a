"""Frames and case tables shared by tests/test_flow_content_oracle.py (CPU: the cases are what they claim and the yardstick binds)
and tests/test_gpu_flow_content.py (GPU: the kernels meet it): image CONTENT the rest of the suite never feeds the flow network.
Every other parity test uses windows of one well-textured value-noise canvas (synthetic.make_frames); here a channel's variance
is small against its mean (constant, saturated and low-contrast frames: rstd of the InstanceNorm chain up to 1 / sqrt(eps) = 316,
near-uniform attention rows, correlation rows of near-identical entries), and the pairs of one launch are unlike each other
(a black pair beside a textured one: per-image statistics that leaked between the images of a launch would show).

Pure NumPy (RandomState), no torch RNG. A frame pair is [2, 3, H, W] float32 with integer values 0..255.

Geometries: 128x128 (one attention tile, 8x16x64 encoder tiles), 184x328 (ragged: partial 32-row statistics groups, 23x41
features), 376x1232 (several key ranges, 12x16 statistics tiles; `sky_road` and, inside the B = 16 launch, `black` only).
"""
import numpy as np

from atdn_vslam_amd import synthetic as syn

SMALL, RAGGED, KITTI = (128, 128), (184, 328), (376, 1232)
SEED_FRAMES = 4          # the seed of test_gpu_flow_geometry.py: `textured` is that module's pair 0
SEED_NOISE = 11


_SEQ = {}


def _textured(hw, n=2):
    """make_frames(n) of the geometry, a fresh copy (generated once: the canvas depends on n, so the 2-frame `textured` pair and
    the 17-frame sequence of the B = 16 launch are different images)."""
    if (hw, n) not in _SEQ:
        _SEQ[(hw, n)] = syn.make_frames(n, hw[0], hw[1], seed=SEED_FRAMES)
    return _SEQ[(hw, n)].copy()


def _const(hw, v):
    return np.full((2, 3, hw[0], hw[1]), float(v), dtype=np.float32)


def black(hw):
    return _const(hw, 0)


def white(hw):
    return _const(hw, 255)


def grey(hw):
    """Normalised input 2 * 128 / 255 - 1 = 0.0039: almost nothing but the biases is left."""
    return _const(hw, 128)


def lowcontrast(hw):
    r = np.random.RandomState(SEED_NOISE)
    return (128 + r.randint(-1, 2, (2, 3, hw[0], hw[1]))).astype(np.float32)


def faint(hw):
    """The textured pair compressed to 120 +- 4 grey levels."""
    return np.rint(120 + (_textured(hw) - 128) * 4 / 128).astype(np.float32)


def identical(hw):
    f = _textured(hw)
    return np.stack([f[0], f[0]])


def half_saturated(hw):
    f = _textured(hw)
    f[:, :, :, :hw[1] // 2] = 255
    return f


def top_black(hw):
    f = _textured(hw)
    f[:, :, :40, :] = 0
    return f


def checker(hw):
    """0 / 255 at pixel pitch; the second frame is the first moved by one pixel (its inverse)."""
    y, x = np.mgrid[0:hw[0], 0:hw[1]]
    c = (((y + x) & 1) * 255).astype(np.float32)
    return np.stack([np.broadcast_to(c, (3,) + hw), np.broadcast_to(255 - c, (3,) + hw)]).copy()


def impulse(hw):
    """Black with one 255 pixel that moves 3 px to the right between the two frames."""
    f = _const(hw, 0)
    y, x = hw[0] // 2 + 3, hw[1] // 2 - 5
    f[0, :, y, x] = 255
    f[1, :, y, x + 3] = 255
    return f


def sky_road(hw):
    """Top third 255 (over-exposed sky), middle third textured, bottom third the texture compressed to 90 +- 3 (road)."""
    f = _textured(hw)
    a, b = hw[0] // 3, 2 * hw[0] // 3
    f[:, :, b:, :] = np.rint(90 + (f[:, :, b:, :] - 128) * 3 / 128)
    f[:, :, :a, :] = 255
    return f


def textured(hw):
    return _textured(hw)


CONTENTS = {f.__name__: f for f in (black, white, grey, lowcontrast, faint, identical, half_saturated, top_black, checker, impulse,
                                    sky_road, textured)}
CONSTANTS = {"black": 0, "white": 255, "grey": 128}
# Largest rstd of fnet's first InstanceNorm in the fp64 oracle (test_flow_content_oracle.py): the factor by which a frame amplifies
# a rounding error of the stem's output and of its statistics. FLAT: above 30 (grey 315 = almost 1 / sqrt(eps), lowcontrast 114,
# faint 125; textured frames: 10). BORDER_ONLY: the stem's output is exactly constant wherever its window is whole, so ALL of a
# channel's variance comes from the zero-padding border: rstd 12 at 128x128, 16 at 184x328, 26 at 376x1232 (the border's share
# of the map shrinks).
FLAT = ("grey", "lowcontrast", "faint")
BORDER_ONLY = ("black", "white", "checker")
BORDER = 4               # features this close to the map's edge carry the zero padding of the encoder's convolutions: on black and
                         # white frames their logits stand 7 to 46 apart from the interior's (grey: max / min < 2 over ALL features)


def make_pair(content, hw):
    """-> [2, 3, H, W] float32, integer values 0..255."""
    f = CONTENTS[content](tuple(hw))
    assert f.shape == (2, 3, hw[0], hw[1]) and f.dtype == np.float32
    assert f.min() >= 0 and f.max() <= 255 and np.array_equal(f, np.rint(f))
    return f


# (precision, low_latency) of test_gpu_flow_geometry._net. TWO_PASS = the f16 mode's op sequence in split-f16 arithmetic: the stem as a
# statistics pass (stem_sf_kernel<1>) and a recompute + normalise pass (<2>), and in_apply_sf_kernel between the convolutions of every
# residual block instead of normalise-on-load — code that otherwise only precision="f16" runs, under tolerances that hide it.
TWO_PASS = ("split_f16_two_pass", False)
MODES = (("split_f16", False), ("f32", False), ("split_f16", True), TWO_PASS)
HARD = ("black", "grey", "lowcontrast", "sky_road")

# (geometry, content, precision, low_latency), all B = 1
CASES = ([(SMALL, c, "split_f16", False) for c in CONTENTS] +
         [(SMALL, c, p, ll) for c in HARD for p, ll in MODES[1:]] +
         [(RAGGED, c, "split_f16", False) for c in ("black", "white", "grey", "lowcontrast", "sky_road")] +
         [(RAGGED, "sky_road", "f32", False)] +
         [(RAGGED, c) + TWO_PASS for c in ("grey", "lowcontrast", "sky_road")] +
         [(KITTI, "sky_road", "split_f16", False)])


def case_id(c):
    return "%dx%d-%s-%s%s" % (c[0][0], c[0][1], c[1], c[2], "-ll" if c[3] else "")


# Mixed launches: (name, geometry, contents by position, oracled positions, modes, also run in reversed order).
# Each pair keeps its (image1, image2); "textured+i" is pair i of the 17-frame make_frames sequence (frames i -> i + 1).
_K16 = ["textured+%d" % i for i in range(16)]
_K16[0], _K16[7], _K16[15] = "sky_road", "black", "sky_road"
MIXED = [
    ("small-bright", SMALL, ("black", "textured", "white"), (0, 1, 2), MODES, True),
    ("small-flat", SMALL, ("grey", "sky_road", "lowcontrast"), (0, 1, 2), MODES, True),
    ("ragged", RAGGED, ("white", "sky_road", "black"), (0, 1, 2), MODES, False),
    # (the low-latency form is for one to four pairs per call: at B = 16 the default path and the exact-fp32 mode)
    # (nor the two-pass encoder plumbing: its per-image indexing is held at B = 3 above, ragged geometry included)
    ("kitti16", KITTI, tuple(_K16), (0, 7), MODES[:2], False),
]
MIXED_CASES = [(m, p, ll) for m in MIXED for p, ll in m[4]]


def mixed_id(c):
    return "%s-%s%s" % (c[0][0], c[1], "-ll" if c[2] else "")


def mixed_pair(name, hw):
    """One position of a mixed launch -> [2, 3, H, W]."""
    if name.startswith("textured+"):
        i = int(name[9:])
        return _textured(hw, 17)[i:i + 2].copy()
    return make_pair(name, hw)


def oracled():
    """Every (geometry, content) the fp64 oracle runs on, each once: the B = 1 cases and the oracled positions of the launches."""
    seen = []
    for hw, c, _, _ in CASES:
        if (hw, c) not in seen:
            seen.append((hw, c))
    for _, hw, contents, pos, _, _ in MIXED:
        for p in pos:
            if (hw, contents[p]) not in seen:
                seen.append((hw, contents[p]))
    return seen


def sequence_frames(hw):
    """[textured 0, black, textured 1, lowcontrast, textured 2] -> [5, 3, H, W]: a clip that passes through flat frames."""
    t = _textured(hw, 3)
    return np.stack([t[0], black(hw)[0], t[1], lowcontrast(hw)[0], t[2]])


# ---- the yardstick:  max|x_hip - x64| <= min(M * max|x32 - x64| + FLOOR * max|x64|, cap)
TOL_LOW, TOL_UP, TOL_ACT = 2e-4, 1e-3, 1e-4       # the stated tolerances of test_gpu_flow_geometry.py
CORR_SCALE = 25.0                                 # test_gpu_parity.py states 1e-4 absolute for "values of O(1)-O(25)"; synthetic.py
CORR_KEYS = ("pyr0", "pyr1", "pyr2", "pyr3", "lookup0")   # tunes |corr| to about 25. Flat content reaches 33-59.
REL_CAP = 1e-3                                    # parity_check.CAP

# (geometry, content, tensor) whose fp32 oracle is NOT within half of its absolute cap: compared under the same M-bound with
# REL_CAP * max|x64| in place of the absolute cap. Correlation-valued tensors of `grey` only (test_flow_content_oracle.py asserts
# exactly that); nothing else may ever be listed. Measured: 5.6e-5 of 1e-4 / 2 (128x128, both), 6.5e-5 of 1.33e-4 / 2 and 5.2e-5 to
# 5.8e-5 of 1.33e-4 / 2 (184x328 pyr0 / lookup0: at the line, on either side of it from host to host).
RELATIVE_CAP = [
    (SMALL, "grey", "pyr0"), (SMALL, "grey", "lookup0"),
    (RAGGED, "grey", "pyr0"), (RAGGED, "grey", "lookup0"),
]


def tensor_key(name):
    """'p1/pyr0' / 'flow_low@1' / 'low1' -> the tensor's name in the tables above."""
    k = name.split("/")[-1]
    return {"low1": "flow_low", "up1": "flow_up"}.get(k, k.split("@")[0])


def absolute_cap(key, scale, attn_max=None):
    """The stated tolerance of tensor `key` whose fp64 oracle has max |x64| = scale."""
    key = tensor_key(key)
    if key == "flow_low":
        return TOL_LOW
    if key == "flow_up" or key.startswith("pred"):
        return TOL_UP
    if key == "attn":
        return 1e-6 + 1e-4 * (scale if attn_max is None else attn_max)
    if key in CORR_KEYS:
        return TOL_ACT * max(1.0, scale / CORR_SCALE)
    return TOL_ACT


def cap(hw, content, key, scale):
    if (tuple(hw), content, tensor_key(key)) in RELATIVE_CAP:
        return REL_CAP * scale
    return absolute_cap(key, scale)
