"""Cases shared by tests/test_flow_limits_oracle.py (CPU: the yardstick is meaningful) and tests/test_gpu_flow_limits.py (GPU: the
kernels meet it): the geometries that put a strip, padding or brick boundary next to a single live element, and the flow_init
that moves the in-network lookup off the integer grid.

Geometries (frame -> 1/8 map, N = pixels of the map), each the smallest with its property:
  152x216 -> 19x27, N = 513 = 4 * 128 + 1 = 16 * 32 + 1: ONE live row in the fifth 128-pixel strip, in the seventeenth 32-cell
        level-0 brick group and in the last group of ldN = 544; levels 9x13, 4x6, 2x3 (all odd somewhere, level 3 under one brick).
  248x264 -> 31x33, N = 1023 = 8 * 128 - 1: ONE dead row in the last strip; 33 columns = one live column in the third 16-column tile.
  128x1024 -> 16x128, N = 2048: every level a whole number of bricks (2048, 512, 128, 32 cells), N a whole number of strips: no
        padding cell and no tail anywhere.
  1024x128 -> 128x16: the same transposed.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import gma_ref

ODD, DEAD1, FULL, FULL_T = (152, 216), (248, 264), (128, 1024), (1024, 128)
# geometry -> (frames in its sequence = largest B + 1, pairs run through the oracle); the layout of test_gpu_flow_geometry.SEQ
SEQ = {ODD: (4, (0, 1, 2)), DEAD1: (2, (0,)), FULL: (3, (0, 1)), FULL_T: (2, (0,))}
# (geometry, B, precision, low_latency)
CASES = [(ODD, 1, "split_f16", False), (ODD, 3, "split_f16", False), (ODD, 1, "split_f16", True), (ODD, 1, "f32", False),
         (DEAD1, 1, "split_f16", False), (DEAD1, 1, "split_f16", True), (DEAD1, 1, "f32", False),
         (FULL, 1, "split_f16", False), (FULL, 2, "split_f16", False), (FULL_T, 1, "split_f16", False),
         # the two-pass encoder plumbing at split precision (flow_content_cases.TWO_PASS). The stem's 8 x 32-pixel tiles on the
         # half-resolution map: 76x108 = 4 of 8 rows and 12 of 32 columns live in the last tiles (the statistics pass's pixel
         # counts matter), 124x132 = 4 rows and 4 columns, 64x512 = whole tiles only
         (ODD, 1, "split_f16_two_pass", False), (ODD, 3, "split_f16_two_pass", False),
         (DEAD1, 1, "split_f16_two_pass", False), (FULL, 1, "split_f16_two_pass", False)]
INIT_CASES = [(hw, prec) for hw in (ODD, DEAD1) for prec in ("split_f16", "f32")]
REJECTED = [(64, 64), (120, 136), (136, 120)]
SEED_INIT = 7
INIT_KEYS = ("lookup0", "cor1", "mf0", "mfg0", "net1", "mask1", "flow_low", "flow_up")


def case_id(c):
    return "%dx%d-B%d-%s%s" % (c[0][0], c[0][1], c[1], c[2], "-ll" if c[3] else "")


def make_flow_init(hw):
    """-> (flow_init [1,2,H8,W8] fp32, {probe name: (y, x)}, [(y, x) of the pixels whose windows miss the map at every level]).
    Uniform +-6 px, then planted pixels (flow = (fx, fy); a level-l window is the 9 x 9 positions c / 2^l - 4 ... + 4, each
    with taps at floor and floor + 1). No planted component exceeds 64 px."""
    H8, W8 = hw[0] // 8, hw[1] // 8
    fi = np.random.RandomState(SEED_INIT).uniform(-6.0, 6.0, (1, 2, H8, W8)).astype(np.float32)
    my, mx = H8 // 2, W8 // 2
    probes = {
        "integer": ((my, mx), (3.0, -2.0)),                     # every bilinear weight 0 or 1
        "half": ((my, mx + 1), (2.5, -1.5)),                    # all four weights 0.25 at level 0, other fractions below
        "neg_frac_l3": ((1, 2), (-5.0, -4.25)),                 # coords (-3, -3.25): level 3 at (-0.375, -0.40625)
        "left": ((my, 0), (-3.25, 0.5)),                        # the window leaves through each side, partly inside
        "right": ((my, W8 - 1), (3.25, 0.5)),
        "top": ((0, mx), (0.5, -3.25)),
        "bottom": ((H8 - 1, mx), (0.5, 3.25)),
        "last_is_first": ((0, 1), (-5.0, -4.0)),                # coords (-4, -4): the window's last cell is the map's first
        "far_corner_last_pixel": ((H8 - 1, W8 - 1), (4.5, 4.5)),  # pixel N - 1: the window leaves through the far corner
        "outside_neg": ((2, 5), (-64.0, -64.0)),                # coords (-59, -62): c / 2^l + 5 < 0 at every level
        "outside_pos": ((3, 6), (64.0, 64.0)),                  # coords (70, 67): c / 2^l - 4 >= W_l, H_l at every level
    }
    for (y, x), (fx, fy) in probes.values():
        fi[0, 0, y, x], fi[0, 1, y, x] = fx, fy
    where = {k: v[0] for k, v in probes.items()}
    return torch.from_numpy(fi), where, [where["outside_neg"], where["outside_pos"]]


def windows_outside_everywhere(hw, fi, yx):
    """True when every tap of every level's window of pixel (y, x) lies outside the map (what make_flow_init promises)."""
    H8, W8 = hw[0] // 8, hw[1] // 8
    y, x = yx
    cx, cy = x + float(fi[0, 0, y, x]), y + float(fi[0, 1, y, x])
    for l in range(4):
        Wl, Hl = W8 >> l, H8 >> l
        px, py = cx / 2 ** l, cy / 2 ** l
        out_x = px + 4 < -1 or px - 4 >= Wl     # taps floor(p), floor(p) + 1 of all nine offsets
        out_y = py + 4 < -1 or py - 4 >= Hl
        if not (out_x or out_y):
            return False
    return True


def _pix(t):
    return t[0].reshape(t.shape[1], -1).t().contiguous()


@torch.no_grad()
def oracle_flow_init(sd, frames, fi, dtype):
    """One iteration from flow_init in `dtype`: the tensors of INIT_KEYS, activations pixel-major [N, C]."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    taps = {}
    low, up = gma_ref.gma_forward(sd, frames[0:1].to(dtype), frames[1:2].to(dtype), iters=1, flow_init=fi.to(dtype), taps=taps)
    p = "update_block.encoder.convc1."
    cor1 = F.relu(F.conv2d(taps["lookup0"], sd[p + "weight"], sd[p + "bias"]))
    return {"lookup0": _pix(taps["lookup0"]), "cor1": _pix(cor1), "mf0": _pix(taps["mf0"])[:, :126],
            "mfg0": _pix(taps["mfg0"])[:, :126], "net1": _pix(taps["net1"]), "mask1": _pix(gma_ref.up_mask(taps["net1"], sd)),
            "flow_low": low[0], "flow_up": up[0]}
