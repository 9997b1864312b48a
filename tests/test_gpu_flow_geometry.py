"""GMA flow network, stage by stage, against the fp64 oracle across batch sizes, arithmetic modes and geometries.

Yardstick (per tensor, as in tests/test_gpu_train_geometry.py): the fp32 CPU oracle's own error on that tensor,

    max|x_hip - x64| <= min(M * max|x32 - x64| + FLOOR * max|x64|,  TOL)

with TOL the tolerance the suite has always stated: flow_low 2e-4 px, flow_up 1e-3 px, activations 1e-4 absolute, attention
1e-6 + 1e-4 * max. x64 and x32 come from oracle/gma_ref.py run on the same frames with fp64 and fp32 weights.

Calibrated once on the MI355X (17 cases, 678 comparisons, FLOOR 1e-6): the worst (max|x_hip - x64| - FLOOR * max|x64|) /
max|x32 - x64| was 2.36, the hidden state after one iteration in the exact-fp32 mode (376x1232, B = 16, pair 1); split-f16 at
most 1.60 (attention rows, 128x128, B = 3), low-latency 1.33 (net1, 376x1232, B = 4). M = 9 (3.8x). Closest to a cap: lookup0 at
376x1232, B = 16, 5.5e-5 of TOL 1e-4 (the fp32 oracle's own error there is 5.4e-5). The final flow at KITTI size: flow_low
6.5e-5 px for all three of split-f16, exact-fp32 mode and the fp32 oracle (coordinates up to 153 px held in fp32: the same
roundings in all three), flow_up 1.9e-4 / 1.8e-4 / 1.8e-4 px. Running `pytest -s` prints every comparison ("PARITY" lines).

Cases. One 17-frame sequence per geometry (pair i = frames i -> i + 1 at every batch size); the oracle runs once per listed
pair (12 iterations; the iteration-1 taps come from the same run). After one iteration: fmap1 / fmap2, the four pyramid levels
(the first four pairs of a launch), inp, attention rows (where the tap fits: B <= 2 at KITTI size), the 324 lookup samples,
cor1 = relu(convc1(lookup)), the 126 convolved channels of motion_features and of the aggregate, net, the upsampling mask,
flow_low and flow_up; then flow_low / flow_up after 12 iterations. Pyramid and attention rows: the first and last, both sides of
every 128-pixel strip boundary and 32 seeded rows (all rows where N <= 1024). Every case ends with debug_read("sf_clamped") == 0.

Two-pass encoder plumbing (precision "split_f16_two_pass": the f16 mode's op sequence in split-f16 arithmetic — stem_sf_kernel<1>
statistics pass, stem_sf_kernel<2> recompute + normalise, in_apply_sf_kernel without residual / with an sf residual / with the raw
down-sample shortcut normalised on the fly — which otherwise only precision="f16" runs, under 0.03 / 0.15 px). 128x128 B = 1 (whole
8 x 32 stem tiles), 184x328 B = 1 / 3 (92x164 stem map: 4 of 8 rows and 4 of 32 columns in the last tiles; at B = 3 six images x
92 x 164 x 16 float4 = 1,448,448 against in_apply_sf's 4096 x 256 threads: the grid-stride loop runs a second, ragged, time),
376x1232 B = 2. Measured on the MI355X: worst need_m 2.12 (mf0, 128x128), 1.44 (mfg0, 184x328, both B), 1.26 (net1, 376x1232 pair 1);
the four cases add 126 comparisons.

Kernels each case reaches (rocprofv3 --kernel-trace, one iteration; conv_sf6_kernel<TH, 16, BN, ...> = TH x 16-pixel tiles x BN
channels, GEMM tiles from choose_tile):
  376x1232 (47x154, N = 7238)   split-f16 B = 1: the 3x3 convolutions at 1/8 resolution (motion encoder, cnet layer3) and every
        ConvGRU 1x5 / 5x1 on 4x16x64 tiles (47 rows: a 3-row last tile row); encoder statistics convolutions on 12x16x64 /
        12x16x96; flow head on 8x16x128; GEMMs 64x64, 128x64, 128x96; attention x V in one key range.
    B = 2: GRU z|r on 8x16x64, q still 4x16x64; GEMMs add 128x128.   B = 4: GRU z|r on 8x16x128, q on 8x16x64; no 64x64 GEMM.
    B = 16: GRU z|r and q on 8x16x128, a 3x3 on 8x16x256, convc2 + convf2 as ONE conv_sf6_pair_kernel<12, 16, 64>, no 4x16 tile
        anywhere, GEMMs 128x128 / 128x64 / 128x96 — no kernel of the motion encoder or the GRU is shared with B = 1.
    low-latency B = 1 / 2 / 4: the same convolutions as the default path at that B; attn_v3_kernel split into 8 / 4 / 2 key
        ranges (232 blocks each) + attn_reduce_kernel.
    f32 (exact-fp32 mode) B = 1 / 16: conv_mfma_kernel tiles 64x64 ... 128x128, logits GEMM + softmax_rows_kernel, row-major
        pyramid + lookup_kernel.
  184x328 (23x41, N = 943; 11x20, 5x10, 2x5 below)   B = 1 / 3 split-f16 and low-latency (4 key ranges), f32 B = 1; 4x16x64 motion
        encoder / GRU tiles at both batch sizes, GEMMs 64x64 / 128x96.
  1232x376 (154x47)   split-f16 B = 1: the 376-wide half-resolution map (188 px) leaves a 12-px last tile column in every
        encoder convolution; same kernels as 376x1232 B = 1.
  128x128 (16x16; 8x8, 4x4, 2x2 below)   split-f16 B = 1 / 3, f32 B = 1: 8x16x64 encoder tiles, a single attention tile.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import RAFTGMA
from oracle import gma_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

M, FLOOR = 9.0, 1e-6                         # worst observed need 2.36 (see above)
TOL_LOW, TOL_UP, TOL_ACT = 2e-4, 1e-3, 1e-4
ITERS = 12
KITTI, RAGGED, TALL, SMALL = (376, 1232), (184, 328), (1232, 376), (128, 128)
# geometry -> (frames in its sequence, pairs run through the oracle)
SEQ = {KITTI: (17, (0, 1, 2, 3, 7, 15)), RAGGED: (4, (0, 1, 2)), TALL: (2, (0,)), SMALL: (4, (0, 1, 2))}
SEED_FRAMES = 4
ATTN_MAX_FLOATS = 2 * 7238 * 7264          # the attention tap is read where it fits: B <= 2 at KITTI size
PYR_MAX_PAIRS = 4                           # pyramid levels of the first four pairs of a launch (pyr0 at B = 16 is 3.4 GB)


def _sd():
    return syn.to_torch(syn.make_gma_state(seed=1))


def _rows(N):
    """Pyramid / attention rows compared: all of them for small N, else the ends, both sides of every 128-pixel strip boundary
    (the brick layout's strips) and 32 seeded rows."""
    if N <= 1024:
        return torch.arange(N)
    r = {0, N - 1}
    for s in range(128, N, 128):
        r.update((s - 1, s))
    r.update(np.random.RandomState(N).choice(N, 32, replace=False).tolist())
    return torch.tensor(sorted(r))


def _pix(t):
    """[1, C, H8, W8] -> [N, C] (the library's pixel-major layout)."""
    return t[0].reshape(t.shape[1], -1).t().contiguous()


@torch.no_grad()
def _oracle_pair(sd, frames, i, dtype, rows, keep_preds):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    a, b = frames[i:i + 1].to(dtype), frames[i + 1:i + 2].to(dtype)
    taps, preds = {}, ([] if keep_preds else None)
    low, up = gma_ref.gma_forward(sd, a, b, iters=ITERS, taps=taps, predictions=preds)
    N = taps["inp"].shape[2] * taps["inp"].shape[3]
    mask1 = gma_ref.up_mask(taps["net1"], sd)
    # flow after one iteration as the forward forms it, (coords0 + delta) - coords0 in `dtype`: at KITTI size the rounding of
    # coordinates up to 153 px is 8e-6 px in fp32, ten times the fp32 error of delta itself
    c0 = gma_ref.coords_grid(1, taps["inp"].shape[2], taps["inp"].shape[3], dtype)
    low1 = (c0 + taps["delta0"]) - c0
    p = "update_block.encoder.convc1."
    cor1 = F.relu(F.conv2d(taps["lookup0"], sd[p + "weight"], sd[p + "bias"]))
    o = {"fmap1": _pix(taps["fmap1"]), "fmap2": _pix(taps["fmap2"]), "inp": _pix(taps["inp"]),
         "lookup0": _pix(taps["lookup0"]), "cor1": _pix(cor1), "mf0": _pix(taps["mf0"])[:, :126],
         "mfg0": _pix(taps["mfg0"])[:, :126], "net1": _pix(taps["net1"]), "mask1": _pix(mask1),
         "low1": low1[0], "up1": gma_ref.convex_upsample(low1, mask1)[0],
         "flow_low": low[0], "flow_up": up[0], "attn": taps["attn"][0][rows].clone()}
    for lvl, pyr in enumerate(taps["pyramid"]):
        o["pyr%d" % lvl] = pyr.reshape(N, -1)[rows].clone()
    if keep_preds:
        o["preds"] = torch.stack([q[0] for q in preds])
    return o


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return _sd()


@pytest.fixture(scope="module")
def oracle(sd):
    """(H, W) -> (frames, rows, {pair: (fp32 oracle, fp64 oracle)}), each pair computed once per module."""
    cache = {}

    def get(hw, pairs):
        if hw not in cache:
            n = SEQ[hw][0]
            cache[hw] = (torch.from_numpy(syn.make_frames(n, hw[0], hw[1], seed=SEED_FRAMES)), _rows((hw[0] // 8) * (hw[1] // 8)), {})
        frames, rows, res = cache[hw]
        for i in pairs:
            if i not in res:
                keep = i == 0 and hw == KITTI
                res[i] = tuple(_oracle_pair(sd, frames, i, dt, rows, keep) for dt in (torch.float32, torch.float64))
        return frames, rows, res
    return get


class Checker:
    """Collects every comparison (the calibration table) and every violation (reported together at the end)."""

    def __init__(self, case):
        self.case, self.rows, self.bad = case, [], []

    def __call__(self, name, hip, x32, x64, tol):
        hip, x32, x64 = hip.detach().cpu().double().flatten(), x32.double().flatten(), x64.double().flatten()
        assert hip.shape == x64.shape, (name, hip.shape, x64.shape)
        assert bool(torch.isfinite(hip).all()), name
        scale = float(x64.abs().max())
        e_hip, e32 = float((hip - x64).abs().max()), float((x32 - x64).abs().max())
        bound = min(M * e32 + FLOOR * scale, tol)
        need = max(0.0, e_hip - FLOOR * scale) / e32 if e32 > 0 else (0.0 if e_hip <= FLOOR * scale else float("inf"))
        self.rows.append((name, e_hip, e32, need, scale))
        if not e_hip <= bound:
            self.bad.append("%s: max|hip-64| %.3e > bound %.3e (max|64| %.3e, max|32-64| %.3e, TOL %.1e)" % (name, e_hip, bound, scale, e32, tol))

    def finish(self):
        for name, e_hip, e32, need, scale in self.rows:
            print("PARITY %s %s err_hip=%.3e err_32=%.3e max64=%.3e need_m=%.3g" % (self.case, name, e_hip, e32, scale, need))
        worst = max(self.rows, key=lambda r: r[3])
        print("PARITY-WORST %s %s need_m=%.3g" % (self.case, worst[0], worst[3]))
        assert not self.bad, "%s:\n  " % self.case + "\n  ".join(self.bad)


def _net(sd, B, precision, low_latency):
    m = RAFTGMA(max_batch=B, precision=precision, low_latency=low_latency)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _check_taps(chk, net, hw, B, pairs, rows, res, cap=None):
    """`cap(p, key, x64, tol)`, if given, returns the cap of pair p's tensor `key` in place of the stated tolerance `tol`."""
    H, W = hw
    N = (H // 8) * (W // 8)
    ldN = (N + 31) // 32 * 32
    fmap = net.debug_read("fmap", (2, B, N, 256), H, W)
    x = net.debug_read("x", (B, N, 384), H, W)
    reads = {k: net.debug_read(k, (B, N, c), H, W) for k, c in (("corrfeat", 352), ("cor1", 256), ("net", 128), ("mask", 576))}
    npyr = min(B, PYR_MAX_PAIRS)
    pyr = [net.debug_read("pyr%d" % l, (npyr, N, ((H // 8) >> l) * ((W // 8) >> l)), H, W) for l in range(4)]
    attn = net.debug_read("attn", (B, N, ldN), H, W) if B * N * ldN <= ATTN_MAX_FLOATS else None
    for p in pairs:
        o32, o64 = res[p]
        t = lambda k, tol=TOL_ACT: (o32[k], o64[k], tol if cap is None else cap(p, k, o64[k], tol))   # noqa: E731
        chk("p%d/fmap1" % p, fmap[0, p], *t("fmap1"))
        chk("p%d/fmap2" % p, fmap[1, p], *t("fmap2"))
        if p < npyr:
            for l in range(4):
                chk("p%d/pyr%d" % (p, l), pyr[l][p][rows], *t("pyr%d" % l))
        chk("p%d/inp" % p, x[p, :, 0:128], *t("inp"))
        if attn is not None:
            a64 = o64["attn"]
            chk("p%d/attn" % p, attn[p][rows, :N], *t("attn", 1e-6 + 1e-4 * float(a64.max())))
            assert float((attn[p][:, :N].double().sum(1) - 1).abs().max()) < 1e-5
        chk("p%d/lookup0" % p, reads["corrfeat"][p, :, :324], *t("lookup0"))
        chk("p%d/cor1" % p, reads["cor1"][p], *t("cor1"))
        chk("p%d/mf0" % p, x[p, :, 128:254], *t("mf0"))
        chk("p%d/mfg0" % p, x[p, :, 256:382], *t("mfg0"))
        chk("p%d/net1" % p, reads["net"][p], *t("net1"))
        chk("p%d/mask1" % p, reads["mask"][p], *t("mask1"))


def _sf_clamped(net, hw):
    return float(net.debug_read("sf_clamped", (1,), hw[0], hw[1])[0])


def _run_case(sd, oracle, hw, B, precision="split_f16", low_latency=False):
    _, oracled = SEQ[hw]
    preds = hw == KITTI and B == 1 and precision == "split_f16" and not low_latency
    pairs = tuple(p for p in oracled if p < B)
    frames, rows, res = oracle(hw, pairs)
    tag = "%dx%d/B%d/%s%s" % (hw[0], hw[1], B, precision, "/ll" if low_latency else "")
    net = _net(sd, B, precision, low_latency)
    f1, f2 = frames[0:B].to(DEV), frames[1:B + 1].to(DEV)
    chk = Checker(tag)
    low1, up1 = net(f1, f2, iters=1, test_mode=True)
    torch.cuda.synchronize()
    _check_taps(chk, net, hw, B, pairs, rows, res)
    for p in pairs:
        chk("p%d/flow_low@1" % p, low1[p], res[p][0]["low1"], res[p][1]["low1"], TOL_LOW)
        chk("p%d/flow_up@1" % p, up1[p], res[p][0]["up1"], res[p][1]["up1"], TOL_UP)
    low, up = net(f1, f2, iters=ITERS, test_mode=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(low).all()) and bool(torch.isfinite(up).all()), tag
    for p in pairs:
        chk("p%d/flow_low" % p, low[p], res[p][0]["flow_low"], res[p][1]["flow_low"], TOL_LOW)
        chk("p%d/flow_up" % p, up[p], res[p][0]["flow_up"], res[p][1]["flow_up"], TOL_UP)
    if preds:
        pr = net(f1, f2, iters=ITERS)
        assert len(pr) == ITERS
        for it in range(ITERS):
            chk("p0/pred%d" % it, pr[it][0], res[0][0]["preds"][it], res[0][1]["preds"][it], TOL_UP)
        assert torch.equal(pr[-1], up)
    assert _sf_clamped(net, hw) == 0.0, tag
    del net
    torch.cuda.empty_cache()
    chk.finish()


TWO_PASS = "split_f16_two_pass"
CASES = ([(KITTI, B, "split_f16", False) for B in (1, 2, 4, 16)] + [(KITTI, B, "split_f16", True) for B in (1, 2, 4)] +
         [(KITTI, B, "f32", False) for B in (1, 16)] +
         [(RAGGED, 1, "split_f16", False), (RAGGED, 3, "split_f16", False), (RAGGED, 1, "split_f16", True), (RAGGED, 1, "f32", False)] +
         [(TALL, 1, "split_f16", False)] +
         [(SMALL, 1, "split_f16", False), (SMALL, 3, "split_f16", False), (SMALL, 1, "f32", False)] +
         # the f16 mode's encoder plumbing (two-pass stem, separate in_apply_sf passes) in split-f16 arithmetic: whole 8 x 32 stem
         # tiles (128x128); a ragged stem map, and at B = 3 six images of 92x164x64 = more float4 than in_apply_sf's grid covers in
         # one stride (184x328); many stem groups per image (376x1232, pairs 0 and 1)
         [(SMALL, 1, TWO_PASS, False), (RAGGED, 1, TWO_PASS, False), (RAGGED, 3, TWO_PASS, False), (KITTI, 2, TWO_PASS, False)])


def _case_id(c):
    return "%dx%d-B%d-%s%s" % (c[0][0], c[0][1], c[1], c[2], "-ll" if c[3] else "")


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_flow_stages_match_the_fp64_oracle(sd, oracle, case):
    """Every stage tap after one iteration and the flow after twelve, for the oracled pairs of the launch; at 376x1232, B = 1
    (split-f16) also RAFTGMA.forward(test_mode=False): the upsampled flow of every one of the 12 iterations."""
    hw, B, precision, ll = case
    _run_case(sd, oracle, hw, B, precision, ll)
