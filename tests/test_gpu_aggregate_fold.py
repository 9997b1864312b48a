"""The aggregator folded into the ConvGRU weights: attention x V multiplies the attention matrix with the motion features as they
are stored (agg = A . mf, transposed LDS reads), and to_v, gamma and the residual of gma.py:111-115 live in the gate weights.

What can go wrong is a key order inside a 32-key chunk (the transposed reads), the tail chunk's clamp, the second pair's rows,
and the weight algebra. With the synthetic state's attention (row maximum ~0.02 against 0.004 uniform) a wrong key order would
hardly show, so `att.to_qk.weight` is multiplied by 4: median row maximum 0.84 / 0.81 (pairs 0 / 1) at 128x128 and 0.70 / 0.79
at 136x152 with the frames used here (asserted > 0.5), and the oracle's own aggregate with the keys of every 32-key chunk
reversed is asserted to differ from the true one by more than 100 x the tolerance the tap is held to (it differs by 0.32-0.40;
the tap's bound is 1.5e-5 to 3e-5).

Geometries: 128x128 (N = 256: exactly 8 chunks, one 8-strip tile) and 136x152 (N = 323: a tail chunk with 3 live keys, a second
tile with three live strips, a partial strip); B = 1 and 2 (the second pair's rows behind the first, the clamp at the last pair).

Yardstick for split-f16: the Checker of tests/test_gpu_flow_geometry.py with its constants (M = 9, FLOOR = 1e-6, activations
1e-4, flow_low 2e-4 px, flow_up 1e-3 px) against the fp32 and fp64 oracle on the same frames. The f16 mode (hi x hi products only)
has a stated tolerance for the flow only (tests/test_gpu_parity.py: flow_low 0.03 px, flow_up 0.15 px) and none for its taps:
against the oracle its error is dominated by what lies upstream of the aggregate (f16 logits 16 x as large as usual under the
softmax), which says nothing about the kernels changed here. So in that mode the two kernels are checked against their OWN
operands, read back from the same run (`attn` rows, x[:, 128:256]) and multiplied on the CPU in fp64:
  agg:  |agg - attn @ mf| <= (2^-10 + (N + 8) * 2^-24) * max|mf|. The product uses the f16 hi part of either operand (relative
        error 2^-11 each, so (2^-10 + 2^-22) a|v| per term, summed over a row of attention that sums to 1); the fp32
        accumulation of N terms, the row normalisation, the tap's own decode and the sf store of the result are a few fp32
        roundings each.
  x[:, 256:382] (motion_global rebuilt from the stored aggregate, fp32): against mf + gamma * agg @ Wv^T elementwise within
        130 * 2^-24 * (|mf| + gamma * |agg| @ |Wv|^T): a 128-term fp32 dot product, one product and one sum.
Measured on the MI355X (11 tests, 6 s): split-f16 worst need_m (M = 9) 1.92 (agg, 128x128, B = 2, pair 1), otherwise 0.85-1.14; f16
agg against its own operands 1.8e-4 to 2.4e-4 of a bound of 7.9e-4 to 1.1e-3, the rebuilt motion_global 2e-7 (3e-6 inside its
bound), flow_up after two iterations 4.5e-3 to 5.7e-3 px of 0.15. (At these sizes attn_v_splits gives one key range — a range
has at least 8 chunks — so the low-latency handle differs from the default one by its parallel graph branches; the split form and
attn_reduce_kernel are reached by the low-latency cases of tests/test_gpu_flow_limits.py and test_gpu_flow_geometry.py.)
(A first version of this file held the f16 taps to 2^-9 of their largest magnitude against the oracle; that figure forgot the
softmax: a logit error d changes a probability by e^d. Measured then: agg 2.17e-3 on 1.03, net1 2.04e-3 on 0.95.)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_flow_geometry as fg  # noqa: E402
from atdn_vslam_amd import synthetic as syn  # noqa: E402
from oracle import gma_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = fg.DEV
GEOMS = ((128, 128), (136, 152))
SEED_FRAMES = 7
F16_LOW, F16_UP = 0.03, 0.15


def _state(gamma=None):
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    sd["att.to_qk.weight"] = sd["att.to_qk.weight"] * 4
    if gamma is not None:
        sd["update_block.aggregator.gamma"] = torch.full_like(sd["update_block.aggregator.gamma"], gamma)
    return sd


@torch.no_grad()
def oracle_pair(sd, frames, i, dtype):
    """Two iterations of the oracle on pair i in `dtype`; activations pixel-major [N, C]."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    taps = {}
    low, up = gma_ref.gma_forward(sd, frames[i:i + 1].to(dtype), frames[i + 1:i + 2].to(dtype), iters=2, taps=taps)
    h8, w8 = taps["inp"].shape[2], taps["inp"].shape[3]
    c0 = gma_ref.coords_grid(1, h8, w8, dtype)
    low1 = (c0 + taps["delta0"]) - c0
    attn, mf = taps["attn"][0], fg._pix(taps["mf0"])
    return {"attn": attn, "mf": mf, "agg": attn @ mf, "mf0": mf[:, :126], "mfg0": fg._pix(taps["mfg0"])[:, :126],
            "net1": fg._pix(taps["net1"]), "net2": fg._pix(taps["net_final"]), "low1": low1[0],
            "up1": gma_ref.convex_upsample(low1, gma_ref.up_mask(taps["net1"], sd))[0], "low2": low[0], "up2": up[0]}


def chunk_reversed_aggregate(attn, mf):
    """attn @ mf with the keys of every 32-key chunk taken in reverse order (what a wrong operand order would compute)."""
    N = attn.shape[0]
    ldN = (N + 31) // 32 * 32
    a = torch.zeros(N, ldN, dtype=attn.dtype)
    a[:, :N] = attn
    v = torch.zeros(ldN, mf.shape[1], dtype=mf.dtype)
    v[:N] = mf
    a = a.reshape(N, ldN // 32, 32).flip(2).reshape(N, ldN)
    return a @ v


def agg_bound(o32, o64):
    """The bound fg.Checker holds the `agg` tap to."""
    return min(fg.M * float((o32["agg"].double() - o64["agg"]).abs().max()) + fg.FLOOR * float(o64["agg"].abs().max()), fg.TOL_ACT)


@pytest.fixture(scope="module")
def oracle():
    """(state key, (H, W), pair) -> (fp32 oracle, fp64 oracle), each computed once; the preconditions are asserted here."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    cache, frames, states = {}, {}, {None: _state(), 0.0: _state(0.0)}

    def get(hw, pair, gamma=None):
        if hw not in frames:
            frames[hw] = torch.from_numpy(syn.make_frames(3, hw[0], hw[1], seed=SEED_FRAMES))
        key = (gamma, hw, pair)
        if key not in cache:
            o32, o64 = (oracle_pair(states[gamma], frames[hw], pair, dt) for dt in (torch.float32, torch.float64))
            peak = float(o64["attn"].max(1).values.median())
            assert peak > 0.5, "attention not peaked: median row maximum %.3f" % peak
            d = float((chunk_reversed_aggregate(o64["attn"], o64["mf"]) - o64["agg"]).abs().max())
            assert d > 100 * agg_bound(o32, o64), (d, agg_bound(o32, o64))
            cache[key] = (o32, o64)
        return states[gamma], frames[hw], cache[key]
    return get


def _net(sd, B, precision, low_latency=False):
    return fg._net(sd, B, precision, low_latency)


def _check_f16_kernels(tag, sd, attn, x, agg):
    """f16 mode: attention x V and the rebuilt motion_global against their own operands (module docstring). One pair:
    attn [N, ldN], x [N, 384], agg [N, 128] as read back."""
    N = attn.shape[0]
    a, mf, g = attn[:, :N].double(), x[:, 128:256].double(), agg.double()
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(agg).all()), tag
    # (the 126 convolved channels: the two flow channels of x have been overwritten by the iteration's flow update since)
    e = float((g - a @ mf)[:, :126].abs().max())
    mx = float(mf[:, :126].abs().max())
    bound = (2.0 ** -10 + (N + 8) * 2.0 ** -24) * mx
    print("PARITY-F16 %s agg-vs-own-operands err=%.3e bound=%.3e max|mf|=%.3e" % (tag, e, bound, mx))
    assert e <= bound, (tag, e, bound)
    wv = sd["update_block.aggregator.to_v.weight"][:, :, 0, 0].double()
    gamma = float(sd["update_block.aggregator.gamma"])
    want = mf + gamma * (g @ wv.t())
    lim = 130 * 2.0 ** -24 * (mf.abs() + abs(gamma) * (g.abs() @ wv.abs().t()))
    err = (x[:, 256:382].double() - want[:, :126]).abs()   # (the 126 convolved channels, as above)
    over = float((err - lim[:, :126]).max())
    print("PARITY-F16 %s mfg-rebuilt err=%.3e worst(err - bound)=%.3e" % (tag, float(err.max()), over))
    assert over <= 0, (tag, over)


def _run(oracle, hw, B, precision, low_latency=False, gamma=None):
    H, W = hw
    N = (H // 8) * (W // 8)
    tag = "%dx%d/B%d/%s%s%s" % (H, W, B, precision, "/ll" if low_latency else "", "" if gamma is None else "/gamma=%g" % gamma)
    res = {}
    for p in range(B):
        sd, frames, res[p] = oracle(hw, p, gamma)
    net = _net(sd, B, precision, low_latency)
    f1, f2 = frames[0:B].to(DEV), frames[1:B + 1].to(DEV)
    f16 = precision == "f16"
    ldN = (N + 31) // 32 * 32
    chk = fg.Checker(tag)
    low1, up1 = net(f1, f2, iters=1, test_mode=True)
    torch.cuda.synchronize()
    agg = net.debug_read("agg", (B, N, 128), H, W)
    x = net.debug_read("x", (B, N, 384), H, W)
    net1 = net.debug_read("net", (B, N, 128), H, W)
    attn = net.debug_read("attn", (B, N, ldN), H, W) if f16 else None
    low2, up2 = net(f1, f2, iters=2, test_mode=True)
    torch.cuda.synchronize()
    net2 = net.debug_read("net", (B, N, 128), H, W)
    clamped = fg._sf_clamped(net, hw)
    del net
    torch.cuda.empty_cache()
    for p in range(B):
        o32, o64 = res[p]
        t = lambda k: (o32[k], o64[k])   # noqa: E731
        if f16:
            _check_f16_kernels("%s/p%d" % (tag, p), sd, attn[p], x[p], agg[p])
            for name, got, key, tol in (("flow_low@1", low1, "low1", F16_LOW), ("flow_up@1", up1, "up1", F16_UP),
                                        ("flow_low@2", low2, "low2", F16_LOW), ("flow_up@2", up2, "up2", F16_UP)):
                e = float((got[p].cpu().double() - o64[key]).abs().max())
                print("PARITY-F16 %s/p%d %s err=%.3e bound=%.3e" % (tag, p, name, e, tol))
                assert e <= tol, (tag, p, name, e)
            assert bool(torch.isfinite(net1).all()) and bool(torch.isfinite(net2).all()), tag
            continue
        chk("p%d/agg" % p, agg[p], *t("agg"), fg.TOL_ACT)
        chk("p%d/mf0" % p, x[p, :, 128:254], *t("mf0"), fg.TOL_ACT)
        chk("p%d/mfg0" % p, x[p, :, 256:382], *t("mfg0"), fg.TOL_ACT)
        chk("p%d/net1" % p, net1[p], *t("net1"), fg.TOL_ACT)
        chk("p%d/net2" % p, net2[p], *t("net2"), fg.TOL_ACT)
        chk("p%d/flow_low@1" % p, low1[p], *t("low1"), fg.TOL_LOW)
        chk("p%d/flow_up@1" % p, up1[p], *t("up1"), fg.TOL_UP)
        chk("p%d/flow_low@2" % p, low2[p], *t("low2"), fg.TOL_LOW)
        chk("p%d/flow_up@2" % p, up2[p], *t("up2"), fg.TOL_UP)
    assert clamped == 0.0, tag
    if not f16:
        chk.finish()
    return low2, up2


CASES = [(hw, B, prec) for hw in GEOMS for B in (1, 2) for prec in ("split_f16", "f16")]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-B%d-%s" % (c[0] + c[1:]) for c in CASES])
def test_aggregate_and_folded_gates_match_the_fp64_oracle(oracle, case):
    """The `agg` tap against attn @ mf, x[:, 256:382] (rebuilt motion_global) against mfg0, the hidden state after one and after
    two iterations (the folded weights are then used four times), the flow after each; sf_clamped == 0."""
    hw, B, precision = case
    _run(oracle, hw, B, precision)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("hw", GEOMS, ids=["%dx%d" % hw for hw in GEOMS])
def test_low_latency_handle_at_one_pair(oracle, hw):
    """The low-latency handle at B = 1: the same checks against the oracle, and the flow within 2.5e-4 px of the default path's
    (the bound of tests/test_gpu_low_latency.py at KITTI size)."""
    _, up_ll = _run(oracle, hw, 1, "split_f16", low_latency=True)
    sd, frames, _ = oracle(hw, 0)
    base = _net(sd, 1, "split_f16")
    _, up = base(frames[0:1].to(DEV), frames[1:2].to(DEV), iters=2, test_mode=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(up_ll).all())
    assert float((up_ll - up).abs().max()) < 2.5e-4
    assert base.check_saturation(raise_on_clamp=False) == 0


@pytest.mark.timeout(600)
def test_gamma_zero(oracle):
    """gamma = 0: the agg block of the gate weights is all zeros, motion_global is the motion features themselves, and the
    stored aggregate is still attn @ mf."""
    hw = GEOMS[1]
    _run(oracle, hw, 1, "split_f16", gamma=0.0)
    _, _, (o32, o64) = oracle(hw, 0, 0.0)
    assert torch.equal(o64["mfg0"], o64["mf0"]) and float(o64["agg"].abs().max()) > 0
