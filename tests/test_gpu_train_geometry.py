"""CLVO trainer and inference encoder against the fp64 oracle at every KITTI geometry the network accepts.

The reference's loader crops only widths above 1232 (odometry/datasets.py), so sequence 03 reaches the network as 375x1232
and sequences 04-10 as 370x1226; 353x1217 is the smallest accepted size and odd at every level (177/89/45/23 rows,
609/305/153/77 columns). Every gradient element, prediction and running statistic is compared with the oracle run in fp64.
The yardstick of each tensor is the fp32 CPU oracle's own error on it:

    max|x_hip - x64| <= min(M * max|x32 - x64| + floor * max|x64|,  1e-3 * max|x64|)

Calibrated once on the MI355X: the worst (max|x_hip - x64| - floor * max|x64|) / max|x32 - x64| over every tensor of every case
was 5.82 for one training iteration (grad of encoder_CNN.1.conv.bias, 375x1232, B = 5, T = 3; floor 1e-5) and 0.72 for the
encoder and the stateful head (the scanned rotation, floor 1e-6); M_ITER and M_ENC are at most 4x those. The worst gradient,
relative to its own max|g64|, was 4.2e-4 (that same stem bias, a sum over every pixel that BatchNorm nearly cancels; the fp32
oracle's own error there is 1.2e-4); no tensor needs the 1e-3 cap. Running `pytest -s` prints every comparison ("PARITY" lines)."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import ATDNVO
from atdn_vslam_amd.training import CLVOTrainer
from oracle import clvo_ref
from oracle import clvo_train_ref as ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parity_check import CAP, Checker  # noqa: E402,F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

M_ITER, FLOOR = 20.0, 1e-5       # one training iteration (observed 5.82)
M_ENC, FLOOR_ENC = 2.5, 1e-6      # inference encoder and head (observed 0.72)
TRAJ = 1e-4                       # four iterations end to end, relative to max|x64| (observed 2.5e-5)

GEOMS = [(376, 1232), (375, 1232), (370, 1226), (353, 1217)]
SHAPES = [(2, 1), (3, 2), (5, 3)]
HP = dict(lr=1e-3, weight_decay=1e-2, eps=1e-8, total_steps=5, eta_min=1e-9)
SEED_W = 3


def _ids(v):
    return "x".join(str(x) for x in v)


def _inputs(B, T, H, W, seed):
    flows = torch.from_numpy(syn.make_flow(B * T, H, W, seed=seed)).view(B, T, 2, H, W)
    r = np.random.RandomState(seed + 1)
    rot = torch.from_numpy(r.normal(0, 0.01, (B, T, 3)).astype(np.float32))
    tr = torch.from_numpy(r.normal(0, 0.5, (B, T, 3)).astype(np.float32))
    return flows, rot, tr


def _oracle_iteration(sd, inputs, dtype):
    P, S = ref.split_state(sd, dtype)
    loss, pr, pt = ref.train_iteration(P, S, *inputs)
    return {"loss": loss.reshape(1), "pred_rot": pr, "pred_tr": pt, "P": P, "stat": S,
            "grad": {k: p.grad for k, p in P.items() if p.grad is not None},
            "nograd": sorted(k for k, p in P.items() if p.grad is None)}


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return syn.to_torch(syn.make_clvo_state(seed=SEED_W))


@pytest.fixture(scope="module")
def oracle(sd):
    """(H, W, B, T) -> inputs and the fp32 / fp64 oracle iteration on them, computed once per module."""
    cache = {}

    def get(H, W, B, T):
        key = (H, W, B, T)
        if key not in cache:
            inputs = _inputs(B, T, H, W, seed=1000 + 7 * B + 131 * T + H + W)
            cache[key] = (inputs, _oracle_iteration(sd, inputs, torch.float32), _oracle_iteration(sd, inputs, torch.float64))
        return cache[key]
    return get


def _check_iteration(chk, trainer, got, o32, o64):
    loss, pr, pt = got
    chk("loss", torch.tensor([loss]), o32["loss"], o64["loss"])
    chk("pred_rot", pr, o32["pred_rot"], o64["pred_rot"])
    chk("pred_tr", pt, o32["pred_tr"], o64["pred_tr"])
    for k, g64 in o64["grad"].items():
        chk("grad/" + k, trainer.gradient(k), o32["grad"][k], g64)
    assert o64["nograd"] == ["polar_norm.bias", "polar_norm.weight"]
    for k in o64["nograd"]:
        assert float(trainer.gradient(k).abs().max()) == 0.0, k   # forward() never touches polar_norm
    st = trainer.state_dict()
    for k, s64 in o64["stat"].items():
        chk("stat/" + k, st[k], o32["stat"][k], s64)


def _run_case(sd, oracle, H, W, B, T, m=M_ITER, tag=""):
    inputs, o32, o64 = oracle(H, W, B, T)
    tr = CLVOTrainer(sd, B, T, hw=(H, W), device=DEV, **HP)
    got = tr.forward_backward(inputs[0].to(DEV), inputs[1], inputs[2])
    torch.cuda.synchronize()
    chk = Checker("%dx%d/B%d/T%d%s" % (H, W, B, T, tag), m)
    _check_iteration(chk, tr, got, o32, o64)
    chk.finish()


CASES = [(hw, bt) for hw in GEOMS for bt in SHAPES] + [((370, 1226), (2, 32))]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("hw,bt", CASES, ids=["%s-%s" % (_ids(hw), _ids(bt)) for hw, bt in CASES])
def test_training_iteration_matches_the_fp64_oracle(sd, oracle, hw, bt):
    """One forward_backward: loss, every prediction, every element of every gradient, every running statistic; polar_norm
    gradients exactly zero. Odd H / W at each level exercise the stem tiles, the zero-stuffed data gradients with an output
    padding, the weight-gradient column staging and the BatchNorm partial-row remainders; (2, 32) is the longest clip."""
    _run_case(sd, oracle, hw[0], hw[1], bt[0], bt[1])


def test_adamw_over_four_steps_matches_fp64_adamw_on_the_trainers_gradients(sd):
    """Four iterations at 370x1226 with total_steps = 5 (the cosine rate moves every step) and weight decay 1e-2. After each
    optimizer_step every parameter element equals an fp64 AdamW step (fp64 m / v carried from step 1) applied to the
    trainer's own parameters and gradients, within a few fp32 ulps: bias correction at t = 1..4, decay on every trained
    range (biases, BatchNorm gamma / beta and the bias-free *_regressor.2.weight included), polar_norm left untouched."""
    H, W, B, T = 370, 1226, 2, 2
    tr = CLVOTrainer(sd, B, T, hw=(H, W), device=DEV, **HP)
    keys = [k for k in sd if not (k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"))]
    M = {k: torch.zeros(sd[k].shape, dtype=torch.float64) for k in keys}
    V = {k: torch.zeros(sd[k].shape, dtype=torch.float64) for k in keys}
    f32 = lambda x: float(np.float32(x))                      # noqa: E731  (the kernel receives fp32 scalars)
    u = 2.0 ** -23
    lrs, moved = [], []
    for it in range(4):
        flows, rot, trn = _inputs(B, T, H, W, seed=500 + it)
        tr.forward_backward(flows.to(DEV), rot, trn)
        before = {k: tr.parameter(k).double() for k in keys}
        grads = {k: tr.gradient(k).double() for k in keys}
        lr = tr.current_lr()
        lrs.append(lr)
        tr.optimizer_step()
        for k in keys:
            after = tr.parameter(k).double()
            if k.startswith("polar_norm."):
                assert torch.equal(after, before[k]), k
                continue
            want = before[k].clone()
            ref.adamw_step(want, grads[k], M[k], V[k], it + 1, f32(lr), f32(HP["weight_decay"]), f32(HP["eps"]))
            tol = 6 * u * (want.abs() + f32(lr))
            err = (after - want).abs()
            assert bool((err <= tol).all()), (it, k, float(err.max()), float((err / tol).max()))
            moved.append((after != before[k]).flatten())
    assert len(set(lrs)) == 4 and lrs[0] == HP["lr"]
    assert float(torch.cat(moved).double().mean()) > 0.9


def test_four_iterations_end_to_end_follow_the_fp64_trajectory(sd):
    """The same four iterations against the oracle's own trajectory (fp64 parameters, AdamW state and running statistics):
    loss, predictions and running statistics of every iteration within 1e-4 of their largest magnitude (worst observed 2.5e-5,
    the rotation of iteration 3). The fp32 oracle is no yardstick here: over the same trajectory it drifts 8e-4 from fp64."""
    H, W, B, T = 370, 1226, 2, 2
    tr = CLVOTrainer(sd, B, T, hw=(H, W), device=DEV, **HP)
    P, S = ref.split_state(sd, torch.float64)
    M = {k: torch.zeros_like(p) for k, p in P.items()}
    V = {k: torch.zeros_like(p) for k, p in P.items()}
    bad = []
    for it in range(4):
        inputs = _inputs(B, T, H, W, seed=500 + it)
        l64, r64, t64 = ref.train_iteration(P, S, *inputs)
        lr = ref.cosine_lr(it, HP["lr"], HP["total_steps"], HP["eta_min"])
        with torch.no_grad():
            for k, p in P.items():
                if p.grad is not None:
                    ref.adamw_step(p, p.grad, M[k], V[k], it + 1, lr, HP["weight_decay"], HP["eps"])
        loss, pr, pt = tr.forward_backward(inputs[0].to(DEV), inputs[1], inputs[2])
        st = tr.state_dict()
        tr.optimizer_step()
        chk = Checker("trajectory/it%d" % it, 0.0, TRAJ)
        chk("loss", torch.tensor([loss]), l64.reshape(1), l64.reshape(1))
        chk("pred_rot", pr, r64, r64)
        chk("pred_tr", pt, t64, t64)
        for k, s64 in S.items():
            chk("stat/" + k, st[k], s64, s64)
        try:
            chk.finish()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


ENC_GEOMS = [(370, 1226), (375, 1232), (353, 1217)]


@pytest.fixture(scope="module")
def head_sd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.mark.parametrize("hw", ENC_GEOMS, ids=[_ids(hw) for hw in ENC_GEOMS])
def test_encoder_matches_the_fp64_oracle(head_sd, hw):
    """ATDNVO.encode (clvo.hip and the 8x64 / 4x32 / 2x32 tiles of launch_conv16_eval) at batch 1, 5 and 16."""
    H, W = hw
    fl = torch.from_numpy(syn.make_flow(16, H, W, seed=60 + H + W))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in head_sd.items()}
    f32, f64 = clvo_ref.clvo_encode(head_sd, fl), clvo_ref.clvo_encode(sd64, fl.double())
    head = ATDNVO()
    head.load_state_dict(head_sd)
    head = head.to(DEV).eval()
    for b in (1, 5, 16):
        chk = Checker("encode/%dx%d/B%d" % (H, W, b), M_ENC, FLOOR_ENC)
        chk("feat", head.encode(fl[:b].to(DEV)), f32[:b], f64[:b])
        chk.finish()


def test_stateful_head_over_twenty_frames_matches_the_fp64_oracle(head_sd):
    """20 consecutive frames at 370x1226, stepped one frame per call at batch 1 (evaluate_odometry.py's pattern, per-step
    kernel) and as ATDNVO.scan over the 20 encoded features (persistent scan, T >= 16), against the oracle stepped frame by
    frame in fp64."""
    H, W, N = 370, 1226, 20
    fl = torch.from_numpy(syn.make_flow(N, H, W, seed=71))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in head_sd.items()}
    want = {}
    for dt, s in ((torch.float32, head_sd), (torch.float64, sd64)):
        feats = clvo_ref.clvo_encode(s, fl.to(dt))
        state, rots, trs = clvo_ref.zero_state(1, dt), [], []
        for t in range(N):
            r, x, state = clvo_ref.clvo_step(s, feats[t:t + 1], state)
            rots.append(r)
            trs.append(x)
        want[dt] = (torch.cat(rots), torch.cat(trs), torch.stack([z[0] for z in state]))
    head = ATDNVO(batch_size=1)
    head.load_state_dict(head_sd)
    head = head.to(DEV).eval()
    rots, trs = [], []
    for t in range(N):
        r, x = head(fl[t:t + 1].to(DEV))
        rots.append(r)
        trs.append(x)
    stepped = (torch.cat(rots), torch.cat(trs), torch.stack([head.lstm1_h[0], head.lstm1_c[0], head.lstm2_h[0], head.lstm2_c[0]]))
    feats = head.encode(fl.to(DEV))
    r, x, st = head.scan(feats[:, None, :], hw=(H, W))
    scanned = (r[:, 0], x[:, 0], st[:, 0])
    (r32, t32, s32), (r64, t64, s64) = want[torch.float32], want[torch.float64]
    for tag, got in (("stepped", stepped), ("scan", scanned)):
        chk = Checker("head20/%s" % tag, M_ENC, FLOOR_ENC)
        chk("rot", got[0], r32, r64)
        chk("tr", got[1], t32, t64)
        chk("state", got[2], s32, s64)
        chk.finish()


@pytest.mark.parametrize("hw", [(352, 1232), (449, 1232), (376, 1216)], ids=_ids)
def test_sizes_outside_the_accepted_range_are_rejected(sd, head_sd, hw):
    with pytest.raises(RuntimeError, match="16x4x13"):
        CLVOTrainer(sd, 2, 2, hw=hw, device=DEV, **HP)
    head = ATDNVO()
    head.load_state_dict(head_sd)
    head = head.to(DEV)
    with pytest.raises(RuntimeError, match="16x4x13"):
        head.encode(torch.zeros(1, 2, hw[0], hw[1], device=DEV))


def test_batch_and_clip_limits_are_rejected_and_a_later_trainer_is_sound(sd, oracle):
    """B = 1 (BatchNorm in training mode needs two samples; the reference accepts it, this trainer does not), B = 65,
    T = 0 and T = 33 are refused; a trainer built afterwards in the same process still matches the oracle."""
    for B, T in ((1, 2), (65, 2), (2, 0), (2, 33)):
        with pytest.raises(RuntimeError, match="out of range"):
            CLVOTrainer(sd, B, T, hw=(370, 1226), device=DEV, **HP)
    _run_case(sd, oracle, 370, 1226, 2, 1, tag="/after-rejections")
