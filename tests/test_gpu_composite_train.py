"""The composite pose loss through CLVOTrainer (B = 2, T = 4, w = 3 at 376x1232: two overlapping windows per clip, predictions
step-major inside the trainer) against the CPU oracle (oracle/clvo_train_ref.py), with the project's own bounds for this
comparison (tests/test_gpu_train.py): loss to 1e-4 * max(1, ref), every gradient norm to 3e-3 relative.

  composite="reference"  oracle.train_iteration(..., alpha, w): the composite term is evaluated without graph. On top of that
                         every gradient is 0.5 x the alpha = 1 gradient bit for bit: a power-of-two scale commutes with fp32
                         rounding through the whole (linear) backward pass, so any leak of the composite term would show.
  alpha = 1              with the new arguments given: torch.equal to a trainer built without them.
  composite="gradient"   CPU autograd of oracle.forward_train stepped over the clip + the differentiable restatement of the
                         loss (tests/composite_ref.py).
The GPU iterations and the two oracle runs are computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, synthetic as syn
from atdn_vslam_amd.training import CLVOTrainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, W, ALPHA = 2, 4, 3, 0.5
HP = dict(lr=1e-3, weight_decay=1e-3, eps=1e-8, total_steps=10, eta_min=1e-9)


@pytest.fixture(scope="module")
def inputs():
    sd = syn.to_torch(syn.make_clvo_state(seed=3))
    flows = torch.from_numpy(syn.make_flow(B * T, 376, 1232, seed=91)).view(B, T, 2, 376, 1232)
    r = np.random.RandomState(17)
    # targets of the size of the fixture's: chained rotations where the s1*s2*s3 cross terms matter (the head's predictions at
    # these synthetic weights are small, so the composite error is dominated by the targets' windows)
    true_rot = torch.from_numpy((r.uniform(-1, 1, (B, T, 3)) * np.array((0.6, 0.3, 0.4))).astype(np.float32))
    true_tr = torch.from_numpy(r.uniform(-0.5, 1.5, (B, T, 3)).astype(np.float32))
    return sd, flows, true_rot, true_tr


@pytest.fixture(scope="module")
def gpu_runs(inputs):
    sd, flows, true_rot, true_tr = inputs
    fl = flows.to(DEV)
    out = {}
    for name, kw in (("plain", {}), ("alpha1", dict(alpha=1.0, w=W, composite="gradient")),
                     ("reference", dict(alpha=ALPHA, w=W, composite="reference")),
                     ("gradient", dict(alpha=ALPHA, w=W, composite="gradient"))):
        tr = CLVOTrainer(sd, B, T, device=DEV, **HP, **kw)
        assert tr.loss_terms is None
        if name == "alpha1":   # (the constructor leaves the library's default loss alone for alpha = 1: select it explicitly too)
            _lib.check(_lib.lib().atdn_clvo_trainer_set_loss(tr._h, 1.0, W, 1))
        loss, pr, pt = tr.forward_backward(fl, true_rot, true_tr)
        out[name] = dict(loss=loss, pr=pr.cpu(), pt=pt.cpu(), grads=tr.grads.clone().cpu(), terms=tr.loss_terms, trainer=tr)
    return out


def _check_against_oracle(run, ref_loss, P):
    loss = run["loss"]
    print("loss %.6f, oracle %.6f" % (loss, ref_loss))
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, ref_loss), (loss, ref_loss)
    worst = 0.0
    for k, p in P.items():
        if p.grad is None:
            continue
        ref_n = float(p.grad.double().norm())
        got_n = float(run["trainer"].gradient(k).flatten().double().norm())
        rel = abs(got_n - ref_n) / (ref_n + 1e-12)
        worst = max(worst, rel)
        assert rel < 3e-3, (k, got_n, ref_n)
    print("worst gradient-norm deviation %.2e" % worst)


def test_reference_mode_matches_the_oracle(inputs, gpu_runs):
    from oracle import clvo_train_ref as ref
    sd, flows, true_rot, true_tr = inputs
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    P, S = ref.split_state(sd)
    ref_loss, ref_pr, ref_pt = ref.train_iteration(P, S, flows, true_rot, true_tr, ALPHA, W)
    run = gpu_runs["reference"]
    np.testing.assert_allclose(run["pr"].numpy(), ref_pr.numpy(), rtol=0, atol=5e-5)
    np.testing.assert_allclose(run["pt"].numpy(), ref_pt.numpy(), rtol=0, atol=5e-5)
    _check_against_oracle(run, float(ref_loss), P)
    rel, com = run["terms"]
    assert abs(ALPHA * rel + (1 - ALPHA) * com - run["loss"]) <= 1e-6 * max(1.0, run["loss"])


def test_reference_mode_gradients_are_half_the_alpha_one_gradients_bit_for_bit(gpu_runs):
    half, full = gpu_runs["reference"], gpu_runs["plain"]
    assert torch.equal(half["pr"], full["pr"]) and torch.equal(half["pt"], full["pt"])
    keep = full["grads"].abs() >= 1e-30          # (below that, halving leaves the normal range and rounds)
    assert int(keep.sum()) > 0.5 * keep.numel()
    assert torch.equal(half["grads"][keep], ALPHA * full["grads"][keep])
    assert float(half["grads"][~keep].abs().max()) <= 1e-30
    # the relative-pose term reported beside the total is the alpha = 1 loss: the same fp32 products summed in double, one rounding
    assert abs(half["terms"][0] - full["loss"]) <= 2e-7 * max(1.0, full["loss"])
    assert full["terms"] is None


def test_alpha_one_with_the_new_arguments_is_the_parent_path(gpu_runs):
    a, b = gpu_runs["alpha1"], gpu_runs["plain"]
    assert a["loss"] == b["loss"] and a["terms"] is None
    assert torch.equal(a["pr"], b["pr"]) and torch.equal(a["pt"], b["pt"])
    assert torch.equal(a["grads"], b["grads"])


def test_gradient_mode_matches_cpu_autograd(inputs, gpu_runs):
    from oracle import clvo_train_ref as ref
    sd, flows, true_rot, true_tr = inputs
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    P, S = ref.split_state(sd)
    state = [torch.zeros(B, 512) for _ in range(4)]
    rots, trs = [], []
    for j in range(T):
        r, t, state = ref.forward_train(P, S, flows[:, j], state)
        rots.append(r)
        trs.append(t)
    loss = cr.clvo_loss(torch.stack(rots, dim=1), torch.stack(trs, dim=1), true_rot, true_tr, ALPHA, W)
    loss.backward()
    run = gpu_runs["gradient"]
    _check_against_oracle(run, float(loss.detach()), P)
    # the composite term did reach the weights: these gradients are not the reference mode's
    assert not torch.equal(run["grads"], gpu_runs["reference"]["grads"])
    assert run["loss"] == gpu_runs["reference"]["loss"] and run["terms"] == gpu_runs["reference"]["terms"]


def test_window_outside_the_clip_raises(inputs):
    sd = inputs[0]
    for w in (0, T + 1):
        with pytest.raises(ValueError, match="sequence_length"):
            CLVOTrainer(sd, B, T, device=DEV, **HP, alpha=ALPHA, w=w, composite="gradient")
    with pytest.raises(ValueError, match="composite"):
        CLVOTrainer(sd, B, T, device=DEV, **HP, alpha=ALPHA, w=W, composite="both")
