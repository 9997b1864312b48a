"""GPU parity of the composite pose loss on its own (`training.clvo_loss` -> `atdn_clvo_loss`, one launch of
clvo_loss_composite_kernel) on the cases of tests/golden/composite.npz: one window, overlapping windows, w = 1, w = T, the
BASELINE batch, and more windows than one workgroup has threads.

Bounds. Loss value: `tol_loss` of the fixture (3e-6 relative to max(1, L64)), ten times what the reference's own fp32
evaluation deviates from the float64 oracle on these cases. Gradient of the composite term: 4e-5 of the tensor's largest
element against float64 autograd of tests/composite_ref.py, ten times what fp32 autograd of the same restatement deviates.
Reference-mode gradient: alpha x 2*100*(pr-tr)/B and alpha x 2*(pt-tt)/B in fp32 torch, rtol 1e-6 (a few roundings)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd.training import clvo_loss

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CASES = 8
MODES = ("reference", "gradient")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "composite.npz"))


def _case(g, i):
    B, T, w, alpha = g["cases"][i]
    x = [torch.from_numpy(g["%s%d" % (k, i)]) for k in ("pred_rot", "pred_tr", "true_rot", "true_tr")]
    return int(B), int(T), int(w), float(alpha), x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", range(N_CASES))
def test_loss_value_matches_the_float64_oracle(golden, case, mode):
    B, T, w, alpha, x = _case(golden, case)
    tol = float(golden["tol_loss"])
    assert 3e-6 <= tol < 1e-5
    dx = [t.to(DEV) for t in x]
    loss, _, _, (rel, com) = clvo_loss(*dx, alpha=alpha, w=w, composite=mode)
    l64, rel64, com64 = (float(golden["%s_%d" % (k, case)]) for k in ("loss64", "rel64", "com64"))
    print("case %d %s: L %.9g (fp64 %.12g, %.2e), L_rel %.9g (%.2e), L_com %.9g (%.2e)"
          % (case, mode, loss, l64, abs(loss - l64) / max(1, l64), rel, abs(rel - rel64) / max(1, rel64), com,
             abs(com - com64) / max(1, com64)))
    assert abs(loss - l64) <= tol * max(1.0, l64), (loss, l64)
    assert abs(rel - rel64) <= tol * max(1.0, rel64), (rel, rel64)
    assert abs(com - com64) <= tol * max(1.0, com64), (com, com64)
    # each term on its own: alpha = 1 is the relative-pose term, alpha = 0 the composite term
    only_rel = clvo_loss(*dx, alpha=1.0, w=w, composite=mode)[0]
    only_com = clvo_loss(*dx, alpha=0.0, w=w, composite=mode)[0]
    assert abs(only_rel - rel64) <= tol * max(1.0, rel64), (only_rel, rel64)
    assert abs(only_com - com64) <= tol * max(1.0, com64), (only_com, com64)


@pytest.mark.parametrize("case", range(N_CASES))
def test_reference_mode_gradient_is_alpha_times_the_relative_pose_gradient(golden, case):
    B, T, w, alpha, x = _case(golden, case)
    _, d_rot, d_tr, _ = clvo_loss(*[t.to(DEV) for t in x], alpha=alpha, w=w, composite="reference")
    want_rot = alpha * (2 * 100 * (x[0] - x[2]) / B)
    want_tr = alpha * (2 * (x[1] - x[3]) / B)
    torch.testing.assert_close(d_rot.cpu(), want_rot, rtol=1e-6, atol=0)
    torch.testing.assert_close(d_tr.cpu(), want_tr, rtol=1e-6, atol=0)


def _autograd64(x, alpha, w):
    d = [t.double() for t in x]
    d[0].requires_grad_(True)
    d[1].requires_grad_(True)
    cr.clvo_loss(*d, alpha, w).backward()
    return d[0].grad, d[1].grad


@pytest.mark.parametrize("case", range(N_CASES))
def test_gradient_mode_matches_float64_autograd(golden, case):
    B, T, w, alpha, x = _case(golden, case)
    dx = [t.to(DEV) for t in x]
    _, d_rot, d_tr, _ = clvo_loss(*dx, alpha=alpha, w=w, composite="gradient")
    want_rot, want_tr = _autograd64(x, alpha, w)
    for name, got, want in (("d_rot", d_rot, want_rot), ("d_tr", d_tr, want_tr)):
        err, scale = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
        print("case %d %s: max error %.3e of max %.3e (%.2e)" % (case, name, err, scale, err / scale))
        assert err <= 4e-5 * scale, (name, err, scale)
    # two consecutive calls: the same bits (fixed summation order, no atomics)
    _, again_rot, again_tr, _ = clvo_loss(*dx, alpha=alpha, w=w, composite="gradient")
    assert torch.equal(again_rot, d_rot) and torch.equal(again_tr, d_tr)


@pytest.mark.parametrize("case", [1, 6])
def test_alpha_one_ignores_the_mode(golden, case):
    B, T, w, _, x = _case(golden, case)
    dx = [t.to(DEV) for t in x]
    a = clvo_loss(*dx, alpha=1.0, w=w, composite="reference")
    b = clvo_loss(*dx, alpha=1.0, w=w, composite="gradient")
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    torch.testing.assert_close(a[1].cpu(), 2 * 100 * (x[0] - x[2]) / B, rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", MODES)
def test_pitch_of_exactly_half_pi_stays_finite(mode):
    """One clip whose single window sits on the Euler singularity (C12 = -1: the radicand 1 - C12^2 rounds to 0 or below, where the
    reference's sqrt / its derivative give NaN / inf). The clamps keep the loss and both gradients finite."""
    half_pi = np.float32(math.pi / 2)
    pr = torch.tensor([[[0.3, half_pi, 0.2]]], dtype=torch.float32)
    tr_ = torch.tensor([[[0.3, half_pi, 0.2]]], dtype=torch.float32) + torch.tensor([0.01, 0.0, -0.01])
    pt, tt = torch.tensor([[[0.5, -0.2, 1.0]]]), torch.tensor([[[0.4, -0.1, 1.1]]])
    loss, d_rot, d_tr, terms = clvo_loss(pr.to(DEV), pt.to(DEV), tr_.to(DEV), tt.to(DEV), alpha=0.5, w=1, composite=mode)
    assert math.isfinite(loss) and all(math.isfinite(t) for t in terms)
    assert bool(torch.isfinite(d_rot).all()) and bool(torch.isfinite(d_tr).all())


@pytest.mark.parametrize("w", [0, 5])
def test_window_outside_the_clip_raises(golden, w):
    B, T, _, alpha, x = _case(golden, 1)
    assert T == 4
    with pytest.raises(RuntimeError, match="sequence length"):
        clvo_loss(*[t.to(DEV) for t in x], alpha=alpha, w=w, composite="gradient")


def test_unknown_mode_raises(golden):
    _, _, w, alpha, x = _case(golden, 0)
    with pytest.raises(ValueError):
        clvo_loss(*[t.to(DEV) for t in x], alpha=alpha, w=w, composite="both")
