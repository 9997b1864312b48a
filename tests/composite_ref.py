"""Differentiable restatement of CLVO_Loss (odometry/loss.py:25-118) for the composite-term tests (test infrastructure).

The reference builds its rotation matrices and Euler vectors with `torch.tensor([...])`, which cuts the autograd graph;
here the same expressions are assembled with `torch.stack`, so autograd of this function in float64 is the yardstick for
the trainer's `composite="gradient"` mode. The value is the reference's: tests/golden/composite.npz pins it.
"""
import torch

DELTA, KHI = 1.0, 100.0   # loss.py:20-21


def transform(rot, tr):
    """[...,3] Euler angles ("yxz", transforms.py:79-81) and [...,3] translations -> [...,4,4] homogeneous matrices."""
    c1, c2, c3 = torch.cos(rot[..., 0]), torch.cos(rot[..., 1]), torch.cos(rot[..., 2])
    s1, s2, s3 = torch.sin(rot[..., 0]), torch.sin(rot[..., 1]), torch.sin(rot[..., 2])
    zero, one = torch.zeros_like(c1), torch.ones_like(c1)
    rows = [torch.stack([c1 * c3 + s1 * s2 * s3, c3 * s1 * s2 - c1 * s3, c2 * s1, tr[..., 0]], -1),
            torch.stack([c2 * s3, c2 * c3, -s2, tr[..., 1]], -1),
            torch.stack([c1 * s2 * s3 - c3 * s1, c1 * c3 * s2 + s1 * s3, c1 * c2, tr[..., 2]], -1),
            torch.stack([zero, zero, zero, one], -1)]
    return torch.stack(rows, -2)


def matrix2euler(m):
    """transforms.py:41-44 on [...,4,4] (or [...,3,3]) matrices -> [...,3]."""
    a = torch.atan2(m[..., 0, 2], m[..., 2, 2])
    b = torch.atan2(-m[..., 1, 2], torch.sqrt(1 - m[..., 1, 2] ** 2))
    g = torch.atan2(m[..., 1, 0], m[..., 1, 1])
    return torch.stack([a, b, g], -1)


def transform_loss(pr, pt, tr_, tt):
    return DELTA * ((pt - tt) ** 2).sum(-1) + KHI * ((pr - tr_) ** 2).sum(-1)


def window_products(rot, tr, w):
    """[B,T,3] x 2 -> [B,T-w+1,4,4]: P_j P_{j+1} ... P_{j+w-1} for every window start j."""
    m = transform(rot, tr)
    T = rot.shape[1]
    out = []
    for j in range(T - w + 1):
        c = m[:, j]
        for i in range(j + 1, j + w):
            c = c @ m[:, i]
        out.append(c)
    return torch.stack(out, 1)


def clvo_loss_terms(pred_rot, pred_tr, true_rot, true_tr, w):
    """(mean_b L_rel, mean_b L_com), both differentiable in the predictions."""
    l_rel = transform_loss(pred_rot, pred_tr, true_rot, true_tr).sum(-1)
    cp, ct = window_products(pred_rot, pred_tr, w), window_products(true_rot, true_tr, w)
    l_com = transform_loss(matrix2euler(cp), cp[..., :3, 3], matrix2euler(ct), ct[..., :3, 3]).sum(-1)
    return l_rel.mean(), l_com.mean()


def clvo_loss(pred_rot, pred_tr, true_rot, true_tr, alpha, w):
    rel, com = clvo_loss_terms(pred_rot, pred_tr, true_rot, true_tr, w)
    return alpha * rel + (1 - alpha) * com
