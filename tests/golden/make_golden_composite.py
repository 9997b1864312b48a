"""Golden fixture for the composite pose loss, produced by running the REFERENCE's `CLVO_Loss(alpha, w)`
(odometry/loss.py:25-118) on seeded poses. Per case (B, T, w, alpha) stored: the fp32 inputs, the reference's loss on them
(fp32 arithmetic), the oracle's float64 loss and its two terms (`oracle.clvo_train_ref.clvo_loss` on the inputs cast to
double, with alpha, 1 and 0), and the largest |C12| over all windows of predictions and targets. `tol_loss` is the relative
bound the GPU tests use for the loss value: 3e-6, or ten times the worst deviation of the reference's own fp32 evaluation
from the float64 oracle if that is larger.

Targets: rotations uniform in +-(0.6, 0.3, 0.4) rad per axis (+-(0.3, 0.12, 0.2) for w = 6), translations uniform in
[-0.5, 1.5]; predictions are the targets + N(0, 0.02) (rotations) and N(0, 0.3) (translations). Every window keeps
|C12| <= 0.9 and |a|, |g| <= 2.5 (asserted): away from the Euler singularity and the +-pi seam.

Run only in the build container (needs /root/reference):   python tests/golden/make_golden_composite.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"

from make_golden import install_stubs  # noqa: E402

# (B, T, w, alpha)
CASES = ((1, 3, 3, 0.5), (2, 4, 3, 0.5), (3, 5, 3, 0.25), (2, 6, 2, 0.0), (5, 6, 1, 0.3), (3, 6, 6, 0.7), (24, 6, 3, 0.5),
         (300, 3, 2, 0.5))
SEED = 600


def make_inputs(i, B, T, w):
    r = np.random.RandomState(SEED + i)
    amp = np.array((0.3, 0.12, 0.2) if w == 6 else (0.6, 0.3, 0.4))
    true_rot = r.uniform(-1.0, 1.0, (B, T, 3)) * amp
    true_tr = r.uniform(-0.5, 1.5, (B, T, 3))
    pred_rot = true_rot + r.normal(0, 0.02, (B, T, 3))
    pred_tr = true_tr + r.normal(0, 0.3, (B, T, 3))
    return [torch.from_numpy(x.astype(np.float32)) for x in (pred_rot, pred_tr, true_rot, true_tr)]


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from atdn_vslam.odometry.loss import CLVO_Loss
    from oracle import clvo_train_ref as oracle
    import composite_ref as cr

    out = {"cases": np.array(CASES, dtype=np.float64)}
    worst = 0.0
    for i, (B, T, w, alpha) in enumerate(CASES):
        pr, pt, tr_, tt = make_inputs(i, B, T, w)
        ref = float(CLVO_Loss(alpha, w=w, device="cpu")(pr, pt, tr_, tt, device="cpu"))
        d = [x.double() for x in (pr, pt, tr_, tt)]
        l64 = float(oracle.clvo_loss(*d, alpha, w))
        rel64 = float(oracle.clvo_loss(*d, 1.0, w))
        com64 = float(oracle.clvo_loss(*d, 0.0, w))
        assert abs(alpha * rel64 + (1 - alpha) * com64 - l64) <= 1e-12 * max(1.0, l64)
        big_c12, big_ang = 0.0, 0.0
        for rot, tr in ((d[0], d[1]), (d[2], d[3])):
            c = cr.window_products(rot, tr, w)
            e = cr.matrix2euler(c)
            big_c12 = max(big_c12, float(c[..., 1, 2].abs().max()))
            big_ang = max(big_ang, float(e[..., 0].abs().max()), float(e[..., 2].abs().max()))
        assert big_c12 <= 0.9 and big_ang <= 2.5, (i, big_c12, big_ang)
        dev = abs(ref - l64) / max(1.0, l64)
        worst = max(worst, dev)
        for k, v in (("pred_rot", pr), ("pred_tr", pt), ("true_rot", tr_), ("true_tr", tt)):
            out["%s%d" % (k, i)] = v.numpy()
        out["ref_loss%d" % i], out["loss64_%d" % i] = np.float64(ref), np.float64(l64)
        out["rel64_%d" % i], out["com64_%d" % i] = np.float64(rel64), np.float64(com64)
        out["max_c12_%d" % i], out["max_angle_%d" % i] = np.float64(big_c12), np.float64(big_ang)
        print("case %d %s: reference %.9g, oracle fp64 %.12g (deviation %.2e), max |C12| %.3f, max angle %.3f"
              % (i, (B, T, w, alpha), ref, l64, dev, big_c12, big_ang))
    out["ref_worst_deviation"] = np.float64(worst)
    out["tol_loss"] = np.float64(max(3e-6, 10 * worst))
    np.savez_compressed(os.path.join(HERE, "composite.npz"), **out)
    print("composite golden written; worst reference deviation %.2e, tol_loss %.2e" % (worst, out["tol_loss"]))


if __name__ == "__main__":
    main()
