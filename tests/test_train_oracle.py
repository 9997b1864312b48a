"""The CLVO training-iteration oracle against the imported reference's numbers (tests/golden/train.npz)."""
import os

import numpy as np
import torch

from atdn_vslam_amd import synthetic as syn
from oracle import clvo_train_ref as tr


def test_training_iteration_oracle_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "train.npz"))
    B, T = int(g["B"]), int(g["T"])
    P, S = tr.split_state(syn.to_torch(syn.make_clvo_state(seed=int(g["seed_weights"]))))
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    lr0, wd, eps = float(g["hp_lr"]), float(g["hp_wd"]), float(g["hp_eps"])
    for it in range(2):
        fl = torch.from_numpy(syn.make_flow(B * T, 376, 1232, seed=int(g["seed_flow"]) + it)).view(B, T, 2, 376, 1232)
        loss, pr, pt = tr.train_iteration(P, S, fl, torch.from_numpy(g["true_rot%d" % it]),
                                          torch.from_numpy(g["true_tr%d" % it]), float(g["hp_alpha"]), int(g["hp_w"]))
        assert abs(float(loss) - float(g["loss%d" % it])) < 2e-5 * max(1.0, float(g["loss%d" % it])), it
        np.testing.assert_allclose(pr.numpy(), g["pred_rot%d" % it], rtol=0, atol=2e-6)
        np.testing.assert_allclose(pt.numpy(), g["pred_tr%d" % it], rtol=0, atol=2e-6)
        lr = tr.cosine_lr(it, lr0, int(g["hp_total_steps"]), float(g["hp_eta_min"]))
        assert abs(lr - float(g["lr%d" % it])) < 1e-12
        for k, p in P.items():
            if "nograd/" + k in g.files:
                assert p.grad is None, k   # polar_norm is never used by forward()
                continue
            if it == 0:
                gr = p.grad.flatten().double()
                ref_n = float(g["gnorm/" + k])
                assert abs(float(gr.norm()) - ref_n) <= 2e-4 * ref_n + 1e-7, (k, float(gr.norm()), ref_n)
                np.testing.assert_allclose(gr[g["gidx/" + k]].numpy(), g["gval/" + k], rtol=2e-3,
                                           atol=2e-5 * ref_n + 1e-8, err_msg=k)
            with torch.no_grad():
                tr.adamw_step(p, p.grad, M[k], V[k], it + 1, lr, wd, eps)
        for k, p in P.items():
            ref_n = float(g["pnorm%d/" % it + k])
            assert abs(float(p.detach().double().norm()) - ref_n) <= 1e-5 * ref_n + 1e-7, (it, k)
        for k, s in S.items():
            if "stat%d/" % it + k in g.files:
                np.testing.assert_allclose(s.double().numpy(), g["stat%d/" % it + k], rtol=2e-5, atol=1e-6, err_msg=k)


def test_fp64_oracle_agrees_with_fp32_at_a_kitti_04_geometry():
    """The oracle is dtype-generic: run in fp64 it is the yardstick the GPU trainer is measured against at the other
    KITTI geometries (tests/test_gpu_train_geometry.py). At 370x1226 (sequences 04-10, odd at three of five levels),
    B = 2, T = 2, the fp32 and fp64 oracles agree on loss, predictions, every element of every gradient and every
    running statistic to fp32 rounding (worst gradient max|g32 - g64| / max|g64| was 1.2e-4, encoder_CNN.1.conv.bias)."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    B, T, H, W = 2, 2, 370, 1226
    sd = syn.to_torch(syn.make_clvo_state(seed=3))
    flows = torch.from_numpy(syn.make_flow(B * T, H, W, seed=90)).view(B, T, 2, H, W)
    r = np.random.RandomState(91)
    true_rot = torch.from_numpy(r.normal(0, 0.01, (B, T, 3)).astype(np.float32))
    true_tr = torch.from_numpy(r.normal(0, 0.5, (B, T, 3)).astype(np.float32))
    out = {}
    for dt in (torch.float32, torch.float64):
        P, S = tr.split_state(sd, dt)
        loss, pr, pt = tr.train_iteration(P, S, flows, true_rot, true_tr)
        assert loss.dtype == dt and pr.dtype == dt and all(s.dtype == dt for s in S.values())
        out[dt] = (loss, pr, pt, {k: p.grad for k, p in P.items()}, S)
    (l32, r32, t32, g32, s32), (l64, r64, t64, g64, s64) = out[torch.float32], out[torch.float64]
    assert abs(float(l32) - float(l64)) <= 1e-5 * abs(float(l64)), (float(l32), float(l64))
    for a, b in ((r32, r64), (t32, t64)):
        assert float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max())
    assert sorted(k for k, g in g64.items() if g is None) == ["polar_norm.bias", "polar_norm.weight"]
    for k, g in g64.items():
        if g is None:
            assert g32[k] is None, k
            continue
        assert g32[k].dtype == torch.float32 and g.dtype == torch.float64, k
        err, scale = float((g32[k].double() - g).abs().max()), float(g.abs().max())
        assert scale > 0 and err <= 5e-4 * scale, (k, err / scale)
    for k, s in s64.items():
        assert float((s32[k].double() - s).abs().max()) <= 1e-5 * float(s.abs().max()) + 1e-9, k
