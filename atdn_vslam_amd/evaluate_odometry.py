"""`evaluate_odometry.py` of the reference on the HBM flow bank.

    python -m atdn_vslam_amd.evaluate_odometry --config config.yaml --stage 4 --sequence 09 --exp 6 --forward 0 \\
        (--flow-weights gma-kitti.pth [--geometry slam|crop] | --flows2) [--weights PATH] [--out-dir DIR]

`--forward 1` runs the pose head over flows 0 .. n-2 of the sequence in order, `--forward -1` over -flow[n-2] .. -flow[0]:
FlowKittiDataset2(sequence_length=1, augment=forward) walked from the start or from the end (evaluate_odometry.py:21-81).
The flows come out of the bank by atdn_flow_gather_clips in chunks, the head runs as ATDNVO.encode + one ordered
ATDNVO.scan (the stateful per-frame calls of the reference, its LSTM state carried over the whole sequence), and the
trajectory is transforms.rel2abs. Poses are written in the KITTI format as `<exp>_ATDNVO_c_<seq>_{f,b}.txt`
(save_results, :84-99). `--forward 0` does both runs and, when dataset/poses/<seq>.txt exists, also the Kalman-fused
trajectory (`..._fused.txt`) and ATE / RPE of all three (evaluation.py).

Checkpoint: `atdn_vslam/checkpoints/<exp>_<stage>_atdnvo_c.pth` as the reference names it (:38), or `--weights`.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import evaluation, flowbank as fb, transforms
from .modules import ATDNVO


def run_inference(head, bank, sequence, forward, chunk=64):
    """(rot [n,3], tr [n,3]) fp32 of the head over the n flows of `sequence`: forward (1) or the negated flows from the
    last one back (-1). The head's own LSTM state is not used or changed."""
    s = bank.sequence(sequence)
    n = s.n_flows
    if forward == 1:
        starts, rev = s.first + np.arange(n), np.zeros(n, dtype=np.int32)
    elif forward == -1:
        starts, rev = s.first + np.arange(n - 1, -1, -1), np.ones(n, dtype=np.int32)
    else:
        raise ValueError("forward must be 1 or -1, got %r" % (forward,))
    H, W = bank.hw
    buf = torch.empty((chunk, 1, 2, H, W), dtype=torch.float32, device=bank.device)
    feats = []
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        out = bank.gather(starts[c0:c0 + m], rev[c0:c0 + m], 1, out=buf[:m])
        feats.append(head.encode(out.view(m, 2, H, W)))
    rot, tr, _ = head.scan(torch.cat(feats)[:, None, :], hw=bank.hw)
    return rot[:, 0], tr[:, 0]


def result_name(exp, sequence, forward):
    return "%s_ATDNVO_c_%s_%s.txt" % (exp, sequence, "f" if forward > 0 else "b")


def evaluate(head, bank, sequence, exp, forward, out_dir, gt_poses=None):
    """Runs the requested direction(s), writes the pose files, returns {name: [T,4,4] float64} (+ "metrics")."""
    os.makedirs(out_dir, exist_ok=True)
    runs = {}
    for d in ((1, -1) if forward == 0 else (forward,)):
        rot, tr = run_inference(head, bank, sequence, d)
        poses = transforms.rel2abs(rot.cpu().numpy(), tr.cpu().numpy()).numpy()
        evaluation.save_kitti_poses(os.path.join(out_dir, result_name(exp, sequence, d)), poses)
        runs["f" if d > 0 else "b"] = poses
    if forward == 0 and gt_poses is not None:
        gt = evaluation._hom(gt_poses)
        back = evaluation.reverse_backward_run(runs["b"])
        std = evaluation.motion_std(gt, runs["f"], back)
        fused = evaluation.fuse_forward_backward(runs["f"], runs["b"], std)
        evaluation.save_kitti_poses(os.path.join(out_dir, "%s_ATDNVO_c_%s_fused.txt" % (exp, sequence)), fused)
        runs["fused"] = fused
        metrics = {}
        for k, p in (("forward", runs["f"]), ("backward", back), ("fused", fused)):
            t_rpe, r_rpe = evaluation.rpe(p, gt)
            metrics[k] = {"ate_se3": evaluation.ate_rmse(p, gt), "rpe_trans": t_rpe, "rpe_rot": r_rpe}
        runs["metrics"] = metrics
    return runs


def main(argv=None):
    from .train_odometry import build_bank, load_config, Config
    ap = argparse.ArgumentParser(description="ATDNVO evaluation on the HBM flow bank (the reference's evaluate_odometry.py)")
    ap.add_argument("--stage", type=int, required=True)
    ap.add_argument("--sequence", type=str, default="00")
    ap.add_argument("--exp", type=int, default=6)
    ap.add_argument("--forward", type=int, required=True, choices=(-1, 0, 1))
    ap.add_argument("--config", default=None, help="the reference's config.yaml (for data_path)")
    ap.add_argument("--data-path", default=None, help="instead of --config")
    ap.add_argument("--weights", default=None, help="ATDNVO checkpoint (default: atdn_vslam/checkpoints/<exp>_<stage>_atdnvo_c.pth)")
    ap.add_argument("--flow-weights", default=None)
    ap.add_argument("--flows2", action="store_true")
    ap.add_argument("--geometry", default="slam", choices=fb.GEOMETRIES)
    ap.add_argument("--out-dir", default=None, help="default: atdn_vslam/eval/results/<exp>/ATDNVO_c")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    data_path = a.data_path or load_config(a.config).data_path
    dev = torch.device(a.device)
    cfg = Config(data_path=data_path, train_sequences=[a.sequence])
    bank = build_bank(cfg, dev, flow_weights=a.flow_weights, flows2=a.flows2, geometry=a.geometry)
    weights = a.weights or os.path.join("atdn_vslam", "checkpoints", "%d_%d_atdnvo_c.pth" % (a.exp, a.stage))
    head = ATDNVO()
    head.load_state_dict(torch.load(weights, map_location="cpu"))
    head = head.to(dev).eval()
    gt_file = os.path.join(data_path, "dataset", "poses", a.sequence + ".txt")
    gt = np.loadtxt(gt_file).reshape(-1, 12) if os.path.exists(gt_file) else None
    out_dir = a.out_dir or os.path.join("atdn_vslam", "eval", "results", str(a.exp), "ATDNVO_c")
    runs = evaluate(head, bank, a.sequence, a.exp, a.forward, out_dir, gt_poses=gt)
    if "metrics" in runs:
        print(json.dumps(runs["metrics"]))


if __name__ == "__main__":
    main()
