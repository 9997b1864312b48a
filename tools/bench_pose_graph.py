"""Timing and accuracy of pose-graph optimisation (atdn_pose_graph_solve, csrc/pose_graph.hip) on one GPU, against the host form
of the same rule on the same machine in the same run. Seeded scenes; nothing is read from outside the tree.

    python tools/bench_pose_graph.py [--reps 20] [--out profiles/pose_graph_bench.json]

Scene: a ring driven twice, N nodes about 1 m apart; odometry edges with 0.5 mrad / 5 mm of noise per step plus the same again as
a constant bias, the start the chain of those measurements (the drift); on the second lap every 32nd node has a loop edge to the
node that stood at the same place on the first lap (1 mrad / 10 mm of noise), under the Geman-McClure loss. N in {64, 256, 1024},
B in {1, 64} (B copies of the graph, each its own workgroup). Per call — three solves of 10 steps each, robust scales 1000, 30 and 5
in turn (the drift is far beyond the last scale, where every loop edge would saturate), cg_iters 64, cg_tol 1e-8 —: the kernel by device
events, the median of `reps` calls after a warm-up; the host form by the host clock, the median of `reps` calls (of 3 where one call
takes more than 2 s: the host form solves the B graphs one after the other). ATE (evaluation.ate_rmse, SE(3)-aligned) of the start
and of the result. No time is asserted anywhere: the reason for the device form is residency, capture and the batch; for B = 1
the host form may well be faster."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from atdn_vslam_amd import evaluation, transforms  # noqa: E402

DEV = torch.device("cuda:0")
ODOMETRY_SIGMA, LOOP_SIGMA, ROBUST_SCALE = (1e-3, 1e-2), (1e-2, 1e-1), (1000.0, 30.0, 5.0)


def _rot(v):
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def scene(N, seed=1):
    """-> (start [N,4,4], edge_index [2,E], edge_pose [E,4,4], edge_weight [E,2], edge_robust [E], truth [N,4,4]) host tensors"""
    rs = np.random.RandomState(seed)
    lap = N // 2
    radius = lap / (2.0 * np.pi)
    truth = np.stack([_T(_rot([0.0, a, 0.0]), [radius * np.sin(a), 0.0, radius * np.cos(a)])
                      for a in 2.0 * np.pi * np.arange(N) / lap])
    bias_r, bias_t = rs.normal(size=3) * 5e-4, rs.normal(size=3) * 5e-3
    pairs = [(k, k + 1) for k in range(N - 1)] + [(k, k - lap) for k in range(lap, N, 32)]
    meas, start = [], [truth[0]]
    for n, (i, j) in enumerate(pairs):
        chain = n < N - 1
        noise = _T(_rot(rs.normal(size=3) * 5e-4 + bias_r), rs.normal(size=3) * 5e-3 + bias_t) if chain else \
            _T(_rot(rs.normal(size=3) * 1e-3), rs.normal(size=3) * 1e-2)
        meas.append(np.linalg.inv(truth[i]) @ truth[j] @ noise)
        if chain:
            start.append(start[-1] @ meas[-1])
    L = len(pairs) - (N - 1)
    weight = [[1.0 / ODOMETRY_SIGMA[0] ** 2, 1.0 / ODOMETRY_SIGMA[1] ** 2]] * (N - 1) + \
             [[1.0 / LOOP_SIGMA[0] ** 2, 1.0 / LOOP_SIGMA[1] ** 2]] * L
    return (torch.from_numpy(np.stack(start)).float(), torch.tensor(pairs, dtype=torch.int32).t().contiguous(),
            torch.from_numpy(np.stack(meas)).float(), torch.tensor(weight, dtype=torch.float64),
            torch.tensor([0] * (N - 1) + [1] * L, dtype=torch.uint8), truth)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(20, a.reps)
    rows = []
    for N in (64, 256, 1024):
        start, index, meas, weight, robust, truth = scene(N)
        for B in (1, 64):
            host = [t[None].repeat((B,) + (1,) * t.dim()).contiguous() for t in (start, index, meas, weight, robust)]
            dev = [t.to(DEV) for t in host]
            solve = lambda args: transforms.pose_graph_optimize(*args, robust_scale=ROBUST_SCALE, iters=10)   # noqa: E731
            out_dev = solve(dev)                                       # warm-up
            torch.cuda.synchronize()
            times = []
            for _ in range(reps):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                solve(dev)
                ev[1].record()
                torch.cuda.synchronize()
                times.append(ev[0].elapsed_time(ev[1]))
            t0 = time.perf_counter()
            out_host = solve(host)
            first = time.perf_counter() - t0
            host_reps = reps if first <= 2.0 else 3
            htimes = []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                solve(host)
                htimes.append((time.perf_counter() - t0) * 1e3)
            same = all(torch.equal(x.cpu(), y) for x, y in zip(out_dev, out_host))
            poses = out_host[0][0].numpy().astype(np.float64)
            row = dict(N=N, E=int(index.shape[1]), B=B, device_ms=round(statistics.median(times), 3),
                       device_ms_min=round(min(times), 3), device_ms_max=round(max(times), 3), device_reps=reps,
                       host_ms=round(statistics.median(htimes), 3), host_reps=host_reps, same_bits=bool(same),
                       accepted_steps=int(out_host[3][0, 2]), cg_iterations=int(out_host[3][0, 3]),
                       cost_before=float(out_host[1][0, 0]), cost_after=float(out_host[1][0, 1]),
                       ate_before_m=round(evaluation.ate_rmse(start.numpy().astype(np.float64), truth), 4),
                       ate_after_m=round(evaluation.ate_rmse(poses, truth), 4))
            print(json.dumps(row), flush=True)
            rows.append(row)
    result = dict(device=torch.cuda.get_device_name(0), launches_per_call=len(ROBUST_SCALE), iters=10, cg_iters=64, cg_tol=1e-8, robust_scale=ROBUST_SCALE, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
