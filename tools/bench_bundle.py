"""Timing and accuracy of the windowed bundle adjustment (atdn_bundle_adjust, csrc/bundle.hip) on one GPU. The synthetic drive
of tools/bench_multiview.py (closed forms; nothing is read from outside the tree) with deterministic pose errors of up to
0.004 rad, 3 % and 0.03 m. Every leg runs in a child process of its own (`--leg`), with its own time limit; the parent only
starts the children and collects their JSON lines.

    python tools/bench_bundle.py [--reps 20] [--out profiles/bundle_bench.json]

Legs: 376 x 1232, B = 1, S = 16, iters = 8, stride 1, 2 and 4. Per leg:

solve     `transforms.bundle_adjust` by device events over `reps` solves in five rounds, the median; 18 launches per solve.
terms     `transforms.bundle_terms` (one evaluation: the terms kernel and the ordered sum) likewise.
host      the library's host form on CPU tensors, one thread, wall clock, one call; whether it gives the same bits.
accuracy  per view the rotation error (rad) and the translation error (m, in the held gauge: the poses scaled so that the held
          coordinate agrees with the truth) before and after, medians and maxima; and the median relative depth error of
          `transforms.multiview_depth` over its valid pixels with the initial and with the refined poses (depths scaled by the same
          gauge factor).
No time and no accuracy is asserted anywhere.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from atdn_vslam_amd import transforms  # noqa: E402
from bench_multiview import CALIB, H, W, _events, _scene  # noqa: E402

ROUNDS = 5
S, ITERS = 16, 8
STRIDES = (1, 2, 4)
LEG_TIMEOUT = 900
OPTIONS = dict(scale_px=4.0, inlier_px=2.0, min_z=0.1, min_views=2)


def _perturb(poses):
    """poses [N,12] float32 (host) with deterministic errors: up to 0.004 rad per axis, 3 % of scale, 0.03 m per axis."""
    out = []
    for k, row in enumerate(poses.double()):
        M = row.view(3, 4)
        a = [0.004 * math.sin(1.1 * k + 0.3 + 2.1 * i) for i in range(3)]
        K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
        R = torch.linalg.matrix_exp(K) @ M[:, :3]
        t = M[:, 3] * (1.0 + 0.03 * math.cos(0.9 * k + 1.0)) + torch.tensor([0.03 * math.sin(0.5 * k + i) for i in range(3)])
        out.append(torch.cat([R, t.view(3, 1)], dim=1).reshape(12))
    return torch.stack(out).float()


def _internal(row):
    M = row.double().view(3, 4)
    return M[:, :3].t(), -(M[:, :3].t() @ M[:, 3])


def _errors(got, true):
    """(rotation errors [S] rad, translation errors [S] m in the held gauge, the gauge factor)"""
    rg, tg = zip(*[_internal(p) for p in got])
    rt, tt = zip(*[_internal(p) for p in true])
    j = int(tt[-1].abs().argmax())
    k = float(tt[-1][j] / tg[-1][j])
    rot = [float(torch.linalg.norm(a.t() @ b - torch.eye(3, dtype=torch.float64)) / math.sqrt(2.0)) for a, b in zip(rg, rt)]
    tr = [float(torch.linalg.norm(a * k - b)) for a, b in zip(tg, tt)]
    return torch.tensor(rot), torch.tensor(tr), k


def leg(stride, reps):
    dev = torch.device("cuda:0")
    acc, alive, true_poses, init = _scene(dev)
    poses = _perturb(true_poses.cpu()).to(dev)
    slots = torch.arange(S, dtype=torch.int32, device=dev)[None]
    Z = None

    def solve():
        return transforms.bundle_adjust(acc, alive, poses, slots, CALIB, init, stride=stride, iters=ITERS, **OPTIONS)

    def terms():
        return transforms.bundle_terms(acc, alive, poses, slots, CALIB, init, stride=stride, **OPTIONS)

    for _ in range(2):
        solve()
        terms()
    per = max(1, reps // ROUNDS)
    ts, tt = [], []
    for _ in range(ROUNDS):
        ts.append(_events(solve, per))
        tt.append(_events(terms, per))
    out_poses, depth, cost, counts = solve()
    cpu = [t.cpu() for t in (acc, alive, poses, slots, init)]
    t0 = time.perf_counter()
    host = transforms.bundle_adjust(cpu[0], cpu[1], cpu[2], cpu[3], CALIB, cpu[4], stride=stride, iters=ITERS, **OPTIONS)
    host_s = time.perf_counter() - t0
    same = all(torch.equal(h.contiguous().view(torch.uint8), d.cpu().contiguous().view(torch.uint8))
               for h, d in zip(host, (out_poses, depth, cost, counts)))
    r0, t0e, k0 = _errors(poses.cpu(), true_poses.cpu())
    r1, t1e, k1 = _errors(out_poses[0].cpu(), true_poses.cpu())
    # the multi-view depth against the initial and the refined poses, both in their gauge
    ref_depth = transforms.multiview_depth(acc, alive, true_poses, slots, CALIB, depth_init=init)[0]
    err = []
    for p, k in ((poses, k0), (out_poses[0].contiguous(), k1)):
        d = transforms.multiview_depth(acc, alive, p, slots, CALIB, depth_init=init)[0]
        ok = (d > 0) & (ref_depth > 0)
        err.append(float(((d.double() * k - ref_depth.double()).abs() / ref_depth.double())[ok].median()))
    n_cand = int(counts[0, 0])
    ms = sorted(ts)[ROUNDS // 2]
    row = {"stride": stride, "S": S, "iters": ITERS, "B": 1, "H": H, "W": W, "solves": per * ROUNDS, "candidates": n_cand,
           "counts": counts[0].tolist(), "cost": cost[0].tolist(),
           "solve_ms": round(ms, 4), "solve_ms_min_max": [round(min(ts), 4), round(max(ts), 4)],
           "terms_ms": round(sorted(tt)[ROUNDS // 2], 4), "terms_ms_min_max": [round(min(tt), 4), round(max(tt), 4)],
           "ns_per_candidate_evaluation": round(ms * 1e6 / (max(n_cand, 1) * (ITERS + 1)), 3),
           "workspace_mib": round(transforms._lib.lib().atdn_bundle_workspace_bytes(1, S, H, W, stride) / 2 ** 20, 2),
           "host_form_s": round(host_s, 3), "host_over_kernel": round(host_s * 1e3 / ms, 1), "host_form_same_bits": bool(same),
           "rot_err_median_before_after": [float(r0.median()), float(r1.median())],
           "rot_err_max_before_after": [float(r0.max()), float(r1.max())],
           "tr_err_median_before_after": [float(t0e.median()), float(t1e.median())],
           "tr_err_max_before_after": [float(t0e.max()), float(t1e.max())],
           "multiview_median_rel_depth_error_initial_refined": err}
    print(json.dumps(row), flush=True)


def _child(what, a):
    """Run one leg in a fresh process under its own time limit; its last output line is the leg's JSON."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", what, "--reps", str(a.reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_TIMEOUT)
    if r.returncode != 0:
        raise SystemExit("leg %s failed with status %d" % (what, r.returncode))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leg", default=None, help="internal: the stride — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bundle.py needs a GPU: nothing is measured without one")
    if a.leg:
        leg(int(a.leg), a.reps)
        return
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "options": OPTIONS,
           "legs": [_child(str(s), a) for s in STRIDES[::-1]]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
