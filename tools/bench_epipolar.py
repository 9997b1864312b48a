"""Timing of pose-from-flow (atdn_epipolar_terms / atdn_epipolar_solve, csrc/epipolar.hip) on one GPU, with pose-from-depth
(atdn_pnp_terms / atdn_pnp_solve) at the same size in the same process as the yardstick. Synthetic scenes from seeds; nothing is
read from outside the tree.

    python tools/bench_epipolar.py [--reps 400] [--out profiles/epipolar_bench.json]

Every timing runs in a child process of its own (`--leg`), so that no leg inherits another's allocator or clocks:
kernel B: one evaluation (`transforms.epipolar_terms`: the terms kernel and the order-fixed sum, two launches) and the 16-step solve
    (`transforms.pose_from_flow`: 34 launches) at 376 x 1232, B = 1 and 16, by device events over `reps` calls in five rounds after
    a warm-up, alternating round by round with `transforms.reprojection_terms` / `pose_from_depth` on the same scene (the same 28
    sums through the same tree; 13 bytes per pixel instead of 9). Per call: microseconds, microseconds per launch, the bytes an
    evaluation must move and the ratio to the yardstick. Back-to-back calls re-read the same buffers from the Infinity Cache, so
    these are the kernels' own rates, not HBM's.
host: the host form (CPU tensors, one thread) at 376 x 1232, B = 1, by the host clock.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from atdn_vslam_amd import transforms  # noqa: E402

ROUNDS = 5
ITERS = 16
H, W = 376, 1232


def _direction_error_deg(a, b):
    cross = torch.linalg.cross(a, b).norm(dim=1)
    return torch.rad2deg(torch.atan2(cross, (a * b).sum(dim=1)))


def leg_kernel(B, reps):
    from bench_pnp import CALIB, _events, _scene
    depth, flow, mask, pose, start = _scene(B)
    calls = {
        "terms": lambda: transforms.epipolar_terms(flow, start, CALIB, mask),
        "solve": lambda: transforms.pose_from_flow(flow, start, CALIB, mask, iters=ITERS),
        "pnp_terms": lambda: transforms.reprojection_terms(depth, flow, start, CALIB, mask),
        "pnp_solve": lambda: transforms.pose_from_depth(depth, flow, start, CALIB, mask, iters=ITERS),
    }
    for _ in range(5):
        for fn in calls.values():
            fn()
    per = max(1, reps // ROUNDS)
    ev = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ev[k].append(_events(fn, per if k.endswith("terms") else max(1, per // 8)))
    n = B * H * W
    row = {"B": B, "H": H, "W": W, "calls": per * ROUNDS, "solve_iters": ITERS}
    for name, launches, per_pixel in (("terms", 2, 9), ("solve", 2 * (ITERS + 1), 9 * (ITERS + 1)), ("pnp_terms", 2, 13),
                                      ("pnp_solve", 2 * (ITERS + 1), 13 * (ITERS + 1))):
        ms = sorted(ev[name])[len(ev[name]) // 2]
        row[name] = {"launches": launches, "bytes": n * per_pixel, "us_events": round(ms * 1e3, 3),
                     "us_events_min": round(min(ev[name]) * 1e3, 3), "us_events_max": round(max(ev[name]) * 1e3, 3),
                     "us_per_launch": round(ms * 1e3 / launches, 3), "tbps": round(n * per_pixel / (ms * 1e-3) / 1e12, 3)}
    row["terms_over_pnp_terms"] = round(row["terms"]["us_events"] / row["pnp_terms"]["us_events"], 3)
    row["solve_over_pnp_solve"] = round(row["solve"]["us_events"] / row["pnp_solve"]["us_events"], 3)
    row["solve_over_evaluations"] = round(row["solve"]["us_events"] / ((ITERS + 1) * row["terms"]["us_events"]), 2)
    got, cost, counts = calls["solve"]()
    true_t, start_t = pose.view(B, 3, 4)[:, :, 3], start.view(B, 3, 4)[:, :, 3]
    row["counts"] = counts[:2].tolist()
    row["direction_error_deg_start"] = [round(float(e), 4) for e in _direction_error_deg(start_t, true_t)[:2].tolist()]
    row["direction_error_deg"] = [round(float(e), 4) for e in _direction_error_deg(got[:, :3, 3], true_t)[:2].tolist()]
    row["rotation_error_max_abs"] = [round(float(e), 7) for e in
                                     (got[:, :3, :3] - pose.view(B, 3, 4)[:, :, :3]).abs().amax(dim=(1, 2))[:2].tolist()]
    return row


def leg_host(reps):
    from bench_pnp import CALIB, _scene
    depth, flow, mask, pose, start = (t.cpu() for t in _scene(1))
    torch.set_num_threads(1)
    out = {"B": 1, "H": H, "W": W, "solve_iters": ITERS}
    for name, fn, n in (("terms", lambda: transforms.epipolar_terms(flow, start, CALIB, mask), 3),
                        ("solve", lambda: transforms.pose_from_flow(flow, start, CALIB, mask, iters=ITERS), 2)):
        fn()
        times = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"] = round(sorted(times)[len(times) // 2], 3)
    return out


def _child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("bench_epipolar.py: leg %s failed with status %d" % (args, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--leg", choices=["kernel", "host"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "epipolar_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epipolar.py needs a GPU: nothing is measured without one")
    if a.leg == "kernel":
        print(json.dumps(leg_kernel(a.batch, a.reps)), flush=True)
        return
    if a.leg == "host":
        print(json.dumps(leg_host(a.reps)), flush=True)
        return
    res = {"device": torch.cuda.get_device_name(0), "kernel": [], "host": None}
    for B in (1, 16):
        res["kernel"].append(_child(["--leg", "kernel", "--batch", str(B), "--reps", str(a.reps)]))
        print(json.dumps(res["kernel"][-1]), flush=True)
    res["host"] = _child(["--leg", "host"])
    print(json.dumps(res["host"]), flush=True)
    k1 = res["kernel"][0]
    res["host_over_device_solve_b1"] = round(res["host"]["solve_ms"] * 1e3 / k1["solve"]["us_events"], 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
