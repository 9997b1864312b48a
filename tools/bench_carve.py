"""Timing of the visibility votes and the carving (atdn_voxel_votes / atdn_voxel_remove, csrc/carve.hip) on one GPU. The synthetic
street of tools/bench_voxel_map.py; nothing is read from outside the tree. Every leg runs in a child process of its own
(`--leg`), with its own time limit; the parent only starts the children, collects their JSON lines and stops at the first leg
that fails.

    python tools/bench_carve.py [--reps 20] [--out profiles/carve_bench.json]

Legs: 376 x 1232, K = 16 and 64 keyframes one metre apart, the map of all K keyframes at the defaults of VoxelMap (0.25 m, 0.5
to 40 m, stride 1), the votes' defaults (rel 0.05, abs_tol one voxel, radius 1). Per leg, by device events, medians over `reps`:

votes      atdn_voxel_votes of every voxel against all K keyframes in one call with accumulate = 0 (the clear and the kernel).
batched    VoxelMap.votes: the extraction, then the keyframes eight at a time with accumulate = 1.
carve      the whole VoxelMap.carve(min_free=2): extraction, votes, the decision in torch, the removal and its one
           synchronisation; the table is restored outside the events.
baseline   the same votes with stock torch ops on the device — float64 elementwise, nine gathers — what a user would write
           without the kernel.
host       the library's host form on CPU tensors, one thread, wall clock, once.

Every leg checks the kernel's votes, the batched votes and the baseline's against the host form in every bit, and the carved
cloud against the host form's, and fails otherwise. No time is asserted anywhere.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from atdn_vslam_amd import _lib  # noqa: E402
from atdn_vslam_amd.voxel_map import VoxelMap  # noqa: E402
from bench_voxel_map import CALIB, GRID, H, W, _median_us, _scene  # noqa: E402

THRESHOLDS = dict(near=GRID["min_z"], far=GRID["max_z"], rel=0.05, abs_tol=GRID["voxel"], radius=1)
LEGS = (16, 64)
LEG_TIMEOUT = 420


def torch_votes(points, depth, poses, near, far, rel, abs_tol, radius):
    """The rule with stock torch ops on the device: votes [M,3] int32."""
    fx, fy, cx, cy = CALIB
    p = points.double()
    votes = torch.zeros((p.shape[0], 3), dtype=torch.int32, device=p.device)
    for k in range(depth.shape[0]):
        P = poses[k].double()
        d = [p[:, 0] - P[3], p[:, 1] - P[7], p[:, 2] - P[11]]
        c = [(P[a] * d[0] + P[4 + a] * d[1]) + P[8 + a] * d[2] for a in range(3)]
        z = c[2]
        a = ((c[0] / z) * fx + cx) + 0.5
        b = ((c[1] / z) * fy + cy) + 0.5
        view = (z >= near) & (z <= far) & (a >= radius) & (a < W - radius) & (b >= radius) & (b < H - radius)
        x = torch.where(view, a, torch.full_like(a, radius)).long()
        y = torch.where(view, b, torch.full_like(b, radius)).long()
        band = rel * z + abs_tol
        lo, hi = z - band, z + band
        D = depth[k].double()
        m = D[y, x]
        support = view & (m >= near) & (m <= far) & (lo <= m) & (m <= hi)
        free = view.clone()
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                w = D[y + dy, x + dx]
                free &= (w >= near) & (w <= far) & (w > hi)
        votes += torch.stack([view, support, free], dim=1).int()
    return votes


def leg(K, reps):
    import ctypes as C
    dev = torch.device("cuda:0")
    depth, poses, images = _scene(K, dev)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    vm = VoxelMap(dev, **GRID)
    for a in range(0, K, 8):                                             # eight keyframes per call, as KeyframeMap.voxel_map does
        vm.integrate(depth, poses, CALIB, images=images, indices=list(range(a, min(a + 8, K))))
    points, _, _, keys = vm.extract()
    M = int(points.shape[0])
    points = points.contiguous()
    votes = torch.empty((M, 3), dtype=torch.int32, device=dev)
    th = (THRESHOLDS["near"], THRESHOLDS["far"], THRESHOLDS["rel"], THRESHOLDS["abs_tol"], THRESHOLDS["radius"])

    def run():
        _lib.check(L.atdn_voxel_votes(p(points), M, p(depth), p(poses), None, K, K, H, W, *CALIB, *th, 0, p(votes), stream()))

    run()
    vote_us = _median_us(run, reps)
    batched_us = _median_us(lambda: vm.votes(depth, poses, CALIB), reps)
    batched = vm.votes(depth, poses, CALIB)[1]
    base_us = _median_us(lambda: torch_votes(points, depth, poses, *th), max(1, reps // 4))
    base = torch_votes(points, depth, poses, *th)
    pristine = vm.table.clone()
    report = {}

    def carve():
        report.update(vm.carve(depth, poses, CALIB, min_free=2))

    carve_us = _median_us(carve, reps, before=lambda: vm.table.copy_(pristine))
    carved = vm.extract()
    # the host form
    hm = VoxelMap("cpu", capacity=vm.capacity, **GRID)
    hm.table.copy_(pristine.cpu())
    hm._counts, hm.has_colors = vm.counts, True
    t0 = time.perf_counter()
    from atdn_vslam_amd.transforms import visibility_votes
    host = visibility_votes(points.cpu(), depth.cpu(), poses.cpu(), CALIB, **THRESHOLDS)
    host_ms = (time.perf_counter() - t0) * 1e3
    host_report = hm.carve(depth.cpu(), poses.cpu(), CALIB, min_free=2)
    same = {"votes": torch.equal(votes.cpu(), host), "batched": torch.equal(batched.cpu(), host), "baseline": torch.equal(base.cpu(), host),
            "carve": host_report == report and all(torch.equal(a.cpu(), b) for a, b in zip(carved, hm.extract()))}
    if not all(same.values()):
        raise SystemExit("K=%d: not the host form's bits: %s" % (K, same))
    pairs = M * K
    in_view = int(host[:, 0].sum())
    row = {"K": K, "H": H, "W": W, "voxels": M, "pairs": pairs, "pairs_in_view": in_view, "thresholds": THRESHOLDS, "launches": reps,
           "votes_us": round(vote_us[0], 1), "votes_us_min_max": [round(vote_us[1], 1), round(vote_us[2], 1)],
           "pairs_per_s": round(pairs / (vote_us[0] * 1e-6), 0), "ns_per_pair": round(vote_us[0] * 1e3 / pairs, 4),
           "batched_votes_us": round(batched_us[0], 1), "carve_us": round(carve_us[0], 1),
           "carve_us_min_max": [round(carve_us[1], 1), round(carve_us[2], 1)], "carve_report": report,
           "baseline_torch_us": round(base_us[0], 1), "baseline_over_votes": round(base_us[0] / vote_us[0], 1),
           "host_form_ms": round(host_ms, 1), "host_over_votes": round(host_ms * 1e3 / vote_us[0], 1), "same_bits_as_host_form": same}
    print(json.dumps(row), flush=True)


def _child(K, a):
    """Run one leg in a fresh process under its own time limit; its last output line is the leg's JSON."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", str(K), "--reps", str(a.reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_TIMEOUT)
    if r.returncode != 0:
        raise SystemExit("leg K=%d failed with status %d" % (K, r.returncode))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leg", type=int, default=None, help="internal: K — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carve_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_carve.py needs a GPU: nothing is measured without one")
    if a.leg:
        leg(a.leg, a.reps)
        return
    res = {"device": torch.cuda.get_device_name(0), "grid": GRID, "legs": [_child(K, a) for K in LEGS]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
