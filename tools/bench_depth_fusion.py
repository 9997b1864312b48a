"""Timing of the keyframe depth-fusion kernel (atdn_depth_fuse, csrc/depth_fusion.hip) on one GPU. A synthetic scene from closed
forms; nothing is read from outside the tree. Every timing leg runs in a child process of its own (`--leg`), with its own time
limit, so no leg inherits another's allocator state or clocks; the parent only starts the children and collects their JSON lines.

    python tools/bench_depth_fusion.py [--reps 200] [--out profiles/depth_fusion_bench.json]

Legs: 376 x 1232, a map of 24 keyframes (a forward drive over a ground plane between two walls, 10 % holes, a 0.2 % smooth
disturbance), B = 1 and 16 targets, S = 2, 4, 8 sources per target (the nearest neighbours on both sides). Per leg, by device
events over `reps` launches in five rounds, medians:

kernel    `transforms.fuse_depths` (memset + kernel per launch, as a caller issues it).
baseline  the same computation written with stock torch ops on the device in float32 — `grid_sample` for the bilinear reads (of
          the depth and of its validity), element-wise ops for the two projections and the tests, one pass per source slot —,
          which is what a user would write without this kernel. It is float32 and its hole test is a threshold on an interpolated
          validity, so it is not bit-equal to the rule; the share of pixels on which its `kept` agrees with the kernel's is
          reported, not asserted. It runs reps / 10 times per round.

bytes: what a launch must move at least — 4 read + 5 written per target pixel, and 4 per target pixel and source for the taps
(each tap line counted once; neighbouring pixels share them and targets share source planes, so the true traffic is lower).
No time is asserted anywhere.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from atdn_vslam_amd import depth as depth_mod, transforms  # noqa: E402

ROUNDS = 5
H, W, N = 376, 1232, 24
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))
THRESHOLDS = dict(max_reproj=1.0, max_rel_depth=0.01, min_views=2, min_z=0.1)
LEGS = [(B, S) for B in (1, 16) for S in (2, 4, 8)]
LEG_TIMEOUT = 240


def _events(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _scene(dev):
    """(bank [N,H,W] float32, poses [N,12] float32) on the device: the ground Y = 1.65, walls X = -5 and X = 6, a front wall
    Z = 80; keyframe k stands at z = 0.8 k with a small yaw and side step."""
    g = torch.Generator(device="cpu").manual_seed(11)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), device=dev, dtype=torch.float64),
                          torch.arange(float(W), device=dev, dtype=torch.float64), indexing="ij")
    a = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)])
    bank, poses = [], []
    for k in range(N):
        yaw, side = 0.01 * float(torch.sin(torch.tensor(0.7 * k))), 0.05 * float(torch.cos(torch.tensor(1.3 * k)))
        R = torch.tensor([[1.0, 0.0, yaw], [0.0, 1.0, 0.0], [-yaw, 0.0, 1.0]], dtype=torch.float32)
        t = torch.tensor([side, 0.0, 0.8 * k], dtype=torch.float32)
        d = torch.einsum("ij,jhw->ihw", R.double().to(dev), a)
        best = torch.full((H, W), float("inf"), dtype=torch.float64, device=dev)
        for axis, level in ((1, 1.65), (0, -5.0), (0, 6.0), (2, 80.0)):
            s = (level - float(t[axis])) / d[axis]
            best = torch.where((s > 0) & torch.isfinite(s) & (s < best), s, best)
        best = best * (1.0 + 0.002 * torch.sin(6.28 * (1.3 * x / W + 0.7 * y / H) + 0.9 * k))
        holes = (torch.rand((H, W), generator=g) < 0.1).to(dev)
        bank.append(torch.where(holes, torch.zeros_like(best), best).float())
        poses.append(torch.cat([R, t.view(3, 1)], dim=1).reshape(12))
    return torch.stack(bank).contiguous(), torch.stack(poses).to(dev).contiguous()


def _lists(B, S):
    """B targets from the middle of the map, each with its S nearest neighbours, S / 2 on either side."""
    first = (N - B) // 2
    targets = list(range(first, first + B))
    offsets = [d for d in range(-(S // 2), S // 2 + 1) if d != 0]
    return targets, [[k + d for d in offsets] for k in targets]


def torch_fuse(bank, poses, targets, sources, calib, max_reproj, max_rel_depth, min_views, min_z):
    """The rule with stock torch ops in float32 (see the module docstring): (fused [B,1,H,W], views [B,H,W] uint8)."""
    fx, fy, cx, cy = calib
    dev = bank.device
    t_ix = torch.as_tensor(targets, device=dev)
    s_ix = torch.as_tensor(sources, device=dev)
    B, S = s_ix.shape
    y, x = torch.meshgrid(torch.arange(float(H), device=dev), torch.arange(float(W), device=dev), indexing="ij")
    P = poses.view(-1, 3, 4)
    z = bank[t_ix]                                                   # [B,H,W]
    has = z > 0
    X = torch.stack([z * ((x - cx) / fx), z * ((y - cy) / fy), z], dim=1)          # [B,3,H,W]
    n = torch.zeros_like(z)
    zsum = z.clone()
    valid = (bank > 0).float()
    for s in range(S):
        j = s_ix[:, s]
        Ri, ti, Rj, tj = P[t_ix, :, :3], P[t_ix, :, 3], P[j, :, :3], P[j, :, 3]
        R = Rj.transpose(1, 2) @ Ri
        t = (Rj.transpose(1, 2) @ (ti - tj).unsqueeze(2))
        Xs = torch.einsum("bij,bjhw->bihw", R, X) + t.view(B, 3, 1, 1)
        u, v = fx * (Xs[:, 0] / Xs[:, 2]) + cx, fy * (Xs[:, 1] / Xs[:, 2]) + cy
        grid = torch.stack([2.0 * u / (W - 1) - 1.0, 2.0 * v / (H - 1) - 1.0], dim=3)
        ds = F.grid_sample(bank[j].unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        full = F.grid_sample(valid[j].unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]
        ok = has & (Xs[:, 2] >= min_z) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (full > 0.9999)
        Y = torch.stack([ds * ((u - cx) / fx), ds * ((v - cy) / fy), ds], dim=1) - t.view(B, 3, 1, 1)
        Yt = torch.einsum("bji,bjhw->bihw", R, Y)
        xr, yr = fx * (Yt[:, 0] / Yt[:, 2]) + cx, fy * (Yt[:, 1] / Yt[:, 2]) + cy
        e2 = (xr - x) ** 2 + (yr - y) ** 2
        rd = (Yt[:, 2] - z).abs() / z
        consistent = ok & (Yt[:, 2] >= min_z) & (e2 <= max_reproj * max_reproj) & (rd <= max_rel_depth)
        n = n + consistent
        zsum = torch.where(consistent, zsum + Yt[:, 2], zsum)
    kept = has & (n >= min_views)
    return torch.where(kept, zsum / (n + 1), torch.zeros_like(z)).unsqueeze(1), n.to(torch.uint8)


def leg(B, S, reps):
    dev = torch.device("cuda:0")
    bank, poses = _scene(dev)
    targets, sources = _lists(B, S)
    dt = torch.tensor(targets, dtype=torch.int32, device=dev)
    ds = torch.tensor(sources, dtype=torch.int32, device=dev)

    def kernel():
        return transforms.fuse_depths(bank, poses, dt, ds, CALIB, **THRESHOLDS)

    def baseline():
        return torch_fuse(bank, poses, targets, sources, CALIB, **THRESHOLDS)

    for _ in range(3):
        kernel()
        baseline()
    per_k, per_b = max(1, reps // ROUNDS), max(1, reps // ROUNDS // 10)
    tk, tb = [], []
    for _ in range(ROUNDS):
        tk.append(_events(kernel, per_k))
        tb.append(_events(baseline, per_b))
    n = B * H * W
    nbytes = n * 9 + n * S * 4
    ms_k, ms_b = sorted(tk)[ROUNDS // 2], sorted(tb)[ROUNDS // 2]
    fused, views, counts = kernel()
    bf, _ = baseline()
    agree = float(((fused > 0) == (bf > 0)).float().mean())
    row = {"B": B, "S": S, "H": H, "W": W, "N": N, "launches": per_k * ROUNDS, "baseline_launches": per_b * ROUNDS, "bytes": nbytes,
           "kernel_us": round(ms_k * 1e3, 2), "kernel_us_min_max": [round(min(tk) * 1e3, 2), round(max(tk) * 1e3, 2)],
           "baseline_torch_fp32_us": round(ms_b * 1e3, 2),
           "baseline_us_min_max": [round(min(tb) * 1e3, 2), round(max(tb) * 1e3, 2)],
           "baseline_over_kernel": round(ms_b / ms_k, 2), "kernel_tbps_of_min_bytes": round(nbytes / (ms_k * 1e-3) / 1e12, 4),
           "ns_per_pixel_and_source": round(ms_k * 1e6 / (n * S), 4), "counts": counts[:2].tolist(),
           "baseline_kept_agreement": round(agree, 5)}
    print(json.dumps(row), flush=True)


def _child(B, S, a):
    """Run one leg in a fresh process under its own time limit; its last output line is the leg's JSON."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "%d,%d" % (B, S), "--reps", str(a.reps)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LEG_TIMEOUT)
    if r.returncode != 0:
        raise SystemExit("leg B=%d S=%d failed with status %d" % (B, S, r.returncode))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--leg", default=None, help="internal: B,S — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_fusion.py needs a GPU: nothing is measured without one")
    if a.leg:
        B, S = (int(v) for v in a.leg.split(","))
        leg(B, S, a.reps)
        return
    name = torch.cuda.get_device_name(0)
    res = {"device": name, "rounds": ROUNDS, "thresholds": THRESHOLDS, "legs": [_child(B, S, a) for B, S in LEGS]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
