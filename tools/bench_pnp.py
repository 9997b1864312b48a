"""Timing of pose-from-depth (atdn_pnp_terms / atdn_pnp_solve, csrc/pnp.hip) on one GPU. Synthetic scenes and weights from
seeds; nothing is read from outside the tree.

    python tools/bench_pnp.py [--reps 400] [--queries 12] [--out profiles/pnp_bench.json]

kernel: one evaluation (`transforms.reprojection_terms`: the terms kernel and the order-fixed sum, two launches) and the
16-step solve (`transforms.pose_from_depth`: 34 launches) at 376 x 1232, B = 1 and 16, by device events over `reps` calls in five
rounds, with `atdn_flow_two_view_depth` — a streaming kernel of the same frame — timed in the same process, alternating round by
round, as the yardstick. Per call: microseconds, microseconds per launch, the bytes an evaluation must move (13 per pixel: depth,
two planes of flow, mask; the two-view kernel: 12) and the ratio of one evaluation to the yardstick per byte moved. Back-to-back
calls re-read the same buffers from the Infinity Cache, so these are the kernels' own rates, not HBM's.

relocalize: `NeuralSLAM.relocalize_batch(verify=True)` with and without `geometric=True` on a three-keyframe map whose keyframes
all have a (synthetic) depth, two queries, top_k = 3 (six pairs), the two alternating call by call (host clock, every call ends
with its results on the host); synthetic weights.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from atdn_vslam_amd import depth as depth_mod, synthetic as syn, transforms  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 5
ITERS = 16
H, W = 376, 1232
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))


def _events(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _scene(B):
    """A forward-driving scene on the device: depths of 4 .. 120 m with 20 % holes, a small rotation, t = (0.05, -0.02, 1), 10 % of
    the flows off by 25 px; the start is 0.02 rad and 0.3 m off. (depth [B,H,W], flow [B,2,H,W], mask, true pose, start pose)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), device=DEV, dtype=torch.float64),
                          torch.arange(float(W), device=DEV, dtype=torch.float64), indexing="ij")
    depths, flows, poses, starts = [], [], [], []
    for b in range(B):
        Z = 4.0 + 116.0 * (0.5 + 0.5 * torch.cos(6.28 * (x / W * (1 + b % 4) + 0.1 * b))) * (0.5 + 0.5 * torch.cos(3.14 * y / H))
        Z = Z.float().double()
        a, c = 0.01 + 0.001 * b, -0.005
        R = torch.tensor([[1.0, -c, a], [c, 1.0, 0.0], [-a, 0.0, 1.0]], dtype=torch.float64, device=DEV)   # small angles
        t = torch.tensor([0.05, -0.02, 1.0], dtype=torch.float64, device=DEV)
        X1 = torch.stack([Z * (x - cx) / fx, Z * (y - cy) / fy, Z])
        X2 = torch.einsum("ji,jhw->ihw", R, X1 - t.view(3, 1, 1))
        out = torch.rand((H, W), generator=g, device=DEV) < 0.10
        u = fx * X2[0] / X2[2] + cx - x + 25.0 * out
        v = fy * X2[1] / X2[2] + cy - y - 25.0 * out
        hole = torch.rand((H, W), generator=g, device=DEV) < 0.20
        depths.append(torch.where(hole, torch.zeros_like(Z), Z).float())
        flows.append(torch.stack([u, v]).float())
        poses.append(torch.cat([R, t.view(3, 1)], dim=1).reshape(12).float())
        S = torch.tensor([[1.0, 0.0, 0.02], [0.0, 1.0, 0.0], [-0.02, 0.0, 1.0]], dtype=torch.float64, device=DEV) @ R
        starts.append(torch.cat([S, (t + torch.tensor([0.2, -0.1, 0.2], dtype=torch.float64, device=DEV)).view(3, 1)], dim=1).reshape(12).float())
    mask = (torch.rand((B, H, W), generator=g, device=DEV) < 0.9).to(torch.uint8)
    return (torch.stack(depths).contiguous(), torch.stack(flows).contiguous(), mask, torch.stack(poses).contiguous(),
            torch.stack(starts).contiguous())


def leg_kernel(a):
    out = []
    for B in (1, 16):
        depth, flow, mask, pose, start = _scene(B)

        def terms():
            return transforms.reprojection_terms(depth, flow, start, CALIB, mask)

        def solve():
            return transforms.pose_from_depth(depth, flow, start, CALIB, mask, iters=ITERS)

        def two_view():
            return transforms.two_view_depth(flow, pose, CALIB, mask)

        for _ in range(5):
            terms(), solve(), two_view()
        per = max(1, a.reps // ROUNDS)
        ev = {"terms": [], "solve": [], "two_view": []}
        for _ in range(ROUNDS):
            ev["terms"].append(_events(terms, per))
            ev["two_view"].append(_events(two_view, per))
            ev["solve"].append(_events(solve, max(1, per // 8)))
        n = B * H * W
        row = {"B": B, "H": H, "W": W, "calls": per * ROUNDS, "solve_iters": ITERS}
        for name, launches, per_pixel in (("terms", 2, 13), ("solve", 2 * (ITERS + 1), 13 * (ITERS + 1)), ("two_view", 1, 13)):
            ms = sorted(ev[name])[len(ev[name]) // 2]
            row[name] = {"launches": launches, "bytes": n * per_pixel, "us_events": round(ms * 1e3, 3),
                         "us_events_min": round(min(ev[name]) * 1e3, 3), "us_events_max": round(max(ev[name]) * 1e3, 3),
                         "us_per_launch": round(ms * 1e3 / launches, 3), "tbps": round(n * per_pixel / (ms * 1e-3) / 1e12, 3)}
        # (the yardstick with a mask: 8 + 1 read and 4 written per pixel, 13 as well)
        row["terms_over_two_view_per_byte"] = round(
            (row["terms"]["us_events"] / row["terms"]["bytes"]) / (row["two_view"]["us_events"] / row["two_view"]["bytes"]), 2)
        row["solve_over_evaluations"] = round(row["solve"]["us_events"] / ((ITERS + 1) * row["terms"]["us_events"]), 2)
        got, cost, counts = solve()
        err = (got[:, :3, 3] - pose.view(B, 3, 4)[:, :, 3]).norm(dim=1)
        row["counts"] = counts[:2].tolist()
        row["translation_error_m"] = [round(float(e), 6) for e in err[:2].tolist()]
        row["reprojection_score"] = [round(float(s), 4) for s in transforms.reprojection_score(counts)[:2].tolist()]
        print(json.dumps(row), flush=True)
        out.append(row)
        del depth, flow, mask, pose, start
        torch.cuda.empty_cache()
    return out


def leg_relocalize(a):
    from atdn_vslam_amd.slam import NeuralSLAM

    class Args:
        device = "cuda:0"

    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, H, W, seed=8))
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "rgb"))
        os.makedirs(os.path.join(root, "depth"))
        depth = _scene(3)[0].cpu()
        for i in range(3):
            torch.save(frames[i].byte(), os.path.join(root, "rgb", "%06d.pth" % i))
            torch.save(depth[i][None].contiguous(), os.path.join(root, "depth", "%06d.pth" % i))
        poses = torch.eye(4)[:3].reshape(1, 12).repeat(3, 1)
        poses[:, 3] = torch.arange(3.0)
        torch.save(poses, os.path.join(root, "poses.pth"))
        torch.save(vsd, os.path.join(root, "MappingVAE_weights.pth"))
        args = Args()
        args.keyframes_path = root
        slam = NeuralSLAM(args, odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True, calib=CALIB)
        batch = [frames[1].byte().float(), frames[4].byte().float()]
        for _ in range(2):
            slam.relocalize_batch(batch, top_k=3, verify=True)
            slam.relocalize_batch(batch, top_k=3, verify=True, geometric=True)
        times = {"plain": [], "geometric": []}
        for k in range(a.queries):
            order = (("plain", False), ("geometric", True)) if k % 2 == 0 else (("geometric", True), ("plain", False))
            for name, geo in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = slam.relocalize_batch(batch, top_k=3, verify=True, geometric=geo)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
                if geo:
                    geo_counts = out[7].tolist()
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = {"calls": a.queries, "queries": 2, "top_k": 3, "pairs": 6, "ms_per_call_plain": round(med["plain"], 3),
           "ms_per_call_geometric": round(med["geometric"], 3),
           "ms_per_call_plain_min_max": [round(min(times["plain"]), 3), round(max(times["plain"]), 3)],
           "ms_per_call_geometric_min_max": [round(min(times["geometric"]), 3), round(max(times["geometric"]), 3)],
           "geometric_minus_plain_ms": round(med["geometric"] - med["plain"], 3),
           "geometric_over_plain": round(med["geometric"] / med["plain"], 4), "geo_counts_synthetic_weights": geo_counts}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--queries", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pnp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pnp.py needs a GPU: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "kernel": leg_kernel(a), "relocalize": leg_relocalize(a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
