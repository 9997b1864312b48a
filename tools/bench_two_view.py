"""Timing of the two-view depth kernel (atdn_flow_two_view_depth, csrc/two_view.hip) on one GPU. Synthetic scenes and weights
from seeds; nothing is read from outside the tree.

    python tools/bench_two_view.py [--reps 2000] [--frames 24] [--out profiles/two_view_bench.json]

kernel: `atdn_flow_two_view_depth` alone at 376 x 1232, B = 1 and 16, by device events over `reps` launches in five rounds
(memset + kernel per launch, as a caller issues it), with `atdn_flow_consistency` — a streaming kernel of the same kind — timed
in the same process, the two alternating round by round, as the yardstick. Per kernel: microseconds per launch, the bytes it must
move (two-view: 8 read + 4 written per pixel; consistency: 16 + 1; counts, pose and re-read taps not counted) over 8 TB/s, and
for the two-view kernel the ratio to the yardstick per byte moved. Back-to-back launches re-read the same buffers (89 MB at
B = 16) from the 256 MiB Infinity Cache, so these are the kernels' own rates, not HBM's; at B = 1 a launch is a few microseconds
and the figure is bounded by the launch rate as much as by the kernel.

odometry: `VisualOdometry` per frame (host clock, every call ends with the pose on the host) with and without `calib`, the two
objects alternating frame by frame on the same frames; 12 iterations, synthetic weights.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from atdn_vslam_amd import depth as depth_mod, synthetic as syn, transforms  # noqa: E402

DEV = torch.device("cuda:0")
HBM_TBPS = 8.0
ROUNDS = 5
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
    """A forward-driving scene on the device: depths of 4 .. 120 m, a small rotation, t = (0.05, -0.02, 1), a disturbance of
    1.5 px — every outcome of the rule occurs. (flow [B,2,H,W], pose [B,12], backward flow for the yardstick)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), device=DEV, dtype=torch.float64),
                          torch.arange(float(W), device=DEV, dtype=torch.float64), indexing="ij")
    flows, poses = [], []
    for b in range(B):
        Z = 4.0 + 116.0 * (0.5 + 0.5 * torch.cos(6.28 * (x / W * (1 + b % 4) + 0.1 * b))) * (0.5 + 0.5 * torch.cos(3.14 * y / H))
        a, c = 0.01 + 0.001 * b, -0.005
        R = torch.tensor([[1.0, -c, a], [c, 1.0, 0.0], [-a, 0.0, 1.0]], dtype=torch.float64, device=DEV)   # small angles
        t = torch.tensor([0.05, -0.02, 1.0], dtype=torch.float64, device=DEV)
        X1 = torch.stack([Z * (x - cx) / fx, Z * (y - cy) / fy, Z])
        X2 = torch.einsum("ji,jhw->ihw", R, X1 - t.view(3, 1, 1))
        u = fx * X2[0] / X2[2] + cx - x + 1.5 * torch.sin(x / 130.0 + y / 170.0 + b)
        v = fy * X2[1] / X2[2] + cy - y + 1.5 * torch.cos(x / 210.0 - y / 90.0 + b)
        flows.append(torch.stack([u, v]).float())
        poses.append(torch.cat([R, t.view(3, 1)], dim=1).reshape(12).float())
    flow = torch.stack(flows).contiguous()
    bw = (-flow + 0.45 * torch.randn(flow.shape, generator=g, device=DEV)).contiguous()
    return flow, torch.stack(poses).contiguous(), bw


def leg_kernel(a):
    out = []
    for B in (1, 16):
        flow, pose, bw = _scene(B)

        def two_view():
            return transforms.two_view_depth(flow, pose, CALIB)

        def consistency():
            return transforms._flow_consistency_counts(flow, bw, 0.01, 0.5)

        for _ in range(10):
            two_view()
            consistency()
        per = max(1, a.reps // ROUNDS)
        tv, fc = [], []
        for _ in range(ROUNDS):
            tv.append(_events(two_view, per))
            fc.append(_events(consistency, per))
        n = B * H * W
        row = {"B": B, "H": H, "W": W, "launches": per * ROUNDS}
        for name, ev, per_pixel in (("two_view", tv, 12), ("consistency", fc, 17)):
            ms = sorted(ev)[len(ev) // 2]
            nbytes = n * per_pixel
            floor_ms = nbytes / (HBM_TBPS * 1e12) * 1e3
            row[name] = {"bytes": nbytes, "us_events": round(ms * 1e3, 3), "us_events_min": round(min(ev) * 1e3, 3),
                         "us_events_max": round(max(ev) * 1e3, 3), "floor_us_at_8TBps": round(floor_ms * 1e3, 3),
                         "times_the_floor": round(ms / floor_ms, 2), "tbps": round(nbytes / (ms * 1e-3) / 1e12, 3)}
        row["two_view_over_consistency_per_byte"] = round(
            (row["two_view"]["us_events"] / row["two_view"]["bytes"]) / (row["consistency"]["us_events"] / row["consistency"]["bytes"]), 2)
        depth, counts = two_view()
        row["counts"] = counts[:2].tolist()
        row["epipolar_score"] = [round(float(s), 4) for s in transforms.epipolar_score(counts)[:2].tolist()]
        print(json.dumps(row), flush=True)
        out.append(row)
        del flow, pose, bw, depth, counts
        torch.cuda.empty_cache()
    return out


def leg_odometry(a):
    from atdn_vslam_amd.pipeline import VisualOdometry
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    frames = torch.from_numpy(syn.make_frames(6, H, W, seed=8)).to(DEV)
    plain = VisualOdometry(gsd, hsd, device=DEV)
    withc = VisualOdometry(gsd, hsd, device=DEV, calib=CALIB)
    for k in range(4):                                            # warm-up: both objects, a few pairs
        plain(frames[k % 6])
        withc(frames[k % 6])
    times = {"plain": [], "calib": []}
    for k in range(a.frames):
        f = frames[(k + 4) % 6]
        for name, vo in (("plain", plain), ("calib", withc)) if k % 2 == 0 else (("calib", withc), ("plain", plain)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vo(f)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = {"frames": a.frames, "iters": 12, "ms_per_frame_plain": round(med["plain"], 4), "ms_per_frame_calib": round(med["calib"], 4),
           "ms_per_frame_plain_min_max": [round(min(times["plain"]), 4), round(max(times["plain"]), 4)],
           "ms_per_frame_calib_min_max": [round(min(times["calib"]), 4), round(max(times["calib"]), 4)],
           "calib_minus_plain_ms": round(med["calib"] - med["plain"], 4), "last_epipolar_score_synthetic_weights": withc.epipolar_score()}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "two_view_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_two_view.py needs a GPU: nothing is measured without one")
    res = {"device": torch.cuda.get_device_name(0), "kernel": leg_kernel(a), "odometry": leg_odometry(a)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
