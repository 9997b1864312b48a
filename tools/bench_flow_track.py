"""Timing of the flow-track kernel (atdn_flow_track_step, csrc/flow_track.hip) on one GPU. Synthetic scenes and weights from
seeds; nothing is read from outside the tree. Every timing leg runs in a child process of its own (`--leg`), so no leg inherits
another's allocator state or clocks; the parent only starts the children and collects their JSON lines.

    python tools/bench_flow_track.py [--reps 2000] [--frames 24] [--out profiles/flow_track_bench.json]

kernel (one child per batch size): at 376 x 1232, B = 1 and 16, by device events over `reps` launches in five rounds (memset +
kernel per launch, as a caller issues it), three forms alternating round by round in one process: `chain` — the chain-only form
(pose = NULL); `full` — chain and depth in one launch; `three_steps` — the same work as three steps: the chain-only form, then
atdn_flow_two_view_depth with mask = alive, then torch's `d != 0` and torch.where into the depth map. All three are out of place
from the same state (the second step of a track; `counts_entering` is the number of tracks alive), so every launch does the same
work. Per form: microseconds per launch and the bytes it must move (chain: 9 read + 9 written per pixel; full: + 4 read + 4
written of depth; three steps: the chain's 18, + 9 + 4 of the two-view call, + 4 + 1 of the comparison, + 9 + 4 of the select; the
flow taps, the mask byte, pose and counts not counted) over 8 TB/s. Back-to-back launches re-read the same buffers: with the
flow and the mask a launch of the full form touches 35 bytes per pixel — 16 MB at B = 1, all of it in the 256 MiB Infinity Cache,
and 259 MB at B = 16, about the size of that cache — so these are the kernels' own rates, not HBM's; at B = 1 a launch is a few
microseconds and the figure is bounded by the launch rate as much as by the kernel.

slam (one child): `NeuralSLAM` per frame (host clock, every call ends with the pose on the host) for calib=None,
keyframe_depth="pair" and keyframe_depth="track", the three objects alternating frame by frame on the same frames; 12 iterations,
synthetic weights, a keyframe every fourth pair (so "pair" triangulates every fourth frame and "track" extends on every frame and
writes a file every fourth).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBPS = 8.0
ROUNDS = 5
H, W = 376, 1232


def _events(torch, fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _scene(torch, calib, B, dev):
    """Two steps of a forward drive on the device: depths of 4 .. 120 m, a small rotation, t = (0.05, -0.02, 1) per step, a
    disturbance of 1.5 px — every outcome of the rule occurs. (flows [2][B,2,H,W], accumulated poses [2][B,12], a mask with 10 %
    zeros)."""
    g = torch.Generator(device=dev).manual_seed(5)
    fx, fy, cx, cy = calib
    y, x = torch.meshgrid(torch.arange(float(H), device=dev, dtype=torch.float64),
                          torch.arange(float(W), device=dev, dtype=torch.float64), indexing="ij")
    flows, poses = [[], []], [[], []]
    for b in range(B):
        a, c = 0.01 + 0.001 * b, -0.005
        R = torch.tensor([[1.0, -c, a], [c, 1.0, 0.0], [-a, 0.0, 1.0]], dtype=torch.float64, device=dev)   # small angles
        t = torch.tensor([0.05, -0.02, 1.0], dtype=torch.float64, device=dev)
        rel = torch.eye(4, dtype=torch.float64, device=dev)
        rel[:3, :3], rel[:3, 3] = R, t
        P = torch.eye(4, dtype=torch.float64, device=dev)
        for k in range(2):
            Z = 4.0 + 116.0 * (0.5 + 0.5 * torch.cos(6.28 * (x / W * (1 + b % 4) + 0.1 * b + 0.05 * k))) * (0.5 + 0.5 * torch.cos(3.14 * y / H))
            X1 = torch.stack([Z * (x - cx) / fx, Z * (y - cy) / fy, Z])
            X2 = torch.einsum("ji,jhw->ihw", R, X1 - t.view(3, 1, 1))
            u = fx * X2[0] / X2[2] + cx - x + 1.5 * torch.sin(x / 130.0 + y / 170.0 + b + k)
            v = fy * X2[1] / X2[2] + cy - y + 1.5 * torch.cos(x / 210.0 - y / 90.0 + b + k)
            flows[k].append(torch.stack([u, v]).float())
            P = P @ rel
            poses[k].append(P[:3].reshape(12).float())
    mask = (torch.rand((B, H, W), generator=g, device=dev) > 0.1).to(torch.uint8)
    return [torch.stack(f).contiguous() for f in flows], [torch.stack(p).contiguous() for p in poses], mask


def leg_kernel(a, B):
    import torch
    from atdn_vslam_amd import depth as depth_mod, transforms
    dev = torch.device("cuda:0")
    calib = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))
    flows, poses, mask = _scene(torch, calib, B, dev)
    zero, ones = torch.zeros((B, 2, H, W), device=dev), torch.ones((B, H, W), dtype=torch.uint8, device=dev)
    acc, alive, depth, _ = transforms.flow_track_step(flows[0], zero, ones, pose=poses[0], calib=calib, mask=mask)
    flow, pose = flows[1], poses[1]
    a_out, l_out = torch.empty_like(acc), torch.empty_like(alive)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    d_full, d_three = depth.clone(), depth.clone()

    def chain():
        return transforms.flow_track_step(flow, acc, alive, mask=mask, out=(a_out, l_out, counts))

    def full():
        return transforms.flow_track_step(flow, acc, alive, pose=pose, calib=calib, mask=mask, depth=d_full, out=(a_out, l_out, counts))

    def three_steps():
        transforms.flow_track_step(flow, acc, alive, mask=mask, out=(a_out, l_out, counts))
        d, c = transforms.two_view_depth(a_out, pose, calib, mask=l_out)
        return torch.where(d != 0, d, d_three)

    forms = (("chain", chain, 18), ("full", full, 26), ("three_steps", three_steps, 18 + 13 + 5 + 13))
    for _ in range(10):
        for _, fn, _ in forms:
            fn()
    per = max(1, a.reps // ROUNDS)
    times = {name: [] for name, _, _ in forms}
    for _ in range(ROUNDS):
        for name, fn, _ in forms:
            times[name].append(_events(torch, fn, per))
    n = B * H * W
    row = {"B": B, "H": H, "W": W, "launches": per * ROUNDS}
    for name, _, per_pixel in forms:
        ev = times[name]
        ms = sorted(ev)[len(ev) // 2]
        nbytes = n * per_pixel
        floor_ms = nbytes / (HBM_TBPS * 1e12) * 1e3
        row[name] = {"bytes": nbytes, "us_events": round(ms * 1e3, 3), "us_events_min": round(min(ev) * 1e3, 3),
                     "us_events_max": round(max(ev) * 1e3, 3), "floor_us_at_8TBps": round(floor_ms * 1e3, 3),
                     "times_the_floor": round(ms / floor_ms, 2), "tbps": round(nbytes / (ms * 1e-3) / 1e12, 3)}
    row["three_steps_over_full"] = round(row["three_steps"]["us_events"] / row["full"]["us_events"], 2)
    # the three-step form gives the full form's depth
    d_full.copy_(depth)
    full()
    row["counts_entering"] = [int(alive[0].sum())]
    row["counts_full"] = counts[:1].tolist()
    row["three_steps_equal_full"] = bool(torch.equal(three_steps(), d_full))
    return row


def leg_slam(a):
    import tempfile
    import torch
    from atdn_vslam_amd import depth as depth_mod, synthetic as syn
    from atdn_vslam_amd.slam import KeyframePolicy, NeuralSLAM
    dev = "cuda:0"
    calib = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))

    class EveryFourth(KeyframePolicy):
        calls = 0

        def __call__(self, pred_mat):
            self.calls += 1
            return self.calls % 4 == 0

    class Args:
        def __init__(self, path):
            self.device, self.keyframes_path = dev, path

    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    frames = torch.from_numpy(syn.make_frames(6, H, W, seed=8)).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        slams = {}
        for name, kw in (("plain", {}), ("pair", dict(calib=calib, keyframe_depth="pair")),
                         ("track", dict(calib=calib, keyframe_depth="track"))):
            path = os.path.join(tmp, name)
            os.makedirs(path)
            slams[name] = NeuralSLAM(Args(path), odometry_weights=hsd, flow_weights=gsd, **kw)
            slams[name]._policy = EveryFourth()
            slams[name].start_odometry()
        names = list(slams)
        for k in range(5):                                            # warm-up: every object, a few pairs
            for name in names:
                slams[name](frames[k % 6])
        times = {name: [] for name in names}
        for k in range(a.frames):
            f = frames[(k + 5) % 6]
            for name in names[k % 3:] + names[:k % 3]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                slams[name](f)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    row = {"frames": a.frames, "iters": 12, "keyframe_every": 4}
    for name in names:
        row["ms_per_frame_" + name] = round(med[name], 4)
        row["ms_per_frame_%s_min_max" % name] = [round(min(times[name]), 4), round(max(times[name]), 4)]
    row["pair_minus_plain_ms"] = round(med["pair"] - med["plain"], 4)
    row["track_minus_plain_ms"] = round(med["track"] - med["plain"], 4)
    return row


def _child(leg, a):
    """Run one leg in a fresh process; its last output line is the leg's JSON."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(a.reps), "--frames", str(a.frames)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("leg %s failed with status %d" % (leg, r.returncode))
    row = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--leg", default=None, help="internal: kernel1, kernel16 or slam — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_track_bench.json"))
    a = ap.parse_args()
    if a.leg:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_flow_track.py needs a GPU: nothing is measured without one")
        row = leg_slam(a) if a.leg == "slam" else leg_kernel(a, int(a.leg[len("kernel"):]))
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        return
    res = {"kernel": [_child("kernel1", a), _child("kernel16", a)], "slam": _child("slam", a)}
    res["device"] = res["slam"].pop("device")
    for row in res["kernel"]:
        row.pop("device")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
