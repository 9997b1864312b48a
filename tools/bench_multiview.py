"""Timing of the multi-view keyframe depth kernel (atdn_multiview_depth, csrc/multiview_depth.hip) on one GPU, and of what
depth.FlowTrack(history=16) adds to an `extend` step. A synthetic scene from closed forms; nothing is read from outside the tree.
Every timing leg runs in a child process of its own (`--leg`), with its own time limit, so no leg inherits another's allocator
state or clocks; the parent only starts the children and collects their JSON lines.

    python tools/bench_multiview.py [--reps 100] [--out profiles/multiview_bench.json]

Kernel legs: 376 x 1232, B = 1, S = 4, 8, 16 views (a forward drive, 0.5 m per view, over a ground plane towards a wall; 0.3 px
noise on every correspondence, 5 % dead pixels per view, the initial depth 3 % off with 10 % holes), iters = 0 and 4. Per leg,
by device events over `reps` launches in five rounds, medians:

kernel    `transforms.multiview_depth` (memset + kernel per launch, as a caller issues it).
baseline  the same rule written with stock torch ops on the device in float64, vectorised over the pixels with the views in a
          Python loop — what a user would write without this kernel. The share of pixels on which its `valid` agrees with the
          kernel's and the largest relative difference of the depths are reported, not asserted. It runs reps / 10 times per round.
host      the library's host form on CPU tensors, one thread, wall clock, the median of three calls.

bytes: what a launch must move at least — S * 9 read per pixel (two flow planes and a liveness byte per view), 4 of the initial
depth, 9 written. `share_of_copy_roof`: the time a float4 copy at the 6.29 TB/s measured on this card (the roof of the
map search) would need for those bytes, over the kernel's time.

History legs: FlowTrack.extend at 376 x 1232 with history = 0 and history = 16, three child processes each, alternating; the
ratio of the medians of their medians.
No time is asserted anywhere.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from atdn_vslam_amd import depth as depth_mod, transforms  # noqa: E402

ROUNDS = 5
H, W, N = 376, 1232, 16
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))
OPTIONS = dict(scale_px=4.0, inlier_px=2.0, min_z=0.1, min_views=2, max_rel_sigma=0.25, max_depth=80.0)
LEGS = [(S, iters) for S in (4, 8, 16) for iters in (0, 4)]
HISTORY_LEGS = [0, 16, 0, 16, 0, 16]
LEG_TIMEOUT = 240
COPY_ROOF_TBPS = 6.29
DBL_MAX, FLT_MAX, FLT_MIN = sys.float_info.max, 3.4028234663852886e38, 1.1754943508222875e-38


def _events(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _scene(dev):
    """(acc [N,2,H,W] float32, alive [N,H,W] uint8, poses [N,12] float32, depth_init [1,1,H,W] float32) on the device."""
    g = torch.Generator(device="cpu").manual_seed(11)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), dtype=torch.float64), torch.arange(float(W), dtype=torch.float64), indexing="ij")
    ground = torch.where(y - cy > 0, 1.65 * fy / (y - cy).clamp(min=1e-9), torch.full_like(x, float("inf")))
    wall = 8.0 + 60.0 * (0.5 + 0.5 * torch.cos(6.28 * x / W))
    Z = torch.minimum(ground, wall).float().double()
    X1 = torch.stack([Z * (x - cx) / fx, Z * (y - cy) / fy, Z])
    acc, alive, poses = [], [], []
    for k in range(N):
        yaw, side = 0.01 * float(torch.sin(torch.tensor(0.7 * k))), 0.05 * float(torch.cos(torch.tensor(1.3 * k)))
        R = torch.tensor([[1.0, 0.0, yaw], [0.0, 1.0, 0.0], [-yaw, 0.0, 1.0]], dtype=torch.float32)
        t = torch.tensor([side, 0.0, 0.5 * (k + 1)], dtype=torch.float32)
        X2 = torch.einsum("ji,jhw->ihw", R.double(), X1 - t.double().view(3, 1, 1))
        near = X2[2] < 0.5
        zz = torch.where(near, torch.ones_like(Z), X2[2])
        u = fx * X2[0] / zz + cx - x + 0.3 * torch.randn((H, W), generator=g, dtype=torch.float64)
        v = fy * X2[1] / zz + cy - y + 0.3 * torch.randn((H, W), generator=g, dtype=torch.float64)
        acc.append(torch.stack([u, v]).float())
        alive.append((~near & (torch.rand((H, W), generator=g) > 0.05)).to(torch.uint8))
        poses.append(torch.cat([R, t.view(3, 1)], dim=1).reshape(12))
    init = Z * (1.0 + 0.03 * torch.randn((H, W), generator=g, dtype=torch.float64))
    init = torch.where(torch.rand((H, W), generator=g) < 0.1, torch.zeros_like(init), init).float()
    return (torch.stack(acc).to(dev).contiguous(), torch.stack(alive).to(dev).contiguous(), torch.stack(poses).to(dev).contiguous(),
            init.view(1, 1, H, W).to(dev).contiguous())


def torch_multiview(acc, alive, poses, slots, calib, depth_init, iters, scale_px, inlier_px, min_z, min_views, max_rel_sigma,
                    max_depth):
    """The rule with stock torch ops in float64 for one problem (see the module docstring): (depth [H,W] float32, valid)."""
    fx, fy, cx, cy = calib
    dev = acc.device
    c2, thr = scale_px * scale_px, inlier_px * inlier_px
    e = float(H + W)
    rho_behind = (0.5 * (e * e)) / (1.0 + (e * e) / c2)
    y, x = torch.meshgrid(torch.arange(float(H), device=dev, dtype=torch.float64),
                          torch.arange(float(W), device=dev, dtype=torch.float64), indexing="ij")
    a0, a1 = (x - cx) / fx, (y - cy) / fy
    host_poses = poses.double().cpu()
    views = []
    num, den, n_obs = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for k in slots:
        M = host_poses[k].view(3, 4)
        r, t = M[:, :3], M[:, 3]
        rc = r.t()
        tc = [float(-((r[0, i] * t[0] + r[1, i] * t[1]) + r[2, i] * t[2])) for i in range(3)]
        x2, y2 = x + acc[k, 0].double(), y + acc[k, 1].double()
        obs = (alive[k] != 0) & (x2 >= 0) & (x2 <= W - 1) & (y2 >= 0) & (y2 <= H - 1)
        m = [(float(rc[i, 0]) * a0 + float(rc[i, 1]) * a1) + float(rc[i, 2]) for i in range(3)]
        kx, ky = fx * (tc[0] * m[2] - m[0] * tc[2]), fy * (tc[1] * m[2] - m[1] * tc[2])
        xt, yt = x2 - cx, y2 - cy
        Ax, Bx = fx * tc[0] - xt * tc[2], xt * m[2] - fx * m[0]
        Ay, By = fy * tc[1] - yt * tc[2], yt * m[2] - fy * m[1]
        num = torch.where(obs, num + (Ax * Bx + Ay * By), num)
        den = torch.where(obs, den + (Ax * Ax + Ay * Ay), den)
        n_obs = n_obs + obs
        views.append((obs, m, tc, kx, ky, x2, y2))

    def evaluate(rho):
        g, h, cost, n_in = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
        zlim = min_z * rho
        for obs, m, tc, kx, ky, x2, y2 in views:
            P = [m[i] + rho * tc[i] for i in range(3)]
            use = obs & (P[2] >= zlim)
            iz = 1.0 / P[2]
            rx, ry = ((fx * P[0]) * iz + cx) - x2, ((fy * P[1]) * iz + cy) - y2
            e2 = rx * rx + ry * ry
            s = 1.0 + e2 / c2
            w = 1.0 / (s * s)
            Jx, Jy = (kx * iz) * iz, (ky * iz) * iz
            g = torch.where(use, g + ((w * Jx) * rx + (w * Jy) * ry), g)
            h = torch.where(use, h + ((w * Jx) * Jx + (w * Jy) * Jy), h)
            cost = torch.where(use, cost + (0.5 * e2) / s, torch.where(obs, cost + rho_behind, cost))
            n_in = n_in + (use & (e2 <= thr))
        return g, h, cost, n_in

    one = torch.ones_like(x)
    cand = n_obs >= min_views
    rho_lin = num / den
    lin_ok = cand & (rho_lin > 0) & (rho_lin <= DBL_MAX)
    z0 = depth_init.view(H, W).double()
    init_ok = cand & (z0 > 0) & (z0 <= FLT_MAX)
    rho_0 = 1.0 / z0
    gl, hl, cl, nl = evaluate(torch.where(lin_ok, rho_lin, one))
    gi, hi, ci, ni = evaluate(torch.where(init_ok, rho_0, one))
    from_init = init_ok & (~lin_ok | (ci < cl))
    solved = lin_ok | init_ok
    rho = torch.where(from_init, rho_0, rho_lin)
    g, h, cost, n_in = (torch.where(from_init, a, b) for a, b in ((gi, gl), (hi, hl), (ci, cl), (ni, nl)))
    lam = torch.full_like(x, 1e-3)
    for _ in range(iters):
        r_t = rho - g / (h + lam * h)
        ok = solved & (r_t > 0) & (r_t <= DBL_MAX)
        gt, ht, ct, nt = evaluate(torch.where(ok, r_t, one))
        accept = ok & (ct < cost)
        rho, g, h, cost, n_in = (torch.where(accept, a, b) for a, b in ((r_t, rho), (gt, g), (ht, h), (ct, cost), (nt, n_in)))
        lam = torch.where(accept, (lam / 3.0).clamp(min=1e-9), (4.0 * lam).clamp(max=1e6))
    z = 1.0 / rho
    ri = (h * rho) * rho
    valid = solved & (n_in >= min_views) & (ri >= 1.0 / (max_rel_sigma * max_rel_sigma)) & (z >= FLT_MIN) & (z <= max_depth)
    return torch.where(valid, z, torch.zeros_like(z)).float(), valid


def leg(S, iters, reps):
    dev = torch.device("cuda:0")
    acc, alive, poses, init = _scene(dev)
    slots = list(range(S))
    ds = torch.tensor([slots], dtype=torch.int32, device=dev)

    def kernel():
        return transforms.multiview_depth(acc, alive, poses, ds, CALIB, depth_init=init, iters=iters, **OPTIONS)

    def baseline():
        return torch_multiview(acc, alive, poses, slots, CALIB, init, iters, **OPTIONS)

    for _ in range(3):
        kernel()
    baseline()
    per_k, per_b = max(1, reps // ROUNDS), max(1, reps // ROUNDS // 10)
    tk, tb = [], []
    for _ in range(ROUNDS):
        tk.append(_events(kernel, per_k))
        tb.append(_events(baseline, per_b))
    cpu = [t.cpu() for t in (acc, alive, poses, init)]
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = transforms.multiview_depth(cpu[0], cpu[1], cpu[2], [slots], CALIB, depth_init=cpu[3], iters=iters, **OPTIONS)
        th.append(time.perf_counter() - t0)
    n = H * W
    nbytes = n * (S * 9 + 4 + 9)
    ms_k, ms_b = sorted(tk)[ROUNDS // 2], sorted(tb)[ROUNDS // 2]
    depth, info, views, counts = kernel()
    bd, bvalid = baseline()
    torch.cuda.synchronize()
    both = (depth[0, 0] > 0) & bvalid
    rel = float(((depth[0, 0] - bd).abs() / depth[0, 0].clamp(min=1e-30))[both].max()) if bool(both.any()) else 0.0
    row = {"S": S, "iters": iters, "B": 1, "H": H, "W": W, "launches": per_k * ROUNDS, "baseline_launches": per_b * ROUNDS,
           "bytes": nbytes, "kernel_us": round(ms_k * 1e3, 2), "kernel_us_min_max": [round(min(tk) * 1e3, 2), round(max(tk) * 1e3, 2)],
           "baseline_torch_fp64_us": round(ms_b * 1e3, 2), "baseline_us_min_max": [round(min(tb) * 1e3, 2), round(max(tb) * 1e3, 2)],
           "baseline_over_kernel": round(ms_b / ms_k, 2), "host_form_ms": round(sorted(th)[1] * 1e3, 1),
           "host_over_kernel": round(sorted(th)[1] * 1e3 / ms_k, 1),
           "kernel_tbps_of_min_bytes": round(nbytes / (ms_k * 1e-3) / 1e12, 4),
           "share_of_copy_roof": round(nbytes / (COPY_ROOF_TBPS * 1e12) / (ms_k * 1e-3), 4),
           "ns_per_pixel_view_evaluation": round(ms_k * 1e6 / (n * S * (iters + 2)), 5), "counts": counts[0].tolist(),
           "host_form_same_bits": bool(torch.equal(host[0], depth.cpu()) and torch.equal(host[1], info.cpu())
                                       and torch.equal(host[2], views.cpu()) and torch.equal(host[3], counts.cpu())),
           "baseline_valid_agreement": round(float(((depth[0, 0] > 0) == bvalid).float().mean()), 6),
           "baseline_max_rel_depth_difference": rel}
    print(json.dumps(row), flush=True)


def history_leg(K, reps):
    """FlowTrack.extend with history=K: the median over five rounds of the time per step, by device events."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    flow = (0.5 * torch.randn((1, 2, H, W), generator=g)).to(dev)
    step = torch.eye(4, dtype=torch.float64)
    step[2, 3] = 0.05
    track = depth_mod.FlowTrack((H, W), CALIB, dev, history=K)

    def run():
        track.extend(flow, step)

    for _ in range(5):
        run()
    per = max(1, reps // ROUNDS)
    ts = []
    for _ in range(ROUNDS):
        track.start()
        ts.append(_events(run, per))
    print(json.dumps({"history": K, "steps": per * ROUNDS, "extend_us": round(sorted(ts)[ROUNDS // 2] * 1e3, 2),
                      "extend_us_min_max": [round(min(ts) * 1e3, 2), round(max(ts) * 1e3, 2)]}), flush=True)


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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--leg", default=None, help="internal: S,iters or history,K — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiview_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiview.py needs a GPU: nothing is measured without one")
    if a.leg:
        first, second = a.leg.split(",")
        if first == "history":
            history_leg(int(second), a.reps)
        else:
            leg(int(first), int(second), a.reps)
        return
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "options": OPTIONS, "copy_roof_tbps": COPY_ROOF_TBPS,
           "legs": [_child("%d,%d" % (S, iters), a) for S, iters in LEGS],
           "history_legs": [_child("history,%d" % K, a) for K in HISTORY_LEGS]}
    med = {K: sorted(r["extend_us"] for r in res["history_legs"] if r["history"] == K)[1] for K in (0, 16)}
    res["extend_us_history0"], res["extend_us_history16"] = med[0], med[16]
    res["history16_over_history0"] = round(med[16] / med[0], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
