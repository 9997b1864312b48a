"""Timing of the ground-plane fit (atdn_ground_solve / atdn_ground_terms / atdn_ground_classify, csrc/ground.hip) on one GPU.
Synthetic scenes from seeds; nothing is read from outside the tree.

    python tools/bench_ground.py [--reps 200] [--out profiles/ground_bench.json]

Per case — 376 x 1232, B = 1 and 16, the default band (the rows below the principal point) and all rows —: device time per
`transforms.ground_plane` call (the vote and 8 steps: 2 + 2 * 9 = 20 launches), per `ground_terms` (2 launches) and per
`ground_classify` (1 launch) by device events over `reps` calls in five rounds (the median round; min and max beside it),
microseconds per launch, and the bytes the terms kernels must move (4 per pixel of the band, no mask). Against it: the host form
on the same inputs by the host clock (and whether it gives the same bits), and the same rule written in stock torch float64
operations on the device (the same vote by bit pattern, the same terms and the same damped step; sums in torch's own order, so
not the same bits — its height is reported beside the kernels'). Back-to-back calls re-read the same depth from the Infinity
Cache, so these are the kernels' own rates, not HBM's.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from atdn_vslam_amd import depth as depth_mod, transforms  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 5
ITERS = 8
H, W = 376, 1232
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))
OPTS = dict(transforms.GROUND_DEFAULTS)
HEIGHT = 1.65


def _events(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _scene(B):
    """A street on the device: the nearer of a road 1.65 m below the camera and a smooth wall of 6 .. 40 m that covers about half
    of the rows below the horizon, depth scale 1 - 0.02 b, 2 % Gaussian depth noise, 20 % holes, 5 % gross outliers. [B,H,W]."""
    g = torch.Generator(device=DEV).manual_seed(5)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), device=DEV, dtype=torch.float64),
                          torch.arange(float(W), device=DEV, dtype=torch.float64), indexing="ij")
    out = []
    for b in range(B):
        wall = 6.0 + 34.0 * (0.5 + 0.5 * torch.cos(6.28 * (x / W + 0.13 * b))) * (0.35 + 0.65 * (0.5 + 0.5 * torch.cos(3.14 * y / H)))
        road = torch.where(y - cy > 0, HEIGHT * fy / (y - cy).clamp(min=1e-9), torch.full_like(y, float("inf")))
        z = (1.0 - 0.02 * b) * torch.minimum(wall, road) * (1.0 + 0.02 * torch.randn((H, W), generator=g, device=DEV, dtype=torch.float64))
        pick = torch.rand((H, W), generator=g, device=DEV)
        z = torch.where(pick < 0.05, z * (0.3 + 2.7 * torch.rand((H, W), generator=g, device=DEV, dtype=torch.float64)), z)
        z = torch.where(pick > 0.8, torch.zeros_like(z), z)
        out.append(z.float())
    return torch.stack(out).contiguous()


def torch_ground_plane(depth, rows, n0=(0.0, 1.0, 0.0), iters=ITERS, scale_rel=0.05, inlier_rel=0.05, min_z=0.1, max_depth=80.0,
                       min_votes=64):
    """The rule in stock torch float64 operations on the depth's device, batched: (q [B,3], inliers [B])."""
    fx, fy, cx, cy = CALIB
    B = depth.shape[0]
    y0, y1 = rows
    dev = depth.device
    z = depth[:, y0:y1].double().reshape(B, -1)
    yy, xx = torch.meshgrid(torch.arange(y0, y1, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    a = torch.stack([((xx - cx) / fx).reshape(-1), ((yy - cy) / fy).reshape(-1), torch.ones(xx.numel(), device=dev, dtype=torch.float64)])
    used = (z >= min_z) & (z <= max_depth)
    n0 = torch.tensor(n0, dtype=torch.float64, device=dev)
    hgt = z * (n0 @ a)[None]
    k = (hgt.view(torch.int64) >> 47) - 1019 * 32
    vote = used & (k >= 0) & (k < 320)
    hist = torch.zeros((B, 322), dtype=torch.int64, device=dev)
    hist.scatter_add_(1, torch.where(vote, k + 1, torch.zeros_like(k)), vote.long())
    hist[:, 0] = 0
    sm = hist[:, :-2] + hist[:, 1:-1] + hist[:, 2:]
    mode = torch.argmax(sm * (z.shape[1] + 1) + hist[:, 1:-1], dim=1)
    centre = (((mode + 1019 * 32) << 47) | (1 << 46)).view(torch.float64)
    q = n0[None] / centre[:, None]
    c2 = scale_rel * scale_rel

    def terms(q):
        e = z * (q @ a) - 1.0
        e2 = e * e
        s = 1.0 + e2 / c2
        w = torch.where(used, 1.0 / (s * s), torch.zeros_like(s))
        J = z[:, None, :] * a[None]                                             # [B,3,n]
        Hm = torch.einsum("bn,bin,bjn->bij", w, J, J)
        g = torch.einsum("bn,bin->bi", w * e, J)
        cost = torch.where(used, 0.5 * e2 / s, torch.zeros_like(s)).sum(1)
        return Hm, g, cost, (used & (e2 <= inlier_rel * inlier_rel)).sum(1)

    lam = torch.full((B,), 1e-3, dtype=torch.float64, device=dev)
    Ha, ga, ca, ia = terms(q)
    qa = q
    for _ in range(iters):
        A = Ha + lam[:, None, None] * torch.diag_embed(torch.diagonal(Ha, dim1=1, dim2=2))
        qt = qa + torch.linalg.solve(A, -ga[..., None])[..., 0]
        Ht, gt, ct, it = terms(qt)
        acc = ct < ca
        qa = torch.where(acc[:, None], qt, qa)
        Ha, ga = torch.where(acc[:, None, None], Ht, Ha), torch.where(acc[:, None], gt, ga)
        ca, ia = torch.where(acc, ct, ca), torch.where(acc, it, ia)
        lam = torch.where(acc, (lam / 3.0).clamp(min=1e-9), (4.0 * lam).clamp(max=1e6))
    return qa, ia


def _stats(ms, launches):
    med = sorted(ms)[len(ms) // 2]
    return {"launches": launches, "us_events": round(med * 1e3, 3), "us_events_min": round(min(ms) * 1e3, 3),
            "us_events_max": round(max(ms) * 1e3, 3), "us_per_launch": round(med * 1e3 / launches, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "ground_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ground.py needs a GPU: nothing is measured without one")
    rows_out = []
    for B in (1, 16):
        depth = _scene(B)
        host_depth = depth.cpu()
        for band, rows in (("default", transforms.ground_rows(CALIB, H)), ("all", (0, H))):
            kw = dict(rows=rows, iters=ITERS, **OPTS)

            def solve():
                return transforms.ground_plane(depth, CALIB, **kw)

            q, sums, counts = solve()
            ck = {k: OPTS[k] for k in ("inlier_rel", "min_z", "max_depth")}
            tk = {k: OPTS[k] for k in ("scale_rel", "inlier_rel", "min_z", "max_depth")}

            def terms():
                return transforms.ground_terms(depth, q, CALIB, rows=rows, **tk)

            def classify():
                return transforms.ground_classify(depth, q, CALIB, rows=rows, **ck)

            def stock():
                return torch_ground_plane(depth, rows, iters=ITERS, **OPTS)

            for _ in range(3):
                solve(), terms(), classify(), stock()
            per = max(1, a.reps // ROUNDS)
            ev = {"solve": [], "terms": [], "classify": [], "torch": []}
            for _ in range(ROUNDS):
                ev["solve"].append(_events(solve, per))
                ev["terms"].append(_events(terms, per))
                ev["classify"].append(_events(classify, per))
                ev["torch"].append(_events(stock, max(1, per // 10)))
            t0 = time.perf_counter()
            hq, hs, hc = transforms.ground_plane(host_depth, CALIB, **kw)
            host_ms = (time.perf_counter() - t0) * 1e3
            tq, ti = stock()
            n = B * (rows[1] - rows[0]) * W
            row = {"B": B, "H": H, "W": W, "rows": list(rows), "band": band, "iters": ITERS, "calls": per * ROUNDS,
                   "band_bytes": 4 * n, "solve": _stats(ev["solve"], 2 + 2 * (ITERS + 1)), "terms": _stats(ev["terms"], 2),
                   "classify": _stats(ev["classify"], 1), "torch_ops": _stats(ev["torch"], 1), "host_ms": round(host_ms, 2)}
            row["terms"]["tbps"] = round(4 * n / (row["terms"]["us_events"] * 1e-6) / 1e12, 3)
            row["host_same_bits"] = bool(torch.equal(q.cpu(), hq) and torch.equal(sums.cpu(), hs) and torch.equal(counts.cpu(), hc))
            row["host_over_device"] = round(host_ms * 1e3 / row["solve"]["us_events"], 1)
            row["torch_over_device"] = round(row["torch_ops"]["us_events"] / row["solve"]["us_events"], 1)
            _, height = transforms.ground_height(q)
            _, theight = transforms.ground_height(tq)
            row["height"] = [round(float(h), 5) for h in height[:2].tolist()]
            row["height_true"] = [round(HEIGHT * (1.0 - 0.02 * b), 5) for b in range(min(B, 2))]
            row["height_torch_ops"] = [round(float(h), 5) for h in theight[:2].tolist()]
            row["counts"] = counts[:2].tolist()
            row["sigma"] = [round(float(s), 6) for s in transforms.ground_sigma(q, sums)[:2].tolist()]
            print(json.dumps(row), flush=True)
            rows_out.append(row)
        del depth
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "options": OPTS, "cases": rows_out}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
