"""Timing of the voxel map (atdn_voxel_integrate / extract / rehash, csrc/voxel_map.hip) on one GPU. A synthetic drive from
closed forms; nothing is read from outside the tree. Every leg runs in a child process of its own (`--leg`), with its own time
limit, so no leg inherits another's allocator state or clocks; the parent only starts the children, collects their JSON lines
and stops at the first leg that fails.

    python tools/bench_voxel_map.py [--reps 20] [--out profiles/voxel_map_bench.json]

Legs: 376 x 1232, K = 16 and 64 keyframes one metre apart along a street (a ground plane 1.65 m below the camera, a wall between
6 and 60 m, random colours), stride 1 and 2, the defaults of VoxelMap (0.25 m, 0.5 to 40 m). Per leg, by device events, medians
over `reps` launches:

integrate_fresh   atdn_voxel_integrate into a table that was just cleared (every voxel is claimed by a compare-and-swap); the
                  clear is outside the events. The table has the capacity the VoxelMap object would give it.
integrate_again   the same call into the table as the first left it (every key is found by a plain read): what a later keyframe
                  that sees known ground costs.
extract           atdn_voxel_extract of all voxels, and the torch.sort by key plus the gathers the Python layer adds.
object            VoxelMap.integrate (wall clock, with its one synchronisation) into a table that is large enough from the
                  start, and into one that starts at 64 slots: the growth path's cost (new tables, clear, rehash).
baseline          the same map with stock torch ops on the device — keys in float64, torch.unique, index_add_ — what a user
                  would write without the kernel; its keys and counts are compared with the kernel's (reported, not asserted).
host              the library's host form on CPU tensors, one thread, wall clock, once.

bytes: what an integrate must read at least — 4 of depth and 3 of colour per pixel that takes part. `share_of_copy_rate`: the
time a device-to-device copy at the rate measured in the same leg (1 GiB, read + write bytes) would need for those bytes, over
the kernel's time. Every leg checks that the kernel's cloud equals the host form's in every bit and fails otherwise.
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

from atdn_vslam_amd import _lib, depth as depth_mod  # noqa: E402
from atdn_vslam_amd.voxel_map import VoxelMap  # noqa: E402

H, W = 376, 1232
CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (H, W))
GRID = dict(voxel=0.25, origin=(0.0, 0.0, 0.0), min_z=0.5, max_z=40.0)
LEGS = [(K, stride) for K in (16, 64) for stride in (1, 2)]
LEG_TIMEOUT = 300


def _scene(K, dev):
    """(depth [K,H,W] float32, poses [K,12] float32, images [K,3,H,W] uint8) on the device."""
    g = torch.Generator(device="cpu").manual_seed(11)
    fx, fy, cx, cy = CALIB
    y, x = torch.meshgrid(torch.arange(float(H), dtype=torch.float64), torch.arange(float(W), dtype=torch.float64), indexing="ij")
    ground = torch.where(y - cy > 0, 1.65 * fy / (y - cy).clamp(min=1e-9), torch.full_like(x, float("inf")))
    depth, poses = [], []
    for k in range(K):
        wall = 6.0 + 54.0 * (0.5 + 0.5 * torch.cos(6.28 * x / W + 0.2 * k))
        depth.append(torch.minimum(ground, wall).float())
        yaw, side = 0.02 * float(torch.sin(torch.tensor(0.7 * k))), 0.1 * float(torch.cos(torch.tensor(1.3 * k)))
        R = torch.tensor([[1.0, 0.0, yaw], [0.0, 1.0, 0.0], [-yaw, 0.0, 1.0]], dtype=torch.float32)
        poses.append(torch.cat([R, torch.tensor([side, 0.0, 1.0 * k]).view(3, 1)], dim=1).reshape(12))
    images = torch.randint(0, 256, (K, 3, H, W), generator=g, dtype=torch.uint8)
    return torch.stack(depth).to(dev).contiguous(), torch.stack(poses).to(dev).contiguous(), images.to(dev).contiguous()


def torch_voxel_map(depth, poses, images, stride):
    """The rule with stock torch ops on the device: (keys [M] int64 ascending, sums [M,7] int64 = n, S, C)."""
    fx, fy, cx, cy = CALIB
    dev = depth.device
    K = depth.shape[0]
    y, x = torch.meshgrid(torch.arange(0.0, H, stride, device=dev, dtype=torch.float64),
                          torch.arange(0.0, W, stride, device=dev, dtype=torch.float64), indexing="ij")
    z = depth[:, ::stride, ::stride].double()
    P = poses.double().view(K, 3, 4, 1, 1)
    c0, c1 = ((x - cx) / fx) * z, ((y - cy) / fy) * z
    ok = (z >= GRID["min_z"]) & (z <= GRID["max_z"])
    key = torch.zeros_like(z, dtype=torch.int64)
    cols = [torch.ones_like(key)]
    for a in range(3):
        p = ((P[:, a, 0] * c0 + P[:, a, 1] * c1) + P[:, a, 2] * z) + P[:, a, 3]
        g = (p - GRID["origin"][a]) / GRID["voxel"]
        inside = (g >= -1048576.0) & (g < 1048576.0)
        ok = ok & inside
        g = torch.where(inside, g, torch.zeros_like(g))
        k = torch.floor(g)
        cols.append(((g - k) * 65536.0).long())
        key = (key << 21) | (k.long() + 1048576)
    cols += [images[:, a, ::stride, ::stride].long() for a in range(3)]
    uniq, inv = torch.unique(key[ok], return_inverse=True)
    sums = torch.zeros((uniq.shape[0], 7), dtype=torch.int64, device=dev)
    sums.index_add_(0, inv, torch.stack([c[ok] for c in cols], dim=1))
    return uniq, sums


def _median_us(fn, reps, before=None):
    """Median over `reps` calls of fn, each between its own pair of device events (`before` runs outside them)."""
    pairs = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in pairs)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3


def _copy_rate_tbps():
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda:0")
    dst = torch.empty_like(src)
    dst.copy_(src)
    us, _, _ = _median_us(lambda: dst.copy_(src), 10)
    return 2 * src.numel() * 4 / (us * 1e-6) / 1e12


def leg(K, stride, reps):
    import ctypes as C
    dev = torch.device("cuda:0")
    depth, poses, images = _scene(K, dev)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    pixels = K * ((H + stride - 1) // stride) * ((W + stride - 1) // stride)
    # the object: presized, and grown from 64 slots
    cap = 64
    while cap < 2 * pixels:
        cap *= 2
    wall = {}
    for name, c0 in (("presized", cap), ("from_64", 64), ("presized_2", cap), ("from_64_2", 64)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vm = VoxelMap(dev, capacity=c0, **GRID)
        vm.integrate(depth, poses, CALIB, images=images, stride=stride)
        wall[name] = (time.perf_counter() - t0) * 1e3
    counts = vm.counts
    assert vm.capacity == cap and counts["dropped"] == 0
    cloud = vm.extract()
    table = vm.table

    def clear():
        _lib.check(L.atdn_voxel_clear(p(table), cap, stream()))

    def integrate():
        _lib.check(L.atdn_voxel_integrate(p(depth), p(poses), p(images), None, None, K, K, H, W, *CALIB, stride, GRID["voxel"],
                                          *GRID["origin"], GRID["min_z"], GRID["max_z"], 0, p(table), cap, None, stream()))

    M = counts["voxels"]
    out = (torch.empty((M, 3), device=dev), torch.empty((M, 3), dtype=torch.uint8, device=dev),
           torch.empty((M,), dtype=torch.int32, device=dev), torch.empty((M,), dtype=torch.int64, device=dev))
    found = torch.zeros((1,), dtype=torch.int64, device=dev)

    def extract():
        _lib.check(L.atdn_voxel_extract(p(table), cap, 1, GRID["voxel"], *GRID["origin"], M, *(p(o) for o in out), p(found), stream()))

    def order():
        keys, idx = torch.sort(out[3])
        return out[0][idx], out[1][idx], out[2][idx], keys

    fresh = _median_us(integrate, reps, before=clear)
    again = _median_us(integrate, reps)
    clear_us = _median_us(clear, reps)
    clear()
    integrate()
    ext = _median_us(extract, reps)
    srt = _median_us(order, reps)
    got = order()
    torch.cuda.synchronize()
    assert int(found.item()) == M
    base = _median_us(lambda: torch_voxel_map(depth, poses, images, stride), max(1, reps // 4))
    bk, bs = torch_voxel_map(depth, poses, images, stride)
    rehash_src = table.clone()

    def rehash():
        _lib.check(L.atdn_voxel_rehash(p(rehash_src), cap, p(table), cap, stream()))

    reh = _median_us(rehash, max(1, reps // 4), before=clear)
    t0 = time.perf_counter()
    hm = VoxelMap("cpu", capacity=cap, **GRID)
    hm.integrate(depth.cpu(), poses.cpu(), CALIB, images=images.cpu(), stride=stride)
    host_ms = (time.perf_counter() - t0) * 1e3
    host = hm.extract()
    same = hm.counts == counts and all(torch.equal(a.cpu(), b) for a, b in zip(cloud, host)) and \
        all(torch.equal(a.cpu(), b) for a, b in zip(got, host))
    if not same:
        raise SystemExit("K=%d stride=%d: the kernel's cloud differs from the host form's" % (K, stride))
    rate = _copy_rate_tbps()
    nbytes = pixels * 7
    row = {"K": K, "stride": stride, "H": H, "W": W, "pixels": pixels, "capacity": cap, "table_bytes": 64 + 64 * cap, "counts": counts,
           "launches": reps, "integrate_fresh_us": round(fresh[0], 1), "integrate_fresh_us_min_max": [round(fresh[1], 1), round(fresh[2], 1)],
           "integrate_again_us": round(again[0], 1), "integrate_again_us_min_max": [round(again[1], 1), round(again[2], 1)],
           "points_per_s_fresh": round(counts["inserted"] / (fresh[0] * 1e-6), 0),
           "points_per_s_again": round(counts["inserted"] / (again[0] * 1e-6), 0),
           "min_bytes": nbytes, "copy_rate_tbps": round(rate, 3),
           "share_of_copy_rate_fresh": round(nbytes / (rate * 1e12) / (fresh[0] * 1e-6), 4),
           "share_of_copy_rate_again": round(nbytes / (rate * 1e12) / (again[0] * 1e-6), 4),
           "clear_us": round(clear_us[0], 1), "extract_us": round(ext[0], 1), "sort_and_gather_us": round(srt[0], 1),
           "rehash_same_capacity_us": round(reh[0], 1),
           "object_integrate_ms_presized": round(min(wall["presized"], wall["presized_2"]), 2),
           "object_integrate_ms_from_64_slots": round(min(wall["from_64"], wall["from_64_2"]), 2),
           "baseline_torch_us": round(base[0], 1), "baseline_over_fresh": round(base[0] / fresh[0], 1),
           "baseline_same_keys_and_counts": bool(torch.equal(bk, got[3]) and torch.equal(bs[:, 0].int(), got[2])),
           "host_form_ms": round(host_ms, 1), "host_over_fresh": round(host_ms * 1e3 / fresh[0], 1), "host_form_same_bits": True}
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
    ap.add_argument("--leg", default=None, help="internal: K,stride — run that leg in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_map_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel_map.py needs a GPU: nothing is measured without one")
    if a.leg:
        K, stride = (int(v) for v in a.leg.split(","))
        leg(K, stride, a.reps)
        return
    res = {"device": torch.cuda.get_device_name(0), "grid": GRID, "legs": [_child("%d,%d" % (K, s), a) for K, s in LEGS]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("written", a.out)


if __name__ == "__main__":
    main()
