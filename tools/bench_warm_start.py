"""What warm start costs and what each (iters, warm_start) setting of the per-frame path takes, on one MI355X.

    python tools/bench_warm_start.py [--rounds 5] [--parent-tree DIR] [--out profiles/warm_start_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_warm_start.py --kernel-only     (kernel-only time)

* the forward-interpolation kernel (csrc/warm_start.hip): device events around 200 back-to-back launches at the KITTI grid
  (47 x 154) for B = 1 and B = 16 — launch-to-launch time on one stream, which for a kernel this short is mostly the launch;
  the rocprofv3 run gives the kernel alone;
* one refinement iteration of ONE pair (what warm start is meant to save): RAFTGMA(low_latency=True).profile(mode="continued"),
  per-stage device time, as (time at 12 iterations - time at 4) / 8, next to the whole forward / iters;
* pipeline.VisualOdometry per frame (host uint8 frame -> pose on the host) over the frames of bench.py's per-frame leg: legs
  iters in {12, 8, 6} x warm_start in {off, on}, alternated round after round inside this one process, five warm-up frames per
  leg, median and min-max over the rounds;
* --parent-tree DIR: a checkout of the parent commit with its library built. The cold iters = 12 leg then also runs as child
  processes, alternately from DIR and from this tree (a library is loaded once per process), to show that defaults cost what
  they did.

This measures the PRICE of the feature and the latency of each setting. How many iterations warm start saves at equal flow error
needs the real checkpoints and KITTI; random weights say nothing about it, and nothing here claims it."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
H_KITTI, W_KITTI, CLIP = 376, 1241, 33      # bench.py: clip of 2 * 16 + 1 frames, seed 100 on rank 0
WARMUP, FRAMES = 5, 24


def _frames(torch, syn):
    base = torch.from_numpy(syn.make_frames(CLIP, H_KITTI, W_KITTI, seed=100)).round().clamp(0, 255).to(torch.uint8)
    return base[:WARMUP + FRAMES].contiguous().pin_memory()


def _leg(torch, vo, frames):
    """ms per frame of one leg: reset, WARMUP frames, FRAMES timed frames."""
    vo.reset()
    for k in range(WARMUP):
        vo(frames[k])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(WARMUP, WARMUP + FRAMES):
        pose = vo(frames[k])
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / FRAMES * 1e3
    assert bool(torch.isfinite(pose).all())
    return ms


def _stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4), "legs": len(xs)}


def child(tree, rounds):
    """Cold iters = 12 legs of the package found in `tree`; prints one JSON line."""
    sys.path.insert(0, tree)
    import torch
    from atdn_vslam_amd import synthetic as syn
    from atdn_vslam_amd.pipeline import VisualOdometry
    vo = VisualOdometry(syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1)), device=DEV, iters=12)
    frames = _frames(torch, syn)
    print(json.dumps({"tree": tree, "ms": [_leg(torch, vo, frames) for _ in range(rounds)]}), flush=True)


def kernel_times(torch, launches=200):
    from atdn_vslam_amd import _lib
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for B in (1, 16):
        x = torch.randn(B, 2, 47, 154, device=DEV) * 3
        y = torch.empty_like(x)

        def launch():
            _lib.check(L.atdn_flow_forward_interpolate(C.c_void_p(x.data_ptr()), B, 47, 154, C.c_void_p(y.data_ptr()), st))
        for _ in range(10):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        e1.synchronize()
        out["B%d" % B] = round(e0.elapsed_time(e1) * 1e3 / launches, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.rounds)
    sys.path.insert(0, ROOT)
    import torch
    if a.kernel_only:
        print(json.dumps({"events_us_per_launch_47x154": kernel_times(torch)}))
        return
    res = {"frames_per_leg": FRAMES, "warmup_frames_per_leg": WARMUP, "rounds": a.rounds}

    # ---- defaults against the parent commit: child processes, alternated (before this process opens the device)
    if a.parent_tree:
        ms = {"parent": [], "this": []}
        for r in range(3):
            for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--rounds", "3"], stdout=subprocess.PIPE,
                                   text=True, check=True, timeout=300)
                ms[name] += json.loads(p.stdout.strip().splitlines()[-1])["ms"]
        res["cold_iters12_child_processes"] = {k: dict(_stats(v), all_ms=[round(x, 4) for x in v]) for k, v in ms.items()}
        print(json.dumps(res["cold_iters12_child_processes"]), flush=True)

    from atdn_vslam_amd import synthetic as syn
    from atdn_vslam_amd.modules import RAFTGMA
    from atdn_vslam_amd.pipeline import VisualOdometry
    res["device"] = torch.cuda.get_device_name(0)
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))

    # ---- the kernel
    res["kernel_events_us_per_launch_47x154"] = kernel_times(torch)
    print(json.dumps(res["kernel_events_us_per_launch_47x154"]), flush=True)

    # ---- one refinement iteration of one pair (eager, per-stage device events)
    net = RAFTGMA(max_batch=1, low_latency=True)
    net.load_state_dict(gsd)
    net = net.to(DEV).eval()
    net.profile(376, 1232, 1, iters=12, reps=1, mode="continued")
    t12 = sum(net.profile(376, 1232, 1, iters=12, reps=5, mode="continued").values())
    t4 = sum(net.profile(376, 1232, 1, iters=4, reps=5, mode="continued").values())
    res["profile_B1_continued"] = {"ms_12_iters": round(t12, 4), "ms_4_iters": round(t4, 4),
                                   "ms_per_iteration": round((t12 - t4) / 8, 4), "ms_forward_over_iters": round(t12 / 12, 4)}
    print(json.dumps(res["profile_B1_continued"]), flush=True)
    del net

    # ---- the per-frame path
    frames = _frames(torch, syn)
    legs = [(it, w) for it in (12, 8, 6) for w in (False, True)]
    vos = {leg: VisualOdometry(gsd, hsd, device=DEV, iters=leg[0], warm_start=leg[1]) for leg in legs}
    ms = {leg: [] for leg in legs}
    for r in range(a.rounds):
        for leg in legs:
            ms[leg].append(_leg(torch, vos[leg], frames))
    res["per_frame"] = [dict({"iters": it, "warm_start": w}, **_stats(ms[(it, w)])) for it, w in legs]
    for row in res["per_frame"]:
        print(json.dumps(row), flush=True)
    k1 = res["kernel_events_us_per_launch_47x154"]["B1"] * 1e-3
    res["interpolation_over_one_iteration"] = {
        "events_launch_to_launch_vs_profile_iteration": round(k1 / res["profile_B1_continued"]["ms_per_iteration"], 4),
        "per_frame_ms_saved_per_dropped_iteration_cold": round((res["per_frame"][0]["median_ms"] - res["per_frame"][4]["median_ms"]) / 6, 4),
        "per_frame_ms_added_by_warm_start_at_12": round(res["per_frame"][1]["median_ms"] - res["per_frame"][0]["median_ms"], 4)}
    print(json.dumps(res["interpolation_over_one_iteration"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
