"""Timing of the HBM-resident keyframe map (atdn_vslam_amd/keyframe_map.py) on one GPU. Synthetic weights, embeddings and
frames from seeds; nothing is read from outside the tree (the end-to-end leg writes its keyframe directory to a temporary
directory and removes it).

    python tools/bench_reloc.py --leg search [--K 455,4096,16384] [--Q 1,16] [--reps 200] [--no-loop]
    python tools/bench_reloc.py --leg e2e    [--keyframes 455] [--reps 200]
    python tools/bench_reloc.py --leg all --out profiles/reloc_bench.json
    python tools/bench_reloc.py --leg verify [--parent-lib PATH/libatdn_hip.so]     (writes profiles/reloc_verify_bench.json)

search: `atdn_map_search` (distances + top-1) on a bank of K embeddings of 15,360 floats, Q queries per call, against the
per-keyframe `torch.norm` loop of the default relocalisation path on the same embeddings (one query). The two alternate in
rounds inside one process. Per variant: device-event time per call over `reps` calls (what the stream is busy for; at a few
hundred keyframes this is bounded by the launch rate of the host, not by the kernel: take the kernel's own time from
`rocprofv3 --kernel-trace --stats -- python tools/bench_reloc.py --leg search --no-loop --K 16384`), and host time per call
including the read-back of the winner's index, as a caller sees it. bytes = (K + Q) * D * 4: bank and queries read once.
A loop that repeats a search re-reads the same bank: 455 keyframes (28 MB) and 4,096 (252 MB) fit the 256 MiB Infinity
Cache, so only the 16,384 case (1 GB) streams from HBM; `bank_residence` says which.

e2e: one relocalisation query from the image to the host pose (embedding + search + keyframe image + flow + head + pose
algebra): the default path (`NeuralSLAM(...)`: torch.norm loop, keyframe image read from its file, batch 1), the resident
map's single query (`resident_map=True`), and `relocalize_batch` at 16 queries per call, per query. Host clock; every call
ends with host tensors, i.e. synchronised.

verify (not part of `all`): what `relocalize_batch(verify=True)` costs — ms per query against verify=False at Q = 1, 16 and
top_k = 1, 3 with 455 keyframes, every timing process a child of its own, alternating with the same verify=False leg on the
parent commit's library when --parent-lib names one — and `atdn_flow_consistency` alone by device events at 376 x 1232,
B = 1, 16, against bytes / 8 TB/s. See leg_verify.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from atdn_vslam_amd import keyframe_map as km, synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")
D = 15360                      # 6 x 20 x 128: the embedding of a 376 x 1232 frame
COPY_TBPS = 6.29               # float4 copy on the MI355X (microarchitecture guide): the roof for a streaming kernel
INFINITY_CACHE = 256 << 20
ROUNDS = 5


def _events(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def _host(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def leg_search(a):
    out = []
    g = torch.Generator(device=DEV).manual_seed(7)
    for K in a.K:
        bank = torch.randn((K, D), generator=g, device=DEV)
        frames = [bank[k].view(1, 128, 6, 20) for k in range(K)]       # what the default path's Frame.embedding list holds
        for Q in a.Q:
            queries = torch.randn((Q, D), generator=g, device=DEV)
            mu = queries[0].view(1, 128, 6, 20)

            def kernel():
                return km.search_bank(bank, queries, 1)

            def kernel_call():
                return int(kernel()[1][0, 0])

            def loop_call():
                d = torch.stack([torch.norm(f - mu, p=2) for f in frames], dim=0)
                return int(torch.argmin(d))

            with_loop = a.loop and Q == 1
            # the loop issues ~3K launches per call: fewer repetitions, sized to a few seconds in all
            loop_reps = max(3, min(a.reps, int(a.reps * 455 / K))) if with_loop else 0
            assert kernel_call() == (loop_call() if with_loop else kernel_call())
            per = max(1, a.reps // ROUNDS)
            ev, host, loop = [], [], []
            for _ in range(3):
                kernel_call()
            for _ in range(ROUNDS):
                ev.append(_events(kernel, per))
                host.append(_host(kernel_call, per))
                if with_loop:
                    loop.append(_host(loop_call, max(1, loop_reps // ROUNDS)))
            nbytes = (K + Q) * D * 4
            ms = sorted(ev)[len(ev) // 2]
            row = {"K": K, "Q": Q, "D": D, "reps": per * ROUNDS, "bytes": nbytes,
                   "bank_residence": "infinity cache (re-read by the loop)" if K * D * 4 <= INFINITY_CACHE else "HBM",
                   "search_ms_events": round(ms, 5), "search_ms_events_min": round(min(ev), 5),
                   "search_ms_events_max": round(max(ev), 5),
                   "tbps": round(nbytes / (ms * 1e-3) / 1e12, 3),
                   "share_of_copy_roof": round(nbytes / (ms * 1e-3) / 1e12 / COPY_TBPS, 3),
                   "search_call_ms_host": round(sorted(host)[len(host) // 2], 5)}
            if with_loop:
                lm = sorted(loop)[len(loop) // 2]
                row.update({"loop_reps": max(1, loop_reps // ROUNDS) * ROUNDS, "torch_norm_loop_ms_host": round(lm, 4),
                            "loop_over_search_call": round(lm / row["search_call_ms_host"], 1)})
            print(json.dumps(row), flush=True)
            out.append(row)
        del frames, bank
        torch.cuda.empty_cache()
    return out


class _Args:
    def __init__(self, path):
        self.device = str(DEV)
        self.keyframes_path = path


def leg_e2e(a):
    from atdn_vslam_amd.slam import NeuralSLAM
    K = a.keyframes
    gsd = syn.to_torch(syn.make_gma_state(seed=1))
    hsd = syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    distinct = torch.from_numpy(syn.make_frames(17, 376, 1232, seed=5)).byte()
    root = tempfile.mkdtemp(prefix="reloc_bench_")
    try:
        kf = os.path.join(root, "kf")
        os.makedirs(os.path.join(kf, "rgb"))
        for i in range(K):                                  # 16 distinct frames, each with its index stamped in a corner
            im = distinct[i % 16].clone()
            im[:, :2, :16] = torch.tensor([(i >> b) & 1 for b in range(16)], dtype=torch.uint8) * 255
            torch.save(im, os.path.join(kf, "rgb", "%06d.pth" % i))
        poses = torch.eye(4).flatten()[:12].repeat(K, 1)
        poses[:, 3] = torch.arange(K, dtype=torch.float32)
        torch.save(poses, os.path.join(kf, "poses.pth"))
        torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
        t0 = time.perf_counter()
        default = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        resident = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        query = distinct[16].float()
        batch = torch.stack([distinct[(3 * j) % 17].float() for j in range(16)])
        for _ in range(3):
            default(query), resident(query), resident.relocalize_batch(batch)
        assert int(torch.argmin(default(query)[2])) == int(torch.argmin(resident(query)[2]))
        per = max(1, a.reps // ROUNDS)
        t = {"default": [], "resident": [], "batch16": []}
        for _ in range(ROUNDS):
            t["default"].append(_host(lambda: default(query), max(1, per // 4)))
            t["resident"].append(_host(lambda: resident(query), per))
            t["batch16"].append(_host(lambda: resident.relocalize_batch(batch), max(1, per // 8)) / 16)
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        row = {"leg": "e2e", "keyframes": K, "reps_resident": per * ROUNDS,
               "start_relocalization_s_default": round(t1 - t0, 2), "start_relocalization_s_resident": round(t2 - t1, 2),
               "query_ms_default_path": round(med["default"], 3), "query_ms_resident": round(med["resident"], 3),
               "query_ms_relocalize_batch_16": round(med["batch16"], 3),
               "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}}
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(row), flush=True)
    return row


HBM_TBPS = 8.0                 # peak HBM3E bandwidth of the MI355X: the floor bytes / 8 TB/s of the consistency kernel
VERIFY_CONFIGS = [(1, 1), (1, 3), (16, 1), (16, 3)]      # (Q, top_k)


def _verify_directory(root, K, vsd, distinct):
    kf = os.path.join(root, "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    for i in range(K):
        im = distinct[i % 16].clone()
        im[:, :2, :16] = torch.tensor([(i >> b) & 1 for b in range(16)], dtype=torch.uint8) * 255
        torch.save(im, os.path.join(kf, "rgb", "%06d.pth" % i))
    poses = torch.eye(4).flatten()[:12].repeat(K, 1)
    poses[:, 3] = torch.arange(K, dtype=torch.float32)
    torch.save(poses, os.path.join(kf, "poses.pth"))
    torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
    return kf


def leg_verify_child(a):
    """One process of the verify leg, on whatever library ATDN_LIB_PATH names: ms per query of relocalize_batch(verify=False)
    and — with --with-verify — of verify=True, host clock around calls that end with host tensors, the variants alternating in
    rounds. The processes that compare the two libraries time verify=False alone, so that both do exactly the same work (the
    heavy verify=True batches in between would leave the card in another clock and thermal state). --parent-abi: the library
    is the parent commit's, which lacks the two flow-consistency entry points; they are taken out of the ctypes table before it
    loads (verify=False never calls them)."""
    from atdn_vslam_amd import _lib
    if a.parent_abi:
        for name in ("atdn_flow_consistency", "atdn_flow_consistency_host"):
            _lib.SIGNATURES.pop(name)
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd = syn.to_torch(syn.make_gma_state(seed=1))
    hsd = syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    distinct = torch.from_numpy(syn.make_frames(17, 376, 1232, seed=5)).byte()
    root = tempfile.mkdtemp(prefix="reloc_verify_")
    try:
        kf = _verify_directory(root, a.keyframes, vsd, distinct)
        slam = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True)
        batches = {1: distinct[16:17].float(), 16: torch.stack([distinct[(3 * j) % 17].float() for j in range(16)])}
        variants = [(Q, k, False) for Q, k in VERIFY_CONFIGS]
        if a.with_verify:
            variants += [(Q, k, True) for Q, k in VERIFY_CONFIGS]
        for Q, k, v in variants:                               # warm-up: every shape of the timed window, twice
            for _ in range(2):
                slam.relocalize_batch(batches[Q], top_k=k, verify=v)
        t = {v: [] for v in variants}
        for _ in range(ROUNDS):
            for Q, k, v in variants:
                reps = max(1, (a.reps // ROUNDS) // (1 if Q == 1 else 8))
                t[(Q, k, v)].append(_host(lambda: slam.relocalize_batch(batches[Q], top_k=k, verify=v), reps) / Q)
        rows = [{"Q": Q, "top_k": k, "verify": v, "ms_per_query": round(sorted(x)[len(x) // 2], 4),
                 "min": round(min(x), 4), "max": round(max(x), 4)} for (Q, k, v), x in t.items()]
        scores = None
        if a.with_verify:
            scores = slam.relocalize_batch(batches[16], top_k=3, verify=True)[4].tolist()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    res = {"library": _lib.LIB_PATH, "parent_abi": bool(a.parent_abi), "keyframes": a.keyframes, "rows": rows,
           "scores_q16_top3_synthetic_weights": scores}
    with open(a.child_out, "w") as f:
        json.dump(res, f)
    return res


def _consistency_kernel(a):
    """atdn_flow_consistency alone at 376 x 1232, B = 1 and 16: device events over `reps` launches (5 rounds), against the
    bytes it must move (16 read + 1 written per pixel; the count and the re-read taps are not counted) over 8 TB/s. Back-to-back
    launches re-read the same 59 MB (B = 16) from the 256 MiB Infinity Cache, so this is the kernel's own rate, not HBM's."""
    from atdn_vslam_amd import transforms
    out = []
    g = torch.Generator(device=DEV).manual_seed(11)
    y, x = torch.meshgrid(torch.arange(376.0, device=DEV), torch.arange(1232.0, device=DEV), indexing="ij")
    for B in (1, 16):
        # smooth forward flows of ~2 px, backward = -forward + noise: both outcomes occur, the taps are local
        ph = torch.rand((B, 1, 1), generator=g, device=DEV) * 6.28
        fw = torch.stack([2.0 * torch.sin(x / 130.0 + y / 170.0 + ph), 2.0 * torch.cos(x / 210.0 - y / 90.0 + ph)], dim=1).contiguous()
        bw = -fw + 0.45 * torch.randn(fw.shape, generator=g, device=DEV)
        for _ in range(10):
            transforms._flow_consistency_counts(fw, bw, 0.01, 0.5)
        per = max(1, a.reps // ROUNDS)
        ev = [_events(lambda: transforms._flow_consistency_counts(fw, bw, 0.01, 0.5), per) for _ in range(ROUNDS)]
        ms = sorted(ev)[len(ev) // 2]
        nbytes = B * 376 * 1232 * 17
        floor_ms = nbytes / (HBM_TBPS * 1e12) * 1e3
        row = {"B": B, "H": 376, "W": 1232, "launches": per * ROUNDS, "bytes": nbytes, "ms_events": round(ms, 5),
               "ms_events_min": round(min(ev), 5), "ms_events_max": round(max(ev), 5), "floor_ms_at_8TBps": round(floor_ms, 5),
               "times_the_floor": round(ms / floor_ms, 2), "tbps": round(nbytes / (ms * 1e-3) / 1e12, 3),
               "consistent_share": [round(float(s), 4) for s in transforms.flow_consistency(fw, bw)[1].tolist()[:2]]}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def leg_verify(a):
    """Price of verify=True. Every timing process is a child of its own (a process loads ONE library). With --parent-lib:
    verify=False alone on the parent commit's library and on this one, alternating (parent, new, parent, new, ...),
    `--verify-runs` of each — the new library's figures must lie inside the spread of the parent's own runs. Then two processes
    on this library that alternate verify=False and verify=True: the ratio of the two in the same process (expected: about
    2 * top_k flow passes per query instead of one, plus noise)."""
    import subprocess
    here = os.path.abspath(__file__)
    tmp = tempfile.mkdtemp(prefix="reloc_verify_out_")
    runs = {"new": [], "parent": [], "full": []}
    try:
        order = (["parent", "new"] * a.verify_runs if a.parent_lib else []) + ["full"] * min(2, a.verify_runs)
        for i, which in enumerate(order):
            out = os.path.join(tmp, "%d.json" % i)
            env = dict(os.environ)
            cmd = [sys.executable, here, "--leg", "verify-child", "--child-out", out, "--keyframes", str(a.keyframes),
                   "--reps", str(a.reps)]
            if which == "parent":
                env["ATDN_LIB_PATH"] = os.path.abspath(a.parent_lib)
                cmd.append("--parent-abi")
            else:
                env.pop("ATDN_LIB_PATH", None)
                if which == "full":
                    cmd.append("--with-verify")
            subprocess.run(cmd, env=env, check=True, timeout=a.child_timeout)
            with open(out) as f:
                runs[which].append(json.load(f))
            print(json.dumps({"run": i, "library": which, "rows": runs[which][-1]["rows"]}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    def med(which, Q, k, v):
        return [r["ms_per_query"] for run in runs[which] for r in run["rows"] if (r["Q"], r["top_k"], r["verify"]) == (Q, k, v)]

    table = []
    for Q, k in VERIFY_CONFIGS:
        new_off, par = med("new", Q, k, False), med("parent", Q, k, False)
        full_off, full_on = med("full", Q, k, False), med("full", Q, k, True)
        row = {"Q": Q, "top_k": k, "verify_false_ms_per_query_new": new_off if new_off else "not measured (no --parent-lib)",
               "same_process": {"verify_false_ms_per_query": full_off, "verify_true_ms_per_query": full_on},
               "verify_true_over_false": [round(x / y, 2) for x, y in zip(full_on, full_off)],
               "flow_passes_per_query": {"verify_false": 1, "verify_true": 2 * k},
               "verify_false_ms_per_query_parent": par if par else "not measured (no --parent-lib)"}
        if par:
            # the spread of the parent's runs: every per-round figure of every parent process, not only their medians
            lo = min(r["min"] for run in runs["parent"] for r in run["rows"] if (r["Q"], r["top_k"], r["verify"]) == (Q, k, False))
            hi = max(r["max"] for run in runs["parent"] for r in run["rows"] if (r["Q"], r["top_k"], r["verify"]) == (Q, k, False))
            row["parent_spread_ms"] = [lo, hi]
            row["new_inside_parent_spread"] = all(lo <= x <= hi for x in new_off)
        table.append(row)
    res = {"leg": "verify", "keyframes": a.keyframes, "runs_per_library": a.verify_runs, "end_to_end": table,
           "kernel": _consistency_kernel(a),
           "scores_q16_top3_synthetic_weights": runs["full"][-1]["scores_q16_top3_synthetic_weights"] if runs["full"] else None,
           "note": "synthetic weights: the scores show that the mechanism runs, not that it ranks candidates correctly"}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("search", "e2e", "all", "verify", "verify-child"), default="all")
    ap.add_argument("--parent-lib", default=None, help="verify: the parent commit's libatdn_hip.so, for the alternating comparison")
    ap.add_argument("--verify-runs", type=int, default=2, help="verify: processes per library (0: the kernel alone)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--parent-abi", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-verify", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--K", type=lambda s: [int(x) for x in s.split(",")], default=[455, 4096, 16384])
    ap.add_argument("--Q", type=lambda s: [int(x) for x in s.split(",")], default=[1, 16])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--keyframes", type=int, default=455)
    ap.add_argument("--no-loop", dest="loop", action="store_false")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reloc.py measures on the GPU: no device found")
    res = {}
    if a.leg in ("search", "all"):
        res["search"] = leg_search(a)
    if a.leg in ("e2e", "all"):
        res["e2e"] = leg_e2e(a)
    if a.leg == "verify-child":
        leg_verify_child(a)
    if a.leg == "verify":
        res["verify"] = leg_verify(a)
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reloc_verify_bench.json")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
