"""Throughput of the HBM flow bank (atdn_vslam_amd/flowbank.py) on one GPU. One leg per call, one JSON line each:

    python tools/bench_flowbank.py --leg build  [--frames 161] [--batch 16]   # bank build, pairs/s, both geometries
    python tools/bench_flowbank.py --leg gather [--reps 50]                   # atdn_flow_gather_clips at 24x6
    python tools/bench_flowbank.py --leg iter   [--steps 10]                  # iteration from the bank vs a resident batch
    python tools/bench_flowbank.py --leg epoch                                # one epoch on a bank of the real size

build: synthetic uint8 frames of 376x1241 in pinned host memory, a synthetic GMA checkpoint, 12 iterations, after one
warm-up sequence. gather: event-timed kernel time and bytes/s against the bytes it moves (fp16 read + fp32 write; run it
under `rocprofv3 --kernel-trace --stats` for the kernel's own figure). iter: the same CLVOTrainer alternates between
steps fed by a gather from the bank (with host targets) and steps on a resident fp32 batch. epoch: 19,330 flows
(the nine training sequences of the reference configuration: 35.8 GB), batch 24 x 6, one full epoch of train_odometry.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from atdn_vslam_amd import evaluation, flowbank as fb, synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")
KITTI_TRAIN_FRAMES = {"00": 4541, "01": 1101, "02": 4661, "03": 801, "04": 271, "06": 1101, "08": 4071, "09": 1591, "10": 1201}


def _poses(n, seed):
    r = np.random.RandomState(seed)
    return evaluation.integrate_motions(r.uniform(-0.02, 0.02, (n - 1, 3)), r.uniform(-0.5, 0.5, (n - 1, 3)))


def _fill(bank, n, seed=1):
    """Synthetic flows in the first n slots (a block of 64 distinct flows repeated)."""
    blk = min(64, n)
    bank.data[:blk].copy_(torch.from_numpy(syn.make_flow(blk, *fb.BANK_HW, seed=seed)).half())
    for s in range(blk, n, blk):
        e = min(s + blk, n)
        bank.data[s:e].copy_(bank.data[:e - s])


def leg_build(a):
    from atdn_vslam_amd.modules import RAFTGMA
    net = RAFTGMA(max_batch=a.batch)
    net.load_state_dict(syn.to_torch(syn.make_gma_state(seed=1)))
    net = net.to(DEV).eval()
    frames = torch.from_numpy(syn.make_frames(a.frames, 376, 1241, seed=4)).to(torch.uint8).pin_memory()
    out = {"leg": "build", "pairs": a.frames - 1, "batch": a.batch}
    for geometry in fb.GEOMETRIES:
        bank = fb.FlowBank(DEV, 2 * (a.frames - 1))
        bank.add_sequence("warm", frames, None, net, geometry=geometry, batch=a.batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bank.add_sequence("timed", frames, None, net, geometry=geometry, batch=a.batch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[geometry + "_pairs_per_s"] = round((a.frames - 1) / dt, 1)
        del bank
    print(json.dumps(out), flush=True)


def leg_gather(a):
    B, T, n = 24, 6, 512
    bank = fb.FlowBank(DEV, n)
    _fill(bank, n)
    r = np.random.RandomState(0)
    out = torch.empty((B, T, 2) + fb.BANK_HW, dtype=torch.float32, device=DEV)
    starts = [r.randint(0, n - T + 1, B) for _ in range(a.reps)]
    revs = [r.randint(0, 2, B) for _ in range(a.reps)]
    for i in range(5):
        fb.gather_clips(bank.data, starts[i], revs[i], T, out=out)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for i in range(a.reps):
        fb.gather_clips(bank.data, starts[i], revs[i], T, out=out)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / a.reps
    moved = B * T * fb.FlowBank.bytes_per_flow() * 3   # fp16 read + fp32 write
    print(json.dumps({"leg": "gather", "B": B, "T": T, "ms_per_call": round(ms, 4), "bytes_moved": moved,
                      "GB_per_s": round(moved / ms / 1e6, 1)}), flush=True)


def leg_iter(a):
    from atdn_vslam_amd.training import CLVOTrainer
    B, T = 24, 6
    n = 512
    bank = fb.FlowBank(DEV, n)
    _fill(bank, n)
    bank._commit(bank._reserve("s", n + 1, _poses(n + 1, 3)))
    seq = bank.sequences[0]
    tr = CLVOTrainer(syn.to_torch(syn.make_clvo_state(seed=1)), B, T, device=DEV, total_steps=4 * a.steps + 8)
    buf = torch.empty((B, T, 2) + fb.BANK_HW, dtype=torch.float32, device=DEV)
    resident = torch.from_numpy(syn.make_flow(B * T, *fb.BANK_HW, seed=9)).view(B, T, 2, *fb.BANK_HW).to(DEV)
    r = np.random.RandomState(1)
    rot0 = torch.from_numpy(r.uniform(-0.02, 0.02, (B, T, 3)).astype(np.float32)).to(DEV)
    tr0 = torch.from_numpy(r.uniform(-0.5, 0.5, (B, T, 3)).astype(np.float32)).to(DEV)

    def from_bank():
        ci = r.randint(0, n - T + 1, B)
        rv = r.randint(0, 2, B)
        bank.gather(seq.first + ci, rv, T, out=buf)
        rot, t_ = fb.batch_targets([seq], np.zeros(B, dtype=np.int64), ci, rv, T)
        tr.step(buf, torch.from_numpy(rot).float(), torch.from_numpy(t_).float())

    def resident_step():
        tr.step(resident, rot0, tr0)

    for f in (from_bank, resident_step, from_bank, resident_step):
        f()
    torch.cuda.synchronize()
    times = {"bank": [], "resident": []}
    for _ in range(a.rounds):
        for name, f in (("bank", from_bank), ("resident", resident_step)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    mb, mr = float(np.median(times["bank"])), float(np.median(times["resident"]))
    print(json.dumps({"leg": "iter", "B": B, "T": T, "ms_bank": round(mb, 3), "ms_resident": round(mr, 3),
                      "overhead_pct": round(100 * (mb / mr - 1), 2), "rounds": times}), flush=True)


def leg_epoch(a):
    from atdn_vslam_amd import train_odometry as tro
    n = sum(v - 1 for v in KITTI_TRAIN_FRAMES.values())
    t0 = time.perf_counter()
    bank = fb.FlowBank(DEV, n)
    _fill(bank, n)
    for k, (name, f) in enumerate(KITTI_TRAIN_FRAMES.items()):
        bank._commit(bank._reserve(name, f, _poses(f, k)))
    torch.cuda.synchronize()
    t_fill = time.perf_counter() - t0
    cfg = tro.Config(batch_size=24, sequence_length=6, epochs=1, lr=1e-3, wd=1e-3, epsilon=1e-8, stage=1, alpha=1, w=3,
                     augment_flow=False, train_sequences=list(KITTI_TRAIN_FRAMES))
    steps = []
    t1 = time.perf_counter()
    _, hist = tro.train(cfg, bank, DEV, save=False, on_step=lambda *x: steps.append(time.perf_counter()))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    print(json.dumps({"leg": "epoch", "flows": n, "bank_GB": round(n * fb.FlowBank.bytes_per_flow() / 1e9, 2),
                      "iterations": len(hist[0]), "epoch_s": round(dt, 2), "ms_per_iteration": round(1e3 * dt / len(hist[0]), 3),
                      "fill_s": round(t_fill, 2), "loss_first": hist[0][0], "loss_last": hist[0][-1],
                      "finite": bool(np.isfinite(hist[0]).all())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=("build", "gather", "iter", "epoch"))
    ap.add_argument("--frames", type=int, default=161)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.set_device(DEV)
    {"build": leg_build, "gather": leg_gather, "iter": leg_iter, "epoch": leg_epoch}[a.leg](a)


if __name__ == "__main__":
    main()
