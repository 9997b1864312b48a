"""Rate of the range-probe kernel (csrc/range_probe.hip, a pure read) against the float4-copy rate of tools/microbench_stream.py
measured in the SAME process: device events around >= 200 launches per tensor.

    python tools/bench_range_probe.py [--launches 200] [--out profiles/range_probe_bench.json]

Needs the diagnostic library as well (python -m atdn_vslam_amd.build --microbench)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from atdn_vslam_amd import _lib  # noqa: E402

DEV = "cuda:0"

# (label, rows, cols, pitch): dense tensors of 16 MB, 210 MB (the KITTI-size correlation volume of one pair), 1 GiB and 4.3 GB,
# and the two padded shapes of the flow network (attention rows with pitch ldN, motion features inside the GRU input)
CASES = [
    ("16 MB dense", 1, 4 << 20, 4 << 20),
    ("210 MB dense (7238 x 7238)", 7238, 7238, 7238),
    ("1 GiB dense", 1, 1 << 28, 1 << 28),
    ("4.3 GB dense (2^30 + 12 values)", 1, (1 << 30) + 12, (1 << 30) + 12),
    ("7238 x 7238, pitch 7264", 7238, 7238, 7264),
    ("7238 x 126, pitch 384", 7238, 126, 384),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    mb = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libatdn_microbench.so"))
    mb.atdn_microbench_stream.argtypes = [C.c_long, C.c_int, C.POINTER(C.c_float)]
    rates = (C.c_float * 7)()
    assert mb.atdn_microbench_stream(1 << 30, 10, rates) == 0
    copy_gbs, load_gbs = float(rates[3]), float(rates[2])
    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches,
           "same_job_copy_GBps_1GiB": round(copy_gbs, 1), "same_job_16B_loads_GBps_1GiB": round(load_gbs, 1), "cases": []}
    print("same job, 1 GiB: float4 copy %.0f GB/s (read + write bytes), 16-byte loads %.0f GB/s" % (copy_gbs, load_gbs), flush=True)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slot = torch.zeros(6, dtype=torch.int32, device=DEV)
    for label, rows, cols, ld in CASES:
        n = (rows - 1) * ld + cols
        x = torch.empty(n, dtype=torch.float32, device=DEV)
        x.normal_()
        slot.zero_()

        def launch():
            _lib.check(L.atdn_range_probe_launch(C.c_void_p(x.data_ptr()), rows, cols, ld, C.c_void_p(slot.data_ptr()), st))
        for _ in range(5):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.launches
        gbs = rows * cols * 4 / (us * 1e-6) / 1e9
        row = {"case": label, "rows": rows, "cols": cols, "pitch": ld, "valid_MB": round(rows * cols * 4 / 1e6, 1),
               "us_per_launch": round(us, 2), "GBps_valid_bytes": round(gbs, 1), "share_of_same_job_copy": round(gbs / copy_gbs, 3)}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
