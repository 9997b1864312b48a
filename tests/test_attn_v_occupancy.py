"""Register and LDS guard for attention x V (no GPU: reads the code objects of the built library, as tests/test_run_tile_occupancy.py
does for the run-tile kernels). attn_v3_kernel is an eight-wave block — two waves per SIMD — that holds 64 accumulator
registers, the operands of a chunk and three chunks of attention per wave: it needs 256 registers or fewer and no spill to be
launchable as designed, and its three-image ring of motion-feature chunks has to fit the CU's LDS."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024   # gfx950


@pytest.mark.timeout(900)
def test_attention_v_kernels_fit_256_registers_without_spills():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the ROCm LLVM tools to read the code objects")
    if not (shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt")):
        pytest.skip("no demangler (c++filt / llvm-cxxfilt): the kernels are found by their demangled names")
    from atdn_vslam_amd import _lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "diag", "kernel_regs.py"), _lib.LIB_PATH, "attn_v3_kernel<"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines()[1:]:
        name, rest = line[:140].strip(), line[140:].split()
        if len(rest) == 5:
            v, _, sp, lds, w = (int(x) for x in rest)
            got[name.split("(")[0]] = (v, sp, lds, w)
    # the four forms the product launches: split-f16 and f16 fast mode, one block per tile and the key-split (low-latency) form
    for fast in ("false", "true"):
        for split in ("false", "true"):
            name = "void attn_v3_kernel<%s, %s>" % (fast, split)
            assert name in got, "missing from the library: %s (has %s)" % (name, sorted(got))
    bad = ["%s: %d registers, %d spilled, %d B LDS" % ((k,) + v[:3]) for k, v in sorted(got.items())
           if v[0] > 256 or v[1] > 0 or v[2] > LDS_PER_CU]
    assert not bad, "attention x V must stay within 256 registers, spill nothing and fit one block's LDS on a CU:\n" + "\n".join(bad)
