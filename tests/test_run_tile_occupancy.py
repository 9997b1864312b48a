"""Occupancy guard for the run-tile kernels of the ConvGRU convolutions (no GPU: reads the code objects of the built library, as
tests/test_kernel_occupancy.py does for the kernels of its table). conv_sf6_run_kernel<KH, KW, SfGruZR | SfGruQ, false> are the
largest kernels of the 16-pair forward and sit at 254 of the 256 registers that allow two waves per SIMD: three more registers, or
a spill, would cost every gate launch and no parity test would notice."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_run_tile_kernels_keep_two_waves_per_simd_and_do_not_spill():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the ROCm LLVM tools to read the code objects")
    if not (shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or os.path.exists("/opt/rocm/lib/llvm/bin/llvm-cxxfilt")):
        pytest.skip("no demangler (c++filt / llvm-cxxfilt): the kernels are found by their demangled names")
    from atdn_vslam_amd import _lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "diag", "kernel_regs.py"), _lib.LIB_PATH, "conv_sf6_run_kernel<"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines()[1:]:
        name, rest = line[:140].strip(), line[140:].split()
        if len(rest) == 5:
            v, _, sp, lds, w = (int(x) for x in rest)
            got[name] = (v, sp, lds, w)
    # the kernels the product launches: both passes, both gates and the context convolutions, split-f16 and f16 fast mode
    for kh, kw in ((1, 5), (5, 1)):
        for epi in ("SfGruZR", "SfGruQ", "EpiBias<0>"):
            for fast in ("false", "true"):
                name = "void conv_sf6_run_kernel<%d, %d, %s, %s>(Conv2Geom, %s)" % (kh, kw, epi, fast, epi)
                assert name in got, "missing from the library: %s (has %s)" % (name, sorted(got)[:3])
    bad = ["%s: %d registers, %d spilled, %d B LDS, %d waves per SIMD" % ((k,) + v) for k, v in sorted(got.items()) if v[1] > 0 or v[3] < 2]
    assert not bad, "run-tile kernels must spill nothing and keep two waves per SIMD:\n" + "\n".join(bad)
