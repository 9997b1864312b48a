"""The failure path of the device-memory owner (atdn_vslam_amd/csrc/device_buf.h), on a machine without a GPU: there every
hipMalloc fails cleanly, so tools/diag/device_buf_host_check.cpp drives alloc() / reserve() through their failing branch and
checks that a buffer never keeps a size without memory. Compiled here without sanitizers; DESIGN.md "Device memory ownership"
gives the AddressSanitizer + UBSan command."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_failed_allocation_leaves_the_buffer_empty(tmp_path):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is visible: the failing branch comes from having none")
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    exe = str(tmp_path / "device_buf_host_check")
    r = subprocess.run([HIPCC, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "diag", "device_buf_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    if r.returncode == 2:
        pytest.skip("a GPU is visible: the failing branch comes from having none")
    assert r.returncode == 0, r.stdout[-2000:]
    assert "0 bytes live" in r.stdout
