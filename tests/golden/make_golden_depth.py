"""Golden fixture for atdn_vslam_amd.depth — the outputs of the REFERENCE's own read_calib and project_depth
(atdn_vslam/utils/depth.py).

Run only in the build container (needs /root/reference; it never travels):

    python tests/golden/make_golden_depth.py

Stores numbers only: the text of a small KITTI-style calibration file (four rows of twelve numbers, generated here), what
read_calib returns for it with and without `include_rect`, two seeded depth images (5 x 7 and 47 x 154, 0 = no depth at a tenth of
the pixels) and what project_depth returns for each on the CPU. The reference inverts the float32 calibration matrix and
multiplies in float32; `gap_<name>` is the largest absolute difference between that output and the same function of the
reference run on float64 inputs — the reference's own rounding error, which bounds how closely anything can be asked to agree
with it. The generator prints the gaps; tests/test_two_view_host.py allows four times them.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

CASES = [("5x7", 5, 7, 11), ("47x154", 47, 154, 12)]


def calib_text():
    """Four projection rows in KITTI's layout (`P<i>: twelve numbers`): the same intrinsics, another baseline term per row."""
    fx, cx, cy = 718.856, 607.1928, 185.2157
    lines = []
    for i, tx in enumerate((0.0, -386.1448, 45.38225, -337.2877)):
        row = [fx, 0.0, cx, tx, 0.0, fx, cy, 0.1 * i, 0.0, 0.0, 1.0, 0.001 * i]
        lines.append("P%d: " % i + " ".join("%.12e" % v for v in row))
    return "\n".join(lines) + "\n"


def depth_image(h, w, seed):
    r = np.random.RandomState(seed)
    d = r.uniform(2.0, 80.0, (h, w)).astype(np.float32)
    d[r.uniform(size=(h, w)) < 0.1] = 0.0
    return d


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from atdn_vslam.utils.depth import project_depth, read_calib

    text = calib_text()
    store = {"calib_text": np.array(text)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "calib.txt")
        with open(path, "w") as f:
            f.write(text)
        k3 = read_calib(path)
        k4 = read_calib(path, include_rect=True)
    assert tuple(k3.shape) == (3, 3) and tuple(k4.shape) == (4, 4) and k3.dtype == torch.float32
    store["calib_3x3"] = k3.numpy()
    store["calib_4x4"] = k4.numpy().astype(np.float32)
    names = []
    for name, h, w, seed in CASES:
        d = depth_image(h, w, seed)
        got = project_depth(torch.from_numpy(d), k3, device="cpu")
        assert tuple(got.shape) == (3, h, w) and got.dtype == torch.float32
        wide = project_depth(torch.from_numpy(d).double(), k3.double(), device="cpu")
        gap = float((got.double() - wide).abs().max())
        print("%-8s largest |X|: %.3f, float32-against-float64 gap of the reference: %.3e" % (name, float(wide.abs().max()), gap))
        store["depth_" + name] = d
        store["points_" + name] = got.numpy()
        store["gap_" + name] = np.float64(gap)
        names.append(name)
    np.savez_compressed(os.path.join(HERE, "depth.npz"), names=np.array(names), **store)
    print("written", os.path.join(HERE, "depth.npz"))


if __name__ == "__main__":
    main()
