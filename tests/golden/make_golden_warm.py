"""Golden fixture for transforms.forward_interpolate — the outputs of the REFERENCE's own function, forward_interpolate of
the GMA wheel (core/utils/utils.py:28-56: scipy.interpolate.griddata(method='nearest') on the pushed-forward points).

Run only in the build container (needs /root/reference and scipy; neither travels):

    python tests/golden/make_golden_warm.py

Stores numbers only: the seeded input flows of tests/forward_interpolate_ref.cases() and the wheel's output for each. The
generator asserts that the wheel's output equals the brute-force float64 helper on every stored case (0 differing pixels) and
that every case's smallest gap between best and second-best squared distance is above 1e-9, so no stored case hangs on a tie
(scipy's tie rule is unspecified) or on the last bits of a float64 distance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ROOT, install_stubs  # noqa: E402


def main():
    install_stubs()
    sys.path.insert(0, os.path.join(REF, "GMA-1.0.0-py3-none-any.whl"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from GMA.core.utils.utils import forward_interpolate
    from forward_interpolate_ref import cases, forward_interpolate_ref

    store = {}
    names = []
    for name, h, w, flow in cases():
        got = forward_interpolate(torch.from_numpy(flow)).numpy()
        ref, gap, nvalid = forward_interpolate_ref(flow)
        assert got.dtype == np.float32 and got.shape == flow.shape
        bad = int((got != ref).any(axis=0).sum())
        print("%-22s valid sources %5d of %5d, min gap %.3e, pixels differing from the brute force: %d"
              % (name, nvalid, h * w, gap.min(), bad))
        assert bad == 0, name
        assert gap.min() > 1e-9, (name, gap.min())
        store["in_" + name] = flow
        store["out_" + name] = got
        names.append(name)
    np.savez_compressed(os.path.join(HERE, "warm_start.npz"), names=np.array(names), **store)
    print("written", os.path.join(HERE, "warm_start.npz"))


if __name__ == "__main__":
    main()
