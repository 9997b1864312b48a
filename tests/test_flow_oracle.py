"""The GMA flow oracle (oracle/gma_ref.py) computes in the dtype it is given: with fp64 weights and frames nothing rounds
through fp32 (every output and tap is float64), and at C1 (160x512, 20x64 grid) its fp32 and fp64 results agree within the
tolerances the GPU tests state for the HIP path (tests/test_gpu_parity.py). The fp32 results themselves are pinned bit for bit
by tests/test_oracle_golden.py."""
import os

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from oracle import gma_ref

TAPS = ("fmap1", "fmap2", "net0", "inp", "attn", "lookup0", "mf0", "mfg0", "net1", "delta0", "net_final", "mask")


def _run(sd, fr, dtype, iters):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    fr = fr.to(dtype)
    taps, preds = {}, []
    low, up = gma_ref.gma_forward(sd, fr[0:1], fr[1:2], iters=iters, taps=taps, predictions=preds)
    return low, up, taps, preds


@pytest.fixture(scope="module")
def c1(golden_dir):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    g = np.load(os.path.join(golden_dir, "gma_c1.npz"))
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    fr = torch.from_numpy(syn.make_frames(2, 160, 512, seed=int(g["seed_frames"])))
    iters = int(g["iters"])
    return _run(sd, fr, torch.float32, iters), _run(sd, fr, torch.float64, iters), iters


def test_fp64_oracle_never_rounds_through_fp32(c1):
    (_, _, _, _), (low, up, taps, preds), iters = c1
    assert low.dtype == torch.float64 and up.dtype == torch.float64
    assert tuple(low.shape) == (1, 2, 20, 64) and tuple(up.shape) == (1, 2, 160, 512)
    for k in TAPS:
        assert taps[k].dtype == torch.float64, k
    assert len(taps["pyramid"]) == 4 and all(p.dtype == torch.float64 for p in taps["pyramid"])
    assert len(preds) == iters and all(p.dtype == torch.float64 for p in preds)
    # the helpers follow their inputs too
    assert gma_ref.coords_grid(1, 3, 5, torch.float64).dtype == torch.float64
    assert gma_ref.coords_grid(1, 3, 5).dtype == torch.float32
    look = gma_ref.corr_lookup(taps["pyramid"], gma_ref.coords_grid(1, 20, 64, torch.float64) + 0.37)
    assert look.dtype == torch.float64
    assert torch.equal(preds[-1], up)


def test_fp32_and_fp64_oracles_agree_at_c1(c1):
    (l32, u32, t32, p32), (l64, u64, t64, p64), iters = c1

    def err(a, b):
        return float((a.double() - b).abs().max())

    assert float(l64.abs().max()) > 1.0                      # a real flow, not a near-zero one
    assert err(l32, l64) < 2e-4 and err(u32, u64) < 1e-3
    for it in range(iters):
        assert err(p32[it], p64[it]) < 1e-3, it
    for k in ("fmap1", "fmap2", "net0", "inp", "lookup0", "mf0", "mfg0", "net1", "delta0", "net_final", "mask"):
        assert err(t32[k], t64[k]) < 1e-4, k
    for lvl in range(4):
        assert err(t32["pyramid"][lvl], t64["pyramid"][lvl]) < 1e-4, lvl
    assert err(t32["attn"], t64["attn"]) < 1e-6 + 1e-4 * float(t64["attn"].max())
    # ... and they are not the same computation: fp32 rounding is visible in every stage
    assert err(t32["fmap1"], t64["fmap1"]) > 0 and err(l32, l64) > 0
