"""The MappingVAE oracle (oracle/vae_ref.py) computes in the dtype of the state dict it is given: with fp64 weights nothing rounds
through fp32 (every tap and `mu` is float64, and the ImageNet constants are the float64 roundings of 0.485 ... 0.225, not the
float32 ones), and at 127x191 its fp32 and fp64 results agree within the tolerance the GPU test states for the HIP path
(tests/test_gpu_slam.py: 5e-5 on |mu| <= 10). The fp32 results themselves are pinned by tests/test_oracle_golden.py."""
import os

import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from oracle import vae_ref

TAPS = tuple("enc%d" % i for i in range(7))
H, W = 127, 191


def _run(sd, frames, dtype):
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    taps = {}
    mu = vae_ref.vae_encode(sd, frames, taps)
    return mu, taps


@pytest.fixture(scope="module")
def runs():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(2, H, W, seed=21))
    return sd, frames, _run(sd, frames, torch.float32), _run(sd, frames, torch.float64)


def test_fp64_oracle_never_rounds_through_fp32(runs):
    sd, frames, (mu32, t32), (mu64, t64) = runs
    assert mu32.dtype == torch.float32 and mu64.dtype == torch.float64
    assert tuple(mu64.shape) == (2, 128, 2, 3)
    for k in TAPS:
        assert t32[k].dtype == torch.float32 and t64[k].dtype == torch.float64, k
    # the frames' own dtype does not matter: the state dict decides (fp32 frames hold 0..255 exactly)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    assert torch.equal(vae_ref.vae_encode(sd64, frames.double()), mu64)
    assert torch.equal(vae_ref.vae_encode(sd, frames.double()), mu32)
    # the normalisation follows its input, constants included: in float64 it is the float64 expression, which differs from the
    # float32 one carried to float64 by a float32 rounding (~1e-7), far above float64's own (~1e-16)
    n64 = vae_ref.normalize_rgb(frames.double())
    assert n64.dtype == torch.float64 and vae_ref.normalize_rgb(frames).dtype == torch.float32
    want = (frames.double() / 255.0 - torch.tensor(vae_ref.RGB_MEAN, dtype=torch.float64).view(1, 3, 1, 1)) \
        / torch.tensor(vae_ref.RGB_STD, dtype=torch.float64).view(1, 3, 1, 1)
    assert torch.equal(n64, want)
    through32 = (frames / 255.0 - torch.tensor(vae_ref.RGB_MEAN).view(1, 3, 1, 1)) / torch.tensor(vae_ref.RGB_STD).view(1, 3, 1, 1)
    assert float((n64 - through32.double()).abs().max()) > 1e-8
    # a stage recomputed in float64 from the float64 tap before it reproduces the next tap exactly; from the float32 tap it cannot
    again = vae_ref._res_block(t64["enc1"], sd64, "encoder.2")
    assert torch.equal(again, t64["enc2"])
    assert not torch.equal(vae_ref._res_block(t32["enc1"].double(), sd64, "encoder.2"), t64["enc2"])


def test_fp32_and_fp64_oracles_agree(runs):
    _, _, (mu32, t32), (mu64, t64) = runs

    def err(a, b):
        return float((a.double() - b).abs().max())

    assert 0.5 < float(mu64.abs().max()) < 10.0           # a real embedding, in the range the 5e-5 of the GPU test assumes
    assert err(mu32, mu64) < 5e-5
    for k in TAPS:
        assert err(t32[k], t64[k]) < 2e-5 * max(1.0, float(t64[k].abs().max())), k   # the atol of test_oracle_golden.py
    # ... and they are not the same computation: fp32 rounding is visible in every stage
    assert all(err(t32[k], t64[k]) > 0 for k in TAPS) and err(mu32, mu64) > 0
