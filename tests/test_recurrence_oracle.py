"""The yardstick of tests/test_gpu_recurrence.py, checked where no GPU is needed: Checker(M_ENC, FLOOR_ENC) against the fp64 oracle
must flag every single-point error of the recurrence by a wide margin and pass the fp32 oracle itself, and the saturating input
families must reach what they claim to reach (gate pre-activations beyond 20 / 100, lstm_linear's beyond +-20)."""
import os
import sys

import pytest
import torch

from atdn_vslam_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrence_ref as rr  # noqa: E402
from recurrence_ref import BASE, MISH, MISH_K, SAT30, SAT1000, mish_state  # noqa: E402
from parity_check import CAP, Checker  # noqa: E402

M_ENC, FLOOR_ENC = 2.5, 1e-6      # as tests/test_gpu_train_geometry.py and tests/test_gpu_recurrence.py
MARGIN = 10.0                     # every mutation moves rot and tr by at least 10x the bound (measured: >= 100x)
UNIT = 37                         # the hidden unit the single-unit mutations hit


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def base(sd):
    f, st = rr.make_feats(BASE["T"], BASE["Bs"], BASE["amp"], BASE["seed"]), rr.make_state(BASE["Bs"], BASE["s"], BASE["seed"])
    return f, st, rr.run_oracle(sd, f, st, torch.float32), rr.run_oracle(sd, f, st, torch.float64)


def _zeroed(sd, key, *index):
    out = {k: v.clone() for k, v in sd.items()}
    assert float(out[key][index].abs()) > 1e-3, (key, index)   # zeroing a value that is already ~0 would be no mutation
    out[key][index] = 0.0
    return out


def _stale_feature(f):
    f = f.clone()
    f[-1, -1] = f[-2, -1]
    return f


def _state_with(st, fn):
    st = st.clone()
    fn(st)
    return st


def _swap_c1(st):
    st[1, [0, 1]] = st[1, [1, 0]]


def _zero_h2(st):
    st[2] = 0.0


def _zero_c2(st):
    st[3] = 0.0


# name -> (state dict, features, initial state) of the mutated fp64 run
MUTATIONS = {
    "lstm2.bias_hh of one unit's o gate zeroed": lambda sd, f, st: (_zeroed(sd, "lstm2.bias_hh", 3 * 512 + UNIT), f, st),
    "lstm1.bias_hh of one unit's i gate zeroed": lambda sd, f, st: (_zeroed(sd, "lstm1.bias_hh", 0 * 512 + UNIT), f, st),
    "one element of lstm2.weight_hh zeroed": lambda sd, f, st: (_zeroed(sd, "lstm2.weight_hh", 2 * 512 + UNIT, 5), f, st),
    "lstm_linear bias of one unit zeroed": lambda sd, f, st: (_zeroed(sd, "lstm_linear.linear.bias", UNIT), f, st),
    "last step's last batch row reads the previous step's feature": lambda sd, f, st: (sd, _stale_feature(f), st),
    "c1 of batch rows 0 and 1 swapped": lambda sd, f, st: (sd, f, _state_with(st, _swap_c1)),
    "initial h2 ignored": lambda sd, f, st: (sd, f, _state_with(st, _zero_h2)),
    "initial c2 ignored": lambda sd, f, st: (sd, f, _state_with(st, _zero_c2)),
}


def _bound(x32, x64):
    scale, e32 = float(x64.abs().max()), float((x32.double() - x64).abs().max())
    return min(M_ENC * e32 + FLOOR_ENC * scale, CAP * scale)


def test_the_fp32_oracle_passes_its_own_yardstick(base):
    _, _, o32, o64 = base
    chk = Checker("oracle32/T20/B3", M_ENC, FLOOR_ENC)
    for k in ("rot", "tr") + rr.STATE_NAMES:
        chk(k, o32[k], o32[k], o64[k])
    chk.finish()
    # the bound the GPU tests work with sits near 1e-7, two orders below the 1e-5 most head tests use
    assert _bound(o32["rot"], o64["rot"]) < 3e-7 and _bound(o32["tr"], o64["tr"]) < 3e-7


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_single_point_error_is_flagged_by_a_wide_margin(sd, base, name):
    f, st, o32, o64 = base
    mut = rr.run_oracle(*MUTATIONS[name](sd, f, st), torch.float64)
    chk = Checker("mutation/" + name, M_ENC, FLOOR_ENC)
    for k in ("rot", "tr"):
        chk(k, mut[k], o32[k], o64[k])
        dev, bound = float((mut[k] - o64[k]).abs().max()), _bound(o32[k], o64[k])
        print("MUTATION %s %s dev=%.3e bound=%.3e ratio=%.0f" % (name, k, dev, bound, dev / bound))
        assert dev >= MARGIN * bound, (name, k, dev, bound)
    assert len(chk.bad) == 2, chk.bad   # rot and tr are both flagged
    with pytest.raises(AssertionError):
        chk.finish()


# ---- the input families of test_gpu_recurrence.py: each must reach the branch it is there for (fp64 oracle)
def _finite(run):
    return all(bool(torch.isfinite(v).all()) for v in run.values())


@pytest.mark.parametrize("Bs", [1, 5])
def test_the_amp30_family_saturates_the_gates(sd, Bs):
    f, st = rr.make_feats(130, Bs, SAT30["amp"], SAT30["seed"]), rr.make_state(Bs, SAT30["s"], SAT30["seed"])
    p = rr.preactivations(sd, f, st)
    gate = max(float(p["gate1"].abs().max()), float(p["gate2"].abs().max()))
    pinned = float((p["h1"].abs() > 0.99).double().mean())
    print("COVERAGE amp30 Bs=%d max|gate|=%.1f max|c1|=%.1f h1 beyond 0.99: %.3f" % (Bs, gate, float(p["c1"].abs().max()), pinned))
    assert gate >= 20.0 and float(p["c1"].abs().max()) >= 100.0 and pinned >= 0.02
    assert _finite(rr.run_oracle(sd, f, st, torch.float32))


@pytest.mark.parametrize("Bs", [1, 2])
def test_the_amp1000_family_leaves_the_range_of_expf(sd, Bs):
    f, st = rr.make_feats(24, Bs, SAT1000["amp"], SAT1000["seed"]), rr.make_state(Bs, SAT1000["s"], SAT1000["seed"])
    p = rr.preactivations(sd, f, st)
    gate = float(p["gate1"].abs().max())
    print("COVERAGE amp1000 Bs=%d max|gate1|=%.1f" % (Bs, gate))
    assert gate >= 100.0    # expf overflows beyond 88.7, exp2 beyond 128
    assert _finite(rr.run_oracle(sd, f, st, torch.float32))


@pytest.mark.parametrize("Bs", [1, 2])
def test_the_scaled_lstm_linear_reaches_both_mish_extremes(sd, Bs):
    sdk = mish_state(sd)
    f, st = rr.make_feats(24, Bs, MISH["amp"], MISH["seed"]), rr.make_state(Bs, MISH["s"], MISH["seed"])
    lin = rr.preactivations(sdk, f, st)["lin"]
    hi, lo = float((lin > 20.0).double().mean()), float((lin < -20.0).double().mean())
    print("COVERAGE mish k=%g Bs=%d above +20: %.4f below -20: %.4f range [%.1f, %.1f]" % (MISH_K, Bs, hi, lo, float(lin.min()), float(lin.max())))
    assert hi >= 0.01 and lo >= 0.01
    assert _finite(rr.run_oracle(sdk, f, st, torch.float32))
