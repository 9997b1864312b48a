"""Inputs and fp32 / fp64 oracle runs of the pose head's recurrence (lstm1 -> lstm_linear + Mish -> lstm2 -> both regressors;
oracle/clvo_ref.py: clvo_step) for test_recurrence_oracle.py (CPU) and test_gpu_recurrence.py.

A family of inputs is (Bs, amp, s, seed): features [T, Bs, 512] = (base N(0, 0.12) per batch row + cumulative walk N(0, 0.01) +
noise N(0, 0.03)) * amp and an initial state [4, Bs, 512] ~ N(0, s) (s = None: zeros, the caller passes no state). The three
terms come from three seeded RandomStates filled step by step, so a shorter sequence of a family is the prefix of a longer one
and one oracle run serves every length up to its own: the oracle keeps rot, tr and the four state tensors of EVERY step."""
import numpy as np
import torch

from oracle import clvo_ref

STATE_NAMES = ("h1", "c1", "h2", "c2")


def make_feats(T, Bs, amp=1.0, seed=0):
    base = np.random.RandomState(seed).normal(0, 0.12, (1, Bs, 512))
    walk = np.cumsum(np.random.RandomState(seed + 1).normal(0, 0.01, (T, Bs, 512)), axis=0)
    noise = np.random.RandomState(seed + 2).normal(0, 0.03, (T, Bs, 512))
    return torch.from_numpy(((base + walk + noise) * amp).astype(np.float32))


def make_state(Bs, s, seed=0):
    if s is None:
        return None
    return torch.from_numpy(np.random.RandomState(seed + 3).normal(0, s, (4, Bs, 512)).astype(np.float32))


def state_dict_as(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


@torch.no_grad()
def run_oracle(sd, feats, state, dtype):
    """Steps clvo_ref.clvo_step over feats [T, Bs, 512] from state [4, Bs, 512] (None: zeros) in `dtype`. Returns a dict of
    SEPARATE tensors: rot, tr [T, Bs, 3] and h1, c1, h2, c2 [T, Bs, 512] (the state after every step; [-1] is what a scan returns).
    h and c differ by two orders of magnitude once the gates saturate: one stacked comparison would hide h behind c."""
    sd = state_dict_as(sd, dtype)
    T, Bs, _ = feats.shape
    f = feats.to(dtype)
    st = clvo_ref.zero_state(Bs, dtype) if state is None else [state[i].to(dtype) for i in range(4)]
    out = {k: [] for k in ("rot", "tr") + STATE_NAMES}
    for t in range(T):
        r, x, st = clvo_ref.clvo_step(sd, f[t], st)
        out["rot"].append(r)
        out["tr"].append(x)
        for k, v in zip(STATE_NAMES, st):
            out[k].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def prefix(run, T):
    """What a scan of the first T steps returns: rot, tr [T, Bs, 3] and the state after step T - 1 [Bs, 512]."""
    out = {"rot": run["rot"][:T], "tr": run["tr"][:T]}
    for k in STATE_NAMES:
        out[k] = run[k][T - 1]
    return out


@torch.no_grad()
def preactivations(sd, feats, state):
    """The quantities the kernels' gate functions and Mish see, on the fp64 oracle: gate pre-activations of lstm1 and lstm2
    [T, Bs, 2048] and lstm_linear's pre-activation [T, Bs, 512], plus the h1 / c1 sequences. (A restatement of the cell's input
    sums around clvo_step, which computes the states themselves.)"""
    sd = state_dict_as(sd, torch.float64)
    T, Bs, _ = feats.shape
    f = feats.double()
    st = clvo_ref.zero_state(Bs, torch.float64) if state is None else [state[i].double() for i in range(4)]
    lin = torch.nn.functional.linear
    g1, g2, pl, h1s, c1s = [], [], [], [], []
    for t in range(T):
        g1.append(lin(f[t], sd["lstm1.weight_ih"], sd["lstm1.bias_ih"]) + lin(st[0], sd["lstm1.weight_hh"], sd["lstm1.bias_hh"]))
        _, _, new = clvo_ref.clvo_step(sd, f[t], st)
        p = lin(new[0], sd["lstm_linear.linear.weight"], sd["lstm_linear.linear.bias"])
        pl.append(p)
        x2 = torch.nn.functional.mish(p)
        g2.append(lin(x2, sd["lstm2.weight_ih"], sd["lstm2.bias_ih"]) + lin(st[2], sd["lstm2.weight_hh"], sd["lstm2.bias_hh"]))
        st = new
        h1s.append(st[0])
        c1s.append(st[1])
    return {"gate1": torch.stack(g1), "gate2": torch.stack(g2), "lin": torch.stack(pl), "h1": torch.stack(h1s), "c1": torch.stack(c1s)}


# ---- the input families (test_recurrence_oracle.py asserts on the fp64 oracle that each reaches the branch it is there for)
BASE = dict(T=20, Bs=3, amp=1.0, s=0.2, seed=100)   # ordinary scale: every gate pre-activation below ~1.2
SAT30 = dict(amp=30.0, s=1.0, seed=200)      # T = 130: gates around +-22, |c1| beyond 100, h1 pinned at +-1
SAT1000 = dict(amp=1000.0, s=2.0, seed=300)  # T = 24: pre-activations beyond the range of expf
MISH = dict(amp=1.0, s=0.2, seed=400)        # T = 24 on a checkpoint with lstm_linear scaled by MISH_K
MISH_K = 100.0


def mish_state(sd, k=MISH_K):
    """The checkpoint with lstm_linear's weight and bias times k: its pre-activation (and Mish's argument) grows by k."""
    out = {a: b.clone() for a, b in sd.items()}
    out["lstm_linear.linear.weight"] = out["lstm_linear.linear.weight"] * k
    out["lstm_linear.linear.bias"] = out["lstm_linear.linear.bias"] * k
    return out


_CACHE = {}


def cached_oracle(tag, sd, T, Bs, amp, s, seed, dtype):
    """run_oracle on the family's inputs, computed once per (checkpoint tag, family, dtype) for the module that imports this and
    never modified afterwards; a request for a shorter T reuses the longer run (see `prefix`)."""
    key = (tag, Bs, amp, s, seed, dtype)
    if key not in _CACHE or _CACHE[key]["rot"].shape[0] < T:
        _CACHE[key] = run_oracle(sd, make_feats(T, Bs, amp, seed), make_state(Bs, s, seed), dtype)
    return _CACHE[key]
