"""Windowed bundle adjustment, host form (no GPU): transforms.bundle_adjust / bundle_terms on CPU tensors against the NumPy
restatement tests/bundle_ref.py bit for bit, convergence on exact and on noisy flows, degenerate cases and argument errors."""
import numpy as np
import pytest
import torch

import bundle_ref as br
from atdn_vslam_amd import transforms as T


def _t(sc, slots, init, mask):
    return (torch.from_numpy(sc["acc"]), torch.from_numpy(sc["alive"]), torch.from_numpy(sc["poses"]), torch.from_numpy(slots),
            sc["calib"], torch.from_numpy(init), None if mask is None else torch.from_numpy(mask))


def test_reference_cases_take_every_branch():
    br.check_branches(4)


@pytest.mark.parametrize("iters", [0, 1, 4])
@pytest.mark.parametrize("case", br.CASES, ids=[c[0] for c in br.CASES])
def test_host_form_equals_reference_bit_for_bit(case, iters):
    sc, slots, init, mask, ref = br.reference(case, iters)
    got = T.bundle_adjust(*_t(sc, slots, init, mask), iters=iters, **case[8])
    for name, g, r in zip(("poses", "depth", "cost", "counts"), got, ref[:4]):
        assert br.same_bits64(g.numpy(), r), (case[0], iters, name)


@pytest.mark.parametrize("case", br.CASES, ids=[c[0] for c in br.CASES])
def test_terms_equal_reference_bit_for_bit(case):
    sc, slots, init, mask, ref = br.reference(case, 0)
    sums, counts = T.bundle_terms(*_t(sc, slots, init, mask), **case[8])
    assert tuple(sums.shape) == (case[3], T.bundle_sums(case[4])) and T.bundle_sums(case[4]) == br.n_sums(case[4])
    assert br.same_bits64(sums.numpy(), np.stack([o["sums0"] for o in ref[4]]))
    assert br.same_bits64(counts.numpy(), np.stack([o["counts0"] for o in ref[4]]))
    # the cost of evaluation 0 of a solve is the cost of the terms
    assert br.same_bits64(sums[:, -1].numpy(), ref[2][:, 0])


def _converge(H, W, S, seed, opts, stride, iters):
    """(reference result, rotation and translation errors before, after) of one problem over slots 0 .. S-1."""
    sc, slots, init, _ = br.case_inputs(H, W, 1, S, S, seed, opts)
    slots[0] = np.arange(S)
    o = br.bundle_ref(sc["acc"], sc["alive"], sc["poses"], slots[0], sc["calib"], init[0, 0], None, stride=stride, iters=iters)
    g, j = o["held"] // 6, o["held"] % 6 - 3
    before = br.pose_errors(sc["poses"][slots[0]], sc["true_poses"][slots[0]], g, j)
    after = br.pose_errors(o["poses"], sc["true_poses"][slots[0]], g, j)
    got = T.bundle_adjust(*_t(sc, slots, init, None), stride=stride, iters=iters)
    assert br.same_bits64(got[0].numpy()[0], o["poses"]) and br.same_bits64(got[2].numpy()[0], o["cost"])
    return o, before, after


def test_exact_flows_converge_to_the_true_poses():
    """noise = 0 at 24 x 40, S = 4, stride 1, 10 steps: every view's rotation error < 1e-5 rad and its translation error in the
    held gauge < 1e-4 m (the float32 rounding of the output poses)."""
    o, before, after = _converge(24, 40, 4, 9, dict(noise=0.0), 1, 10)
    print("exact: rot %s -> %s, tr %s -> %s, costs %s" % (before[0], after[0], before[1], after[1], o["costs"]))
    assert after[0].max() < 1e-5 and after[1].max() < 1e-4


def test_noisy_flows_cost_never_increases_and_errors_halve():
    """47 x 154, S = 8 (noise 0.3, outliers 0.1): the cost never increases and the median rotation and translation errors end
    below half their initial values."""
    o, before, after = _converge(47, 154, 8, 5, dict(noise=0.3, outliers=0.1), 1, 10)
    print("noisy: rot %s -> %s, tr %s -> %s, costs %s" % (np.median(before[0]), np.median(after[0]), np.median(before[1]),
                                                          np.median(after[1]), o["costs"]))
    assert all(b <= a for a, b in zip(o["costs"], o["costs"][1:]))
    assert np.median(after[0]) < 0.5 * np.median(before[0]) and np.median(after[1]) < 0.5 * np.median(before[1])


def test_zero_gauge_translation_returns_the_inputs():
    sc, slots, init, mask = br.case_inputs(9, 33, 1, 3, 3, 4, dict(noise=0.1))
    poses = sc["poses"].copy()
    poses[slots[0, -1]].reshape(3, 4)[:, 3] = 0.0
    sc = dict(sc, poses=poses)
    got = T.bundle_adjust(*_t(sc, slots, init, mask), stride=1, iters=3)
    ref = br.reference_batch(sc["acc"], sc["alive"], poses, slots, sc["calib"], init, mask, stride=1, iters=3)
    assert ref[4][0]["held"] == -1
    for g, r in zip(got, ref[:4]):
        assert br.same_bits64(g.numpy(), r)
    assert br.same_bits64(got[0].numpy()[0], poses[slots[0]]) and int(got[3][0, 3]) == 0 and int(got[3][0, 0]) > 0
    cand = got[1].numpy() != 0
    assert br.same_bits64(got[1].numpy()[cand], init[cand]) and got[2][0, 0] == got[2][0, 1]


def test_single_view_and_no_candidates():
    sc, slots, init, mask = br.case_inputs(9, 33, 1, 1, 2, 4, dict(noise=0.1))
    got = T.bundle_adjust(*_t(sc, slots, init, None), stride=1, iters=3, min_views=1)
    ref = br.reference_batch(sc["acc"], sc["alive"], sc["poses"], slots, sc["calib"], init, None, stride=1, iters=3, min_views=1)
    for g, r in zip(got, ref[:4]):
        assert br.same_bits64(g.numpy(), r)
    assert int(got[3][0, 0]) > 0
    none = T.bundle_adjust(*_t(sc, slots, init, np.zeros_like(mask)), stride=1, iters=3, min_views=1)
    assert none[3][0].tolist() == [0, 0, 0, 0] and not none[1].any() and none[2][0].tolist() == [0.0, 0.0]
    assert br.same_bits64(none[0].numpy()[0], sc["poses"][slots[0]])


def test_argument_errors():
    sc, slots, init, mask = br.case_inputs(9, 33, 1, 3, 3, 4, {})
    a = _t(sc, slots, init, mask)
    for f in (T.bundle_adjust, T.bundle_terms):
        with pytest.raises(RuntimeError, match="flow bank"):
            f(a[0][:, :1], *a[1:])
        with pytest.raises(RuntimeError, match="liveness"):
            f(a[0], a[1][:, :4], *a[2:])
        with pytest.raises(RuntimeError, match="poses"):
            f(a[0], a[1], a[2][:2], *a[3:])
        with pytest.raises(RuntimeError, match="slots"):
            f(a[0], a[1], a[2], torch.zeros((1, 1, 3), dtype=torch.int32), *a[4:])
        with pytest.raises(RuntimeError, match="depth"):
            f(*a[:5], None)
        with pytest.raises(RuntimeError, match="depth"):
            f(*a[:5], a[5][:, :, :4])
        with pytest.raises(RuntimeError, match="mask"):
            f(*a[:6], a[6][:, :4])
        with pytest.raises(RuntimeError, match="stride"):
            f(*a, stride=0)
        with pytest.raises(RuntimeError, match="min_views"):
            f(*a, min_views=4)
        with pytest.raises(RuntimeError, match="min_views"):
            f(*a, min_views=0)
        with pytest.raises(RuntimeError, match="scale_px"):
            f(*a, scale_px=0.0)
        with pytest.raises(RuntimeError, match="min_z"):
            f(*a, min_z=float("nan"))
        with pytest.raises(RuntimeError, match="ATDN_MULTIVIEW_MAX_VIEWS"):
            f(a[0], a[1], a[2], torch.zeros((1, 17), dtype=torch.int32), *a[4:])
    with pytest.raises(RuntimeError, match="iters"):
        T.bundle_adjust(*a, iters=17)
    with pytest.raises(RuntimeError, match="iters"):
        T.bundle_adjust(*a, iters=-1)
