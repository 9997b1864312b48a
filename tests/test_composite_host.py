"""Host-side checks of the composite pose loss (no GPU): the C ABI declares it, the training driver hands `alpha`, `w` and
the mode to the trainer and validates them before any GPU work, and the differentiable restatement the GPU tests use as
their gradient yardstick (tests/composite_ref.py) has the value the reference's CLVO_Loss has (tests/golden/composite.npz)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, flowbank as fb, train_odometry as tro, training

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((1, 3, 3, 0.5), (2, 4, 3, 0.5), (3, 5, 3, 0.25), (2, 6, 2, 0.0), (5, 6, 1, 0.3), (3, 6, 6, 0.7), (24, 6, 3, 0.5),
         (300, 3, 2, 0.5))


def test_new_symbols_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "atdn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("atdn_clvo_loss", "atdn_clvo_trainer_set_loss", "atdn_clvo_trainer_loss_terms"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["atdn_clvo_loss"][1]) == 13
    assert len(_lib.SIGNATURES["atdn_clvo_trainer_set_loss"][1]) == 4


def test_fixture_holds_the_cases_and_their_condition(golden_dir):
    g = np.load(os.path.join(golden_dir, "composite.npz"))
    assert [tuple(c) for c in g["cases"].tolist()] == [tuple(float(x) for x in c) for c in CASES]
    for i, (B, T, w, alpha) in enumerate(CASES):
        assert g["pred_rot%d" % i].shape == (B, T, 3) and g["true_tr%d" % i].dtype == np.float32
        assert float(g["max_c12_%d" % i]) <= 0.9 and float(g["max_angle_%d" % i]) <= 2.5
        # the reference's own fp32 evaluation against the float64 oracle: what the GPU tests' loss bound is ten times of
        l64 = float(g["loss64_%d" % i])
        assert abs(float(g["ref_loss%d" % i]) - l64) <= float(g["ref_worst_deviation"]) * max(1.0, l64) * (1 + 1e-9)
    assert float(g["tol_loss"]) == max(3e-6, 10 * float(g["ref_worst_deviation"]))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_differentiable_restatement_has_the_reference_value(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "composite.npz"))
    B, T, w, alpha = CASES[case]
    x = [torch.from_numpy(g["%s%d" % (k, case)]).double() for k in ("pred_rot", "pred_tr", "true_rot", "true_tr")]
    rel, com = cr.clvo_loss_terms(*x, w)
    for got, want in ((float(cr.clvo_loss(*x, alpha, w)), float(g["loss64_%d" % case])), (float(rel), float(g["rel64_%d" % case])),
                      (float(com), float(g["com64_%d" % case]))):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    # and the reference's own fp32 number, to what fp32 can show
    assert abs(float(cr.clvo_loss(*x, alpha, w)) - float(g["ref_loss%d" % case])) <= 3e-7 * max(1.0, float(g["ref_loss%d" % case]))


class _StubBank:
    """What train() needs from a FlowBank, on the host: two short sequences of identity poses and a gather that does nothing."""
    hw = (8, 16)

    def __init__(self):
        self.sequences = [fb.Sequence("00", 0, 12, np.tile(np.eye(4), (12, 1, 1))), fb.Sequence("01", 11, 9, np.tile(np.eye(4), (9, 1, 1)))]

    def sequence(self, name):
        return [s for s in self.sequences if s.name == name][0]

    def gather(self, start, reverse, T, out=None):
        return out


class _StubTrainer:
    built = []

    def __init__(self, state, batch_size, sequence_length, **kw):
        self.args = dict(kw, batch_size=batch_size, sequence_length=sequence_length)
        self.steps = 0
        _StubTrainer.built.append(self)

    def step(self, flows, rot, tr):
        self.steps += 1
        return 1.5


def _cfg(**kw):
    d = dict(batch_size=2, sequence_length=4, epochs=1, lr=1e-3, wd=1e-3, epsilon=1e-8, stage=1, alpha=1, w=3, augment_flow=False,
             train_sequences=["00", "01"], weight_file="unused", log_file="unused", data_path="unused")
    d.update(kw)
    return tro.Config(**d)


@pytest.fixture
def stub_trainer(monkeypatch):
    _StubTrainer.built = []
    monkeypatch.setattr(training, "CLVOTrainer", _StubTrainer)
    return _StubTrainer


@pytest.mark.parametrize("mode", ["reference", "gradient"])
def test_train_hands_alpha_w_and_mode_to_the_trainer(stub_trainer, mode):
    trainer, hist = tro.train(_cfg(alpha=0.5, w=2), _StubBank(), "cpu", save=False, composite=mode)
    assert len(stub_trainer.built) == 1 and trainer.steps > 0 and hist[0] == [1.5] * trainer.steps
    a = trainer.args
    assert (a["alpha"], a["w"], a["composite"]) == (0.5, 2, mode)
    assert (a["batch_size"], a["sequence_length"]) == (2, 4)


def test_train_without_a_mode_builds_the_trainer_as_before(stub_trainer):
    trainer, _ = tro.train(_cfg(), _StubBank(), "cpu", save=False)
    assert not {"alpha", "w", "composite"} & set(trainer.args)


def test_alpha_without_a_mode_is_still_refused(stub_trainer):
    with pytest.raises(NotImplementedError, match="alpha = 1"):
        tro.train(_cfg(alpha=0.5), _StubBank(), "cpu", save=False)
    with pytest.raises(NotImplementedError):
        tro.check_alpha(_cfg(alpha=0.5))
    assert stub_trainer.built == []


@pytest.mark.parametrize("w", [0, 5, -1])
def test_window_outside_the_clip_is_refused_before_a_trainer_is_built(stub_trainer, w):
    with pytest.raises(ValueError, match="sequence_length"):
        tro.train(_cfg(alpha=0.5, w=w), _StubBank(), "cpu", save=False, composite="gradient")
    with pytest.raises(ValueError):
        tro.check_alpha(_cfg(alpha=0.5, w=w), "reference")
    assert stub_trainer.built == []
    tro.check_alpha(_cfg(alpha=0.5, w=4), "reference")   # w = sequence_length is a window


def test_unknown_mode_is_refused(stub_trainer):
    with pytest.raises(ValueError, match="composite"):
        tro.train(_cfg(alpha=0.5), _StubBank(), "cpu", save=False, composite="detached")
    with pytest.raises(ValueError, match="composite"):
        training.composite_mode("both")
    assert stub_trainer.built == []


def test_command_line_takes_the_flag(tmp_path, monkeypatch):
    """--composite reaches train() with the YAML's alpha and w; without it alpha = 0.5 stops main() before any GPU call."""
    p = tmp_path / "config.yaml"
    p.write_text("alpha: 0.5\nw: 2\nbatch_size: 2\ndata_path: unused\nepochs: 1\nepsilon: 1.0e-08\nweight_file: unused\nlog_file: unused\n"
                 "lr: 0.01\nstage: 1\nsequence_length: 4\ntrain_sequences: ['00']\nwd: 0.001\naugment_flow: false\n")
    with pytest.raises(NotImplementedError):
        tro.main(["--config", str(p), "--flows2"])
    seen = {}
    monkeypatch.setattr(tro, "build_bank", lambda cfg, dev, **kw: _StubBank())
    monkeypatch.setattr(tro, "train", lambda cfg, bank, dev, **kw: seen.update(kw, alpha=cfg.alpha, w=cfg.w))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    tro.main(["--config", str(p), "--flows2", "--composite", "gradient"])
    assert (seen["composite"], seen["alpha"], seen["w"]) == ("gradient", 0.5, 2)
