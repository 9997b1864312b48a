"""Host-side checks of the flow bank and the training / evaluation drivers (no GPU): the sampler, targets and initial
weights against the reference (tests/golden/flowbank.npz, tests/golden/make_golden_flowbank.py), the flows2 crop rule,
the configuration loader, the checkpoint / log names and stage chaining, the alpha contract and rank slicing."""
import io
import os

import numpy as np
import pytest
import torch

from atdn_vslam_amd import flowbank as fb
from atdn_vslam_amd import train_odometry as tro
from atdn_vslam_amd.weights_spec import clvo_state_spec

B, N, EPOCHS = 3, 3, 2
FRAMES = (12, 9)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "flowbank.npz")))


def _version_note(g):
    return " (golden written with torch %s, running %s: DataLoader permutations and torch.rand draws are version-bound)" % (
        g["torch_version"], torch.__version__)


def _draw(augment):
    """train_odometry.train's order: seed, sampler, loader, initial weights, then the epochs."""
    torch.manual_seed(fb.TRAIN_SEED)
    index = fb.ClipIndex(FRAMES, N, augment=augment)
    loader = fb.make_loader(index, B)
    state = fb.initial_clvo_state(B)
    batches = [tuple(x.numpy() for x in b) for _ in range(EPOCHS) for b in loader]
    return index, state, batches


@pytest.mark.parametrize("tag,augment", [("true", True), ("false", False), ("m1", -1)])
def test_sampler_and_targets_match_the_reference(golden, tag, augment):
    index, _, batches = _draw(augment)
    assert len(index) == int(golden["len_" + tag])
    code = np.zeros(golden["code_" + tag].shape)
    first = np.zeros_like(code)
    last = np.zeros_like(code)
    rot = np.zeros(golden["rot_" + tag].shape)
    tr = np.zeros_like(rot)
    c0, c1 = fb.crop_slice(1241)
    poses = [golden["poses_00"], golden["poses_05"]]
    for k, (si, ci, rv) in enumerate(batches):
        for b in range(B):
            sign = -1.0 if rv[b] else 1.0
            for t in range(N):
                flow = ci[b] + (N - 1 - t if rv[b] else t)
                code[k, b, t] = sign * (100 * (si[b] + 1) + flow)
                first[k, b, t], last[k, b, t] = sign * c0, sign * (c1 - 1)
        r, t_ = fb.batch_targets([fb.Sequence("00", 0, 12, poses[0]), fb.Sequence("05", 11, 9, poses[1])], si, ci, rv, N)
        rot[k], tr[k] = r, t_
    note = _version_note(golden)
    assert np.array_equal(code, golden["code_" + tag]), "clip order / reverse flags differ from the reference" + note
    assert np.array_equal(np.signbit(code), np.signbit(golden["code_" + tag])), note
    assert np.array_equal(first, golden["first_" + tag]) and np.array_equal(last, golden["last_" + tag])
    np.testing.assert_allclose(rot, golden["rot_" + tag], rtol=0, atol=1e-12)
    np.testing.assert_allclose(tr, golden["tr_" + tag], rtol=0, atol=1e-12)


def test_initial_weights_and_rng_match_the_reference(golden):
    torch.manual_seed(fb.TRAIN_SEED)
    sd = fb.initial_clvo_state(B)
    assert list(sd) == list(golden["state_keys"]) == list(clvo_state_spec())
    for i, (k, v) in enumerate(sd.items()):
        v = v.double()
        assert tuple(v.shape) == tuple(clvo_state_spec()[k][0]), k
        np.testing.assert_allclose(float(v.sum()), golden["state_sum"][i], rtol=1e-12, atol=1e-12, err_msg=k + _version_note(golden))
        np.testing.assert_allclose(float((v ** 2).sum()), golden["state_sumsq"][i], rtol=1e-12, atol=1e-12, err_msg=k)
        f8 = np.pad(v.reshape(-1)[:8].numpy(), (0, max(0, 8 - v.numel())))
        assert np.array_equal(f8, golden["state_first8"][i]), k
    assert np.array_equal(torch.rand(4).double().numpy(), golden["rng_after_init"]), "RNG state after init differs" + _version_note(golden)


def test_crop_rule():
    assert fb.crop_slice(1241) == (4, 1236)
    assert fb.crop_slice(1232) == (0, 1232)
    assert fb.crop_slice(1242) == (5, 1237)
    with pytest.raises(ValueError):
        fb.crop_slice(1226)


def _tree(root, name, n_frames, width, pngs=True, n_flows=None):
    ds = os.path.join(root, "dataset")
    os.makedirs(os.path.join(ds, "poses"), exist_ok=True)
    np.savetxt(os.path.join(ds, "poses", name + ".txt"), np.tile(np.eye(4)[:3].reshape(1, 12), (n_frames, 1)))
    if pngs:
        os.makedirs(os.path.join(ds, "sequences", name, "image_2"), exist_ok=True)
        for i in range(n_frames):
            open(os.path.join(ds, "sequences", name, "image_2", "%06d.png" % i), "wb").close()
    os.makedirs(os.path.join(ds, "flows2", name), exist_ok=True)
    files = []
    for i in range(n_frames - 1 if n_flows is None else n_flows):
        f = torch.arange(2 * 376 * width, dtype=torch.float32).view(1, 2, 376, width).remainder(997).half() + i
        torch.save(f, os.path.join(ds, "flows2", name, "%06d.pt" % i))
        files.append(f)
    return files


class _HostBank(fb.FlowBank):
    """FlowBank on a host buffer (only for the import logic; the product bank refuses a CPU device)."""

    def __init__(self, capacity):
        self.device, self.hw, self.capacity = torch.device("cpu"), fb.BANK_HW, capacity
        self.data = torch.zeros((capacity, 2) + fb.BANK_HW, dtype=torch.float16)
        self.sequences, self.n_flows = [], 0


def test_load_flows2_crops_and_counts(tmp_path):
    wide = _tree(str(tmp_path), "00", 4, 1241)
    exact = _tree(str(tmp_path), "01", 3, 1232, pngs=False)
    bank = _HostBank(5)
    bank.load_flows2(str(tmp_path), ["00", "01"])
    assert [(s.name, s.first, s.n_frames) for s in bank.sequences] == [("00", 0, 4), ("01", 3, 3)]
    for i, f in enumerate(wide):
        assert torch.equal(bank.flows("00")[i], f[0, :, :, 4:-5])
    for i, f in enumerate(exact):
        assert torch.equal(bank.flows("01")[i], f[0])


def test_load_flows2_rejects_narrow_files_and_bad_counts(tmp_path):
    _tree(str(tmp_path / "a"), "00", 3, 1226)
    with pytest.raises(ValueError, match="narrower"):
        _HostBank(4).load_flows2(str(tmp_path / "a"), ["00"])
    _tree(str(tmp_path / "b"), "00", 4, 1232, n_flows=2)
    with pytest.raises(ValueError, match="flow files"):
        _HostBank(4).load_flows2(str(tmp_path / "b"), ["00"])


CONFIG = """{tag}
alpha: {alpha}
batch_size: 24
data_path: /data/kitti
device: cuda:0
epochs: 1
epsilon: 1.0e-08
keyframes_path: /tmp/out
weight_file: ckpt/clvo_generalization4_
log_file: loss_log/generalization4_
lr: 0.01
stage: 1
sequence_length: 6
train_sequences:
- '00'
- '01'
wd: 0.001
augment_flow: false
w : 2
"""


@pytest.mark.parametrize("tag", ["!!python/object:utils.arguments.Arguments",
                                 "!!python/object:atdn_vslam.utils.arguments.Arguments"])
def test_config_loads_with_both_tags(tmp_path, tag):
    p = tmp_path / "config.yaml"
    p.write_text(CONFIG.format(tag=tag, alpha=1))
    cfg = tro.load_config(str(p))
    assert (cfg.batch_size, cfg.sequence_length, cfg.lr, cfg.wd, cfg.epsilon) == (24, 6, 0.01, 0.001, 1e-8)
    assert cfg.train_sequences == ["00", "01"] and cfg.augment_flow is False and cfg.w == 2 and cfg.stage == 1
    tro.check_alpha(cfg)


def test_config_loader_executes_nothing(tmp_path):
    p = tmp_path / "config.yaml"
    p.write_text("!!python/object/apply:os.system ['true']\n")
    with pytest.raises(Exception):
        tro.load_config(str(p))


def test_alpha_other_than_one_is_rejected(tmp_path):
    p = tmp_path / "config.yaml"
    p.write_text(CONFIG.format(tag="!!python/object:utils.arguments.Arguments", alpha=0.5))
    cfg = tro.load_config(str(p))
    with pytest.raises(NotImplementedError, match="alpha = 1"):
        tro.check_alpha(cfg)


def test_checkpoint_log_names_and_stage_chaining(tmp_path):
    wf = str(tmp_path / "clvo_")
    cfg = tro.Config(weight_file=wf, log_file=str(tmp_path / "log_"), stage=3)
    assert tro.checkpoint_path(cfg) == wf + "3_atdnvo_c.pth"
    assert tro.log_path(cfg, 0) == str(tmp_path / "log_") + "2_0.txt"
    with pytest.raises(FileNotFoundError):
        tro.init_path(cfg)
    open(wf + "2_atdnvo_c.pth", "wb").close()
    err = io.StringIO()
    assert tro.init_path(cfg, warn=err) == wf + "2_atdnvo_c.pth"
    assert "2.pth does not exist" in err.getvalue()
    open(wf + "2.pth", "wb").close()
    assert tro.init_path(cfg) == wf + "2.pth"
    assert tro.init_path(cfg, init="x.pth") == "x.pth"
    assert tro.init_path(tro.Config(weight_file=wf, stage=1)) is None


def test_rank_slices():
    assert [fb.rank_slice(24, 2, r) for r in range(2)] == [(0, 12), (12, 24)]
    assert [fb.rank_slice(24, 3, r) for r in range(3)] == [(0, 8), (8, 16), (16, 24)]
    with pytest.raises(ValueError, match="does not divide"):
        fb.rank_slice(10, 3, 0)


def test_gather_validates_before_any_device_call():
    """Argument errors of gather_clips that are caught on the host side of the binding."""
    bank = torch.zeros((4, 2, 4, 8), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="reverse flags"):
        fb.gather_clips(bank, [0, 1], [0], 2)


def test_native_gather_rejects_out_of_range_starts_before_launching():
    """atdn_flow_gather_clips checks every start on the host and returns an error without touching the device (the
    pointers here are host buffers: a launch would be a bug the test would see as a crash, not a pass)."""
    import ctypes as C
    from atdn_vslam_amd import _lib
    L = _lib.lib()
    bank = np.zeros(4 * 2 * 4 * 8 + 8, dtype=np.float16)
    out = np.zeros(2 * 3 * 2 * 4 * 8 + 4, dtype=np.float32)
    bp = bank.ctypes.data + (-bank.ctypes.data) % 16
    op = out.ctypes.data + (-out.ctypes.data) % 16
    for starts in ([0, 2], [-1, 0], [0, 7]):
        s = np.array(starts, dtype=np.int32)
        r = np.zeros(2, dtype=np.int32)
        rc = L.atdn_flow_gather_clips(C.c_void_p(bp), 4, 4, 8, s.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
                                      2, 3, C.c_void_p(op), None)
        assert rc != 0
        assert b"outside [0, 1]" in L.atdn_last_error()
    rc = L.atdn_flow_pack_f16(C.c_void_p(op), 1, 4, 8, 4, 8, C.c_void_p(bp), None)
    assert rc != 0 and b"column window" in L.atdn_last_error()


def test_kitti_sequence_reader(tmp_path):
    from PIL import Image
    d = tmp_path / "dataset" / "sequences" / "07" / "image_2"
    d.mkdir(parents=True)
    r = np.random.RandomState(0)
    imgs = [r.randint(0, 256, (6, 10, 3), dtype=np.uint8) for _ in range(7)]
    for i, a in enumerate(imgs):
        Image.fromarray(a).save(str(d / ("%06d.png" % i)))
    (tmp_path / "dataset" / "poses").mkdir(parents=True)
    np.savetxt(str(tmp_path / "dataset" / "poses" / "07.txt"), np.tile(np.eye(4)[:3].reshape(1, 12), (7, 1)))
    seq = fb.KittiSequence(str(tmp_path), "07", workers=3)
    try:
        assert seq.shape == (7, 3, 6, 10) and seq.dtype == torch.uint8 and not seq.is_cuda
        for s, e in ((0, 4), (3, 7), (6, 7)):
            got = seq[s:e]
            want = torch.from_numpy(np.stack(imgs[s:e]).transpose(0, 3, 1, 2).copy())
            assert torch.equal(got, want)
    finally:
        seq.close()
    assert fb.read_poses(str(tmp_path), "07").shape == (7, 12)
