"""The HBM flow bank on the MI355X: the two kernels against their torch expressions bit for bit, the bank build against
pair-mode flows in both geometries, the flows2 round trip, the training driver against a hand-fed CLVOTrainer and the
evaluation driver against the pose head over torch-negated flows."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, evaluation
from atdn_vslam_amd import flowbank as fb
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import train_odometry as tro
from atdn_vslam_amd.evaluate_odometry import evaluate, result_name, run_inference
from atdn_vslam_amd.modules import ATDNVO, RAFTGMA
from atdn_vslam_amd.training import CLVOTrainer
from atdn_vslam_amd.transforms import InputPadder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H, W = fb.BANK_HW


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("x0", [0, 7])
def test_pack_rounds_like_half(x0):
    g = torch.Generator().manual_seed(5)
    src = torch.randn((3, 2, 9, 48), generator=g) * 300.0
    flat = src.view(-1)
    specials = torch.tensor([0.0, -0.0, 1.0 + 2 ** -11, 1.0 + 3 * 2 ** -11, -(1.0 + 2 ** -11), 2 ** -20, -(2 ** -20), 3e-8,
                             6e-5, 65504.0, 65519.0, 65520.0, 70000.0, -70000.0, float("nan"), float("inf"), -float("inf")])
    idx = torch.randperm(flat.numel(), generator=g)[:specials.numel() * 8]
    flat[idx] = specials.repeat(8)
    src = src.to(DEV)
    Wd = 40 if x0 == 0 else 32
    dst = torch.full((3, 2, 9, Wd), 7.0, dtype=torch.float16, device=DEV)
    fb.pack_f16(src, dst, x0=x0)
    want = src[..., x0:x0 + Wd].half()
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), _bits(want))
    assert torch.isnan(dst).sum() == torch.isnan(want).sum() > 0
    with pytest.raises(RuntimeError, match="column window"):
        fb.pack_f16(src, torch.empty((3, 2, 9, 48), dtype=torch.float16, device=DEV), x0=8)


def test_gather_matches_torch_at_24x6():
    B, T, n = 24, 6, 40
    g = torch.Generator(device=DEV).manual_seed(3)
    bank = (torch.randn((n, 2, H, W), device=DEV, generator=g) * 40).half()
    r = np.random.RandomState(11)
    start = r.randint(0, n - T + 1, B)
    start[0], start[1], start[2], start[3] = 0, n - T, 0, n - T
    rev = r.randint(0, 2, B)
    rev[0], rev[1], rev[2], rev[3] = 0, 0, 1, 1
    out = fb.gather_clips(bank, start, rev, T)
    want = torch.stack([torch.stack([-bank[s + T - 1 - t] if v else bank[s + t] for t in range(T)]) for s, v in zip(start, rev)]).float()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    # out-of-range starts: an error, and nothing written
    sentinel = torch.full_like(out, 123.0)
    for bad in (-1, n - T + 1):
        s2 = start.copy()
        s2[5] = bad
        with pytest.raises(RuntimeError, match="outside"):
            fb.gather_clips(bank, s2, rev, T, out=sentinel)
    torch.cuda.synchronize()
    assert bool((sentinel == 123.0).all())


# ------------------------------------------------------------------------------------------- bank build
def _resize_u8(frames_u8, size):
    out = torch.empty((frames_u8.shape[0], 3) + tuple(size), dtype=torch.float32, device=DEV)
    x = frames_u8.to(DEV).contiguous()
    _lib.check(_lib.lib().atdn_resize_frames_u8(C.c_void_p(x.data_ptr()), x.shape[0] * 3, x.shape[2], x.shape[3], size[0], size[1],
                                                1, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _pair_flows(net, frames_u8, geometry, iters):
    """Pair mode after the same resize / pad / unpad / crop, then .half()."""
    size = (H, W) if geometry == "slam" else fb.CROP_SIZE
    fr = _resize_u8(frames_u8, size)
    padder = InputPadder((3,) + tuple(size))
    out = []
    for s in range(0, fr.shape[0] - 1, 4):
        e = min(s + 4, fr.shape[0] - 1)
        a, b = padder.pad(fr[s:e], fr[s + 1:e + 1])
        _, up = net(a, b, iters=iters, test_mode=True)
        up = padder.unpad(up)
        if geometry == "crop":
            up = up[..., 4:-5]
        out.append(up.half())
    return torch.cat(out)


ITERS = 4


@pytest.fixture(scope="module")
def gma():
    net = RAFTGMA(max_batch=8)
    net.load_state_dict(syn.to_torch(syn.make_gma_state(seed=1)))
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def frames():
    return {"a": torch.from_numpy(syn.make_frames(21, 376, 1241, seed=4)).to(torch.uint8),
            "b": torch.from_numpy(syn.make_frames(9, 376, 1241, seed=8)).to(torch.uint8)}


def _poses(n, seed):
    r = np.random.RandomState(seed)
    rot = r.uniform(-0.02, 0.02, (n - 1, 3))
    tr = r.uniform(-0.5, 0.5, (n - 1, 3)) + np.array([0, 0, 1.0])
    return evaluation.integrate_motions(rot, tr)


@pytest.fixture(scope="module")
def built(gma, frames):
    banks = {}
    for geometry in fb.GEOMETRIES:
        bank = fb.FlowBank(DEV, 20 + 8)
        for k, (name, f) in enumerate(sorted(frames.items())):
            bank.add_sequence(name, f.pin_memory(), _poses(f.shape[0], k), gma, geometry=geometry, batch=8, iters=ITERS)
        banks[geometry] = bank
    torch.cuda.synchronize()
    return banks


@pytest.mark.parametrize("geometry", fb.GEOMETRIES)
def test_add_sequence_matches_pair_mode(built, gma, frames, geometry):
    bank = built[geometry]
    assert [(s.name, s.first, s.n_frames) for s in bank.sequences] == [("a", 0, 21), ("b", 20, 9)] and bank.n_flows == 28
    for name, f in frames.items():
        want = _pair_flows(gma, f, geometry, ITERS)
        got = bank.flows(name)
        assert got.shape == want.shape == (f.shape[0] - 1, 2, H, W)
        assert torch.equal(_bits(got), _bits(want)), "%s / %s: first differing flow %d" % (
            geometry, name, int((_bits(got) != _bits(want)).flatten(1).any(1).nonzero()[0]))


def test_add_sequence_rejects_low_latency(frames):
    net = RAFTGMA(max_batch=1, low_latency=True)
    with pytest.raises(ValueError, match="low-latency"):
        fb.FlowBank(DEV, 30).add_sequence("a", frames["a"], None, net)


def test_flows2_round_trip(built, tmp_path):
    bank = built["crop"]
    bank.save_flows2(str(tmp_path))
    for s in bank.sequences:
        os.makedirs(tmp_path / "dataset" / "poses", exist_ok=True)
        np.savetxt(tmp_path / "dataset" / "poses" / (s.name + ".txt"), evaluation.kitti_rows(s.poses))
        f0 = torch.load(tmp_path / "dataset" / "flows2" / s.name / "000000.pt")
        assert f0.dtype == torch.float16 and tuple(f0.shape) == (1, 2, H, W)
    back = fb.FlowBank(DEV, bank.n_flows)
    back.load_flows2(str(tmp_path), [s.name for s in bank.sequences])
    assert [(s.name, s.first, s.n_frames) for s in back.sequences] == [(s.name, s.first, s.n_frames) for s in bank.sequences]
    assert torch.equal(_bits(back.data[:bank.n_flows]), _bits(bank.data[:bank.n_flows]))


# ------------------------------------------------------------------------------------------- drivers
def _synthetic_bank(frames_per_seq, seed):
    n = sum(f - 1 for f in frames_per_seq)
    bank = fb.FlowBank(DEV, n)
    bank.data.copy_(torch.from_numpy(syn.make_flow(n, H, W, seed=seed)).half())
    for k, f in enumerate(frames_per_seq):
        bank._commit(bank._reserve("s%d" % k, f, _poses(f, 20 + k)))
    return bank


def test_train_driver_matches_a_hand_fed_trainer(tmp_path):
    Bt, N = 4, 3
    bank = _synthetic_bank((9, 9), seed=2)      # 12 clips: three batches of four
    cfg = tro.Config(batch_size=Bt, sequence_length=N, epochs=1, lr=1e-3, wd=1e-3, epsilon=1e-8, stage=1, alpha=1, w=3,
                     augment_flow=True, train_sequences=["s0", "s1"], weight_file=str(tmp_path / "w_"),
                     log_file=str(tmp_path / "log_"))
    seen = []
    trainer, hist = tro.train(cfg, bank, DEV, on_step=lambda e, i, si, ci, rv, loss: seen.append((si, ci, rv, loss)))
    assert len(hist) == 1 and len(hist[0]) == 3 and len(seen) == 3
    assert os.path.exists(tro.checkpoint_path(cfg)) and os.path.exists(tro.log_path(cfg, 0))
    assert np.array_equal(np.loadtxt(tro.log_path(cfg, 0)), np.array(hist[0]))

    torch.manual_seed(fb.TRAIN_SEED)
    index = fb.ClipIndex([9, 9], N, augment=True)
    loader = fb.make_loader(index, Bt)
    ref = CLVOTrainer(fb.initial_clvo_state(Bt), Bt, N, device=DEV, lr=1e-3, weight_decay=1e-3, eps=1e-8, total_steps=len(loader),
                      eta_min=1e-9)
    losses = []
    for k, (si, ci, rv) in enumerate(loader):
        flows, rots, trs = [], [], []
        for s, c, v in zip(si.tolist(), ci.tolist(), rv.tolist()):
            seq = bank.sequences[s]
            first = seq.first + c
            flows.append(torch.stack([-bank.data[first + N - 1 - t] if v else bank.data[first + t] for t in range(N)]).float())
            p = seq.poses[c:c + N + 1]
            r, t_ = evaluation.relative_motions(p[::-1] if v else p)
            rots.append(r)
            trs.append(t_)
        assert np.array_equal(si.numpy(), seen[k][0]) and np.array_equal(ci.numpy(), seen[k][1]) and np.array_equal(rv.numpy(), seen[k][2])
        losses.append(ref.step(torch.stack(flows), torch.from_numpy(np.stack(rots)).float(), torch.from_numpy(np.stack(trs)).float()))
    assert losses == hist[0]
    a, b = trainer.state_dict(), ref.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    saved = torch.load(tro.checkpoint_path(cfg))
    for k in a:
        assert torch.equal(saved[k], a[k]), k


def test_evaluate_driver_matches_the_head_on_negated_flows(tmp_path):
    bank = _synthetic_bank((17,), seed=6)
    head = ATDNVO()
    head.load_state_dict(syn.to_torch(syn.make_clvo_state(seed=2)))
    head = head.to(DEV).eval()
    s = bank.sequences[0]
    gt = s.poses
    runs = evaluate(head, bank, "s0", 6, 0, str(tmp_path), gt_poses=gt)
    for d, tag in ((1, "f"), (-1, "b")):
        fl = bank.data[:s.n_flows].float()
        fl = fl if d == 1 else -fl.flip(0)
        rot, tr, _ = head.scan(head.encode(fl)[:, None, :], hw=(H, W))
        got_r, got_t = run_inference(head, bank, "s0", d)
        assert torch.equal(_bits(got_r), _bits(rot[:, 0])) and torch.equal(_bits(got_t), _bits(tr[:, 0]))
        f = tmp_path / result_name(6, "s0", d)
        assert f.exists() and np.loadtxt(f).shape == (17, 12)
        assert runs[tag].shape == (17, 4, 4)
    assert (tmp_path / "6_ATDNVO_c_s0_fused.txt").exists()
    assert set(runs["metrics"]) == {"forward", "backward", "fused"}
