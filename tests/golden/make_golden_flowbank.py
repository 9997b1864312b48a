"""Golden fixture for the flow bank's sampler, targets and initial weights (atdn_vslam_amd/flowbank.py), produced by
running the REFERENCE: `FlowKittiDataset3` (odometry/datasets.py:133-226) over a temporary KITTI tree batched by the
DataLoader of train_odometry.py:78-85, after `torch.manual_seed(4265664478)` and the construction of `ATDNVO(3)`
(train_odometry.py:64-88), for augment = True, False and -1.

The tree holds two sequences of 12 and 9 frames with seeded poses, empty PNG files (only counted) and fp16 flow files
[1,2,2,1241]: channel 0 of flow i of the s-th sequence holds 100 * (s + 1) + i, channel 1 the column index, so the order, the sign and
the centre crop of every sample are visible. Stored: the dataset length, two epochs of batches (flow code, sign, first and
last column after the crop, float64 rotation / translation targets), the poses, per-key checksums of the initial
state_dict and torch.__version__ (the permutations and the torch.rand draws are those of that version).

Run only in the build container (needs the reference):   python tests/golden/make_golden_flowbank.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, install_stubs  # noqa: E402

SEED = 4265664478
FRAMES = {"00": 12, "05": 9}
B, N, EPOCHS, W_FILE = 3, 3, 2, 1241
AUGMENTS = (("true", True), ("false", False), ("m1", -1))


def seq_poses(seed, n):
    """Seeded smooth trajectory, KITTI rows [n,12] float64."""
    r = np.random.RandomState(seed)
    out = np.zeros((n, 12))
    ang = np.cumsum(r.uniform(-0.05, 0.05, (n, 3)), axis=0)
    pos = np.cumsum(r.uniform(-1.0, 1.0, (n, 3)) + np.array([0.0, 0.0, 1.2]), axis=0)
    for i in range(n):
        a, b, c = ang[i]
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        m = np.concatenate([Ry @ Rx @ Rz, pos[i][:, None]], axis=1)
        out[i] = m.reshape(12)
    return out


def write_tree(root):
    poses = {}
    for k, (name, n) in enumerate(sorted(FRAMES.items())):
        ds = os.path.join(root, "dataset")
        os.makedirs(os.path.join(ds, "sequences", name, "image_2"), exist_ok=True)
        os.makedirs(os.path.join(ds, "poses"), exist_ok=True)
        os.makedirs(os.path.join(ds, "flows2", name), exist_ok=True)
        for i in range(n):
            open(os.path.join(ds, "sequences", name, "image_2", "%06d.png" % i), "wb").close()
        poses[name] = seq_poses(100 + k, n)
        np.savetxt(os.path.join(ds, "poses", name + ".txt"), poses[name])
        for i in range(n - 1):
            f = torch.zeros(1, 2, 2, W_FILE, dtype=torch.float16)
            f[0, 0] = 100 * (k + 1) + i
            f[0, 1] = torch.arange(W_FILE, dtype=torch.float16)[None]
            torch.save(f, os.path.join(ds, "flows2", name, "%06d.pt" % i))
    return poses


def main():
    install_stubs()
    tvio = types.ModuleType("torchvision.io")
    tvio.read_image = lambda path: None
    sys.modules["torchvision.io"] = tvio
    sys.modules["torchvision"].io = tvio
    sys.path.insert(0, REF)
    from torch.utils.data import DataLoader
    from atdn_vslam.odometry.datasets import FlowKittiDataset3
    from atdn_vslam.odometry.network import ATDNVO

    out = {"torch_version": np.array(torch.__version__)}
    with tempfile.TemporaryDirectory() as root:
        poses = write_tree(root)
        for k, name in enumerate(sorted(FRAMES)):
            out["poses_%s" % name] = poses[name]
        seqs = sorted(FRAMES)
        for tag, aug in AUGMENTS:
            torch.manual_seed(SEED)
            ds = FlowKittiDataset3(root, sequences=seqs, augment=aug, sequence_length=N)
            dl = DataLoader(dataset=ds, batch_size=B, shuffle=True, num_workers=0, drop_last=True)
            model = ATDNVO(B, in_channels=2)
            if tag == "true":
                sd = model.state_dict()
                out["state_keys"] = np.array(list(sd))
                out["state_sum"] = np.array([float(v.double().sum()) for v in sd.values()])
                out["state_sumsq"] = np.array([float((v.double() ** 2).sum()) for v in sd.values()])
                out["state_first8"] = np.stack([np.pad(v.double().reshape(-1)[:8].numpy(), (0, max(0, 8 - v.numel())))
                                                for v in sd.values()])
                st = torch.get_rng_state()
                out["rng_after_init"] = torch.rand(4).double().numpy()   # the RNG state the constructor leaves behind
                torch.set_rng_state(st)
            out["len_" + tag] = np.array(len(ds))
            code, first, last, rot, tr = [], [], [], [], []
            for _ in range(EPOCHS):
                for fl, r, t in dl:
                    code.append(fl[:, :, 0, 0, 0].double().numpy())
                    first.append(fl[:, :, 1, 0, 0].double().numpy())
                    last.append(fl[:, :, 1, 0, -1].double().numpy())
                    rot.append(r.numpy())
                    tr.append(t.numpy())
            out["code_" + tag] = np.stack(code)       # [EPOCHS*nb, B, N]: +-(100*(seq+1) + flow index)
            out["first_" + tag] = np.stack(first)     # +-4 (the crop's first column)
            out["last_" + tag] = np.stack(last)       # +-1235
            out["rot_" + tag] = np.stack(rot)         # [EPOCHS*nb, B, N, 3] float64
            out["tr_" + tag] = np.stack(tr)
    np.savez_compressed(os.path.join(HERE, "flowbank.npz"), **out)
    print("wrote", os.path.join(HERE, "flowbank.npz"), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
