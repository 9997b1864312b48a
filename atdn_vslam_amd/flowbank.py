"""CLVO's training set kept in HBM: the fp16 flows of whole KITTI sequences, computed once on the device and gathered
into training batches there (no disk, no host-to-device copy per iteration).

The reference trains from fp16 flow files, one per frame pair under `dataset/flows2/<seq>/%06d.pt`, loaded into host
memory by `FlowKittiDataset3` (odometry/datasets.py:133-226) and batched by a shuffling DataLoader (train_odometry.py:73-85).
Here:

* `FlowBank` holds one fp16 device buffer [capacity,2,376,1232]; flow i of a sequence (frame i -> frame i+1, as in
  `flows2`) sits in slot `first + i`. It is filled by running the flow network over a sequence (`add_sequence`, packed by
  `atdn_flow_pack_f16`), by importing a reference `flows2` tree (`load_flows2`), and can be written back in that layout
  (`save_flows2`). `gather` is `atdn_flow_gather_clips`: the fp32 [B,T,2,H,W] batch of the trainer, reversed clips
  negated and flipped in time.
* `ClipIndex` is FlowKittiDataset3 without the flows: the same length, the same `torch.rand(1)` draw per item and the
  same reverse rule, so a `DataLoader(shuffle=True, drop_last=True)` over it draws the reference's permutations and
  reverse flags under the same seed. `clip_targets` gives the float64 (rotation, translation) targets of a clip.
* `initial_clvo_state` is the default torch initialisation of `ATDNVO(batch_size)` (odometry/network.py:20-119): the
  reference's layer types built in the reference's order, so under `torch.manual_seed(4265664478)` the weights and the
  RNG state after them are the reference's.
* `KittiSequence` reads `dataset/sequences/<seq>/image_2/*.png` (PIL, a thread pool of at most 16 workers, the next
  clip decoded while the GPU works on the current one) and `dataset/poses/<seq>.txt`.
"""
import ctypes as C
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .evaluation import relative_motions
from .transforms import InputPadder

BANK_HW = (376, 1232)       # what the pose head reads (neural_slam.py:198; Linear(832) of network.py:72)
CROP_SIZE = (376, 1241)     # FlowKittiDataset2/3's source width before the centre crop (datasets.py:120-122,184-186)
TRAIN_SEED = 4265664478     # train_odometry.py:64
GEOMETRIES = ("slam", "crop")


def crop_slice(width, target=BANK_HW[1]):
    """The reference's centre crop of a flow wider than 1232 columns, `[d//2 : -d//2]` (datasets.py:120-122,184-186):
    returns (first column, last column + 1). d = 9 -> [4, 1236). A narrower flow is an error (Linear(832) would fail)."""
    d = width - target
    if d < 0:
        raise ValueError("flow of width %d is narrower than %d: the pose head's Linear(832) cannot take it" % (width, target))
    if d == 0:
        return 0, width
    return d // 2, width + (-d) // 2


def _hom(poses):
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim == 2 and p.shape[1] == 12:
        p = p.reshape(-1, 3, 4)
    if p.shape[1] == 3:
        out = np.tile(np.eye(4), (len(p), 1, 1))
        out[:, :3, :] = p
        return out
    return p.copy()


class Sequence:
    """One sequence of the bank: flows first .. first + n_frames - 2, poses float64 [n_frames,4,4]."""

    def __init__(self, name, first, n_frames, poses):
        self.name, self.first, self.n_frames = name, int(first), int(n_frames)
        self.poses = _hom(poses) if poses is not None else None
        self._motions = None

    @property
    def n_flows(self):
        return self.n_frames - 1

    def targets(self, clip, N, reverse):
        """clip_targets(self.poses, clip, N, reverse) from motions computed once per sequence: a forward clip's are
        inverse(P_j) @ P_j+1 for j = clip .. clip+N-1, a reversed clip's inverse(P_j+1) @ P_j from the last j back — the
        same float64 operations on the same matrices, so the same bits, without a 4x4 inverse per frame per iteration."""
        if self._motions is None:
            f = relative_motions(self.poses)
            b = relative_motions(self.poses[::-1])
            self._motions = (f, (b[0][::-1].copy(), b[1][::-1].copy()))
        if reverse:
            r, t = self._motions[1]
            return r[clip:clip + N][::-1], t[clip:clip + N][::-1]
        r, t = self._motions[0]
        return r[clip:clip + N], t[clip:clip + N]


def pack_f16(flow_up, dst, x0=0):
    """`flow_up[..., x0:x0+W].half()` into `dst` [B,2,H,W] fp16 (a range of bank slots), on the device."""
    B, _, H, Ws = flow_up.shape
    W = dst.shape[-1]
    if tuple(dst.shape) != (B, 2, H, W) or dst.dtype != torch.float16 or not dst.is_contiguous():
        raise RuntimeError("pack_f16: dst must be contiguous fp16 [%d,2,%d,W], got %s %s" % (B, H, tuple(dst.shape), dst.dtype))
    src = flow_up.float().contiguous()
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().atdn_flow_pack_f16(_ptr(src), B, H, Ws, int(x0), W, _ptr(dst), _stream()))
    return dst


def gather_clips(bank, start, reverse, T, out=None):
    """bank [n,2,H,W] fp16 -> out [B,T,2,H,W] fp32 with out[b,t] = -bank[start[b]+T-1-t] if reverse[b] else
    bank[start[b]+t] (atdn_flow_gather_clips; the indices are checked on the host before anything is launched)."""
    n, _, H, W = bank.shape
    s = np.ascontiguousarray(np.asarray(start, dtype=np.int64).reshape(-1))
    if s.size and (s.min() < -2 ** 31 or s.max() >= 2 ** 31):
        raise RuntimeError("gather_clips: start outside the int range")
    s = s.astype(np.int32)
    r = np.ascontiguousarray(np.asarray(reverse).reshape(-1).astype(np.int32))
    B = s.size
    if r.size != B:
        raise RuntimeError("gather_clips: %d starts but %d reverse flags" % (B, r.size))
    if out is None:
        out = torch.empty((B, T, 2, H, W), dtype=torch.float32, device=bank.device)
    if tuple(out.shape) != (B, T, 2, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("gather_clips: out must be contiguous fp32 %s" % ((B, T, 2, H, W),))
    with torch.cuda.device(bank.device):
        _lib.check(_lib.lib().atdn_flow_gather_clips(_ptr(bank), n, H, W, s.ctypes.data_as(C.c_void_p),
                                                     r.ctypes.data_as(C.c_void_p), B, int(T), _ptr(out), _stream()))
    return out


class FlowBank:
    """fp16 flows of whole sequences in one device buffer [capacity,2,H,W]."""

    def __init__(self, device, capacity_flows, hw=BANK_HW):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FlowBank lives in device memory: there is no CPU fallback")
        self.hw = tuple(hw)
        self.capacity = int(capacity_flows)
        if self.capacity < 1:
            raise ValueError("FlowBank needs room for at least one flow")
        need = self.capacity * 2 * self.hw[0] * self.hw[1] * 2
        free, total = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise MemoryError("FlowBank: %d flows of 2x%dx%d fp16 need %.2f GB, but %s has %.2f GB free of %.2f GB"
                              % (self.capacity, self.hw[0], self.hw[1], need / 1e9, self.device, free / 1e9, total / 1e9))
        self.data = torch.empty((self.capacity, 2) + self.hw, dtype=torch.float16, device=self.device)
        self.sequences = []
        self.n_flows = 0

    @staticmethod
    def bytes_per_flow(hw=BANK_HW):
        return 2 * hw[0] * hw[1] * 2

    def sequence(self, name):
        for s in self.sequences:
            if s.name == name:
                return s
        raise KeyError("no sequence %r in the bank" % (name,))

    def flows(self, name):
        """The fp16 flows of one sequence, [n_frames-1,2,H,W] (a view of the bank)."""
        s = self.sequence(name)
        return self.data[s.first:s.first + s.n_flows]

    def _reserve(self, name, n_frames, poses):
        if any(s.name == name for s in self.sequences):
            raise ValueError("sequence %r is already in the bank" % (name,))
        if n_frames < 2:
            raise ValueError("sequence %r has %d frame(s): no flow" % (name, n_frames))
        if poses is not None and len(poses) < n_frames:
            raise ValueError("sequence %r: %d poses for %d frames" % (name, len(poses), n_frames))
        if self.n_flows + n_frames - 1 > self.capacity:
            raise MemoryError("FlowBank: sequence %r needs %d slots, %d of %d are free"
                              % (name, n_frames - 1, self.capacity - self.n_flows, self.capacity))
        seq = Sequence(name, self.n_flows, n_frames, poses)
        return seq

    def _commit(self, seq):
        self.sequences.append(seq)
        self.n_flows = seq.first + seq.n_flows

    @torch.no_grad()
    def add_sequence(self, name, frames, poses, flow_net, geometry="slam", batch=16, iters=12, antialias=True):
        """Compute and store the flows of one sequence. frames [T,3,Hin,Win] uint8 in host memory (or any sliceable
        source of such tensors, as OdometryPipeline.run_sequence takes), walked in clips of `batch` pairs: FrameIngest ->
        RAFTGMA.forward_sequence(continued=True) -> atdn_flow_pack_f16 into consecutive slots; the split-f16 range guard
        is read at the end. geometry "slam": resize to 376x1232 (what VisualOdometry / NeuralSLAM feed the head);
        "crop": FlowKittiDataset2/3's convention — resize to 376x1241, pad to 1248, flow, unpad, centre crop [4:-5]."""
        from .pipeline import FrameIngest
        if geometry not in GEOMETRIES:
            raise ValueError("geometry must be one of %s, got %r" % (GEOMETRIES, geometry))
        if getattr(flow_net, "low_latency", False):
            raise ValueError("add_sequence needs a default RAFTGMA handle: the low-latency form is not bit-identical to pair mode")
        if frames.is_cuda or frames.dtype != torch.uint8 or len(frames.shape) != 4 or frames.shape[1] != 3:
            raise RuntimeError("add_sequence: frames must be uint8 [T,3,H,W] in host memory")
        T = int(frames.shape[0])
        seq = self._reserve(name, T, poses)
        size = self.hw if geometry == "slam" else (self.hw[0], CROP_SIZE[1])
        padder = InputPadder((3,) + tuple(size))
        x0 = 0 if geometry == "slam" else padder._pad[0] + crop_slice(size[1], self.hw[1])[0]
        ingest = FrameIngest(tuple(frames.shape[-2:]), batch + 1, size=size, antialias=antialias, device=self.device)
        with torch.cuda.device(self.device):
            s = 0
            while s < T - 1:
                e = min(s + batch, T - 1)
                fr = padder.pad(ingest(frames[s:e + 1]))[0]
                _, up = flow_net.forward_sequence(fr, iters=iters, continued=s > 0)
                pack_f16(up, self.data[seq.first + s:seq.first + e], x0=x0)
                s = e
            flow_net.check_saturation()
        self._commit(seq)
        return seq

    def load_flows2(self, data_path, sequences):
        """Import a reference flows2 tree: `<data_path>/dataset/flows2/<seq>/%06d.pt`, fp16 [1,2,H,W] each (wider than
        1232: the same centre crop as FlowKittiDataset3). Frames are counted from image_2/*.png when that directory exists,
        otherwise from the poses; the number of flow files must be frames - 1."""
        ds = os.path.join(data_path, "dataset")
        for name in sequences:
            poses = read_poses(data_path, name)
            im = os.path.join(ds, "sequences", name, "image_2")
            n_frames = len(glob.glob(os.path.join(im, "*.png"))) if os.path.isdir(im) else len(poses)
            files = sorted(glob.glob(os.path.join(ds, "flows2", name, "*.pt")))
            if len(files) != n_frames - 1:
                raise ValueError("sequence %s: %d flow files for %d frames (expected %d)" % (name, len(files), n_frames, n_frames - 1))
            seq = self._reserve(name, n_frames, poses)
            for i, f in enumerate(files):
                a = torch.load(f, map_location="cpu")
                if a.dim() != 4 or a.shape[0] != 1 or a.shape[1] != 2 or a.shape[2] != self.hw[0]:
                    raise ValueError("%s: expected a flow [1,2,%d,W], got %s" % (f, self.hw[0], tuple(a.shape)))
                c0, c1 = crop_slice(a.shape[-1], self.hw[1])
                self.data[seq.first + i].copy_(a[0, :, :, c0:c1].to(torch.float16), non_blocking=False)
            self._commit(seq)

    def save_flows2(self, data_path, sequences=None):
        """Write the reference's layout, fp16 [1,2,376,1232] per file under `<data_path>/dataset/flows2/<seq>/%06d.pt`
        (FlowKittiDataset2/3 read it unchanged)."""
        for s in self.sequences:
            if sequences is not None and s.name not in sequences:
                continue
            d = os.path.join(data_path, "dataset", "flows2", s.name)
            os.makedirs(d, exist_ok=True)
            host = self.flows(s.name).cpu()
            for i in range(s.n_flows):
                torch.save(host[i:i + 1].clone(), os.path.join(d, "%06d.pt" % i))

    def gather(self, start, reverse, T, out=None):
        """Global slots `start` (see ClipIndex.slot) -> fp32 batch [B,T,2,H,W] on the bank's device."""
        return gather_clips(self.data[:max(self.n_flows, 1)], start, reverse, T, out=out)


# ------------------------------------------------------------------------------------------------ sampler and targets
class ClipIndex(torch.utils.data.Dataset):
    """FlowKittiDataset3 (datasets.py:133-226) without the flows: item -> (sequence index, clip index, reverse).
    Per sequence there are n_frames - N clips; every item draws one `torch.rand(1)` whatever `augment` is, and
    reverse = (a + rand) < 0.5 with a = 0 if augment else 1 for a bool, a = augment for a number."""

    def __init__(self, n_frames, sequence_length, augment=False):
        self.N = int(sequence_length)
        self.augment = (0 if augment else 1) if isinstance(augment, bool) else augment
        self.n_frames = [int(n) for n in n_frames]
        self.ends = np.cumsum([n - self.N for n in self.n_frames]).tolist()

    def __len__(self):
        return self.ends[-1]

    def locate(self, index):
        """Global item -> (sequence index, clip index within it)."""
        si, off = 0, 0
        for i, end in enumerate(self.ends):
            if index >= end:
                si, off = i + 1, end
        return si, index - off

    def __getitem__(self, index):
        reverse = bool(((self.augment + torch.rand(1)) < 0.5).item())
        si, ci = self.locate(index)
        return si, ci, reverse


def make_loader(index, batch_size):
    """The reference's DataLoader (train_odometry.py:78-85) over a ClipIndex: batches of (seq [B], clip [B], reverse [B])."""
    return torch.utils.data.DataLoader(index, batch_size=batch_size, shuffle=True, num_workers=0, drop_last=True)


def clip_targets(poses, clip, N, reverse):
    """float64 targets of a clip: (rot [N,3], tr [N,3]) of inverse(P_i) @ P_{i+1} over poses clip .. clip+N, the list
    reversed first when `reverse` (abs2rel over the reversed list, datasets.py:211-218)."""
    p = _hom(poses)[clip:clip + N + 1]
    if reverse:
        p = p[::-1]
    return relative_motions(p)


def batch_targets(sequences, seq_idx, clips, reverse, N):
    """(rot [B,N,3], tr [B,N,3]) float64 for a batch of the loader."""
    rs, ts = [], []
    for si, ci, rv in zip(np.asarray(seq_idx).tolist(), np.asarray(clips).tolist(), np.asarray(reverse).tolist()):
        r, t = sequences[si].targets(ci, N, bool(rv))
        rs.append(r)
        ts.append(t)
    return np.stack(rs), np.stack(ts)


def rank_slice(batch, world, rank):
    """Rank `rank`'s contiguous share [lo, hi) of a global batch of `batch` clips (data-parallel training)."""
    if batch % world:
        raise ValueError("batch_size %d does not divide by %d ranks" % (batch, world))
    per = batch // world
    return rank * per, (rank + 1) * per


# ------------------------------------------------------------------------------------------------ initial weights
def _conv_block(cin, cout, k, stride=1, padding=0):
    """layers/conv.py Conv: Conv2d, activation, BatchNorm2d, built in that order."""
    m = torch.nn.Module()
    m.conv = torch.nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=padding, bias=True)
    m.activation = torch.nn.Mish()
    m.bn = torch.nn.BatchNorm2d(cout)
    return m


def _residual_block(cin, cout, stride):
    """layers/conv.py ResidualConv: two Conv blocks, the 1x1 skip convolution, then activation + BatchNorm2d."""
    m = torch.nn.Module()
    m.conv = torch.nn.Sequential(_conv_block(cin, cin, 3, 1, 1), _conv_block(cin, cout, 3, stride, 1))
    m.skip_layer = torch.nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=True)
    m.out_block = torch.nn.Sequential(torch.nn.Mish(), torch.nn.BatchNorm2d(cout))
    return m


def _linear_block(cin, cout):
    """layers/linear.py Linear with the shipped options (Mish, no norm, no dropout)."""
    m = torch.nn.Module()
    m.linear = torch.nn.Linear(cin, cout, bias=True)
    m.activation = torch.nn.Mish()
    return m


def initial_clvo_state(batch_size=1):
    """state_dict of a freshly constructed `ATDNVO(batch_size)` under the current torch RNG (it draws what the reference's
    constructor draws, in the same order). Keys and order: weights_spec.clvo_state_spec()."""
    from .weights_spec import clvo_state_spec
    del batch_size   # (the LSTM state tensors it sizes are zeros: no draw, no state-dict entry)
    m = torch.nn.Module()
    m.polar_norm = torch.nn.BatchNorm2d(2)
    m.encoder_CNN = torch.nn.Sequential(
        torch.nn.Conv2d(2, 2, kernel_size=1, groups=2),
        _conv_block(2, 16, 7, 2, 3),
        _residual_block(16, 16, 2), _residual_block(16, 16, 2), _residual_block(16, 16, 2), _residual_block(16, 16, 2),
        _conv_block(16, 16, 3, 3, 0),
        torch.nn.Flatten(),
        _linear_block(832, 512))
    m.lstm1 = torch.nn.LSTMCell(512, 512)
    m.lstm_linear = _linear_block(512, 512)
    m.lstm2 = torch.nn.LSTMCell(512, 512)
    for head in ("translation_regressor", "rotation_regressor"):
        setattr(m, head, torch.nn.Sequential(_linear_block(512, 128), _linear_block(128, 64), torch.nn.Linear(64, 3, bias=False)))
    sd = m.state_dict()
    spec = clvo_state_spec()
    if list(sd) != list(spec):
        raise AssertionError("initial_clvo_state: key order differs from clvo_state_spec")
    return {k: v.detach().clone() for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ KITTI reader
def read_poses(data_path, sequence):
    """`<data_path>/dataset/poses/<seq>.txt` -> float64 [n,12] (KITTI rows)."""
    return np.loadtxt(os.path.join(data_path, "dataset", "poses", sequence + ".txt"), dtype=np.float64).reshape(-1, 12)


def _decode_png(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return torch.from_numpy(a.transpose(2, 0, 1).copy())


class KittiSequence:
    """uint8 frames [T,3,H,W] of `<data_path>/dataset/sequences/<seq>/image_2/*.png`, decoded on demand by a thread pool
    (at most 16 workers). A slice [s:e] returns a pinned host tensor and starts decoding the frames of the next clip of
    the same length (frames e-1 .. e-1+(e-s)): the walk of FlowBank.add_sequence overlaps decoding with the GPU."""

    def __init__(self, data_path, sequence, workers=16):
        self.files = sorted(glob.glob(os.path.join(data_path, "dataset", "sequences", sequence, "image_2", "*.png")))
        if not self.files:
            raise FileNotFoundError("no image_2/*.png for sequence %s under %s" % (sequence, data_path))
        first = _decode_png(self.files[0])
        self.shape = (len(self.files),) + tuple(first.shape)
        self.dtype = torch.uint8
        self.is_cuda = False
        self._pool = ThreadPoolExecutor(max_workers=max(1, min(16, int(workers))))
        self._pending = {0: self._pool.submit(lambda: first)}

    def __len__(self):
        return self.shape[0]

    def _want(self, i):
        if i not in self._pending and 0 <= i < len(self.files):
            self._pending[i] = self._pool.submit(_decode_png, self.files[i])

    def __getitem__(self, sl):
        if not isinstance(sl, slice):
            raise TypeError("KittiSequence takes slices")
        s, e, step = sl.indices(len(self.files))
        if step != 1 or e <= s:
            raise IndexError("KittiSequence takes non-empty contiguous slices")
        for i in range(s, e):
            self._want(i)
        for i in range(e - 1, min(2 * e - s - 1, len(self.files))):   # the next clip of the same length
            self._want(i)
        out = torch.empty((e - s,) + self.shape[1:], dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        for i in range(s, e):
            out[i - s] = self._pending[i].result()
        for i in [k for k in self._pending if k < e - 1]:
            del self._pending[i]
        return out

    def close(self):
        self._pool.shutdown(wait=True, cancel_futures=True)
