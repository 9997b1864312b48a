"""What the GPU tests that drive `NeuralSLAM` share: the arguments object, the calibration of the 376 x 1232 grid, the keyframe
policy that registers every second pair, and the listings and bit comparisons of their assertions. A plain module, imported the
way flow_track_ref is."""
import os

import torch

from atdn_vslam_amd import depth as depth_mod
from atdn_vslam_amd.slam import KeyframePolicy

DEV = "cuda:0"
SLAM_CALIB = depth_mod.resize_calib((718.856, 718.856, 607.1928, 185.2157), (376, 1241), (376, 1232))


class _Args:
    def __init__(self, path):
        self.device = DEV
        self.keyframes_path = path


class EverySecond(KeyframePolicy):
    calls = 0

    def __call__(self, pred_mat):
        self.calls += 1
        return self.calls % 2 == 0


def _files(root):
    """Every file under `root`, relative, sorted."""
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _tree(root):
    """`_files`, then every directory with a trailing slash."""
    return _files(root) + sorted(os.path.relpath(os.path.join(d, s), root) + "/" for d, ss, _ in os.walk(root) for s in ss)


def _bits(a, b):
    """Same dtype, shape and bits (tensors of at least one dimension)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _bits_flat(a, b):
    """`_bits` for tensors of any rank, scalars included."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                      b.reshape(-1).contiguous().view(torch.uint8))
