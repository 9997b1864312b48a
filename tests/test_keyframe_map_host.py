"""Host-side checks of the keyframe map (no GPU): both C entry points refuse bad arguments before anything is launched,
`KeyframeMap.from_directory` validates a directory before any device work, and `NeuralSLAM.relocalize_batch` says how to
enable the resident map."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib
from atdn_vslam_amd.keyframe_map import KeyframeMap, embedding_hw
from atdn_vslam_amd.slam import NeuralSLAM

# never dereferenced: every call below must fail in the host-side argument checks
A = 0x10000          # a 16-byte aligned "device pointer"
D = 15360


def _search(bank=A, K=8, Dv=D, queries=A + 0x100000, Q=1, topk=1, dist=A + 0x200000, idx=A + 0x300000):
    L = _lib.lib()
    rc = L.atdn_map_search(C.c_void_p(bank), K, Dv, C.c_void_p(queries), Q, topk, C.c_void_p(dist), C.c_void_p(idx), None)
    return rc, L.atdn_last_error().decode()


def _gather(bank=A, K=8, plane=3 * 376 * 1232, index=(0,), out=A + 0x100000, n=None):
    L = _lib.lib()
    ix = np.asarray(index, dtype=np.int32)
    ip = ix.ctypes.data_as(C.c_void_p) if index is not None else None
    rc = L.atdn_map_gather_images_u8(C.c_void_p(bank), K, plane, ip, len(ix) if n is None else n, C.c_void_p(out), None)
    return rc, L.atdn_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(K=0), "no keyframe"),
    (dict(Dv=15362), "multiple of 4"),
    (dict(Dv=0), "multiple of 4"),
    (dict(Q=0), "no query"),
    (dict(topk=0), "topk"),
    (dict(K=3, topk=4), "topk"),
    (dict(K=100, topk=17), "topk"),
    (dict(bank=A + 4), "aligned"),
    (dict(queries=A + 8), "aligned"),
    (dict(dist=A + 2), "aligned"),
    (dict(bank=0), "null"),
    (dict(queries=0), "null"),
    (dict(dist=0), "null"),
    (dict(idx=0), "null"),
])
def test_search_argument_errors(kw, word):
    rc, msg = _search(**kw)
    assert rc != 0 and word in msg, msg
    with pytest.raises(RuntimeError, match=word):
        _lib.check(rc)


@pytest.mark.parametrize("kw, word", [
    (dict(index=(-1,)), "outside"),
    (dict(index=(0, 8)), "outside"),
    (dict(index=(3, 2, 1 << 30)), "outside"),
    (dict(K=0), "bad argument"),
    (dict(n=0), "bad argument"),
    (dict(plane=1000), "multiple of 16"),
    (dict(bank=A + 1), "aligned"),
    (dict(out=A + 4), "aligned"),
    (dict(bank=0), "null"),
    (dict(out=0), "null"),
])
def test_gather_argument_errors(kw, word):
    rc, msg = _gather(**kw)
    assert rc != 0 and word in msg, msg


def test_gather_null_index_table():
    L = _lib.lib()
    assert L.atdn_map_gather_images_u8(C.c_void_p(A), 8, 3 * 376 * 1232, None, 1, C.c_void_p(A), None) != 0
    assert b"null" in L.atdn_last_error()


def test_gather_error_names_the_offending_index():
    rc, msg = _gather(index=(0, 5, 9, 1))
    assert rc != 0 and "image 2" in msg and "index 9" in msg and "[0, 8)" in msg, msg


def test_embedding_size_of_the_slam_geometry():
    assert embedding_hw((376, 1232)) == (6, 20)
    assert 6 * 20 * 128 == D


def _directory(tmp_path, n_frames=3, n_poses=3, odd=None, poses=True):
    kf = os.path.join(str(tmp_path), "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    for i in range(n_frames):
        shape = (3, 16, 32) if i != odd else (3, 16, 48)
        torch.save(torch.zeros(shape, dtype=torch.uint8), os.path.join(kf, "rgb", "%06d.pth" % i))
    if poses:
        torch.save(torch.eye(4).flatten()[:12].repeat(n_poses, 1), os.path.join(kf, "poses.pth"))
    return kf


def test_from_directory_validates_before_any_device_work(tmp_path):
    """Each of these is raised while the directory is read, before a device buffer exists: they pass on a machine with
    no GPU, where the constructor itself could not run."""
    with pytest.raises(FileNotFoundError, match="poses.pth"):
        KeyframeMap.from_directory(_directory(tmp_path / "a", poses=False), "cuda:0")
    with pytest.raises(ValueError, match="2 poses in poses.pth but 3 frames"):
        KeyframeMap.from_directory(_directory(tmp_path / "b", n_poses=2), "cuda:0")
    with pytest.raises(ValueError, match="frame of size"):
        KeyframeMap.from_directory(_directory(tmp_path / "c", odd=2), "cuda:0")
    with pytest.raises(ValueError, match="no keyframe"):
        KeyframeMap.from_directory(_directory(tmp_path / "e", n_frames=0, n_poses=0), "cuda:0")


def test_keyframe_map_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KeyframeMap("cpu")


def test_relocalize_batch_needs_the_resident_map():
    slam = NeuralSLAM.__new__(NeuralSLAM)     # (the constructor needs a GPU; the check under test reads one attribute)
    slam._map = None
    with pytest.raises(RuntimeError, match="resident_map=True"):
        slam.relocalize_batch(torch.zeros(2, 3, 376, 1232))
