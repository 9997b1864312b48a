"""Map view, host form: atdn_view_render_host (transforms.render_points and VoxelMap.render on CPU tensors) against the NumPy
restatement of the rule (tests/map_view_ref.py) — every bit of depth, colours, support and counts. Needs no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_view_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C"))


def _np(out):
    return tuple(None if t is None else t.numpy() for t in out)


def _render(c, colored, **options):
    return _np(transforms.render_points(_t(c["points"]), _t(c["colors"]) if colored else None, _t(c["counts"]), _t(c["poses"]),
                                        c["calib"], c["hw"], R.VOXEL, **options))


@pytest.mark.parametrize("name,H,W,K,seed", R.CASES, ids=[c[0] for c in R.CASES])
def test_host_form_equals_the_restatement(name, H, W, K, seed):
    """5 x 7 B = 1, 9 x 33 B = 3, 47 x 154 B = 2: the street's cloud into its own cameras, with and without colours, min_count 1
    and 3, splat 0.5, 1 and 2."""
    c = R.cloud(H, W, K, seed)
    seen = 0
    for colored, min_count, splat in R.variants():
        want = R.render(c["points"], c["colors"] if colored else None, c["counts"], c["poses"], c["calib"], c["hw"], R.VOXEL,
                        min_count=min_count, splat=splat)
        got = _render(c, colored, min_count=min_count, splat=splat)
        assert got[0].dtype == np.float32 and got[2].dtype == np.uint8 and got[3].dtype == np.int64
        assert (got[1] is None) == (not colored)
        assert R.same_images(got, want), (name, colored, min_count, splat, got[3], want[3])
        seen += int(want[3][:, 2].sum())
    assert seen > 0, "no case covered a pixel"


def test_empty_cloud_and_argument_errors():
    pts, cnt = torch.zeros((0, 3)), torch.zeros((0,), dtype=torch.int32)
    depth, colors, support, counts = transforms.render_points(pts, None, cnt, V.IDENTITY[None], (4.0, 4.0, 3.0, 2.0), (5, 7), 0.25)
    assert colors is None and not depth.any() and not support.any() and counts.tolist() == [[0, 0, 0]]
    one = torch.tensor([[0.0, 0.0, 2.0]])
    n = torch.ones((1,), dtype=torch.int32)
    assert float(np.float32(1.1)) != 1.1                                 # a far that fp32 cannot represent is refused
    for bad in (dict(splat=0.0), dict(max_splat=0), dict(near=0.0), dict(near=2.0, far=1.0), dict(far=float("inf")),
                dict(far=1.1), dict(min_count=0)):
        with pytest.raises(RuntimeError):
            transforms.render_points(one, None, n, V.IDENTITY[None], (4.0, 4.0, 3.0, 2.0), (5, 7), 0.25, **bad)
    with pytest.raises(RuntimeError):
        transforms.render_points(one, None, n, V.IDENTITY[None], (4.0, 4.0, 3.0, 2.0), (5, 7), 0.0)
    assert _lib.lib().atdn_view_workspace_bytes(2, 5, 7) == 8 * 2 * 5 * 7
    for dims in ((0, 5, 7), (1, 0, 7), (1, 5, 0), (2, 32768, 32768)):
        assert _lib.lib().atdn_view_workspace_bytes(*dims) == 0


def test_voxel_map_render_on_the_host_renders_its_extraction():
    """VoxelMap.render on a CPU map: the restatement of the render applied to the restatement of the cloud; near, far and the
    splat's unit are the map's min_z, max_z and voxel."""
    H, W, K = 9, 33, 3
    s = V.scene(H, W, K, 5)
    m = VoxelMap("cpu", capacity=1 << 12)
    m.integrate(_t(s["depth"]), _t(s["poses"]), s["calib"], images=_t(s["images"]))
    got = _np(m.render(_t(s["poses"]), s["calib"], (H, W), min_count=1, splat=2.0))
    (pts, col, cnt, _), _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"])
    want = R.render(pts, col, cnt, s["poses"], s["calib"], (H, W), 0.25, splat=2.0, near=0.5, far=40.0)
    assert R.same_images(got, want) and want[3][:, 2].sum() > 0
