"""Map view on the device: the kernels of atdn_view_render (transforms.render_points, VoxelMap.render, KeyframeMap.render_depths
and NeuralSLAM's map_depth on device tensors, and the raw entry point) against the host form and the NumPy restatement of the
rule (tests/map_view_ref.py) — every bit of depth, colours, support and counts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib, transforms
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.keyframe_map import KeyframeMap
from atdn_vslam_amd.voxel_map import VoxelMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_view_ref as R  # noqa: E402
import voxel_map_ref as V  # noqa: E402
from slam_cases import _Args, EverySecond, SLAM_CALIB, _tree  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the small hand camera: 5 x 7, fx = fy = 4, principal point on pixel (3, 2); with size 0.25 a point at z = 2 has
# hx = 0.5 * splat * 0.25 * 4 / 2 = splat / 4 pixels (0.5 after the clamp for splat <= 2), all exact in binary
HW, CAL, SIZE = (5, 7), (4.0, 4.0, 3.0, 2.0), 0.25
EYE = V.IDENTITY[None].copy()


def _t(a, dev=DEV):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


def _np(out):
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _render(dev, pts, col, cnt, poses, calib, hw, size, **options):
    return _np(transforms.render_points(_t(pts, dev), _t(col, dev), _t(cnt, dev), _t(poses, dev), calib, hw, size, **options))


def _three(pts, col, cnt, poses, calib=CAL, hw=HW, size=SIZE, **options):
    """Kernels == restatement == host form, bit for bit; returns the images."""
    want = R.render(pts, col, cnt, poses, calib, hw, size, **options)
    got = _render(DEV, pts, col, cnt, poses, calib, hw, size, **options)
    assert R.same_images(got, want), (options, got[3], want[3])
    host = _render("cpu", pts, col, cnt, poses, calib, hw, size, **options)
    assert R.same_images(got, host), options
    return got


def _at(u, v, z=2.0):
    """The point that the hand camera sees at pixel coordinates (u, v) and depth z (exact for the values used here)."""
    return [(u - CAL[2]) / CAL[0] * z, (v - CAL[3]) / CAL[1] * z, z]


# ---------------------------------------------------------------------------------------------------- 1. the same cases, three ways
@pytest.mark.parametrize("name,H,W,K,seed", R.CASES, ids=[c[0] for c in R.CASES])
def test_kernels_equal_the_restatement_and_the_host_form(name, H, W, K, seed):
    c = R.cloud(H, W, K, seed)
    for colored, min_count, splat in R.variants():
        _three(c["points"], c["colors"] if colored else None, c["counts"], c["poses"], c["calib"], c["hw"], R.VOXEL,
               min_count=min_count, splat=splat)


# ---------------------------------------------------------------------------------------------------- 2. hand-placed points
def _covered(img):
    return img[0][0] != 0


def test_half_open_footprint_on_both_sides():
    """u = 2.5, hx = 0.5: u - hx = 2 and u + hx = 3 exactly. Column 2 is in (closed on the left), column 3 is out (open on the
    right); rows likewise with v = 1.5."""
    pts, col, cnt = R.hand([_at(2.5, 1.5)], n=[7], rgb=[[1, 2, 3]])
    img = _three(pts, col, cnt, EYE)
    want = np.zeros(HW, dtype=bool)
    want[1, 2] = True
    assert np.array_equal(_covered(img), want) and img[0][0, 1, 2] == 2.0 and img[2][0, 1, 2] == 7
    assert img[1][0, :, 1, 2].tolist() == [1, 2, 3] and img[3].tolist() == [[1, 1, 1]]


@pytest.mark.parametrize("u,v,rows,cols", [(0.0, 2.0, (1, 3), (0, 1)), (6.0, 2.0, (1, 3), (5, 6)), (3.0, 0.0, (0, 1), (2, 4)),
                                           (3.0, 4.0, (3, 4), (2, 4))], ids=["left", "right", "top", "bottom"])
def test_footprint_half_outside_a_border(u, v, rows, cols):
    """splat = 6: hx = 1.5, the footprint [u - 1.5, u + 1.5) is three pixels a side and half of it lies outside."""
    pts, col, cnt = R.hand([_at(u, v)])
    img = _three(pts, col, cnt, EYE, splat=6.0)
    want = np.zeros(HW, dtype=bool)
    want[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = True
    assert np.array_equal(_covered(img), want) and img[3].tolist() == [[1, 1, int(want.sum())]]


@pytest.mark.parametrize("u,v", [(-1.0, 2.0), (7.0, 2.0), (3.0, -1.0), (3.0, 5.0)], ids=["left", "right", "top", "bottom"])
def test_footprint_wholly_outside_by_one_pixel(u, v):
    pts, col, cnt = R.hand([_at(u, v)])
    img = _three(pts, col, cnt, EYE)
    assert not _covered(img).any() and img[3].tolist() == [[1, 0, 0]]


def test_max_splat_caps_and_a_footprint_larger_than_the_image():
    pts, col, cnt = R.hand([_at(3.0, 2.0)])
    img = _three(pts, col, cnt, EYE, splat=6.0, max_splat=2)            # hx = 1.5 capped to 1: [2, 4) x [1, 3)
    want = np.zeros(HW, dtype=bool)
    want[1:3, 2:4] = True
    assert np.array_equal(_covered(img), want)
    img = _three(pts, col, cnt, EYE, splat=100.0)                       # hx = 25: the whole image
    assert _covered(img).all() and img[3].tolist() == [[1, 1, 35]]
    img = _three(pts, col, cnt, EYE, splat=1e300, max_splat=1 << 20)    # an infinite hx is clamped like any other
    assert _covered(img).all()


def test_near_and_far_are_inside_and_the_next_doubles_are_outside():
    """R = I, so z = (double)p_z - (double)t_z exactly: with p_z = 0.5 and t_z = 2^-54 it is the next double below 0.5, with
    p_z = 40 and t_z = -2^-47 the next double above 40."""
    pts, col, cnt = R.hand([_at(3.0, 2.0, 0.5), _at(5.0, 2.0, 40.0)])
    assert _three(pts, col, cnt, EYE, splat=0.5)[3].tolist() == [[2, 2, 2]]          # (splat 0.5: one pixel at z = 0.5 too)
    below, above = EYE.copy(), EYE.copy()
    below[0, 11], above[0, 11] = 2.0 ** -54, -2.0 ** -47
    assert np.float64(0.5) - np.float64(below[0, 11]) == np.nextafter(0.5, 0.0)
    assert np.float64(40.0) - np.float64(above[0, 11]) == np.nextafter(40.0, 50.0)
    img = _three(pts, col, cnt, below, splat=0.5)
    assert img[3].tolist() == [[2, 1, 1]] and img[0][0, 2, 5] == 40.0 and img[0][0, 2, 3] == 0
    img = _three(pts, col, cnt, above, splat=0.5)
    assert img[3].tolist() == [[2, 1, 1]] and img[0][0, 2, 3] == 0.5 and img[0][0, 2, 5] == 0


def test_a_point_behind_the_camera():
    pts, col, cnt = R.hand([_at(3.0, 2.0, -2.0), [0.0, 0.0, 0.0]])
    assert _three(pts, col, cnt, EYE)[3].tolist() == [[2, 0, 0]]


def test_equal_depths_go_to_the_better_supported_point_then_the_smaller_colour():
    p = _at(3.0, 2.0)
    for order in ([0, 1], [1, 0]):
        pts, col, cnt = R.hand([p, p], n=[2, 5], rgb=[[1, 1, 1], [9, 9, 9]])
        img = _three(pts[order], col[order], cnt[order], EYE)
        assert img[2][0, 2, 3] == 5 and img[1][0, :, 2, 3].tolist() == [9, 9, 9]
        pts, col, cnt = R.hand([p, p], n=[300, 255], rgb=[[4, 0, 200], [3, 255, 255]])   # both count as 255
        img = _three(pts[order], col[order], cnt[order], EYE)
        assert img[2][0, 2, 3] == 255 and img[1][0, :, 2, 3].tolist() == [3, 255, 255]
    # nearer beats better supported
    pts, col, cnt = R.hand([p, _at(3.0, 2.0, 1.5)], n=[200, 1])
    assert _three(pts, col, cnt, EYE)[0][0, 2, 3] == 1.5


def test_a_wave_on_one_pixel_and_on_64_rows():
    rs = np.random.RandomState(3)
    z = rs.permutation(64) * 0.25 + 1.0
    pts, col, cnt = R.hand([_at(3.0, 2.0, float(v)) for v in z], n=rs.randint(1, 9, 64), rgb=rs.randint(0, 256, (64, 3)))
    img = _three(pts, col, cnt, EYE)
    assert img[0][0, 2, 3] == 1.0 and img[3].tolist() == [[64, 64, 1]]
    hw = (70, 7)
    pts, col, cnt = R.hand([_at(float(r % 7), 3.0 + r) for r in range(64)], rgb=rs.randint(0, 256, (64, 3)))
    img = _three(pts, col, cnt, EYE, hw=hw)
    assert img[3].tolist() == [[64, 64, 64]] and (_covered(img).sum(axis=1)[3:67] == 1).all()


@pytest.mark.parametrize("M", [0, 1, 63, 64, 65])
def test_point_counts_around_a_wave(M):
    c = R.cloud(9, 33, 3, 2)
    pick = np.random.RandomState(M).permutation(len(c["points"]))[:M]
    img = _three(c["points"][pick], c["colors"][pick], c["counts"][pick], c["poses"], c["calib"], c["hw"], R.VOXEL, splat=2.0)
    assert img[3][:, 0].tolist() == [M] * 3


def test_nan_and_infinity_in_a_pose_and_in_a_point():
    """One pose of three holds a NaN (then an infinity): its camera sees nothing, the others what they saw. One point holds
    a NaN (an infinity): it is a candidate that is not visible, the images are those of the cloud without it."""
    c = R.cloud(9, 33, 3, 2)
    args = (c["calib"], c["hw"], R.VOXEL)
    clean = _three(c["points"], c["colors"], c["counts"], c["poses"], *args)
    M = len(c["points"])
    for bad in (np.nan, np.inf, -np.inf):
        for slot in (3, 0, 10):                                          # t_x, r_00, r_22
            poses = c["poses"].copy()
            poses[1, slot] = bad
            img = _three(c["points"], c["colors"], c["counts"], poses, *args)
            for k in (0, 2):
                assert all(np.array_equal(a[k], b[k]) for a, b in zip(img, clean))
            assert img[3][1].tolist() == [M, 0, 0] and not img[0][1].any() and not img[2][1].any()
        i = int(np.argmax(c["counts"]))
        pts = c["points"].copy()
        pts[i, 1] = bad
        img = _three(pts, c["colors"], c["counts"], c["poses"], *args)
        keep = np.arange(M) != i
        without = _three(c["points"][keep], c["colors"][keep], c["counts"][keep], c["poses"], *args)
        assert all(np.array_equal(a, b) for a, b in zip(img[:3], without[:3]))
        assert (img[3][:, 0] == M).all() and np.array_equal(img[3][:, 1:], without[3][:, 1:])


# ---------------------------------------------------------------------------------------------------- 3. guards
def _raw(L, d, c, shape, out, work, options=(R.VOXEL, 1.0, 64, 0.5, 40.0, 1)):
    B, H, W = shape
    return L.atdn_view_render(_p(d["points"]), _p(d["colors"]), _p(d["counts"]), d["M"], _p(d["poses"]), B, H, W,
                              *c["calib"], *options, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(work), _stream())


def test_guards_around_every_output_at_every_alignment():
    """Every input and output off its natural vector alignment — the byte planes at each of the eight offsets within a word,
    depth at an odd float, counts and the workspace one word off — with guard values before and behind every output and the
    workspace."""
    c = R.cloud(9, 33, 3, 13)
    B, (H, W) = 3, c["hw"]
    n = B * H * W
    L = _lib.lib()
    want = R.render(c["points"], c["colors"], c["counts"], c["poses"], c["calib"], c["hw"], R.VOXEL)
    assert L.atdn_view_workspace_bytes(B, H, W) == 8 * n

    def shifted(a, dtype, fill, by=1):
        flat = torch.full((a.size + by + 1,), fill, dtype=dtype, device=DEV)
        flat[by:by + a.size] = _t(a).reshape(-1)
        return flat[by:]

    d = dict(points=shifted(c["points"], torch.float32, 1.0), colors=shifted(c["colors"], torch.uint8, 9),
             counts=shifted(c["counts"], torch.int32, 1), poses=shifted(c["poses"], torch.float32, 1.0), M=len(c["counts"]))
    for s in range(8):
        depth = torch.full((n + 4,), -7.0, device=DEV)
        colors = torch.full((3 * n + 16,), 7, dtype=torch.uint8, device=DEV)
        support = torch.full((n + 16,), 7, dtype=torch.uint8, device=DEV)
        counts = torch.full((3 * B + 2,), -7, dtype=torch.int64, device=DEV)
        work = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
        f = 1 + s % 2
        out = (depth[f:f + n], colors[s + 1:s + 1 + 3 * n], support[s + 1:s + 1 + n], counts[1:1 + 3 * B])
        _lib.check(_raw(L, d, c, (B, H, W), out, work[1:]))
        assert (depth[:f] == -7).all() and (depth[f + n:] == -7).all(), s
        assert (colors[:s + 1] == 7).all() and (colors[s + 1 + 3 * n:] == 7).all(), s
        assert (support[:s + 1] == 7).all() and (support[s + 1 + n:] == 7).all(), s
        assert counts[0] == -7 and counts[-1] == -7 and work[0] == 0x5A5A5A5A and work[-1] == 0x5A5A5A5A, s
        got = (out[0].view(B, H, W).cpu().numpy(), out[1].view(B, 3, H, W).cpu().numpy(), out[2].view(B, H, W).cpu().numpy(),
               out[3].view(B, 3).cpu().numpy())
        assert R.same_images(got, want), s
    # the guard refuses overlapping and misaligned buffers before anything is launched
    assert _raw(L, d, c, (B, H, W), (out[0], out[1], out[1], out[3]), work[1:]) != 0 and b"overlap" in L.atdn_last_error()
    assert _raw(L, d, c, (B, H, W), (d["points"], out[1], out[2], out[3]), work[1:]) != 0 and b"overlaps" in L.atdn_last_error()
    assert _raw(L, d, c, (B, H, W), (out[0], out[1], out[2], work[1:1 + 3 * B]), work[1:]) != 0 and b"overlap" in L.atdn_last_error()
    odd = C.c_void_p(work.data_ptr() + 4)
    assert L.atdn_view_render(_p(d["points"]), None, _p(d["counts"]), 1, _p(d["poses"]), B, H, W, *c["calib"], R.VOXEL, 1.0, 64, 0.5,
                              40.0, 1, _p(out[0]), None, _p(out[2]), _p(out[3]), odd, _stream()) != 0
    assert b"aligned" in L.atdn_last_error()
    assert _raw(L, d, c, (B, H, W), out, work[1:], options=(R.VOXEL, 1.0, 64, 0.5, float("inf"), 1)) != 0
    assert b"far" in L.atdn_last_error()


# ---------------------------------------------------------------------------------------------------- 4. execution variants
@pytest.fixture(scope="module")
def full_size():
    _, H, W, K, seed = R.FULL_CASE
    s = V.scene(H, W, K, seed)
    m = VoxelMap("cpu", capacity=1 << 21)
    m.integrate(_t(s["depth"], "cpu"), _t(s["poses"], "cpu"), s["calib"], images=_t(s["images"], "cpu"))
    cloud = m.extract()[:3]
    host = _np(transforms.render_points(*cloud, _t(s["poses"], "cpu"), s["calib"], (H, W), 0.25))
    return s, tuple(t.numpy() for t in cloud), host


def test_full_size_two_calls_streams_and_graph(full_size):
    """376 x 1232, B = 2 against the host form. The same bits on a second call into the same buffers, on a side stream, and
    from a captured graph of the three launches (a linear chain) replayed twice over buffers filled with 0 and with ones — a
    capture fails on any host synchronisation, so the replay shows the call has none."""
    s, (pts, col, cnt), host = full_size
    K, H, W = s["depth"].shape
    a = _render(DEV, pts, col, cnt, s["poses"], s["calib"], (H, W), 0.25)
    assert R.same_images(a, host) and a[3][:, 2].min() > H * W // 2
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = _render(DEV, pts, col, cnt, s["poses"], s["calib"], (H, W), 0.25)
    side.synchronize()
    assert R.same_images(a, b)
    L = _lib.lib()
    d = dict(points=_t(pts), colors=_t(col), counts=_t(cnt), poses=_t(s["poses"]), M=len(cnt))
    n = K * H * W
    out = (torch.empty((K, H, W), device=DEV), torch.empty((K, 3, H, W), dtype=torch.uint8, device=DEV),
           torch.empty((K, H, W), dtype=torch.uint8, device=DEV), torch.empty((K, 3), dtype=torch.int64, device=DEV))
    work = torch.empty((n,), dtype=torch.int64, device=DEV)
    for fill in (0, -1):                                                 # a second call into the same buffers
        for o in out + (work,):
            o.fill_(fill)
        _lib.check(_raw(L, d, s, (K, H, W), out, work))
        assert R.same_images(_np(out), a), fill
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_raw(L, d, s, (K, H, W), out, work))
    for fill in (0, -1):
        for o in out + (work,):
            o.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert R.same_images(_np(out), a), fill


# ---------------------------------------------------------------------------------------------------- 5. properties
WALL_HW, WALL_CAL, WALL_VOXEL = (16, 64), (32.0, 32.0, 31.5, 7.5), 0.25
WALL_BOUND = WALL_VOXEL / 2 + WALL_VOXEL / 65536     # a voxel's mean point lies inside the voxel; its sub-voxel part is quantised


def _wall_map(depths):
    m = VoxelMap(DEV, voxel=WALL_VOXEL, capacity=1 << 14)
    d = np.stack(depths).astype(np.float32)
    m.integrate(_t(d), _t(np.repeat(EYE, len(d), axis=0)), WALL_CAL)
    return m


def test_a_wall_rendered_back_into_its_camera():
    """A fronto-parallel wall at 5.1 integrated from one camera and rendered back into it. Every covered pixel's depth is within
    voxel/2 + voxel/65536 of the wall. With splat = 2 no interior pixel is empty: a pixel's own point went into a voxel whose
    mean point is less than one edge from it on every axis, and the footprint reaches one edge to each side."""
    H, W = WALL_HW
    m = _wall_map([np.full(WALL_HW, 5.1)])
    for splat in (1.0, 2.0):
        depth, _, support, counts = _np(m.render(EYE, WALL_CAL, WALL_HW, splat=splat))
        covered = depth[0] != 0
        assert covered.sum() == counts[0, 2] > 0 and (support[0][covered] >= 1).all()
        err = np.abs(depth[0][covered].astype(np.float64) - 5.1)
        print("wall: splat %g, covered %d of %d, max |depth - 5.1| = %.3g (bound %.6g)" % (splat, covered.sum(), H * W, err.max(), WALL_BOUND))
        assert err.max() <= WALL_BOUND
    assert covered[1:-1, 1:-1].all()


def test_a_near_wall_hides_the_far_wall_and_a_sideways_camera_sees_behind_its_edge():
    """Far wall at 8 everywhere, near wall at 4 over the left half (world x < 0), both in the cloud. From the camera they were
    seen from, every pixel that a near point's footprint covers shows the near depth and every other covered pixel the far one.
    From a camera 2 to the right the near wall's edge lies at u = cx - 16 and the far wall's x in (-2, 0) — hidden before — at
    u in (cx - 16, cx - 8): columns 18 .. 22 (with splat = 2 a near footprint ends below 15.5 + 2) show the far wall."""
    H, W = WALL_HW
    split = np.full(WALL_HW, 8.0)
    split[:, :W // 2] = 4.0
    m = _wall_map([np.full(WALL_HW, 8.0), split])
    pts, _, cnt, _ = _np(m.extract())
    near = pts[:, 2] < 6.0
    assert near.any() and (~near).any() and (pts[near, 0] < 0).all()
    depth = _np(m.render(EYE, WALL_CAL, WALL_HW))[0][0]
    _, vis, x0, x1, y0, y1, _ = R.words(pts[near], None, cnt[near], EYE[0], WALL_CAL, WALL_HW, WALL_VOXEL)
    both = np.zeros(WALL_HW, dtype=bool)
    for i in np.flatnonzero(vis):
        both[y0[i]:y1[i] + 1, x0[i]:x1[i] + 1] = True
    assert both.any() and (np.abs(depth[both] - 4.0) <= WALL_BOUND).all()
    rest = ~both & (depth != 0)
    assert rest.any() and (np.abs(depth[rest] - 8.0) <= WALL_BOUND).all()
    # splat = 2 from here on: footprints of neighbouring voxels meet (the wall test), so the near wall has no gaps
    dense = _np(m.render(EYE, WALL_CAL, WALL_HW, splat=2.0))[0][0]
    assert (np.abs(dense[:, 24:30] - 4.0) <= WALL_BOUND).all()
    moved = EYE.copy()
    moved[0, 3] = 2.0
    side = _np(m.render(moved, WALL_CAL, WALL_HW, splat=2.0))[0][0]
    assert (np.abs(side[:, 18:23] - 8.0) <= WALL_BOUND).all()
    assert (np.abs(side[:, :14] - 4.0) <= WALL_BOUND).all()


# ---------------------------------------------------------------------------------------------------- 6. Python and SLAM
def test_voxel_map_render_keeps_its_extraction_until_the_next_integrate(monkeypatch):
    s = V.scene(9, 33, 3, 5)
    m = VoxelMap(DEV, capacity=1 << 12)
    calls = []
    extract = VoxelMap.extract
    monkeypatch.setattr(VoxelMap, "extract", lambda self, *a, **k: calls.append(1) or extract(self, *a, **k))
    d, P, im = _t(s["depth"]), _t(s["poses"]), _t(s["images"])
    m.integrate(d, P, s["calib"], images=im, indices=[0, 1])
    a = _np(m.render(P, s["calib"], (9, 33)))
    b = _np(m.render(P[:1], s["calib"], (9, 33), splat=2.0, min_count=2))
    assert len(calls) == 1 and b[0].shape == (1, 9, 33)
    (pts, col, cnt, _), _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"], indices=[0, 1])
    assert R.same_images(a, R.render(pts, col, cnt, s["poses"], s["calib"], (9, 33), 0.25))
    assert R.same_images(b, R.render(pts, col, cnt, s["poses"][:1], s["calib"], (9, 33), 0.25, splat=2.0, min_count=2))
    m.integrate(d, P, s["calib"], images=im, indices=[2])
    c = _np(m.render(P, s["calib"], (9, 33)))
    assert len(calls) == 2
    (pts, col, cnt, _), _ = V.reference(s["depth"], s["poses"], s["calib"], s["images"])
    assert R.same_images(c, R.render(pts, col, cnt, s["poses"], s["calib"], (9, 33), 0.25))


def test_keyframe_map_render_depths_fills_exactly_the_zero_pixels():
    H, W, N = 16, 48, 4
    s = V.scene(H, W, N, 21, special=False)
    m = KeyframeMap(DEV, hw=(H, W), capacity=2)
    P = torch.cat([torch.from_numpy(s["poses"]).view(N, 3, 4), torch.tensor([0.0, 0, 0, 1]).view(1, 1, 4).repeat(N, 1, 1)], dim=1)
    holes = s["depth"].copy()
    holes[:, :, ::3] = 0                                               # every third column failed
    holes[N - 1] = 0                                                   # the last keyframe measured nothing
    for k in range(N):
        m.append(torch.from_numpy(s["images"][k]), P[k])
        m.set_depth(k, torch.from_numpy(holes[k]))
    vm = m.voxel_map(s["calib"], capacity=1 << 12)
    before = m.depth_bank.clone()
    want = _np(vm.render(_t(s["poses"]), s["calib"], (H, W), splat=2.0))[0]
    out = m.render_depths(vm, s["calib"], splat=2.0, batch=3)
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(m.depth_bank, before)
    cloud = vm.extract()[:3]
    bare = m.render_depths(cloud, s["calib"], indices=[2, 0], size=vm.voxel, splat=2.0)
    assert np.array_equal(bare.cpu().numpy(), want[[2, 0]]) and torch.equal(m.depth_bank, before)
    m.render_depths(vm, s["calib"], indices=[3, 1], fill=True, splat=2.0)
    after, b = m.depth_bank.cpu().numpy(), before.cpu().numpy()
    assert np.array_equal(after[[0, 2]], b[[0, 2]]) and np.array_equal(after[N:], b[N:])
    for k in (1, 3):
        hole = b[k] == 0
        assert np.array_equal(after[k][~hole], b[k][~hole]) and np.array_equal(after[k][hole], want[k][hole])
        assert (want[k][hole] != 0).any()


def test_neuralslam_map_depth(tmp_path):
    """Five synthetic frames, keyframes 0, 2, 4 (as the voxel map's SLAM test). The synthetic weights give arbitrary flows and
    depths: this pins the plumbing — map_depth/ appears only with the option and holds voxel_map.render at the keyframe poses,
    every other file is what it was — not accuracy."""
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd = syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1241, seed=8))

    with pytest.raises(ValueError, match="map_depth"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, map_depth=True)
    with pytest.raises(ValueError, match="map_depth"):
        NeuralSLAM(_Args(str(tmp_path)), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True,
                   voxel_map=True, map_depth="yes")
    options = dict(voxel=0.5, max_z=80.0, stride=2, capacity=1 << 12)
    run = {}
    for name, kw in (("off", {}), ("on", dict(map_depth=True)), ("fill", dict(map_depth="fill"))):
        path = os.path.join(str(tmp_path), name)
        os.makedirs(os.path.join(path, "map_depth"))
        with open(os.path.join(path, "map_depth", "stale.pth"), "w") as f:   # of an earlier session: only the option clears it
            f.write("stale")
        slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, calib=SLAM_CALIB, resident_map=True, voxel_map=True,
                          voxel_options=options, **kw)
        assert os.path.exists(os.path.join(path, "map_depth", "stale.pth")) == (name == "off")
        if name == "off":
            os.remove(os.path.join(path, "map_depth", "stale.pth"))
            os.rmdir(os.path.join(path, "map_depth"))
        slam._policy = EverySecond()
        slam.start_odometry()
        poses = [slam(f).clone() for f in frames]
        slam.end_odometry(mapping_weights=vsd)
        run[name] = (slam, path, poses)
    (off, off_path, off_poses), (slam, path, poses) = run["off"], run["on"]
    assert all(torch.equal(a, b) for a, b in zip(poses, off_poses)) and len(slam) == len(off) == 3
    assert not os.path.exists(os.path.join(off_path, "map_depth"))
    extra = ["map_depth/%06d.pth" % i for i in range(3)] + ["map_depth/"]
    assert sorted(_tree(path)) == sorted(_tree(off_path) + extra)
    for f in _tree(off_path):                                            # every other file, byte for byte
        if not f.endswith("/"):
            assert open(os.path.join(path, f), "rb").read() == open(os.path.join(off_path, f), "rb").read(), f
    assert torch.equal(slam._map.depth_bank, off._map.depth_bank)
    kf_poses = slam._map.poses[:3, :3, :].reshape(3, 12).to(DEV)
    want = slam.voxel_map.render(kf_poses, SLAM_CALIB, (376, 1232))
    print("map depth: counts", want[3].tolist())
    assert want[3][:, 2].sum() > 0
    for i in range(3):
        d = torch.load(os.path.join(path, "map_depth", "%06d.pth" % i))
        assert d.dtype == torch.float32 and tuple(d.shape) == (1, 376, 1232) and torch.equal(d[0], want[0][i].cpu())
    view = slam.render_map(slam._map.poses[:3].clone(), splat=2.0)
    assert all(a is None and b is None or torch.equal(a, b)
               for a, b in zip(view, slam.voxel_map.render(kf_poses, SLAM_CALIB, (376, 1232), splat=2.0)))
    # map_depth="fill": the same files, and the bank's zero pixels, and no others, hold the rendered depth
    filler, fill_path, fill_poses = run["fill"]
    assert all(torch.equal(a, b) for a, b in zip(fill_poses, off_poses)) and sorted(_tree(fill_path)) == sorted(_tree(path))
    for f in _tree(path):
        if not f.endswith("/"):
            assert open(os.path.join(fill_path, f), "rb").read() == open(os.path.join(path, f), "rb").read(), f
    bank = off._map.depth_bank
    assert (bank[:3] == 0).any() and torch.equal(filler._map.depth_bank[:3], torch.where(bank[:3] == 0, want[0], bank[:3]))
    assert torch.equal(filler._map.depth_bank[3:], bank[3:])
    # on demand
    before = slam._map.depth_bank.clone()
    filled = slam.write_map_depth(fill=True)
    assert torch.equal(filled, want[0])
    hole = before[:3] == 0
    assert torch.equal(slam._map.depth_bank[:3][~hole], before[:3][~hole]) and torch.equal(slam._map.depth_bank[:3][hole], want[0][hole])
    assert torch.equal(slam._map.depth_bank[3:], before[3:])
