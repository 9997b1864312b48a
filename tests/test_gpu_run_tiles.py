"""Run tiles of the 1x5 / 5x1 halo-patch convolutions (conv_sf6.h, RUN): an M tile is 128 consecutive pixels of the image in
row-major (1x5) or column-major (5x1) order instead of an 8 x 16 rectangle. Every output pixel accumulates the same taps and
channel chunks in the same order in both forms, so the two must agree bit for bit.

The product's dispatch takes grids as small as the ones below to 4 x 16-pixel tiles, so the convolution-level cases name the
tile form through the test entry atdn_conv2d_nhwc_sf_epi (include/atdn_hip.h): bit 2 of `sf_store` asks for the run tiles where
the shape allows them, bit 1 for the rectangular 8 x 16 x 128 tiles."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from atdn_vslam_amd import _lib
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import RAFTGMA

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


RUN_CASES = [
    # (Cin, Cout, KH, KW, H, W, nimg)
    (64, 128, 1, 5, 3, 43, 2),     # minimum run length: tile 0 holds two run boundaries, tile 1 a single pixel (partial last tile)
    (96, 160, 1, 5, 7, 47, 3),     # three boundaries in a tile; odd chunk count (surplus chunk of the unrolled loop); two N tiles,
                                   # the second partial; image index > 0
    (64, 128, 1, 5, 2, 200, 2),    # a run longer than a tile: tiles without a boundary, a tile that starts in the middle of a run
    (64, 128, 5, 1, 47, 5, 2),     # column-major runs of 47: a tile spans three columns, vertical zero padding at both ends
    (32, 128, 5, 1, 154, 3, 2),    # a single chunk (no patch refresh), a long vertical run
    (64, 128, 1, 5, 4, 42, 2),     # run length 42 is NOT served by the run tiles: the dispatch rules of the product apply
]


@pytest.mark.parametrize("sf_store", [0, 1])
@pytest.mark.parametrize("case", RUN_CASES)
def test_run_tiles_match_rectangular_tiles_and_fp64(case, sf_store):
    """Run tiles against the rectangular 8 x 16 x 128 tiles (same bits) and against an fp64 convolution (2e-5: the bound and the
    input / weight distributions of test_split_f16_halo_kernels_match_fp64 for these kernels).
    sf_store = 0 is the fp32 store of EpiBias, the epilogue of the ConvGRU context convolutions; sf_store = 1 the split-f16 store of
    SfBias, decoded again by from_sf. Both are channel-vector epilogues of the halo-patch kernels (tile_pixel, slab transpose,
    store4); the operand-loading gate epilogues are covered at network level."""
    cin, cout, kh, kw, H, W, nimg = case
    ph, pw = kh // 2, kw // 2
    r = np.random.RandomState(hash(case) & 0xFFFF)
    x = torch.from_numpy(r.normal(0, 1, (nimg, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((r.uniform(-1, 1, (cout, cin, kh, kw)) * np.sqrt(3.0 / (cin * kh * kw))).astype(np.float32))
    b = torch.from_numpy(r.uniform(-0.5, 0.5, (cout,)).astype(np.float32))
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=1, padding=(ph, pw))
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    outs = []
    for form_bit in (4, 2):   # run tiles, rectangular tiles
        out = torch.full((nimg, H, W, cout), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().atdn_conv2d_nhwc_sf_epi(_vp(xd), nimg, H, W, cin, _vp(w), _vp(b), cout, kh, kw, 1, ph, pw,
                                                      sf_store | form_bit, _vp(out), _stream()))
        torch.cuda.synchronize()
        outs.append(out.cpu().permute(0, 3, 1, 2))
    run, rect = outs
    assert torch.isfinite(run).all() and torch.isfinite(rect).all()
    err = _maxerr(run, ref)
    print("case %s sf_store %d: max |run - rect| %.3g, max error against fp64 %.3g" % (case, sf_store, _maxerr(run, rect), err))
    assert torch.equal(run, rect)
    assert err < 2e-5, err


def test_run_tile_clip_matches_single_pairs():
    """344 x 344 frames are 43 x 43 at 1/8 resolution, the smallest geometry at which both passes are served by the run tiles. A
    9-pair clip is 162 rectangular tiles: the dispatcher gives the 256-channel convolutions (the z|r gates and their context convolution) 128-wide
    blocks, hence run tiles, while single-pair calls take the small rectangular tiles. The 128-channel ones (the q gates and their
    context convolution) are narrowed to 8 x 16 x 64 rectangles at this grid size: SfGruQ on run tiles is covered by the KITTI-size
    tests (test_gpu_flow_geometry.py, test_large_batch_tile_path_matches_single_pairs). The K order is the same for
    every tile shape, so each pair comes out of the clip exactly as out of a call of its own. The commit before the run tiles
    satisfies this test as it stands (max |clip - single| = 0 for the three pairs, same GPU job as this library's run), so the
    bound is bit equality."""
    gsd = syn.to_torch(syn.make_gma_state(seed=1))
    net = RAFTGMA(max_batch=9)
    net.load_state_dict(gsd)
    net = net.to(DEV)
    fr = torch.from_numpy(syn.make_frames(10, 344, 344, seed=77)).to(DEV)
    _, up9 = net.forward_sequence(fr, iters=2)
    assert tuple(up9.shape) == (9, 2, 344, 344) and torch.isfinite(up9).all()
    for b in (0, 4, 8):
        _, up1 = net(fr[b:b + 1], fr[b + 1:b + 2], iters=2, test_mode=True)
        print("pair %d: max |clip - single| %.3g" % (b, _maxerr(up9[b:b + 1], up1)))
        assert torch.equal(up9[b:b + 1], up1), b
