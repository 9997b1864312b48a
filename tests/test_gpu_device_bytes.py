"""Device memory ownership through the C ABI (csrc/device_buf.h, atdn_device_bytes_live): every handle gives back exactly the
bytes it took — workspace, weight arena, on-demand scratch — and the unit entries that allocate scratch per call hold nothing
once they return. Each case runs twice in one process: the second cycle must reach the same peak as the first. Shapes are the
smallest that reach every buffer of a handle."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from atdn_vslam_amd import _lib
from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.weights_spec import clvo_state_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KITTI = (376, 1232)   # the pose head flattens a 16x4x13 map: only KITTI-like sizes fit


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _live():
    return int(_lib.lib().atdn_device_bytes_live())


def _twice(cycle):
    """cycle() -> (bytes before create, bytes after finalize, peak, extra); asserts what every handle must satisfy, on two cycles."""
    gc.collect()   # (handles of modules that earlier tests left to the collector must not go away inside a cycle)
    first = None
    for _ in range(2):
        before, finalized, peak, extra = cycle()
        torch.cuda.synchronize()
        assert finalized > before and peak >= finalized
        assert _live() == before, "destroy left %d bytes behind" % (_live() - before)
        if first is None:
            first = (peak - before, extra)
        else:
            assert peak - before == first[0], "second cycle peaks at %d bytes, the first at %d" % (peak - before, first[0])
    return first[1]


# ----------------------------------------------------------------------------- flow network
@pytest.mark.parametrize("precision,low_latency", [(0, False), (1, False), (2, False), (1, True)])
def test_flow_handle_returns_every_byte(precision, low_latency):
    """128 x 128 (the smallest frame with a four-level pyramid), max_batch 2, two iterations: one forward at B = 2, debug reads
    whose scratch grows (split-f16 handles decode into it; the exact-fp32 handle copies straight out), and on the exact-fp32
    handle one probed forward, which allocates the slot table."""
    L = _lib.lib()
    H = W = 128
    state = syn.make_gma_state(seed=1)
    fr = torch.from_numpy(syn.make_frames(3, H, W, seed=5)).to(DEV)
    im1, im2 = fr[0:2].contiguous(), fr[1:3].contiguous()
    low = torch.empty((2, 2, H // 8, W // 8), device=DEV)
    up = torch.empty((2, 2, H, W), device=DEV)
    N = (H // 8) * (W // 8)

    def cycle():
        before = _live()
        h = C.c_void_p()
        _lib.check(L.atdn_gma_create(C.byref(h), H, W, 2, precision))
        if low_latency:
            _lib.check(L.atdn_gma_set_low_latency(h, 1))
        _lib.load_state(L.atdn_gma_load, h, state)
        _lib.check(L.atdn_gma_finalize(h))
        finalized = _live()
        assert finalized - before >= L.atdn_gma_workspace_bytes(h) > 0
        _lib.check(L.atdn_gma_forward(h, _vp(im1), _vp(im2), 2, 2, None, _vp(low), _vp(up), _stream()))
        host = torch.empty(2 * N * 352, dtype=torch.float32)   # corrfeat, the widest of the three: [2 N][352]
        for name in (b"pyr0", b"corrfeat", b"attn"):
            assert L.atdn_gma_debug_read(h, name, _vp(host), host.numel(), _stream()) > 0
        if precision >= 1:
            assert _live() > finalized   # the decode scratch exists now
        if precision == 0:
            _lib.check(L.atdn_gma_set_range_probe(h, 1))
            at = _live()
            _lib.check(L.atdn_gma_forward(h, _vp(im1), _vp(im2), 2, 2, None, _vp(low), _vp(up), _stream()))
            assert L.atdn_gma_range_rows(h) > 0 and _live() > at   # the slot table
        peak = _live()
        torch.cuda.synchronize()
        flow = up.clone()
        L.atdn_gma_destroy(h)
        return before, finalized, peak, flow

    flow = _twice(cycle)
    assert bool(torch.isfinite(flow).all()) and float(flow.abs().max()) > 0


# ----------------------------------------------------------------------------- pose head
def test_pose_head_returns_every_byte_and_growth_drops_its_graphs():
    """T = 4 twice (the second sight captures a graph), T = 6 (the scan scratch grows: the captured graphs hold the old
    addresses and are dropped), T = 4 again, T = 16 (the persistent scan). Every T = 4 call starts from the same state and
    features: the three results are bit-identical."""
    L = _lib.lib()
    state = syn.make_clvo_state(seed=1)
    r = np.random.RandomState(7)
    feat = torch.from_numpy(r.normal(0, 0.15, (16, 1, 512)).astype(np.float32)).to(DEV)
    st0 = torch.from_numpy(r.normal(0, 0.2, (4, 1, 512)).astype(np.float32)).to(DEV)

    def cycle():
        before = _live()
        h = C.c_void_p()
        _lib.check(L.atdn_clvo_create(C.byref(h), KITTI[0], KITTI[1], 1))
        _lib.load_state(L.atdn_clvo_load, h, state)
        _lib.check(L.atdn_clvo_finalize(h))
        finalized = _live()

        def step(T):
            f, st = feat[:T].contiguous(), st0.clone()
            rot, tr = torch.empty((T, 1, 3), device=DEV), torch.empty((T, 1, 3), device=DEV)
            _lib.check(L.atdn_clvo_step(h, _vp(f), T, 1, _vp(st), _vp(rot), _vp(tr), _stream()))
            torch.cuda.synchronize()
            return rot, tr, st

        a, b = step(4), step(4)
        small = _live()
        step(6)
        assert _live() > small > finalized   # the scan scratch grew
        c = step(4)
        long_ = step(16)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z)
        assert all(bool(torch.isfinite(t).all()) for t in a + long_) and float(a[0].std()) > 0
        peak = _live()
        L.atdn_clvo_destroy(h)
        return before, finalized, peak, None

    _twice(cycle)


def test_trainer_returns_every_byte():
    L = _lib.lib()
    B, T = 2, 2
    sd = syn.make_clvo_state(seed=1)
    state = {k: sd[k] for k in clvo_state_spec()}
    flows = torch.from_numpy(syn.make_flow(B * T, KITTI[0], KITTI[1], seed=3)).to(DEV).view(B, T, 2, *KITTI).contiguous()
    r = np.random.RandomState(2)
    true_rot = torch.from_numpy(r.normal(0, 0.01, (B, T, 3)).astype(np.float32)).to(DEV)
    true_tr = torch.from_numpy(r.normal(0, 0.5, (B, T, 3)).astype(np.float32)).to(DEV)

    def cycle():
        before = _live()
        h = C.c_void_p()
        _lib.check(L.atdn_clvo_trainer_create(C.byref(h), KITTI[0], KITTI[1], B, T))
        _lib.load_state(L.atdn_clvo_trainer_load, h, state)
        _lib.check(L.atdn_clvo_trainer_finalize(h))
        finalized = _live()
        loss = C.c_float()
        _lib.check(L.atdn_clvo_trainer_forward_backward(h, _vp(flows), _vp(true_rot), _vp(true_tr), None, None, C.byref(loss),
                                                        _stream()))
        _lib.check(L.atdn_clvo_trainer_adamw_step(h, 1e-3, 1e-3, 1e-8, 1, _stream()))
        torch.cuda.synchronize()
        assert np.isfinite(loss.value) and loss.value > 0
        peak = _live()
        L.atdn_clvo_trainer_destroy(h)
        return before, finalized, peak, None

    _twice(cycle)


def test_mapping_encoder_returns_every_byte():
    L = _lib.lib()
    H = W = 65
    state = syn.make_vae_state(seed=1)
    img = torch.from_numpy(syn.make_frames(1, H, W, seed=4)).to(DEV)

    def cycle():
        before = _live()
        h = C.c_void_p()
        _lib.check(L.atdn_vae_create(C.byref(h), H, W, 1))
        _lib.load_state(L.atdn_vae_load, h, state)
        _lib.check(L.atdn_vae_finalize(h))
        finalized = _live()
        oh, ow = C.c_int(), C.c_int()
        _lib.check(L.atdn_vae_embedding_shape(h, C.byref(oh), C.byref(ow)))
        mu = torch.full((1, oh.value * ow.value, 128), float("nan"), device=DEV)
        _lib.check(L.atdn_vae_encode(h, _vp(img), 1, _vp(mu), _stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(mu).all())
        peak = _live()
        L.atdn_vae_destroy(h)
        return before, finalized, peak, None

    _twice(cycle)


def test_ingest_returns_every_byte():
    """8 x 8 -> 8 x 8, two frames per call, two calls: both staging slots carry a copy."""
    L = _lib.lib()
    r = np.random.RandomState(3)
    frames = [torch.from_numpy(r.randint(0, 256, (2, 3, 8, 8)).astype(np.uint8)) for _ in range(2)]

    def cycle():
        before = _live()
        h = C.c_void_p()
        _lib.check(L.atdn_ingest_create(C.byref(h), 8, 8, 8, 8, 2, 1))
        finalized = _live()
        assert finalized - before == 2 * 2 * 3 * 8 * 8   # two staging slots of max_frames uint8 frames
        outs = [torch.full((2, 3, 8, 8), float("nan"), device=DEV) for _ in range(2)]
        for f, o in zip(frames, outs):
            _lib.check(L.atdn_ingest_frames_u8(h, _vp(f), 2, _vp(o), _stream()))
        torch.cuda.synchronize()
        for f, o in zip(frames, outs):
            assert torch.equal(o.cpu(), f.float())   # equal sizes: the frames come back unchanged
        peak = _live()
        L.atdn_ingest_destroy(h)
        return before, finalized, peak, None

    gc.collect()
    for _ in range(2):
        before, finalized, peak, _ = cycle()
        assert peak == finalized and _live() == before


# ----------------------------------------------------------------------------- unit entries that allocate scratch per call
def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _corr_lookup_bricks():
    B, H8, W8 = 1, 16, 16
    N = H8 * W8
    r = np.random.RandomState(1)
    f1 = torch.from_numpy(r.normal(0, 1, (B, N, 256)).astype(np.float32)).to(DEV)
    f2 = torch.from_numpy(r.normal(0, 1, (B, N, 256)).astype(np.float32)).to(DEV)
    ys, xs = np.meshgrid(np.arange(H8), np.arange(W8), indexing="ij")
    coords = np.stack([xs, ys], -1).reshape(N, 2) + r.uniform(-3, 3, (N, 2))
    coords = torch.from_numpy(coords.astype(np.float32)).to(DEV)
    pyr = [torch.full((B * N, (H8 >> l) * (W8 >> l)), float("nan"), device=DEV) for l in range(4)]
    samples = torch.full((B * N, 324), float("nan"), device=DEV)
    cor1 = torch.full((B * N, 256), float("nan"), device=DEV)
    w = torch.from_numpy((r.uniform(-1, 1, (256, 324)) * np.sqrt(3.0 / 324)).astype(np.float32))
    b = torch.from_numpy(r.uniform(-0.5, 0.5, (256,)).astype(np.float32))
    _lib.check(_lib.lib().atdn_corr_lookup_bricks(_vp(f1), _vp(f2), B, H8, W8, 256, _vp(coords), *[_vp(p) for p in pyr],
                                                  _vp(samples), _vp(w), _vp(b), _vp(cor1), _stream()))
    return pyr + [samples, cor1]


def _conv2d_nhwc():
    r = np.random.RandomState(2)
    x = _nhwc(torch.from_numpy(r.uniform(-1, 1, (1, 16, 47, 61)).astype(np.float32))).to(DEV)
    w = torch.from_numpy((r.uniform(-1, 1, (16, 16, 3, 3)) / 12).astype(np.float32))
    b = torch.from_numpy(r.uniform(-0.5, 0.5, (16,)).astype(np.float32))
    out = torch.full((1, 47, 61, 16), float("nan"), device=DEV)
    _lib.check(_lib.lib().atdn_conv2d_nhwc(_vp(x), 1, 47, 61, 16, _vp(w), _vp(b), 16, 3, 3, 1, 1, 1, 0, _vp(out), _stream()))
    return [out]


def _conv2d_sf_epi(sf_store):
    r = np.random.RandomState(3)
    x = _nhwc(torch.from_numpy(r.normal(0, 1, (1, 64, 23, 37)).astype(np.float32))).to(DEV)
    w = torch.from_numpy((r.uniform(-1, 1, (64, 64, 3, 3)) * np.sqrt(3.0 / 576)).astype(np.float32))
    b = torch.from_numpy(r.uniform(-0.5, 0.5, (64,)).astype(np.float32))
    out = torch.full((1, 23, 37, 64), float("nan"), device=DEV)
    _lib.check(_lib.lib().atdn_conv2d_nhwc_sf_epi(_vp(x), 1, 23, 37, 64, _vp(w), _vp(b), 64, 3, 3, 1, 1, 1, sf_store, _vp(out),
                                                  _stream()))
    return [out]


def _range_probe():
    x = torch.from_numpy(np.random.RandomState(4).normal(0, 3, (7, 5)).astype(np.float32)).to(DEV)
    mx, over, nonf = C.c_float(), C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().atdn_range_probe(_vp(x), 7, 5, 5, C.byref(mx), C.byref(over), C.byref(nonf), _stream()))
    assert mx.value == float(x.abs().max()) and over.value == 0 and nonf.value == 0
    return []


def _composite_loss():
    r = np.random.RandomState(5)
    t = [torch.from_numpy(r.normal(0, 0.1, (2, 4, 3)).astype(np.float32)).to(DEV) for _ in range(4)]
    d_rot, d_tr = torch.full((2, 4, 3), float("nan"), device=DEV), torch.full((2, 4, 3), float("nan"), device=DEV)
    loss3 = (C.c_float * 3)()
    _lib.check(_lib.lib().atdn_clvo_loss(*[_vp(x) for x in t], 2, 4, 0.5, 3, 1, loss3, _vp(d_rot), _vp(d_tr), _stream()))
    assert all(np.isfinite(v) for v in loss3) and loss3[0] > 0
    return [d_rot, d_tr]


@pytest.mark.parametrize("entry", [_corr_lookup_bricks, _conv2d_nhwc, lambda: _conv2d_sf_epi(0), lambda: _conv2d_sf_epi(1),
                                   _range_probe, _composite_loss],
                         ids=["corr_lookup_bricks", "conv2d_nhwc", "conv2d_nhwc_sf_epi", "conv2d_nhwc_sf_epi_sf_store",
                              "range_probe", "clvo_loss"])
def test_unit_entries_hold_nothing_after_the_call(entry):
    gc.collect()
    for _ in range(2):
        before = _live()
        outs = entry()
        assert _live() == before
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(o).all()) for o in outs)
