"""Forward-backward flow consistency on the GPU: the kernel (atdn_flow_consistency, csrc/flow_consistency.hip) against the NumPy
float64 restatement of the rule (tests/flow_consistency_ref.py) and against the library's host form — every mask byte and every
count, exactly (the random cases keep every pixel at least 1e-9 from the threshold, asserted on the helper alone) —,
RAFTGMA.forward_backward against the concatenated `forward` call it is defined as, and relocalisation with `verify=True`
against the same steps done by hand."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms
from atdn_vslam_amd.modules import RAFTGMA

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flow_consistency_ref import MIN_MARGIN, RANDOM_CASES, flow_consistency_ref, reference_batch, smooth_pair  # noqa: E402
from slam_cases import _Args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(fw, bw, alpha1=0.01, alpha2=0.5):
    """The kernel on numpy arrays [B,2,H,W]: (mask, count) as numpy arrays."""
    m, c = transforms._flow_consistency_counts(torch.from_numpy(np.ascontiguousarray(fw)).to(DEV),
                                               torch.from_numpy(np.ascontiguousarray(bw)).to(DEV), alpha1, alpha2)
    torch.cuda.synchronize()
    return m.cpu().numpy(), c.cpu().numpy()


def _const(H, W, vx, vy):
    f = np.empty((1, 2, H, W), dtype=np.float32)
    f[:, 0], f[:, 1] = vx, vy
    return f


def _host(fw, bw, alpha1=0.01, alpha2=0.5):
    m, c = transforms._flow_consistency_counts(torch.from_numpy(np.ascontiguousarray(fw)), torch.from_numpy(np.ascontiguousarray(bw)),
                                               alpha1, alpha2)
    return m.numpy(), c.numpy()


def _check(fw, bw, alpha1=0.01, alpha2=0.5, tag=""):
    """Kernel == helper == host twin; returns the kernel's (mask, count)."""
    ref_mask, ref_count, _, _ = reference_batch(fw, bw, alpha1, alpha2)
    mask, count = _gpu(fw, bw, alpha1, alpha2)
    hmask, hcount = _host(fw, bw, alpha1, alpha2)
    assert mask.dtype == np.uint8 and count.dtype == np.int32
    assert np.array_equal(mask, ref_mask) and np.array_equal(count, ref_count), tag
    assert np.array_equal(mask, hmask) and np.array_equal(count, hcount), tag
    return mask, count


@pytest.fixture(scope="module")
def full_size():
    """The 376 x 1232, B = 2 pair and its reference, computed once."""
    fw, bw = smooth_pair(376, 1232, 0, 2, 2.0)
    return fw, bw, reference_batch(fw, bw)


@pytest.mark.parametrize("name, H, W, B, seed, amplitude", RANDOM_CASES, ids=[c[0] for c in RANDOM_CASES])
def test_kernel_equals_the_helper_and_the_host_twin(name, H, W, B, seed, amplitude):
    """5 x 7 (one workgroup, two quads); 9 x 33, B = 3 (H * W = 297 is odd: the mask planes of b = 1, 2 start at addresses 1 and
    2 mod 4, so their quads are cut off the index grid, with ragged heads and tails and scalar loads); 47 x 154 (8 workgroups)."""
    fw, bw = smooth_pair(H, W, seed, B, amplitude)
    _, count, margin, inside = reference_batch(fw, bw)
    assert margin >= MIN_MARGIN and all(0 < c < H * W for c in count) and inside < 1.0
    _check(fw, bw, tag=name)
    for b in range(B):                                            # every plane alone, through the 3-d form
        m3, s3 = transforms.flow_consistency(torch.from_numpy(fw[b]).to(DEV), torch.from_numpy(bw[b]).to(DEV))
        assert m3.is_cuda and s3.is_cuda and tuple(m3.shape) == (1, H, W) and s3.dim() == 0 and s3.dtype == torch.float32
        assert float(s3) == float(np.float32(np.float64(count[b]) / (H * W)))


def test_kernel_at_full_size_streams_and_graph(full_size):
    """376 x 1232, B = 2: 453 workgroups per image and a ragged last one. The same bits on a second call, on a side stream, and
    from a captured graph (one linear chain: the memset of the count, then the kernel) replayed twice."""
    fw, bw, (ref_mask, ref_count, margin, inside) = full_size
    assert margin >= MIN_MARGIN and all(0 < c < 376 * 1232 for c in ref_count) and inside < 1.0
    dfw, dbw = torch.from_numpy(fw).to(DEV), torch.from_numpy(bw).to(DEV)
    m1, c1 = transforms._flow_consistency_counts(dfw, dbw, 0.01, 0.5)
    m2, s2 = transforms.flow_consistency(dfw, dbw)
    torch.cuda.synchronize()
    assert np.array_equal(m1.cpu().numpy(), ref_mask) and np.array_equal(c1.cpu().numpy(), ref_count)
    assert torch.equal(m1, m2) and tuple(s2.shape) == (2,) and s2.is_cuda
    assert np.array_equal(s2.cpu().numpy(), (ref_count.astype(np.float64) / (376 * 1232)).astype(np.float32))
    hm, hc = _host(fw, bw)
    assert np.array_equal(hm, ref_mask) and np.array_equal(hc, ref_count)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        m3, c3 = transforms._flow_consistency_counts(dfw, dbw, 0.01, 0.5)
    side.synchronize()
    assert torch.equal(m3, m1) and torch.equal(c3, c1)
    # captured: static output buffers, pre-filled before every replay so that unwritten bytes and an un-reset count would show
    import ctypes as C
    from atdn_vslam_amd import _lib
    mask = torch.empty((2, 1, 376, 1232), dtype=torch.uint8, device=DEV)
    count = torch.empty((2,), dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=capture):
        _lib.check(_lib.lib().atdn_flow_consistency(C.c_void_p(dfw.data_ptr()), C.c_void_p(dbw.data_ptr()), 2, 376, 1232, 0.01, 0.5,
                                                    C.c_void_p(mask.data_ptr()), C.c_void_p(count.data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for fill in (0xFF, 0x5A):
        mask.fill_(fill)
        count.fill_(123456)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask, m1) and torch.equal(count, c1), fill


def test_kernel_outputs_are_fully_written():
    """Pre-filled output buffers with guard bytes around them: every byte of the mask and every count is written, nothing else
    is — at an odd H * W with three planes, so that heads and tails of every alignment occur."""
    import ctypes as C
    from atdn_vslam_amd import _lib
    fw, bw = smooth_pair(9, 33, 0, 3, 2.0)
    ref_mask, ref_count, _, _ = reference_batch(fw, bw)
    dfw, dbw = torch.from_numpy(fw).to(DEV), torch.from_numpy(bw).to(DEV)
    n = 3 * 297
    for shift in (0, 1, 2, 3):                                    # the mask itself at every address mod 4
        buf = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        cnt = torch.full((5,), -7, dtype=torch.int32, device=DEV)
        mask = buf[16 + shift:16 + shift + n]
        _lib.check(_lib.lib().atdn_flow_consistency(C.c_void_p(dfw.data_ptr()), C.c_void_p(dbw.data_ptr()), 3, 9, 33, 0.01, 0.5,
                                                    C.c_void_p(mask.data_ptr()), C.c_void_p(cnt[1:].data_ptr()),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert (out[:16 + shift] == 0xFF).all() and (out[16 + shift + n:] == 0xFF).all(), shift
        assert np.array_equal(out[16 + shift:16 + shift + n].reshape(3, 1, 9, 33), ref_mask), shift
        assert cnt.cpu().tolist() == [-7] + ref_count.tolist() + [-7], shift
    # flow_fw at an address that is 4 mod 16 (a view one float into a buffer): scalar loads, the same result
    pad = torch.zeros(fw.size + 1, dtype=torch.float32, device=DEV)
    pad[1:] = dfw.reshape(-1)
    m = torch.full((3, 1, 9, 33), 0xFF, dtype=torch.uint8, device=DEV)
    c = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().atdn_flow_consistency(C.c_void_p(pad[1:].data_ptr()), C.c_void_p(dbw.data_ptr()), 3, 9, 33, 0.01, 0.5,
                                                C.c_void_p(m.data_ptr()), C.c_void_p(c.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), ref_mask) and c.cpu().tolist() == ref_count.tolist()


def test_kernel_analytic_cases():
    # constant flow undone by bw = -fw: ones exactly where the target stays inside
    fw = _const(9, 33, 3.0, -2.0)
    mask, count = _check(fw, -fw)
    want = np.zeros((9, 33), dtype=np.uint8)
    want[2:, :30] = 1
    assert int(count[0]) == 210 and np.array_equal(mask[0, 0], want)
    # zero flows: all ones
    z = np.zeros((2, 2, 9, 33), dtype=np.float32)
    mask, count = _check(z, z)
    assert mask.min() == 1 and count.tolist() == [297, 297]
    # x1 == W - 1 and y1 == H - 1 exactly are inside
    for v, pix in (((32.0, 8.0), (0, 0)), ((-32.0, -8.0), (8, 32))):
        fw = _const(9, 33, *v)
        mask, count = _check(fw, -fw)
        assert int(count[0]) == 1 and mask[0, 0][pix] == 1
    fw = _const(9, 33, 1.0, 1.0)
    mask, count = _check(fw, -fw)
    assert int(count[0]) == 32 * 8 and mask[0, 0, 7, 31] == 1 and mask[0, 0, 8, 31] == 0 and mask[0, 0, 7, 32] == 0
    # contradicting flows at magnitude 5: all zeros
    fw = _const(9, 33, 3.0, 4.0)
    mask, count = _check(fw, fw)
    assert mask.max() == 0 and int(count[0]) == 0
    # alpha1 = alpha2 = 0: only diff == 0 passes
    fw = _const(9, 33, 3.0, -2.0)
    mask, count = _check(fw, -fw, 0.0, 0.0)
    assert int(count[0]) == 210
    fw[0, 0, 4, 10] = 2.5
    mask, count = _check(fw, -_const(9, 33, 3.0, -2.0), 0.0, 0.0)
    assert int(count[0]) == 209 and mask[0, 0, 4, 10] == 0
    f2, b2 = smooth_pair(9, 33, 0, 1, 2.0)
    mask, count = _check(f2, b2, 0.0, 0.0)
    assert int(count[0]) == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_kernel_non_finite_values(bad):
    """A NaN or an infinity in fw at a pixel, or in one of its four taps — zero-weight ones included — gives 0 at that pixel and
    changes no pixel that does not read it; everything equals the helper and the host twin."""
    pix, taps = (3, 10), [(4, 12), (4, 13), (5, 12), (5, 13)]
    fw = _const(9, 33, 2.5, 1.5)
    bw = -fw
    base, base_count = _check(fw, bw)
    assert base[0, 0][pix] == 1
    for c in (0, 1):
        f = fw.copy()
        f[0, c][pix] = bad
        mask, count = _check(f, bw)
        assert np.argwhere(mask[0, 0] != base[0, 0]).tolist() == [list(pix)] and int(count[0]) == int(base_count[0]) - 1
    for tap in taps:
        for c in (0, 1):
            b = bw.copy()
            b[0, c][tap] = bad
            mask, _ = _check(fw, b)
            readers = {(tap[0] - 1 - dy, tap[1] - 2 - dx) for dy in (0, 1) for dx in (0, 1)}
            assert mask[0, 0][pix] == 0
            assert {tuple(p) for p in np.argwhere(mask[0, 0] != base[0, 0]).tolist()} == readers
    fw = _const(9, 33, 2.0, 1.0)                                   # integer flow: three taps of weight zero
    bw = -fw
    base, _ = _check(fw, bw)
    for tap in taps[1:]:
        b = bw.copy()
        b[0, 0][tap] = bad
        mask, _ = _check(fw, b)
        assert mask[0, 0][pix] == 0 and base[0, 0][pix] == 1


def test_kernel_argument_errors():
    z = torch.zeros(1, 2, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="alpha"):
        transforms.flow_consistency(z, z, alpha1=-0.1)
    with pytest.raises(RuntimeError, match="alpha"):
        transforms.flow_consistency(z, z, alpha2=float("nan"))
    with pytest.raises(RuntimeError):
        transforms.flow_consistency(z, torch.zeros(1, 2, 4, 5, device=DEV))
    with pytest.raises(RuntimeError):
        transforms.flow_consistency(z, z.cpu())
    import ctypes as C
    from atdn_vslam_amd import _lib
    L = _lib.lib()
    m = torch.zeros(16, dtype=torch.uint8, device=DEV)
    c = torch.zeros(1, dtype=torch.int32, device=DEV)
    zp, mp, cp = C.c_void_p(z.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(c.data_ptr())
    assert L.atdn_flow_consistency(None, zp, 1, 4, 4, 0.01, 0.5, mp, cp, None) != 0
    assert L.atdn_flow_consistency(zp, zp, 1, 4, 4, 0.01, 0.5, mp, None, None) != 0
    assert L.atdn_flow_consistency(zp, zp, 1, 4, 4, 0.01, 0.5, zp, cp, None) != 0
    assert b"overlap" in L.atdn_last_error()
    assert L.atdn_flow_consistency(zp, zp, 1, 4, 0, 0.01, 0.5, mp, cp, None) != 0


# ----------------------------------------------------------------------------- the flow network
SMALL = (128, 128)      # the smallest geometry of tests/test_gpu_flow_geometry.py


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


def _net(gsd, max_batch, low_latency=False):
    n = RAFTGMA(max_batch=max_batch, low_latency=low_latency)
    n.load_state_dict(gsd)
    return n.to(DEV).eval()


def test_forward_backward_is_the_concatenated_forward(gsd):
    """128 x 128, synthetic weights, 4 iterations, B = 2: one call of four pairs on a max_batch = 4 module, two calls of two
    pairs on a max_batch = 2 module; with and without flow_init (forward half only)."""
    fr = torch.from_numpy(syn.make_frames(4, SMALL[0], SMALL[1], seed=3)).to(DEV)
    a, b = fr[:2].contiguous(), fr[2:].contiguous()
    init = torch.from_numpy(np.random.RandomState(4).randn(2, 2, 16, 16).astype(np.float32)).to(DEV)
    for mb in (4, 2):
        net, ref = _net(gsd, mb), _net(gsd, mb)
        for fi in (None, init):
            fw, bw = net.forward_backward(a, b, iters=4, flow_init=fi)
            assert tuple(fw.shape) == (2, 2) + SMALL and tuple(bw.shape) == (2, 2) + SMALL
            if mb == 4:
                fi2 = None if fi is None else torch.cat([fi, torch.zeros_like(fi)])
                up = ref(torch.cat([a, b]), torch.cat([b, a]), iters=4, flow_init=fi2, test_mode=True)[1]
                want_fw, want_bw = up[:2], up[2:]
            else:
                want_fw = ref(a, b, iters=4, flow_init=fi, test_mode=True)[1]
                want_bw = ref(b, a, iters=4, test_mode=True)[1]
            assert torch.equal(fw, want_fw) and torch.equal(bw, want_bw), (mb, fi is None)
        # the two halves are the flows of the two directions: they differ, and flow_init reaches the forward half only
        fw0, bw0 = net.forward_backward(a, b, iters=4)
        fw1, bw1 = net.forward_backward(a, b, iters=4, flow_init=init)
        assert not torch.equal(fw0, bw0) and not torch.equal(fw0, fw1)
        if mb == 2:
            assert torch.equal(bw0, bw1)
        assert bool(torch.isfinite(fw0).all()) and bool(torch.isfinite(bw0).all())
        with pytest.raises(RuntimeError):
            net.forward_backward(a, b[:1])


@pytest.mark.parametrize("low_latency", [False, True])
def test_forward_backward_leaves_a_consecutive_chain_alone(gsd, low_latency):
    """A warm-started forward_consecutive chain with forward_backward calls between its calls returns the bits of the same
    chain without them (the kept flow survives; the frames are encoded again, which gives the continued form's bits)."""
    fr = [f.clone() for f in torch.from_numpy(syn.make_frames(4, SMALL[0], SMALL[1], seed=5)).to(DEV)]
    plain, mixed = _net(gsd, 2, low_latency), _net(gsd, 2, low_latency)
    for warm in (True, False):
        plain.break_chain(), mixed.break_chain()
        for k in range(1, 4):
            want = plain.forward_consecutive(fr[k - 1], fr[k], iters=4, warm_start=warm)
            got = mixed.forward_consecutive(fr[k - 1], fr[k], iters=4, warm_start=warm)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (warm, k)
            tail, low = mixed._stream_tail, mixed._warm_low
            mixed.forward_backward(fr[0][None], fr[3][None], iters=2)           # 2B <= max_batch: one call
            mixed.forward_backward(torch.stack(fr[:2]), torch.stack(fr[2:]), iters=2)   # two calls
            assert mixed._stream_tail is not None and mixed._stream_tail[0] is tail[0] and mixed._warm_low is low
    # and the warm chain is not the cold one (the test above would pass trivially otherwise)
    plain.break_chain()
    cold = [plain.forward_consecutive(fr[k - 1], fr[k], iters=4)[1] for k in (1, 2)]
    plain.break_chain()
    warm = [plain.forward_consecutive(fr[k - 1], fr[k], iters=4, warm_start=True)[1] for k in (1, 2)]
    assert torch.equal(cold[0], warm[0]) and not torch.equal(cold[1], warm[1])


# ----------------------------------------------------------------------------- relocalisation
def _reloc_directory(golden_dir, vsd, root):
    """The three-keyframe directory of tests/test_gpu_keyframe_map.py (tests/golden/make_golden_slam.py), rebuilt from its seeds."""
    g = np.load(os.path.join(golden_dir, "reloc.npz"))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1232, seed=int(g["seed_frames"])))
    kf = os.path.join(str(root), "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    for i in range(3):
        torch.save(frames[i].byte(), os.path.join(kf, "rgb", "%06d.pth" % i))
    torch.save(torch.from_numpy(g["keyframe_poses"]), os.path.join(kf, "poses.pth"))
    torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
    return g, kf, {"near1": frames[1].byte().float(), "new": frames[4].byte().float()}


def test_verified_relocalization(golden_dir, gsd, tmp_path, monkeypatch):
    """Two queries, top_k = 3: 6 pairs, 12 flows, one chunk of the max_batch = 16 handle. With the synthetic weights the flows
    are arbitrary: on an MI355X all six counts came out 0 (even for the query that IS keyframe 1), so `chosen` is decided by the
    tie rule there; the choice among unequal counts is checked with substituted counts further down."""
    from atdn_vslam_amd.slam import NeuralSLAM
    hsd = syn.to_torch(syn.make_clvo_state(seed=1))
    vsd = syn.to_torch(syn.make_vae_state(seed=2))
    g, kf, queries = _reloc_directory(golden_dir, vsd, tmp_path)
    slam = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True)
    batch = [queries["near1"], queries["new"]]
    slam(queries["near1"])                                        # the head carries a non-zero state from here on
    state = slam._odometry_net._state.clone()
    assert float(state.abs().max()) > 0

    # verify=False: bit-identical to the call without the argument
    plain = slam.relocalize_batch(batch, top_k=3)
    off = slam.relocalize_batch(batch, top_k=3, verify=False)
    assert len(plain) == 4 and len(off) == 4
    for x, y in zip(plain, off):
        assert x.dtype == y.dtype and torch.equal(x, y)

    # verify=True
    out = slam.relocalize_batch(batch, top_k=3, verify=True)
    assert len(out) == 6
    dist, idx, initial, refined, scores, chosen = out
    assert torch.equal(slam._odometry_net._state, state)          # the head's carried state: bit-identical
    assert torch.equal(dist, plain[0]) and torch.equal(idx, plain[1])
    assert tuple(scores.shape) == (2, 3) and scores.dtype == torch.float32 and not scores.is_cuda
    assert tuple(chosen.shape) == (2,) and chosen.dtype == torch.int64
    assert tuple(initial.shape) == (2, 4, 4) and tuple(refined.shape) == (2, 4, 4)
    # by hand: the same pairs through forward_backward in the same chunking (one chunk of 6 pairs), on the same flow handle
    flow_net, head, kmap = slam._flow_for_batches(), slam._odometry_net, slam._map
    assert flow_net.max_batch == 16
    q = torch.stack(batch).to(DEV)
    pairs_k = kmap.images(idx.reshape(-1))
    pairs_q = q.repeat_interleave(3, dim=0)
    fw, bw = flow_net.forward_backward(pairs_k, pairs_q, iters=12)
    mask, score = transforms.flow_consistency(fw, bw)
    assert torch.equal(scores.reshape(-1), score.cpu())           # the same launches: exact
    counts = mask.view(6, -1).sum(dim=1, dtype=torch.int64).cpu().view(2, 3)
    want_chosen = torch.tensor([min(range(3), key=lambda r: (-int(counts[i, r]), r)) for i in range(2)])
    assert torch.equal(chosen, want_chosen)
    print("scores", scores.tolist(), "counts", counts.tolist(), "chosen", chosen.tolist())
    rot, tr, _ = head.scan(head.encode(fw)[None], state=None, hw=(376, 1232))
    rot, tr = rot[0].cpu(), tr[0].cpu()
    for i in range(2):
        p = 3 * i + int(chosen[i])
        assert torch.equal(initial[i], kmap.poses[int(idx[i, int(chosen[i])])])
        want = initial[i] @ transforms.transform(rot[p], tr[p])
        assert torch.equal(refined[i], want), i                   # the same launches: exact
    assert torch.equal(slam._odometry_net._state, state)
    # a second call returns the same bits (the count is an integer sum)
    again = slam.relocalize_batch(batch, top_k=3, verify=True)
    for x, y in zip(out, again):
        assert torch.equal(x, y)

    # the choice itself: with synthetic weights the flows of these images are arbitrary and every count above is 0, so the
    # counts are replaced (the real launches still run) — query 0: ranks 1 and 2 tie above rank 0; query 1: a three-way tie
    real = transforms._flow_consistency_counts
    fake = torch.tensor([5, 9, 9, 7, 7, 7], dtype=torch.int32)

    def patched(fw_, bw_, a1, a2):
        m, c = real(fw_, bw_, a1, a2)
        return m, fake.to(c.device)

    monkeypatch.setattr(transforms, "_flow_consistency_counts", patched)
    picked = slam.relocalize_batch(batch, top_k=3, verify=True)
    monkeypatch.undo()
    assert picked[5].tolist() == [1, 0]
    assert torch.equal(picked[4], (fake.double() / (376 * 1232)).float().view(2, 3))
    for i, r in enumerate((1, 0)):
        assert torch.equal(picked[2][i], kmap.poses[int(idx[i, r])])
        assert torch.equal(picked[3][i], picked[2][i] @ transforms.transform(rot[3 * i + r], tr[3 * i + r]))

    # top_k = 1: the poses of verify=False (flows from a batch of another composition: 1e-4, the bound of the existing batch test
    # between its two paths), and the scores are the confidence the caller lacked
    d1, i1, init1, ref1 = slam.relocalize_batch(batch, top_k=1)
    v = slam.relocalize_batch(batch, top_k=1, verify=True)
    assert torch.equal(v[0], d1) and torch.equal(v[1], i1) and torch.equal(v[2], init1)
    np.testing.assert_allclose(v[3].numpy(), ref1.numpy(), rtol=0, atol=1e-4)
    assert tuple(v[4].shape) == (2, 1) and v[5].tolist() == [0, 0]
    assert torch.equal(slam._odometry_net._state, state)

    # errors
    with pytest.raises(ValueError, match="refine"):
        slam.relocalize_batch(batch, top_k=1, refine=False, verify=True)
    fresh = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization")
    with pytest.raises(RuntimeError, match="resident_map=True"):
        fresh.relocalize_batch(batch, verify=True)
