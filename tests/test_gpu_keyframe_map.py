"""GPU checks of the HBM-resident keyframe map (atdn_vslam_amd/keyframe_map.py, csrc/keyframe_map.hip): the one-launch
search against float64, its top-k order and its invariance to how a launch is cut, the exact image gather, the zero-copy
embedding, and NeuralSLAM with `resident_map=True` against the reference's own numbers (tests/golden/reloc.npz, slam.npz)
and against the default code path.

Tolerance of a distance, from the kernel's summation structure (keyframe_map.hip) and nothing measured: an accumulator takes
at most 64 sequential fused multiply-adds; the partial sums pass through at most 10 levels of a fixed tree (6 shuffle levels
across the lanes of a wave, 2 across the four waves here); the difference a - b is rounded once before it is squared, which
counts once more. With round-to-nearest fp32 (unit roundoff 2^-24) and non-negative terms only (nothing cancels) that is at
most (64 + 10 + 1) * 2^-24 = 4.5e-6 relative on d^2, half of it on d, plus half an ulp of the correctly rounded square
root: 2.3e-6 .. 2.5e-6. REL_TOL = 5e-6 is twice that bound. It holds for D <= 16384 (one partial sum per lane and row).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.keyframe_map import KeyframeMap, gather_images, search_bank
from atdn_vslam_amd.modules import MappingVAE
from atdn_vslam_amd.pipeline import SLAM_SIZE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

REL_TOL = 5e-6
assert 2 * ((64 + 10 + 1) * 2.0 ** -24 / 2 + 2.0 ** -24) <= REL_TOL      # twice the bound derived above

DS = (15360, 3072)
KS = (1, 3, 455, 1000)
QS = (1, 2, 16, 17)
TOPKS = (1, 2, 8, 16)
NQ = max(QS)
LADDER = 33          # the smallest constructed distances, 1 % apart


@functools.lru_cache(maxsize=None)
def _constructed(D, K):
    """Bank [K,D] and queries [17,D] (fp32) whose float64 distances are known by construction, with the float64 oracle.

    Query 0 is q. Constructed row i is q + s_i * u_i with u_i a random unit vector supported on the first half of the
    coordinates and s_i strictly increasing: s_i = 10 * 1.01^i for the LADDER smallest, the rest at least 1 % above those.
    Query j >= 1 is q + t_j * e_j with e_j a unit vector on the OTHER half of the coordinates and t_j <= s_0 / 4, so its
    distance to row i is sqrt(s_i^2 + t_j^2): the same order, and gaps of (just under) 1 %. For K >= 3 the bank also holds a
    row equal to q and one constructed row twice, at two slots. Rows sit in random slots. The gaps are asserted here, on the
    float64 distances of the fp32 values: among the 17 nearest rows of every query two neighbours are either bit-identical
    rows or at least 0.9 % apart (1800 times the tolerance); for query 0 at least 0.99 %."""
    g = torch.Generator().manual_seed(1000 * K + D)
    half = D // 2
    q = torch.randn(D, generator=g, dtype=torch.float64)
    n_rows = K if K < 3 else K - 2                      # distinct constructed rows (one of them is stored twice)
    s = [10.0 * 1.01 ** i for i in range(min(n_rows, LADDER))]
    s += [s[-1] * 1.01 * (1.0 + 0.01 * (i - LADDER)) for i in range(LADDER, n_rows)]
    s = torch.tensor(s, dtype=torch.float64)
    assert bool((s[1:] > s[:-1]).all())
    u = torch.zeros(n_rows, D, dtype=torch.float64)
    u[:, :half] = torch.randn(n_rows, half, generator=g, dtype=torch.float64)
    u /= u.norm(dim=1, keepdim=True)
    rows = [q + s[i] * u[i] for i in range(n_rows)]
    twin = None
    if K >= 3:
        twin = min(5, n_rows - 1)
        rows.append(rows[twin].clone())                 # the same row at a second slot
        rows.append(q.clone())                          # a row equal to query 0
    bank = torch.stack(rows).float()
    perm = torch.randperm(K, generator=g)
    slot_of = torch.empty(K, dtype=torch.long)
    slot_of[perm] = torch.arange(K)
    bank = bank[perm].contiguous()                      # bank[slot] = rows[perm[slot]]
    queries = q.repeat(NQ, 1)
    e = torch.zeros(NQ, D, dtype=torch.float64)
    e[:, half:] = torch.randn(NQ, D - half, generator=g, dtype=torch.float64)
    e /= e.norm(dim=1, keepdim=True)
    t = 2.5 * torch.arange(NQ, dtype=torch.float64) / NQ   # t_0 = 0; all below s_0 / 4
    queries = (queries + t[:, None] * e).float().contiguous()
    assert torch.equal(queries[0], q.float())
    ref = torch.cdist(queries.double(), bank.double(), compute_mode="donot_use_mm_for_euclid_dist")    # [17,K] float64
    order = torch.from_numpy(np.argsort(ref.numpy(), axis=1, kind="stable"))   # equal distances: the lower slot first
    top = torch.gather(ref, 1, order[:, :17])
    for j in range(NQ):
        for a in range(top.shape[1] - 1):
            lo, hi = float(top[j, a]), float(top[j, a + 1])
            same = torch.equal(bank[order[j, a]], bank[order[j, a + 1]])
            assert same or hi >= lo * (1.0099 if j == 0 else 1.009), (D, K, j, a, lo, hi)
    info = {"equal_slot": int(slot_of[K - 1]) if K >= 3 else None,
            "twin_slots": sorted((int(slot_of[twin]), int(slot_of[K - 2]))) if K >= 3 else None}
    return bank, queries, ref, order, info


def _search(bank, queries, top_k=1):
    dist, idx = search_bank(bank.to(DEV), queries.to(DEV), top_k)
    torch.cuda.synchronize()
    return dist.cpu(), idx.cpu().long()


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", DS)
def test_distances_against_float64(D, K, Q):
    bank, queries, ref, order, info = _constructed(D, K)
    dist, idx = _search(bank, queries[:Q])
    assert tuple(dist.shape) == (Q, K) and tuple(idx.shape) == (Q, 1)
    want = ref[:Q]
    rel = ((dist.double() - want).abs() / want.clamp_min(1e-300)).masked_fill(want == 0, 0.0)
    print("D=%d K=%d Q=%d: max relative error of a distance %.3e (tolerance %.1e)" % (D, K, Q, float(rel.max()), REL_TOL))
    assert float(rel.max()) <= REL_TOL
    assert torch.equal(idx[:, 0], torch.argmin(dist, dim=1))
    assert torch.equal(idx[:, 0], order[:Q, 0])
    if K >= 3:
        assert float(dist[0, info["equal_slot"]]) == 0.0 and int(idx[0, 0]) == info["equal_slot"]
        a, b = info["twin_slots"]
        assert torch.equal(dist[:, a], dist[:, b])          # identical rows: bit-equal distances for every query


CASES_TOPK = [(D, K, Q, k) for D in DS for K in KS for Q in QS for k in TOPKS if k <= K]


@pytest.mark.parametrize("D, K, Q, topk", CASES_TOPK)
def test_topk_is_the_float64_order(D, K, Q, topk):
    bank, queries, ref, order, info = _constructed(D, K)
    dist, idx = _search(bank, queries[:Q], topk)
    assert tuple(idx.shape) == (Q, topk)
    assert torch.equal(idx, order[:Q, :topk])
    assert torch.equal(idx[:, 0], torch.argmin(dist, dim=1))
    if K >= 3 and topk >= 8:
        a, b = info["twin_slots"]                            # the tie is inside the first 8: the lower slot comes first
        row = idx[0].tolist()
        assert row.index(b) == row.index(a) + 1


def test_topk_range_is_enforced_on_the_device_path():
    bank, queries, _, _, _ = _constructed(3072, 3)
    for bad in (0, 4, 17):
        with pytest.raises(RuntimeError, match="topk"):
            search_bank(bank.to(DEV), queries[:1].to(DEV), bad)


def test_distance_bits_do_not_depend_on_the_launch():
    """The same row and query give the same bits alone and inside a batch of 16 queries, in a bank of 3 and inside banks of
    1000 and 2500 rows (one, two and four rows per workgroup), and after the row has moved to another slot."""
    for D in DS:
        bank, queries, _, _, _ = _constructed(D, 1000)
        full, _ = _search(bank, queries[:16])
        row, q = 777, 7
        one, _ = _search(bank, queries[q:q + 1])
        assert torch.equal(one[0], full[q])                              # Q = 1 against inside Q = 16
        odd, _ = _search(bank, queries[:NQ])
        assert torch.equal(odd[:16], full) and torch.equal(odd[16], _search(bank, queries[16:17])[0][0])
        small = torch.stack([bank[5], bank[row], bank[900]])
        d3, _ = _search(small, queries[q:q + 1])
        assert float(d3[0, 1]) == float(full[q, row])                    # K = 3 against inside K = 1000
        moved = bank.clone()
        moved[[row, 12]] = moved[[12, row]]
        dm, _ = _search(moved, queries[:16])
        assert torch.equal(dm[:, 12], full[:, row]) and torch.equal(dm[:, row], full[:, 12])
        big = torch.cat([bank, bank.flip(0), bank[:500]])                # K = 2500
        db, _ = _search(big, queries[:16])
        assert torch.equal(db[:, :1000], full) and torch.equal(db[:, 1000:2000], full.flip(1))
        assert torch.equal(db[:, 2000:], full[:, :500])


def test_long_rows_and_partial_vectors():
    """Row lengths that are not a multiple of the workgroup's 1024 floats (a partial last iteration) and one longer than
    16384 floats (two partial sums per lane: one more rounding in the bound)."""
    g = torch.Generator().manual_seed(5)
    for D in (4, 1028, 20004):
        bank = torch.randn(7, D, generator=g)
        queries = torch.randn(3, D, generator=g)
        bank[4] = queries[1]
        dist, idx = _search(bank, queries, 2)
        want = torch.cdist(queries.double(), bank.double(), compute_mode="donot_use_mm_for_euclid_dist")
        rel = ((dist.double() - want).abs() / want.clamp_min(1e-300)).masked_fill(want == 0, 0.0)
        assert float(rel.max()) <= REL_TOL + 2.0 ** -25, D
        assert float(dist[1, 4]) == 0.0 and int(idx[1, 0]) == 4


@pytest.mark.parametrize("hw", [(8, 16), SLAM_SIZE])
def test_gather_is_exact(hw):
    g = torch.Generator().manual_seed(3)
    K = 9
    bank = torch.randint(0, 256, (K, 3) + tuple(hw), generator=g, dtype=torch.uint8)
    m = KeyframeMap(DEV, hw=hw, capacity=2)
    for k in range(K):
        m.append(bank[k] if k % 2 else bank[k].float(), torch.eye(4) * (k + 1))   # uint8 and float inputs, growth 2 -> 16
    assert len(m) == K and m.capacity == 16
    assert torch.equal(m.image_bank[:K].cpu(), bank)
    assert torch.equal(m.poses[:, 0, 0], torch.arange(1, K + 1, dtype=torch.float32))
    for indices in ([0], [8, 8, 0, 3, 3, 7], list(range(K))[::-1], torch.tensor([2, 5, 2])):
        out = m.images(indices)
        ix = torch.as_tensor(indices)
        assert out.dtype == torch.float32 and tuple(out.shape) == (len(ix), 3) + tuple(hw)
        assert torch.equal(out.cpu(), bank[ix].float())
    many = torch.arange(700) % K                                        # more than one table of 512 per call
    if hw == (8, 16):
        assert torch.equal(gather_images(m.image_bank[:K], many).cpu(), bank[many].float())
    for bad in ([K], [-1], [0, 100]):
        with pytest.raises(RuntimeError, match="outside"):
            m.images(bad)


@pytest.fixture(scope="module")
def vsd():
    return syn.to_torch(syn.make_vae_state(seed=2))


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


@pytest.fixture(scope="module")
def hsd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.mark.parametrize("n", [5, 19])
def test_embed_writes_bank_rows_in_place(n, vsd):
    """embed(net, batch=16) lets the encoder write into the bank rows of 16 keyframes at a time; every row must be the
    batch-1 `MappingVAE(image)[0]` of the existing module, permuted to channels-last, bit for bit."""
    frames = torch.from_numpy(syn.make_frames(n, 376, 1232, seed=21)).byte()
    net = MappingVAE()
    net.load_state_dict(vsd)
    net = net.to(DEV).eval()
    m = KeyframeMap(DEV, capacity=4)
    for i in range(n):
        m.append(frames[i], torch.eye(4))
    m.embed(net, batch=16)
    assert m.n_embedded == n and tuple(m.embedding_bank.shape)[1] == 15360
    single = MappingVAE()
    single.load_state_dict(vsd)
    single = single.to(DEV).eval()
    for i in range(n):
        mu = single(frames[i].float().to(DEV))[0]
        assert tuple(mu.shape) == (1, 128, 6, 20)
        assert torch.equal(m.embedding_bank[i], mu.permute(0, 2, 3, 1).reshape(-1)), i
        assert torch.equal(m.embedding(i), mu) and m.embedding(i).data_ptr() == m.embedding_bank[i].data_ptr()
    # both query layouts reach the same rows; a keyframe finds itself at distance exactly 0
    mu = single(frames[:2].float().to(DEV))[0]
    d_a, i_a = m.search(mu, top_k=2)
    d_b, i_b = m.search(mu.permute(0, 2, 3, 1).reshape(2, -1), top_k=2)
    assert torch.equal(d_a, d_b) and torch.equal(i_a, i_b)
    assert i_a[:, 0].tolist() == [0, 1] and float(d_a[0, 0]) == 0.0 and float(d_a[1, 1]) == 0.0
    # more keyframes after an embed (the banks grow), then only the new ones are embedded; new weights embed all again
    before = m.embedding_bank[:n].clone()
    more = torch.from_numpy(syn.make_frames(n + 2, 376, 1232, seed=22)).byte()
    while len(m) < 2 * n + 2:
        m.append(more[len(m) - n], torch.eye(4))
    m.embed(net, batch=16)
    assert m.n_embedded == 2 * n + 2 and torch.equal(m.embedding_bank[:n], before)
    other = MappingVAE()
    other.load_state_dict(syn.to_torch(syn.make_vae_state(seed=3)))
    m.embed(other.to(DEV).eval(), batch=16)
    assert m.n_embedded == 2 * n + 2 and not torch.equal(m.embedding_bank[:n], before)


def _reloc_directory(golden_dir, vsd, root):
    """The keyframe directory of tests/golden/make_golden_slam.py, rebuilt from its seeds."""
    g = np.load(os.path.join(golden_dir, "reloc.npz"))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1232, seed=int(g["seed_frames"])))
    kf = os.path.join(str(root), "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    for i in range(3):
        torch.save(frames[i].byte(), os.path.join(kf, "rgb", "%06d.pth" % i))
    torch.save(torch.from_numpy(g["keyframe_poses"]), os.path.join(kf, "poses.pth"))
    torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
    return g, kf, {"near1": frames[1].byte().float(), "new": frames[4].byte().float()}


def test_resident_relocalization_matches_reference(golden_dir, gsd, hsd, vsd, tmp_path):
    from atdn_vslam_amd.slam import NeuralSLAM
    g, kf, queries = _reloc_directory(golden_dir, vsd, tmp_path)
    slam = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True)
    assert slam.mode() == "relocalization" and len(slam) == 3
    assert slam[1].embedding.data_ptr() == slam._map.embedding_bank[1].data_ptr()      # a view of the bank row
    # sequential queries: the reference's numbers with the tolerances of test_neuralslam_relocalization_matches_reference,
    # the second one with the head's state carried over from the first
    for name in ("near1", "new"):
        init, refined, dist = slam(queries[name])
        assert tuple(dist.shape) == (3,)
        np.testing.assert_allclose(dist.numpy(), g[name + "_distances"], rtol=0, atol=2e-3)
        assert int(torch.argmin(dist)) == int(np.argmin(g[name + "_distances"]))
        np.testing.assert_allclose(init.numpy(), g[name + "_initial"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(refined.numpy(), g[name + "_refined"], rtol=0, atol=5e-5)
    # the batch call
    golden_rows = np.stack([g["near1_distances"], g["new_distances"]])
    gaps = np.diff(np.sort(golden_rows, axis=1), axis=1)
    assert gaps.min() >= 6.0, gaps                    # [47.09, 0, 37.01], [43.42, 62.97, 49.74]
    state = slam._odometry_net._state.clone()
    dist, idx, initial, refined = slam.relocalize_batch([queries["near1"], queries["new"]], top_k=3)
    assert torch.equal(slam._odometry_net._state, state)      # the head's carried state: bit-identical
    assert tuple(dist.shape) == (2, 3) and tuple(idx.shape) == (2, 3)
    assert tuple(initial.shape) == (2, 4, 4) and tuple(refined.shape) == (2, 4, 4)
    assert not dist.is_cuda and not idx.is_cuda and initial.dtype == torch.float32 and refined.dtype == torch.float32
    np.testing.assert_allclose(dist.numpy(), golden_rows, rtol=0, atol=2e-3)
    assert np.array_equal(idx.numpy(), np.argsort(golden_rows, axis=1, kind="stable"))
    np.testing.assert_allclose(initial[0].numpy(), g["near1_initial"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(initial[1].numpy(), g["new_initial"], rtol=0, atol=1e-6)
    # near1: the golden's first query also started from the zero state
    np.testing.assert_allclose(refined[0].numpy(), g["near1_refined"], rtol=0, atol=5e-5)
    # new: from the zero state, so against the default code path asked for `new` as its FIRST query; each path holds 5e-5
    # against the reference, the two together 1e-4
    fresh = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization")
    assert fresh._map is None
    _, fresh_refined, _ = fresh(queries["new"])
    np.testing.assert_allclose(refined[1].numpy(), fresh_refined.numpy(), rtol=0, atol=1e-4)
    # refine=False returns the keyframe poses; the state stays untouched again; a later single query still carries it
    d2, i2, init2, ref2 = slam.relocalize_batch(torch.stack([queries["new"]]), top_k=1, refine=False)
    assert torch.equal(d2[0], dist[1]) and int(i2[0, 0]) == int(idx[1, 0]) and torch.equal(init2, ref2)
    assert torch.equal(slam._odometry_net._state, state)
    with pytest.raises(RuntimeError, match="resident_map=True"):
        fresh.relocalize_batch([queries["new"]])


def _parent_relocalize(slam, image):
    """The relocalisation body as it stood before the resident map existed, on `slam`'s own networks and keyframes."""
    from atdn_vslam_amd import transforms
    mu = slam._mapping_net(image)[0]
    distances = torch.stack([torch.norm(kf.embedding - mu, p=2) for kf in slam._keyframes], dim=0)
    closest = slam._keyframes[int(torch.argmin(distances))]
    initial_pose = closest.pose
    im1 = torch.load(closest.rgb_file_name).unsqueeze(0).to(slam._device).float()
    _, flow = slam._flow_net(im1, image, iters=12, test_mode=True)
    pred_rot, pred_tr = slam._odometry_net(flow)
    pose_diff = transforms.transform(pred_rot.squeeze().cpu(), pred_tr.squeeze().cpu())
    return initial_pose, initial_pose @ pose_diff, distances.cpu()


def test_default_path_is_untouched(golden_dir, gsd, hsd, vsd, tmp_path):
    """resident_map=False (and no argument at all) must return, bit for bit, what the code returned before the switch
    existed: compared with a private copy of the old body run on a second, identically built object."""
    from atdn_vslam_amd.slam import NeuralSLAM
    g, kf, queries = _reloc_directory(golden_dir, vsd, tmp_path)
    a = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=False)
    b = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization")
    assert a._map is None and b._map is None
    for name in ("near1", "new"):
        q = queries[name]
        got = a(q)
        want = _parent_relocalize(b, q.to(DEV).float().unsqueeze(0))
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and torch.equal(x, y), name


def test_odometry_mode_with_the_resident_map(golden_dir, gsd, hsd, vsd, tmp_path):
    """The four-frame run behind tests/golden/slam.npz with the switch on: the same poses and the same files as with it
    off, and the image bank holds the bytes of the saved files. Then the same run with every frame a keyframe and a map
    that starts at capacity 1 (it has to grow twice), embedded from the bank at end_odometry()."""
    from atdn_vslam_amd.slam import KeyframePolicy, NeuralSLAM
    g = np.load(os.path.join(golden_dir, "slam.npz"))
    frames = torch.from_numpy(syn.make_frames(4, 376, 1241, seed=int(g["seed_frames"])))
    for every_frame in (False, True):
        runs = {}
        for resident in (False, True):
            kf = os.path.join(str(tmp_path), "kf_%d_%d" % (every_frame, resident))
            slam = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, resident_map=resident)
            if every_frame:
                slam._policy = KeyframePolicy(rot_threshold_deg=0.0, translation_threshold=0.0)
                if resident:
                    slam._map = KeyframeMap(DEV, hw=SLAM_SIZE, capacity=1)
            slam.start_odometry()
            poses = [slam(frames[i]).clone() for i in range(4)]
            for i in range(4):
                assert float((poses[i] - torch.from_numpy(g["poses"][i])).abs().max()) < 2e-5, i
            assert len(slam) == (4 if every_frame else int(g["n_keyframes"]))
            files = [torch.load(os.path.join(kf, "rgb", "%06d.pth" % i)) for i in range(len(slam))]
            assert sorted(os.listdir(os.path.join(kf, "rgb"))) == ["%06d.pth" % i for i in range(len(slam))]
            runs[resident] = (slam, poses, files)
        (off, poses_off, files_off), (on, poses_on, files_on) = runs[False], runs[True]
        assert off._map is None and len(on._map) == len(on)
        for a, b in zip(poses_off, poses_on):
            assert torch.equal(a, b)
        for i, (a, b) in enumerate(zip(files_off, files_on)):
            assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and torch.equal(a, b)
            assert torch.equal(on._map.image_bank[i].cpu(), b)
            assert torch.equal(on._map.poses[i], on[i].pose) and torch.equal(on[i].pose, off[i].pose)
        if every_frame:
            assert on._map.capacity == 4
            for s in (off, on):
                s.end_odometry(mapping_weights=vsd)
                assert s.mode() == "relocalization"
            assert torch.equal(torch.load(os.path.join(on._base, "poses.pth")), torch.load(os.path.join(off._base, "poses.pth")))
            for i in range(4):
                assert on[i].embedding.data_ptr() == on._map.embedding_bank[i].data_ptr()
                assert torch.equal(on[i].embedding, off[i].embedding)
            init, refined, dist = on(files_on[2].float())
            assert float(dist[2]) == 0.0 and int(torch.argmin(dist)) == 2 and torch.equal(init, on[2].pose)
