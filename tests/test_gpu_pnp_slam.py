"""The geometric leg of relocalisation: KeyframeMap's depth bank and relocalize(..., geometric=True) /
NeuralSLAM.relocalize_batch(..., geometric=True) against the same steps done by hand through transforms, with synthetic weights."""
import os
import sys

import numpy as np
import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd import transforms
from atdn_vslam_amd.keyframe_map import KeyframeMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args, EverySecond, SLAM_CALIB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HW = (376, 1232)


@pytest.fixture(scope="module")
def gsd():
    return syn.to_torch(syn.make_gma_state(seed=1))


@pytest.fixture(scope="module")
def hsd():
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def vsd():
    return syn.to_torch(syn.make_vae_state(seed=2))


def _depth_map(seed):
    """A smooth synthetic depth [1,376,1232] float32 between 4 and 60 with a band of holes."""
    y = torch.arange(HW[0], dtype=torch.float32).view(-1, 1) / HW[0]
    x = torch.arange(HW[1], dtype=torch.float32).view(1, -1) / HW[1]
    d = 4.0 + 56.0 * (0.5 + 0.5 * torch.cos(6.28318 * (x + 0.17 * seed))) * (0.5 + 0.5 * torch.cos(3.14159 * y))
    d[100:140] = 0.0
    return d[None].contiguous()


def _reloc_directory(golden_dir, vsd, root):
    """The three-keyframe directory of tests/test_gpu_keyframe_map.py, rebuilt from its seeds, with depth files for keyframes 0
    and 1; keyframe 2 has none."""
    g = np.load(os.path.join(golden_dir, "reloc.npz"))
    frames = torch.from_numpy(syn.make_frames(5, 376, 1232, seed=int(g["seed_frames"])))
    kf = os.path.join(str(root), "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    os.makedirs(os.path.join(kf, "depth"))
    for i in range(3):
        torch.save(frames[i].byte(), os.path.join(kf, "rgb", "%06d.pth" % i))
    for i in range(2):
        torch.save(_depth_map(i), os.path.join(kf, "depth", "%06d.pth" % i))
    torch.save(torch.from_numpy(g["keyframe_poses"]), os.path.join(kf, "poses.pth"))
    torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
    return kf, [frames[1].byte().float(), frames[4].byte().float()]


def test_geometric_relocalization(golden_dir, gsd, hsd, vsd, tmp_path):
    from atdn_vslam_amd.slam import NeuralSLAM
    kf, batch = _reloc_directory(golden_dir, vsd, tmp_path)
    slam = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True,
                      calib=SLAM_CALIB)
    kmap, flow_net, head = slam._map, slam._flow_for_batches(), slam._odometry_net
    # from_directory loaded the two depth files; keyframe 2 holds zeros
    assert tuple(kmap.depth_bank.shape[1:]) == HW and kmap.depth_bank.dtype == torch.float32 and kmap.depth_bank.is_cuda
    for i in range(2):
        assert torch.equal(kmap.depth_bank[i].cpu(), _depth_map(i)[0])
    assert not bool(kmap.depth_bank[2].any())
    assert torch.equal(kmap.depths([2, 0]), torch.stack([kmap.depth_bank[2], kmap.depth_bank[0]]))

    # geometric=False: the old tuples, bit for bit
    plain = slam.relocalize_batch(batch, top_k=3)
    off = slam.relocalize_batch(batch, top_k=3, geometric=False)
    assert len(plain) == 4 and len(off) == 4 and all(torch.equal(x, y) for x, y in zip(plain, off))
    vplain = slam.relocalize_batch(batch, top_k=3, verify=True)
    assert len(vplain) == 6

    # verify off: the nearest keyframe of every query, by hand
    out = slam.relocalize_batch(batch, top_k=3, geometric=True)
    assert len(out) == 6 and all(torch.equal(x, y) for x, y in zip(out[:4], plain))
    dist, idx, initial, refined, refined_geo, geo_counts = out
    assert tuple(refined_geo.shape) == (2, 4, 4) and refined_geo.dtype == torch.float32 and not refined_geo.is_cuda
    assert tuple(geo_counts.shape) == (2, 4) and geo_counts.dtype == torch.int32 and not geo_counts.is_cuda
    q = torch.stack(batch).to(DEV)
    best = idx[:, 0]
    _, flow = flow_net(kmap.images(best), q, iters=12, test_mode=True)
    rot, tr, _ = head.scan(head.encode(flow)[None], state=None, hw=HW)
    rot, tr = rot[0].cpu(), tr[0].cpu()
    rel = torch.stack([transforms.transform(rot[i], tr[i]) for i in range(2)])
    pose, cost, counts = transforms.pose_from_depth(kmap.depth_bank[best.to(DEV)], flow, rel, SLAM_CALIB)
    assert pose.is_cuda and counts.is_cuda
    for i in range(2):
        assert torch.equal(refined[i], initial[i] @ rel[i])
        assert torch.equal(refined_geo[i], initial[i] @ pose[i].cpu()), i
    assert torch.equal(geo_counts, counts.cpu())
    print("nearest", best.tolist(), "geo counts", geo_counts.tolist(), "score", transforms.reprojection_score(geo_counts).tolist())
    for i in range(2):
        if int(best[i]) == 2:                                     # no depth: exactly the head's pose
            assert torch.equal(refined_geo[i], refined[i]) and geo_counts[i].tolist() == [0, 0, 0, 0]
        else:
            assert int(geo_counts[i, 0]) > 0
    again = slam.relocalize_batch(batch, top_k=3, geometric=True)
    assert all(torch.equal(x, y) for x, y in zip(out, again))

    # verify on: all six pairs, the consistency mask as the mask, the chosen candidate's results
    vout = slam.relocalize_batch(batch, top_k=3, verify=True, geometric=True)
    assert len(vout) == 8 and all(torch.equal(x, y) for x, y in zip(vout[:6], vplain))
    chosen = vout[5]
    flat = idx.reshape(-1)
    fw, bw = flow_net.forward_backward(kmap.images(flat), q.repeat_interleave(3, dim=0), iters=12)
    mask, _ = transforms.flow_consistency(fw, bw)
    rot, tr, _ = head.scan(head.encode(fw)[None], state=None, hw=HW)
    rot, tr = rot[0].cpu(), tr[0].cpu()
    rel = torch.stack([transforms.transform(rot[p], tr[p]) for p in range(6)])
    pose, _, counts = transforms.pose_from_depth(kmap.depths(flat.tolist()), fw, rel, SLAM_CALIB, mask=mask)
    for i in range(2):
        p = 3 * i + int(chosen[i])
        assert torch.equal(vout[6][i], vout[2][i] @ pose[p].cpu()) and torch.equal(vout[7][i], counts[p].cpu()), i
    print("verified geo counts", vout[7].tolist(), "all pairs", counts.cpu().tolist())

    # a map without any depth: refined_geo == refined and zero counts
    bare = KeyframeMap(DEV, hw=HW, capacity=2)
    for i in range(3):
        bare.append(kmap.image_bank[i], kmap.poses[i])            # (the third append doubles the capacity)
    assert bare.depth_bank is None
    bare.embed(slam._mapping_net)
    b = bare.relocalize(torch.stack(batch), flow_net, head, slam._mapping_net, top_k=1, geometric=True, calib=SLAM_CALIB)
    assert torch.equal(b[4], b[3]) and not bool(b[5].any())
    bare.set_depth(1, _depth_map(1))                              # allocated on first use
    assert tuple(bare.depth_bank.shape) == (4,) + HW and not bool(bare.depth_bank[0].any())
    assert torch.equal(bare.depth_bank[1], kmap.depth_bank[1])
    bare.append(kmap.image_bank[0], kmap.poses[0])
    bare.append(kmap.image_bank[0], kmap.poses[0])                # grows: the depths go along
    assert tuple(bare.depth_bank.shape) == (8,) + HW and torch.equal(bare.depth_bank[1], kmap.depth_bank[1])
    assert not bool(bare.depth_bank[4].any())

    # errors
    with pytest.raises(ValueError, match="refine"):
        slam.relocalize_batch(batch, refine=False, geometric=True)
    with pytest.raises(ValueError, match="calib"):
        kmap.relocalize(torch.stack(batch), flow_net, head, slam._mapping_net, geometric=True)
    with pytest.raises(ValueError):
        kmap.set_depth(0, torch.zeros(3, 4))
    with pytest.raises(IndexError):
        kmap.set_depth(3, _depth_map(0))
    nocal = NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, start_mode="relocalization", resident_map=True)
    with pytest.raises(ValueError, match="calib"):
        nocal.relocalize_batch(batch, geometric=True)


@pytest.mark.parametrize("mode", ["pair", "track"])
def test_cold_start_session_fills_the_depth_bank(gsd, hsd, vsd, tmp_path, mode):
    """Four frames, every second pair ends in a keyframe: the session's own map holds the depths it wrote, and from_directory
    loads the same ones."""
    from atdn_vslam_amd.slam import NeuralSLAM

    path = os.path.join(str(tmp_path), mode)
    os.makedirs(path)
    weights = os.path.join(str(tmp_path), "vae_%s.pth" % mode)
    torch.save(vsd, weights)
    slam = NeuralSLAM(_Args(path), odometry_weights=hsd, flow_weights=gsd, resident_map=True, calib=SLAM_CALIB, keyframe_depth=mode)
    slam._policy = EverySecond()
    slam.start_odometry()
    for f in torch.from_numpy(syn.make_frames(4, 376, 1241, seed=8)):
        slam(f)
    slam.end_odometry(mapping_weights=weights)
    assert len(slam) == 2
    files = sorted(os.listdir(os.path.join(path, "depth")))
    assert files == ["000000.pth", "000001.pth"]
    loaded = KeyframeMap.from_directory(path, DEV)
    for k in range(2):
        stored = torch.load(os.path.join(path, "depth", files[k]))
        assert tuple(stored.shape) == (1,) + HW
        assert torch.equal(slam._map.depth_bank[k].cpu(), stored[0]) and torch.equal(loaded.depth_bank[k].cpu(), stored[0]), k
    print(mode, "non-zero depths", [int((loaded.depth_bank[k] != 0).sum()) for k in range(2)])
