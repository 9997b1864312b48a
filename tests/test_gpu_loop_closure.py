"""Loop closure of a keyframe map: loop_closure.find_loops / close_loops and NeuralSLAM(loop_closure=...) against the same steps
done by hand through transforms and the networks, on a five-keyframe directory from synthetic seeds with synthetic weights.
Synthetic weights make the flows, and so the measured loop edges, meaningless: this pins the plumbing, not accuracy (the
solver's accuracy is the subject of tests/test_pose_graph_host.py and tests/test_gpu_pose_graph.py)."""
import math
import os
import sys

import pytest
import torch

from atdn_vslam_amd import loop_closure, transforms
from atdn_vslam_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from slam_cases import _Args  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 5
OPTIONS = dict(min_gap=2, min_score=0.0)


@pytest.fixture(scope="module")
def weights():
    return (syn.to_torch(syn.make_gma_state(seed=1)), syn.to_torch(syn.make_clvo_state(seed=1)),
            syn.to_torch(syn.make_vae_state(seed=2)))


def _poses():
    """Five poses round a small loop, [5,12] float32."""
    out = []
    for k in range(K):
        a = 2.0 * math.pi * k / K
        out.append([math.cos(a), 0.0, math.sin(a), 3.0 * math.sin(a), 0.0, 1.0, 0.0, 0.1 * k, -math.sin(a), 0.0, math.cos(a),
                    3.0 * math.cos(a)])
    return torch.tensor(out, dtype=torch.float32)


def _directory(root, vsd):
    frames = torch.from_numpy(syn.make_frames(K, 376, 1232, seed=3))
    kf = os.path.join(str(root), "kf")
    os.makedirs(os.path.join(kf, "rgb"))
    for i in range(K):
        torch.save(frames[i].byte(), os.path.join(kf, "rgb", "%06d.pth" % i))
    torch.save(_poses(), os.path.join(kf, "poses.pth"))
    torch.save(vsd, os.path.join(kf, "MappingVAE_weights.pth"))
    return kf


def _slam(kf, weights, **kw):
    from atdn_vslam_amd.slam import NeuralSLAM
    gsd, hsd, vsd = weights
    return NeuralSLAM(_Args(kf), odometry_weights=hsd, flow_weights=gsd, **kw)


def test_find_and_close_loops_equal_the_steps_by_hand(weights, tmp_path):
    kf = _directory(tmp_path, weights[2])
    slam = _slam(kf, weights, start_mode="relocalization", resident_map=True)
    kmap, flow_net, head = slam._map, slam._flow_for_batches(), slam._odometry_net
    loops = loop_closure.find_loops(kmap, flow_net, head, **OPTIONS)
    # by hand
    with torch.no_grad():
        dist, _ = kmap.search(kmap.embedding_bank[:K], 1)
        pairs = loop_closure.select_candidates(dist.cpu(), 2, 2)
        assert 3 <= len(pairs) <= 5 and all(j - i >= 2 for i, j in pairs)
        assert len(pairs) <= flow_net.max_batch // 2                      # one chunk
        fw, bw = flow_net.forward_backward(kmap.images([i for i, _ in pairs]), kmap.images([j for _, j in pairs]), iters=12)
        mask, count = transforms._flow_consistency_counts(fw, bw, 0.01, 0.5)
        rot, tr, _ = head.scan(head.encode(fw)[None], state=None, hw=kmap.hw)
    rot, tr = rot[0].cpu(), tr[0].cpu()
    meas = torch.stack([transforms.transform(rot[p], tr[p]) for p in range(len(pairs))])
    scores = (count.cpu().double() / float(376 * 1232)).float()
    assert loops["pairs"].tolist() == [list(p) for p in pairs] and loops["candidates"].tolist() == loops["pairs"].tolist()
    assert torch.equal(loops["edge_pose"].view(torch.int32), meas.view(torch.int32))
    assert torch.equal(loops["scores"], scores) and torch.equal(loops["candidate_scores"], scores)
    # a threshold above every score drops every pair; nothing is solved and nothing changes
    before = kmap.poses.clone()
    none = loop_closure.close_loops(kmap, flow_net, head, min_gap=2, min_score=2.0)
    assert none["counts"] is None and none["loops"]["pairs"].shape == (0, 2) and len(none["loops"]["candidates"]) == len(pairs)
    assert torch.equal(kmap.poses, before)
    # close_loops = pose_graph_optimize on the odometry edges and those loop edges, and the map's poses are replaced
    report = slam.close_loops(**OPTIONS)
    index, odo, weight = loop_closure.odometry_edges(before)
    L = len(pairs)
    index = torch.cat([index, torch.tensor(pairs, dtype=torch.int32).t()], dim=1)
    weight = torch.cat([weight, loop_closure._weights(L, loop_closure.LOOP_SIGMA)])
    robust = torch.tensor([0] * (K - 1) + [1] * L, dtype=torch.uint8)
    want = transforms.pose_graph_optimize(before.to(DEV), index.to(DEV), torch.cat([odo, meas]).to(DEV), weight.to(DEV),
                                          robust.to(DEV), robust_scale=loop_closure.ROBUST_SCALE)
    host = transforms.pose_graph_optimize(before, index, torch.cat([odo, meas]), weight, robust,
                                          robust_scale=loop_closure.ROBUST_SCALE)
    for key, w, h in zip(("poses_after", "cost", "edge_chi2", "counts"), want, host):
        assert torch.equal(report[key], w.cpu()) and torch.equal(w.cpu(), h), key
    assert report["counts"][:2].tolist() == [K - 1 + L, 0] and torch.equal(report["poses_before"], before)
    assert torch.equal(kmap.poses, report["poses_after"]) and torch.equal(kmap.poses[0], before[0])
    assert all(torch.equal(f.pose, kmap.poses[i]) for i, f in enumerate(slam._keyframes))
    closed = torch.load(os.path.join(kf, "poses_closed.pth"))
    assert closed.shape == (K, 12) and torch.equal(closed, report["poses_after"][:, :3, :].reshape(K, 12))
    assert torch.equal(torch.load(os.path.join(kf, "poses.pth")), _poses())


def test_end_odometry_with_and_without_loop_closure(weights, tmp_path):
    from atdn_vslam_amd.slam import NeuralSLAM
    frames = torch.from_numpy(syn.make_frames(K, 376, 1232, seed=3))
    query = frames[1:2].byte().float()
    off = _slam(_directory(tmp_path / "off", weights[2]), weights, start_mode="mapping", mapping_weights=weights[2],
                resident_map=True)
    kf_off = off._args.keyframes_path
    assert sorted(os.listdir(kf_off)) == ["MappingVAE_weights.pth", "poses.pth", "rgb"] and off.loop_report is None
    assert torch.equal(torch.load(os.path.join(kf_off, "poses.pth")), _poses())
    answer_off = off.relocalize_batch(query, top_k=2, verify=True)
    assert torch.equal(answer_off[2][0, :3, :].reshape(12), _poses()[int(answer_off[1][0, answer_off[5][0]])])
    with pytest.raises(ValueError):
        NeuralSLAM(_Args(kf_off), odometry_weights=weights[1], flow_weights=weights[0], start_mode="relocalization",
                   loop_closure=True)
    del off
    on = _slam(_directory(tmp_path / "on", weights[2]), weights, start_mode="mapping", mapping_weights=weights[2],
               resident_map=True, loop_closure=True, loop_options=OPTIONS)
    kf_on = on._args.keyframes_path
    assert sorted(os.listdir(kf_on)) == ["MappingVAE_weights.pth", "poses.pth", "poses_closed.pth", "rgb"]
    assert torch.equal(torch.load(os.path.join(kf_on, "poses.pth")), _poses())           # stays the raw odometry
    closed = torch.load(os.path.join(kf_on, "poses_closed.pth"))
    assert torch.equal(closed, on.loop_report["poses_after"][:, :3, :].reshape(K, 12))
    assert torch.equal(on._map.poses[:, :3, :].reshape(K, 12), closed)
    answer_on = on.relocalize_batch(query, top_k=2, verify=True)
    # the search, the flows and the scores do not depend on the poses; the answer's pose is the closed one
    for i in (0, 1, 4, 5):
        assert torch.equal(answer_on[i], answer_off[i]), i
    assert torch.equal(answer_on[2][0, :3, :].reshape(12), closed[int(answer_on[1][0, answer_on[5][0]])])
    del on
    again = _slam(kf_on, weights, start_mode="relocalization", resident_map=True)       # loads poses_closed.pth
    assert torch.equal(again._map.poses[:, :3, :].reshape(K, 12), closed)
    assert all(torch.equal(f.pose, again._map.poses[i]) for i, f in enumerate(again._keyframes))
    plain = _slam(kf_on, weights, start_mode="relocalization")                           # the list form too
    assert all(torch.equal(f.pose[:3].reshape(12), closed[i]) for i, f in enumerate(plain._keyframes))
