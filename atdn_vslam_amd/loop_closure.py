"""Loop closure of a keyframe map: revisits among the keyframes found by the map's own one-launch search, verified by
forward-backward flow consistency and measured by the pose head (or, with depth and a calibration, by PnP), then the keyframe
poses optimised over the resulting pose graph (`transforms.pose_graph_optimize`: libatdn_hip's solver, one launch). The
reference has no loop closure; nothing here is on by default.

Sigmas. An edge's weights are 1 / sigma^2 of its rotation (rad) and translation (m). The defaults below are NOT MEASURED:
the real checkpoints are absent, so nobody has measured the pose head's error. They are plain values, one
tenth of the keyframe thresholds of `slam.KeyframePolicy` (10 degrees, 15 m), for odometry and loop edges alike."""
import math

import torch

from . import transforms

ODOMETRY_SIGMA = (math.radians(1.0), 1.5)   # rad, m — not measured
LOOP_SIGMA = (math.radians(1.0), 1.5)       # rad, m — not measured
ROBUST_SCALE = (25.0, 5.0)                  # sigmas, large to small — not measured


def _poses44(poses):
    p = torch.as_tensor(poses).detach().cpu().float()
    if p.dim() == 2 and p.shape[1] == 12:
        p = p.view(-1, 3, 4)
    if p.dim() == 3 and tuple(p.shape[1:]) == (3, 4):
        last = torch.tensor([0.0, 0.0, 0.0, 1.0]).view(1, 1, 4).repeat(len(p), 1, 1)
        p = torch.cat([p, last], dim=1)
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
        raise ValueError("poses must be [K,12], [K,3,4] or [K,4,4], got %s" % (tuple(p.shape),))
    return p


def _weights(n, sigma):
    rot, tr = float(sigma[0]), float(sigma[1])
    if not (rot > 0.0 and tr > 0.0 and math.isfinite(rot) and math.isfinite(tr)):
        raise ValueError("sigma must be two finite positive numbers (rad, m), got %r" % (sigma,))
    return torch.tensor([[1.0 / (rot * rot), 1.0 / (tr * tr)]], dtype=torch.float64).repeat(n, 1)


def odometry_edges(poses, sigma=ODOMETRY_SIGMA):
    """The consecutive-keyframe edges of a trajectory, from its stored poses: `poses` [K,4,4] ([K,3,4], [K,12]), K >= 2 ->
    `(edge_index [2,K-1] int32, edge_pose [K-1,4,4] float32, edge_weight [K-1,2] float64)` with edge k = (k, k+1) measuring
    inv(T_k) @ T_{k+1} (formed in float64, rounded once) at weights 1 / sigma^2. Host tensors."""
    p = _poses44(poses).double()
    K = p.shape[0]
    if K < 2:
        raise ValueError("odometry_edges needs at least two poses")
    rel = torch.linalg.inv(p[:-1]) @ p[1:]
    index = torch.stack([torch.arange(K - 1), torch.arange(1, K)]).to(torch.int32)
    return index, rel.float(), _weights(K - 1, sigma)


def select_candidates(distances, min_gap, top_k, max_distance=None):
    """Loop candidates from the distances between the keyframes' embeddings: `distances` [K,K] (row j: from keyframe j). For
    every keyframe j, the `top_k` nearest keyframes i with j - i >= min_gap (>= 1), nearest first, equal distances by the lower
    index, none farther than `max_distance`. A pure host function. Returns the pairs (i, j), i < j, as a list sorted by (j, rank);
    looking back only, every unordered pair appears once."""
    d = torch.as_tensor(distances).detach().cpu().double()
    if d.dim() != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("expected distances [K,K], got %s" % (tuple(d.shape),))
    if int(min_gap) < 1 or int(top_k) < 1:
        raise ValueError("min_gap and top_k must be >= 1")
    pairs = []
    for j in range(int(min_gap), d.shape[0]):
        row = d[j, :j - int(min_gap) + 1].tolist()
        order = sorted(range(len(row)), key=lambda i: (row[i], i))
        keep = [i for i in order if not math.isnan(row[i]) and (max_distance is None or row[i] <= float(max_distance))]
        pairs.extend((i, j) for i in keep[:int(top_k)])
    return pairs


@torch.no_grad()
def find_loops(kmap, flow_net, odometry_net, min_gap=10, top_k=2, min_score=0.5, calib=None, max_distance=None):
    """Revisits among the keyframes of `kmap` (a `KeyframeMap` with all keyframes embedded). The distances between the map's
    own embeddings come from its one-launch search; `select_candidates` picks the pairs; every pair (keyframe i, keyframe j)
    goes through `KeyframeMap._evaluate_pairs` — forward-backward flow, the consistency count, one recurrent step of the pose
    head from the reset state, exactly as a verified relocalisation does — and a pair whose share of consistent pixels is below
    `min_score` is dropped. The measurement of T_i^-1 T_j is `transforms.transform(rot, tr)` of the pose head, or with `calib`
    (the calibration of the map's grid) the PnP pose from keyframe i's depth under the consistency mask where PnP accepted a
    step. Returns a dict of host tensors: `pairs` [L,2] int64 (i < j), `edge_pose` [L,4,4], `scores` [L] float32,
    `candidates` [P,2] (all pairs evaluated) and `candidate_scores` [P]."""
    K = len(kmap)
    empty = dict(pairs=torch.zeros((0, 2), dtype=torch.int64), edge_pose=torch.zeros((0, 4, 4)), scores=torch.zeros(0),
                 candidates=torch.zeros((0, 2), dtype=torch.int64), candidate_scores=torch.zeros(0))
    if K <= int(min_gap):
        return empty
    with torch.cuda.device(kmap.device):
        dist, _ = kmap.search(kmap.embedding_bank[:K], 1)
        pairs = select_candidates(dist.cpu(), min_gap, top_k, max_distance)
        if not pairs:
            return empty
        rot, tr, counts, geo, geo_counts = kmap._evaluate_pairs([i for i, _ in pairs], kmap.images([j for _, j in pairs]),
                                                                flow_net, odometry_net, calib)
    scores = (counts.double() / float(kmap.hw[0] * kmap.hw[1])).float()
    meas = torch.stack([transforms.transform(rot[p], tr[p]) for p in range(len(pairs))], dim=0)
    if geo is not None:
        solved = geo_counts[:, 3] > 0
        meas[solved] = geo[solved]
    cand = torch.tensor(pairs, dtype=torch.int64)
    keep = scores >= float(min_score)
    return dict(pairs=cand[keep], edge_pose=meas[keep], scores=scores[keep], candidates=cand, candidate_scores=scores)


def close_loops(kmap, flow_net, odometry_net, min_gap=10, top_k=2, min_score=0.5, calib=None, max_distance=None,
                odometry_sigma=ODOMETRY_SIGMA, loop_sigma=LOOP_SIGMA, robust_scale=ROBUST_SCALE, iters=10, cg_iters=64,
                cg_tol=1e-8):
    """Close the loops of a keyframe map: `find_loops`, then `transforms.pose_graph_optimize` on the device over the odometry
    edges of the stored poses (`odometry_edges`, quadratic) and the loop edges (Geman-McClure at `robust_scale`, a sequence
    solved large to small), keyframe 0 held; the map's poses are replaced through `KeyframeMap.update_poses`. Without a loop
    nothing is solved and nothing changes. Returns a report (host tensors): `edge_index` [2,E], `edge_pose` [E,4,4],
    `edge_weight` [E,2], `edge_robust` [E], `loops` (the dict of `find_loops`), `scores` [L], `poses_before` and `poses_after`
    [K,4,4], `cost` [2] (before, after; of the last scale), `edge_chi2` [E], `counts` [4]."""
    loops = find_loops(kmap, flow_net, odometry_net, min_gap, top_k, min_score, calib, max_distance)
    before = kmap.poses.clone()
    index, meas, weight = odometry_edges(before, odometry_sigma)
    L = int(loops["pairs"].shape[0])
    index = torch.cat([index, loops["pairs"].t().to(torch.int32)], dim=1)
    meas = torch.cat([meas, loops["edge_pose"]], dim=0)
    weight = torch.cat([weight, _weights(L, loop_sigma)], dim=0)
    robust = torch.cat([torch.zeros(len(before) - 1, dtype=torch.uint8), torch.ones(L, dtype=torch.uint8)])
    report = dict(edge_index=index, edge_pose=meas, edge_weight=weight, edge_robust=robust, loops=loops, scores=loops["scores"],
                  poses_before=before, poses_after=before.clone(), cost=None, edge_chi2=None, counts=None)
    if L == 0:
        return report
    dev = kmap.device
    poses, cost, chi2, counts = transforms.pose_graph_optimize(before.to(dev), index.to(dev), meas.to(dev), weight.to(dev),
                                                               robust.to(dev), robust_scale=robust_scale, iters=iters,
                                                               cg_iters=cg_iters, cg_tol=cg_tol)
    report.update(poses_after=poses.cpu(), cost=cost.cpu(), edge_chi2=chi2.cpu(), counts=counts.cpu())
    kmap.update_poses(report["poses_after"])
    return report
