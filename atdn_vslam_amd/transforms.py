"""Pose algebra of the odometry path (atdn_vslam/utils/transforms.py) and the frame padder
(whl:GMA/core/utils/utils.py:8-25), host side of libatdn_hip."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr


def _np32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().to("cpu")
        x = x.numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def _byte_plane(t, what, B, H, W):
    """A mask or liveness tensor (uint8 or bool, B * H * W values whose last two axes are H, W) -> contiguous uint8."""
    if t.numel() != B * H * W or tuple(t.shape[-2:]) != (H, W):
        raise RuntimeError("expected %s of %d x %d x %d values, got %s" % (what, B, H, W, tuple(t.shape)))
    t = (t != 0).to(torch.uint8) if t.dtype != torch.uint8 else t
    return t.detach().contiguous()


def _min_sin2(min_parallax_deg):
    return math.sin(math.radians(float(min_parallax_deg))) ** 2


def transform(rot, tr):
    """transform(rot, tr) -> 4x4 float32 CPU tensor (transforms.py:97-119, Euler "yxz")."""
    r, t = _np32(rot).reshape(3), _np32(tr).reshape(3)
    out = np.empty(16, dtype=np.float32)
    _lib.check(_lib.lib().atdn_pose_transform_f32(r.ctypes.data, t.ctypes.data, out.ctypes.data))
    return torch.from_numpy(out.reshape(4, 4))


def rel2abs(rotations, translations):
    """rel2abs -> [T+1,4,4] float64 CPU tensor, identity first (transforms.py:147-170). Accepts the
    reference's lists of [1,3] tensors or [T,3] arrays."""
    if isinstance(rotations, (list, tuple)):
        rotations = np.stack([_np32(r).reshape(3) for r in rotations]) if len(rotations) else np.zeros((0, 3))
        translations = np.stack([_np32(t).reshape(3) for t in translations]) if len(translations) else np.zeros((0, 3))
    r, t = _np32(rotations).reshape(-1, 3), _np32(translations).reshape(-1, 3)
    if r.shape != t.shape:
        raise RuntimeError("rotations and translations differ in length")
    out = np.empty((r.shape[0] + 1, 4, 4), dtype=np.float64)
    _lib.check(_lib.lib().atdn_pose_rel2abs(r.ctypes.data, t.ctypes.data, r.shape[0], out.ctypes.data))
    return torch.from_numpy(out)


def accumulate(pose, rot, tr):
    """pose @ transform(rot, tr) in float32, as NeuralSLAM keeps its running pose (neural_slam.py:204-207)."""
    p = _np32(pose).reshape(16).copy()
    r, t = _np32(rot).reshape(3), _np32(tr).reshape(3)
    _lib.check(_lib.lib().atdn_pose_accumulate_f32(p.ctypes.data, r.ctypes.data, t.ctypes.data))
    return torch.from_numpy(p.reshape(4, 4))


def matrix2euler(R):
    """yxz Euler angles of a rotation matrix (transforms.py:41-44)."""
    R = torch.as_tensor(R)
    a = torch.atan2(R[0, 2], R[2, 2])
    b = torch.atan2(-R[1, 2], torch.sqrt(1 - R[1, 2] ** 2))
    g = torch.atan2(R[1, 0], R[1, 1])
    return torch.stack([a, b, g])


def kitti_rows(poses):
    """[T,4,4] -> [T,12] rows of the KITTI pose format (evaluate_odometry.py:86-90)."""
    p = torch.as_tensor(poses)
    return p[:, :3, :].reshape(p.shape[0], 12)


def forward_interpolate(flow):
    """forward_interpolate(flow_low) of the flow package (whl:GMA/core/utils/utils.py:28-56): the 1/8-resolution flow of one
    pair pushed forward along itself, the `flow_init` that warm-starts the next pair of a video. `flow` is [2,h,w] or [B,2,h,w];
    returns float32 of the same shape. A device tensor goes through libatdn_hip's kernel on the current stream and the result
    stays on the device (the wheel's function goes to the host and calls scipy's griddata twice); a CPU tensor goes through the
    library's float64 host form. Nearest valid source in float64, ties to the lowest source index, all zeros when no source
    lands inside the grid (the wheel raises there): include/atdn_hip.h, atdn_flow_forward_interpolate."""
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise RuntimeError("expected a flow [2,h,w] or [B,2,h,w], got %s" % (tuple(flow.shape),))
    src = flow.detach().float().contiguous()
    B = src.shape[0] if src.dim() == 4 else 1
    h, w = src.shape[-2:]
    out = torch.empty_like(src)
    _lib.call("atdn_flow_forward_interpolate", src.device, _ptr(src), B, h, w, _ptr(out))
    return out


def _flow_consistency_counts(flow_fw, flow_bw, alpha1, alpha2):
    """(mask uint8 [B,1,H,W], count int32 [B]) of two flows [B,2,H,W] on one device (atdn_flow_consistency / its host twin)."""
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2:
        raise RuntimeError("expected flows [B,2,H,W], got %s" % (tuple(flow_fw.shape),))
    if flow_bw.shape != flow_fw.shape:
        raise RuntimeError("flow_fw is %s but flow_bw is %s" % (tuple(flow_fw.shape), tuple(flow_bw.shape)))
    if flow_bw.device != flow_fw.device:
        raise RuntimeError("flow_fw on %s but flow_bw on %s" % (flow_fw.device, flow_bw.device))
    fw = flow_fw.detach().float().contiguous()
    bw = flow_bw.detach().float().contiguous()
    B, _, H, W = fw.shape
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=fw.device)
    count = torch.empty((B,), dtype=torch.int32, device=fw.device)
    _lib.call("atdn_flow_consistency", fw.device, _ptr(fw), _ptr(bw), B, H, W, float(alpha1), float(alpha2), _ptr(mask), _ptr(count))
    return mask, count


def flow_consistency(flow_fw, flow_bw, alpha1=0.01, alpha2=0.5):
    """Forward-backward consistency of a flow pair (UnFlow / ARFlow): `flow_fw` is the flow from image 1 to image 2, `flow_bw`
    the flow from image 2 to image 1, both [B,2,H,W] (or [2,H,W]), channel 0 = x. Returns `(mask, score)`: `mask` uint8
    [B,1,H,W] ([1,H,W] for 3-d inputs), 1 where following flow_fw and then flow_bw (bilinear, where flow_fw lands) returns to
    the start within alpha1 * (|fw|^2 + |bw|^2) + alpha2 — the pixels that are visible in both images and whose two flows agree —
    and 0 elsewhere (occluded, left the image, or the flows contradict each other; any NaN or infinity involved); `score`
    float32 [B] (0-d for 3-d inputs) = the share of ones, an exact integer count divided by H * W in float64, then rounded. Two
    images of different places give flows that are noise in both directions and a score near 0. Device tensors go through
    libatdn_hip's kernel on the current stream and the results stay on the device (no synchronisation); CPU tensors go through
    the library's host form. The rule is float64 and stated in full in include/atdn_hip.h, atdn_flow_consistency; the same
    inputs give the same bits on every call and on both paths."""
    if flow_fw.dim() not in (3, 4) or flow_bw.dim() != flow_fw.dim():
        raise RuntimeError("expected two flows [2,H,W] or [B,2,H,W], got %s and %s" % (tuple(flow_fw.shape), tuple(flow_bw.shape)))
    single = flow_fw.dim() == 3
    mask, count = _flow_consistency_counts(flow_fw[None] if single else flow_fw, flow_bw[None] if single else flow_bw, alpha1, alpha2)
    score = (count.double() / float(mask.shape[-2] * mask.shape[-1])).float()
    return (mask[0], score[0]) if single else (mask, score)


def _pose_rows(pose, B, device):
    """[B,4,4], [B,3,4] or [B,12] (one pose without the batch axis when B == 1) -> contiguous float32 [B,12] on `device`."""
    p = torch.as_tensor(pose)
    if B == 1 and (tuple(p.shape) in ((4, 4), (3, 4), (12,))):
        p = p[None]
    if p.dim() == 3 and tuple(p.shape[1:]) in ((4, 4), (3, 4)):
        p = p[:, :3, :].reshape(p.shape[0], 12)
    if p.dim() != 2 or tuple(p.shape) != (B, 12):
        raise RuntimeError("expected %d poses [B,4,4], [B,3,4] or [B,12], got %s" % (B, tuple(torch.as_tensor(pose).shape)))
    return p.detach().to(device=device, dtype=torch.float32).contiguous()


def _pose_matrices(rows):
    """Rows of [R|t], float32 [B,12] -> [B,4,4] with the last row 0 0 0 1."""
    pose = torch.zeros((rows.shape[0], 4, 4), dtype=torch.float32, device=rows.device)
    pose[:, 3, 3] = 1.0
    pose[:, :3, :] = rows.view(-1, 3, 4)
    return pose


def _flow_inputs(flow, pose, mask, depth=None):
    """The checked, contiguous inputs of the functions of a flow, a pose and a mask (and a depth), with the batch axis added to a
    3-d flow: (single, flow [B,2,H,W], depth or None, pose rows [B,12], mask uint8 or None, B, H, W), all on the flow's device."""
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise RuntimeError("expected a flow [2,H,W] or [B,2,H,W], got %s" % (tuple(flow.shape),))
    single = flow.dim() == 3
    f = (flow[None] if single else flow).detach().float().contiguous()
    B, _, H, W = f.shape
    d = None
    if depth is not None:
        d = torch.as_tensor(depth)
        if d.numel() != B * H * W or tuple(d.shape[-2:]) != (H, W):
            raise RuntimeError("expected a depth of %d x %d x %d values, got %s" % (B, H, W, tuple(d.shape)))
        if d.device != f.device:
            raise RuntimeError("flow on %s but depth on %s" % (f.device, d.device))
        d = d.detach().float().contiguous()
    p = _pose_rows(pose, B, f.device)
    m = None
    if mask is not None:
        m = _byte_plane(torch.as_tensor(mask), "a mask", B, H, W)
        if m.device != f.device:
            raise RuntimeError("flow on %s but mask on %s" % (f.device, m.device))
    return single, f, d, p, m, B, H, W


def two_view_depth(flow, pose, calib, mask=None, max_epipolar=1.0, min_parallax_deg=0.05, max_depth=80.0):
    """Depth and epipolar agreement of a flow and a relative pose under a calibration. `flow` [B,2,H,W] (or [2,H,W]) is the flow
    from image 1 to image 2, channel 0 = x; `pose` [B,4,4], [B,3,4] or [B,12] the relative pose with X1 = R X2 + t — what
    `transform(rot, tr)` of the pose head returns, the matrix a running pose is multiplied by; `calib` is (fx, fy, cx, cy) or a 3x3
    / 3x4 calibration matrix without skew, of the grid the flow lives on (depth.resize_calib). `mask` (uint8 or bool, [B,1,H,W],
    [B,H,W] or [H,W]; e.g. the mask of `flow_consistency`) removes the pixels where it is 0. Returns `(depth, counts)` on the flow's
    device: `depth` float32 [B,1,H,W] ([1,H,W] for a 3-d flow), the triangulated depth of every pixel in camera 1 and 0 where there
    is none; `counts` int32 [B,3] ([3]) = (correspondences that land inside image 2, those within `max_epipolar` pixels of their
    epipolar line, those with a valid depth: an inlier whose two rays meet at an angle of at least `min_parallax_deg` degrees, in
    front of both cameras, no farther than `max_depth`). `epipolar_score(counts)` is the share of inliers. Device tensors go through
    libatdn_hip's kernel on the current stream and the results stay on the device (no synchronisation); CPU tensors go through the
    library's host form. The rule is float64 and stated in full in include/atdn_hip.h, atdn_flow_two_view_depth; the same inputs
    give the same bits on every call and on both paths."""
    from .depth import intrinsics
    single, f, _, p, m, B, H, W = _flow_inputs(flow, pose, mask)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=f.device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=f.device)
    _lib.call("atdn_flow_two_view_depth", f.device, _ptr(f), _ptr(p), _ptr(m), B, H, W, *intrinsics(calib), float(max_epipolar),
              _min_sin2(min_parallax_deg), float(max_depth), _ptr(depth), _ptr(counts))
    return (depth[0], counts[0]) if single else (depth, counts)


def _index_tensor(values, what, device):
    """`values` (an integer tensor on `device`, or a host sequence) as contiguous int32 on `device`; a tensor elsewhere raises.
    Values outside the int32 range become -1 and int32's largest: outside every bank, as they were."""
    if isinstance(values, torch.Tensor):
        if values.device != device:
            raise RuntimeError("bank on %s but %s on %s" % (device, what, values.device))
        t = values.detach()
    else:
        t = torch.from_numpy(np.asarray(values, dtype=np.int64))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError("%s must be integers, got %s" % (what, t.dtype))
    return t.to(device).clamp(min=-1, max=2 ** 31 - 1).to(torch.int32).contiguous()


def fuse_depths(bank, poses, targets, sources, calib, max_reproj=1.0, max_rel_depth=0.01, min_views=2, min_z=0.1, average=True):
    """Multi-view consistency filter of depth maps (the geometric-consistency fusion of multi-view stereo). `bank` [N,H,W] float32
    holds N depth maps (0 = no depth), `poses` ([N,12], [N,3,4] or [N,4,4]; rows of [R|t], world <- camera, as `poses.pth` and
    `KeyframeMap.poses` hold them) their cameras, `calib` is (fx, fy, cx, cy) or a calibration matrix without skew. `targets` [B]
    names the maps to fuse and `sources` [B,S] the maps each is compared with (tensors on the bank's device or host sequences;
    a source < 0, >= N or equal to its target is an empty slot). Every target pixel with a depth is projected into each source,
    the source's depth there (bilinear; not across a hole) is projected back, and the source agrees when it returns within
    `max_reproj` pixels and `max_rel_depth` relative depth, in front of both cameras by `min_z`. Returns `(fused, views, counts)`
    on the bank's device: `fused` float32 [B,1,H,W], the target's depth where at least `min_views` sources agree (with `average`
    the mean of it and the agreeing estimates) and 0 elsewhere; `views` uint8 [B,H,W], the number of agreeing sources; `counts`
    int32 [B,3] = (pixels with a depth, pixels some source saw, pixels kept). All targets read the unfused bank. Device tensors go
    through libatdn_hip's kernel on the current stream and the results stay on the device (no synchronisation); CPU tensors go
    through the library's host form. The rule is float64 and stated in full in include/atdn_hip.h, atdn_depth_fuse; the same
    inputs give the same bits on every call and on both paths."""
    from .depth import intrinsics
    if not isinstance(bank, torch.Tensor) or bank.dim() != 3:
        raise RuntimeError("expected a depth bank [N,H,W], got %s" % (tuple(getattr(bank, "shape", ())),))
    if bank.dtype != torch.float32 or not bank.is_contiguous():
        bank = bank.detach().float().contiguous()
    N, H, W = (int(v) for v in bank.shape)
    p = torch.as_tensor(poses)
    if isinstance(poses, torch.Tensor) and poses.device != bank.device:
        raise RuntimeError("bank on %s but poses on %s" % (bank.device, poses.device))
    p = _pose_rows(p, N, bank.device)
    t = _index_tensor(targets, "targets", bank.device).reshape(-1)
    B = int(t.shape[0])
    if B < 1:
        raise RuntimeError("fuse_depths: no target")
    s = _index_tensor(sources, "sources", bank.device)
    s = s.reshape(B, 0) if s.numel() == 0 else s
    if s.dim() != 2 or s.shape[0] != B:
        raise RuntimeError("expected sources [%d,S], got %s" % (B, tuple(s.shape)))
    S = int(s.shape[1])
    fx, fy, cx, cy = intrinsics(calib)
    fused = torch.empty((B, 1, H, W), dtype=torch.float32, device=bank.device)
    views = torch.empty((B, H, W), dtype=torch.uint8, device=bank.device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=bank.device)
    _lib.call("atdn_depth_fuse", bank.device, _ptr(bank), _ptr(p), _ptr(t), _ptr(s) if S else None, N, B, S, H, W, fx, fy, cx, cy,
              float(max_reproj), float(max_rel_depth), int(min_views), float(min_z), 1 if average else 0, _ptr(fused), _ptr(views),
              _ptr(counts))
    return fused, views, counts


def _flow_bank_inputs(acc_bank, alive_bank, poses, slots):
    """The checked, contiguous flow bank of `multiview_depth` and the bundle adjustment: (acc_bank float32 [N,2,H,W], alive uint8,
    pose rows [N,12], slots int32 [B,S], N, B, S, H, W), all on the bank's device."""
    if not isinstance(acc_bank, torch.Tensor) or acc_bank.dim() != 4 or acc_bank.shape[1] != 2:
        raise RuntimeError("expected a flow bank [N,2,H,W], got %s" % (tuple(getattr(acc_bank, "shape", ())),))
    if acc_bank.dtype != torch.float32 or not acc_bank.is_contiguous():
        acc_bank = acc_bank.detach().float().contiguous()
    N, _, H, W = (int(v) for v in acc_bank.shape)
    device = acc_bank.device
    if not isinstance(alive_bank, torch.Tensor) or alive_bank.device != device:
        raise RuntimeError("flow bank on %s but the liveness bank on %s" % (device, getattr(alive_bank, "device", "the host")))
    alive = _byte_plane(alive_bank, "a liveness bank", N, H, W)
    if isinstance(poses, torch.Tensor) and poses.device != device:
        raise RuntimeError("bank on %s but poses on %s" % (device, poses.device))
    p = _pose_rows(torch.as_tensor(poses), N, device)
    s = _index_tensor(slots, "slots", device)
    s = s[None] if s.dim() == 1 else s
    if s.dim() != 2 or s.shape[0] < 1 or s.shape[1] < 1:
        raise RuntimeError("expected slots [B,S], got %s" % (tuple(s.shape),))
    B, S = int(s.shape[0]), int(s.shape[1])
    return acc_bank, alive, p, s, N, B, S, H, W


def multiview_depth(acc_bank, alive_bank, poses, slots, calib, depth_init=None, iters=4, scale_px=4.0, inlier_px=2.0, min_z=0.1,
                    min_views=2, max_rel_sigma=0.25, max_depth=80.0):
    """Depth of an anchor frame from its correspondences in several later frames at once: per pixel the inverse depth that
    minimises the robust (Geman-McClure, `scale_px`) reprojection error over all listed views, by `iters` Levenberg-Marquardt steps
    from the closed-form linear solution (or from `depth_init` where that costs less). `acc_bank` [N,2,H,W] float32: slot k is the
    flow from the anchor to some later frame on the anchor's grid (what `depth.FlowTrack.acc` holds after a step); `alive_bank`
    [N,H,W] uint8 or bool; `poses` ([N,12], [N,3,4] or [N,4,4]) anchor <- that frame, the convention of `two_view_depth`; `slots`
    [B,S] (a tensor on the bank's device or a host sequence; [S] for one problem), S <= 16: the views of problem b in list order, a
    slot < 0 or >= N is empty; `calib` is (fx, fy, cx, cy) or a calibration matrix without skew; `depth_init` [B,1,H,W] float32
    (0 = none) or None. Returns `(depth, info, views, counts)` on the bank's device: `depth` float32 [B,1,H,W], 0 = none; `info`
    float32 [B,1,H,W], the inverse variance of the RELATIVE depth for unit pixel noise (sigma_z / z = noise_px / sqrt(info));
    `views` uint8 [B,H,W], the views whose residual is within `inlier_px`; `counts` int32 [B,3] = (pixels observed in at least
    `min_views` views, pixels solved, pixels valid: at least `min_views` inliers, sigma_z / z <= `max_rel_sigma` at one pixel of
    noise, depth <= `max_depth`). A view the point lies behind (closer than `min_z` times its depth) costs as much as a residual of
    H + W pixels. Device tensors go through libatdn_hip's kernel on the current stream and the results stay on the device (no
    synchronisation); CPU tensors go through the library's host form. The rule is float64 and stated in full in
    include/atdn_hip.h, atdn_multiview_depth; the same inputs give the same bits on every call and on both paths."""
    from .depth import intrinsics
    acc_bank, alive, p, s, N, B, S, H, W = _flow_bank_inputs(acc_bank, alive_bank, poses, slots)
    device = acc_bank.device
    z0 = None
    if depth_init is not None:
        if not isinstance(depth_init, torch.Tensor) or depth_init.device != device:
            raise RuntimeError("bank on %s but depth_init on %s" % (device, getattr(depth_init, "device", "the host")))
        if depth_init.numel() != B * H * W or tuple(depth_init.shape[-2:]) != (H, W):
            raise RuntimeError("expected depth_init [%d,1,%d,%d], got %s" % (B, H, W, tuple(depth_init.shape)))
        z0 = depth_init.detach().float().contiguous()
    fx, fy, cx, cy = intrinsics(calib)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
    info = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
    views = torch.empty((B, H, W), dtype=torch.uint8, device=device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=device)
    _lib.call("atdn_multiview_depth", device, _ptr(acc_bank), _ptr(alive), _ptr(p), _ptr(s), _ptr(z0), N, B, S, H, W, fx, fy, cx, cy,
              float(scale_px), float(inlier_px), float(min_z), int(min_views), float(max_rel_sigma), float(max_depth), int(iters),
              _ptr(depth), _ptr(info), _ptr(views), _ptr(counts))
    return depth, info, views, counts


def bundle_sums(S):
    """The number of float64 sums `bundle_terms` returns per problem of S listed views: with n = 6 S, the n (n + 1) / 2 entries of
    T0, the n of v0, 27 per view (H_s, g_s) and the cost (include/atdn_hip.h, atdn_bundle_adjust)."""
    n = 6 * int(S)
    return n * (n + 1) // 2 + n + 27 * int(S) + 1


def _bundle_inputs(acc_bank, alive_bank, poses, slots, calib, depth_init, mask, stride, min_views):
    from .depth import intrinsics
    acc_bank, alive, p, s, N, B, S, H, W = _flow_bank_inputs(acc_bank, alive_bank, poses, slots)
    device = acc_bank.device
    if not isinstance(depth_init, torch.Tensor):
        raise RuntimeError("bundle adjustment needs an initial depth [B,1,H,W] (a tensor on the bank's device)")
    if depth_init.device != device:
        raise RuntimeError("bank on %s but depth_init on %s" % (device, depth_init.device))
    if depth_init.numel() != B * H * W or tuple(depth_init.shape[-2:]) != (H, W):
        raise RuntimeError("expected depth_init [%d,1,%d,%d], got %s" % (B, H, W, tuple(depth_init.shape)))
    z0 = depth_init.detach().float().contiguous()
    m = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != device:
            raise RuntimeError("bank on %s but mask on %s" % (device, getattr(mask, "device", "the host")))
        m = _byte_plane(mask, "a mask", B, H, W)
    if int(stride) < 1:
        raise RuntimeError("stride must be >= 1, got %r" % (stride,))
    fx, fy, cx, cy = intrinsics(calib)
    ptrs = (_ptr(acc_bank), _ptr(alive), _ptr(p), _ptr(s), _ptr(z0), _ptr(m), N, B, S, H, W, fx, fy, cx, cy, int(stride))
    return ptrs, (acc_bank, alive, p, s, z0, m), device, B, S, H, W


def _bundle_call(name, device, B, S, H, W, stride, *args):
    ws = _lib.workspace("atdn_bundle_workspace_bytes", device, B, S, H, W, int(stride),
                        message="bundle adjustment: batch, view count or image size out of range")
    _lib.call(name, device, *args, workspace=ws)


def bundle_terms(acc_bank, alive_bank, poses, slots, calib, depth, mask=None, stride=2, scale_px=4.0, inlier_px=2.0, min_z=0.1,
                 min_views=2):
    """One evaluation of the windowed bundle adjustment at the given poses and depth: the sums of the reduced normal equations
    and the cost, for scoring a window without solving it. Arguments as for `bundle_adjust`. Returns `(sums, counts)` on the
    bank's device: `sums` float64 [B, bundle_sums(S)] in the layout of include/atdn_hip.h (T0, v0, per view H_s and g_s, and last
    the cost), `counts` int32 [B,3] = (candidates, observations in front of their camera, those within `inlier_px`)."""
    ptrs, keep, device, B, S, H, W = _bundle_inputs(acc_bank, alive_bank, poses, slots, calib, depth, mask, stride, min_views)
    sums = torch.empty((B, bundle_sums(S)), dtype=torch.float64, device=device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=device)
    _bundle_call("atdn_bundle_terms", device, B, S, H, W, stride, *ptrs, float(scale_px), float(inlier_px), float(min_z),
                 int(min_views), _ptr(sums), _ptr(counts))
    return sums, counts


def bundle_adjust(acc_bank, alive_bank, poses, slots, calib, depth_init, mask=None, stride=2, iters=8, scale_px=4.0, inlier_px=2.0,
                  min_z=0.1, min_views=2):
    """Windowed dense bundle adjustment of an anchor frame's flow bank: the poses of the listed views and the inverse depths of
    the anchor's pixels, refined jointly by `iters` Levenberg-Marquardt steps on the robust (Geman-McClure, `scale_px`)
    reprojection error of every correspondence, the depths eliminated by the Schur complement. `acc_bank`, `alive_bank`, `poses`,
    `slots` and `calib` as for `multiview_depth` (the anchor's own pose is the frame of reference and is not refined); `depth_init`
    [B,1,H,W] float32 is mandatory; `mask` [B,H,W] (uint8 or bool) removes the pixels where it is 0. A pixel is a candidate when it
    lies on the grid of `stride`, the mask allows it, it has an initial depth and at least `min_views` listed views observe it.
    Scale is unobservable: the largest coordinate of the last listed view's translation (in that camera's frame) is held at its
    initial value. Returns `(poses, depth, cost, counts)` on the bank's device: `poses` float32 [B,S,12] in the convention of the
    input (an empty slot is all zeros; the inputs' rows if no step was accepted), `depth` float32 [B,1,H,W], the refined depth at
    the candidates and 0 elsewhere, `cost` float64 [B,2] = (initial, final), `counts` int32 [B,4] = (candidates, observations in
    front of their camera at the final state, those within `inlier_px`, accepted steps). Device tensors go through libatdn_hip's
    kernels on the current stream (2 (iters + 1) launches, no synchronisation); CPU tensors go through the library's host form.
    The rule is float64 and stated in full in include/atdn_hip.h, atdn_bundle_adjust; the same inputs give the same bits on every
    call and on both paths."""
    ptrs, keep, device, B, S, H, W = _bundle_inputs(acc_bank, alive_bank, poses, slots, calib, depth_init, mask, stride, min_views)
    poses_out = torch.empty((B, S, 12), dtype=torch.float32, device=device)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=device)
    cost = torch.empty((B, 2), dtype=torch.float64, device=device)
    counts = torch.empty((B, 4), dtype=torch.int32, device=device)
    _bundle_call("atdn_bundle_adjust", device, B, S, H, W, stride, *ptrs, int(iters), float(scale_px), float(inlier_px), float(min_z),
                 int(min_views), _ptr(poses_out), _ptr(depth), _ptr(cost), _ptr(counts))
    return poses_out, depth, cost, counts


def epipolar_score(counts):
    """float32 inliers / inside of the `counts` [B,3] (or [3]) of `two_view_depth`, 0 where no correspondence is inside: the
    share of the flow's correspondences that lie within `max_epipolar` pixels of the epipolar line the pose gives them. Exact
    integer counts divided in float64, then rounded; stays on the counts' device."""
    c = torch.as_tensor(counts)
    inside, inliers = c[..., 0].double(), c[..., 1].double()
    return torch.where(inside > 0, inliers / inside.clamp(min=1.0), torch.zeros_like(inside)).float()


def _pnp_inputs(depth, flow, pose, calib, mask, scale_px, inlier_px, min_z):
    """The checked, contiguous inputs of `reprojection_terms` and `pose_from_depth`, with the batch axis added to 3-d forms."""
    from .depth import intrinsics
    single, f, d, p, m, B, H, W = _flow_inputs(flow, pose, mask, depth=torch.as_tensor(depth))
    ptr = (_ptr(d), _ptr(f), _ptr(m), _ptr(p), B, H, W) + tuple(intrinsics(calib)) + (float(scale_px), float(inlier_px), float(min_z))
    return single, (d, f, m, p), ptr, B, H, W


def reprojection_terms(depth, flow, pose, calib, mask=None, scale_px=4.0, inlier_px=2.0, min_z=0.1):
    """How well a pose explains a depth map and a flow. `depth` [B,H,W] ([B,1,H,W] or [H,W]) is the depth of every pixel of
    image 1 in camera 1 (0 = none; what `two_view_depth` and the keyframe depth maps hold), `flow` [B,2,H,W] (or [2,H,W]) the flow
    from image 1 to image 2, `pose`, `calib` and `mask` as for `two_view_depth` (X1 = R X2 + t). Every pixel with a depth whose
    flow lands inside image 2 is a candidate; its 3-D point is moved into camera 2, projected, and compared with where the flow
    says it is. Returns `(sums, counts)` on the flow's device: `sums` float64 [B,28] ([28]) = the 21 upper-triangle entries of the
    Gauss-Newton Hessian, the 6 gradient entries and the cost of the reprojection error under the Geman-McClure loss of scale
    `scale_px`; `counts` int32 [B,3] ([3]) = (candidates, those at least `min_z` in front of camera 2, those within `inlier_px`
    pixels). `reprojection_score(counts)` is the share of inliers. Device tensors go through libatdn_hip's kernels on the current
    stream and the results stay on the device (no synchronisation); CPU tensors go through the library's host form. The rule is
    float64, fixes the order of every sum and is stated in full in include/atdn_hip.h, atdn_pnp_terms; the same inputs give the
    same bits on every call and on both paths."""
    single, keep, ptr, B, H, W = _pnp_inputs(depth, flow, pose, calib, mask, scale_px, inlier_px, min_z)
    dev = keep[1].device
    sums = torch.empty((B, 28), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.call("atdn_pnp_terms", dev, *ptr, _ptr(sums), _ptr(counts),
              workspace=_lib.workspace("atdn_pnp_workspace_bytes", dev, B, H, W))
    return (sums[0], counts[0]) if single else (sums, counts)


def reprojection_score(counts):
    """float32 inliers / candidates of the `counts` [B,3] or [B,4] (or [3], [4]) of `reprojection_terms` / `pose_from_depth`, 0
    where there is no candidate: the share of the depth's points that the pose projects within `inlier_px` pixels of where the
    flow puts them. Exact integer counts divided in float64, then rounded; stays on the counts' device."""
    c = torch.as_tensor(counts)
    cand, inliers = c[..., 0].double(), c[..., 2].double()
    return torch.where(cand > 0, inliers / cand.clamp(min=1.0), torch.zeros_like(cand)).float()


def pose_from_depth(depth, flow, pose_init, calib, mask=None, iters=16, scale_px=4.0, inlier_px=2.0, min_z=0.1):
    """The relative pose that a depth map and a flow determine (robust PnP): `iters` Levenberg-Marquardt steps from `pose_init` on
    the terms of `reprojection_terms`, every problem of the batch on its own, all on the device. Arguments as for
    `reprojection_terms`. Returns `(pose, cost, counts)` on the flow's device: `pose` float32 [B,4,4] ([4,4] for a 3-d flow) with
    X1 = R X2 + t, `cost` float64 [B] and `counts` int32 [B,4] = (candidates, used, inliers, accepted steps) at it. Where no step
    was accepted — a depth map of zeros, say — `pose` holds the bits of `pose_init`. 2 * (iters + 1) launches on the current
    stream and no synchronisation; CPU tensors go through the library's host form. The rule is stated in full in
    include/atdn_hip.h, atdn_pnp_solve; the same inputs give the same bits on every call and on both paths."""
    single, keep, ptr, B, H, W = _pnp_inputs(depth, flow, pose_init, calib, mask, scale_px, inlier_px, min_z)
    dev = keep[1].device
    rows = torch.empty((B, 12), dtype=torch.float32, device=dev)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("atdn_pnp_solve", dev, *ptr, int(iters), _ptr(rows), _ptr(cost), _ptr(counts),
              workspace=_lib.workspace("atdn_pnp_workspace_bytes", dev, B, H, W))
    pose = _pose_matrices(rows)
    return (pose[0], cost[0], counts[0]) if single else (pose, cost, counts)


def _epipolar_inputs(flow, pose, calib, mask, scale_px, inlier_px):
    """The checked, contiguous inputs of `epipolar_terms` and `pose_from_flow`, with the batch axis added to 3-d forms."""
    from .depth import intrinsics
    single, f, _, p, m, B, H, W = _flow_inputs(flow, pose, mask)
    ptr = (_ptr(f), _ptr(m), _ptr(p), B, H, W) + tuple(intrinsics(calib)) + (float(scale_px), float(inlier_px))
    return single, (f, m, p), ptr, B, H, W


def epipolar_terms(flow, pose, calib, mask=None, scale_px=2.0, inlier_px=1.0):
    """How well a pose explains a flow, without any depth. `flow` [B,2,H,W] (or [2,H,W]) is the flow from image 1 to image 2,
    `pose`, `calib` and `mask` as for `two_view_depth` (X1 = R X2 + t). Every pixel whose flow lands inside image 2 is a candidate;
    its signed pixel distance from the epipolar line the pose gives it is the residual. Returns `(sums, counts)` on the flow's
    device: `sums` float64 [B,28] ([28]) = the 21 upper-triangle entries of the Gauss-Newton Hessian, the 6 gradient entries —
    over a rotation step and a ROTATION of the translation: its length is not observable and never changes — and the cost under
    the Geman-McClure loss of scale `scale_px`; `counts` int32 [B,3] ([3]) = (candidates, those with a line, those within
    `inlier_px` pixels of it). `counts[:, 2] / counts[:, 0]` is the share of inliers: these are not the counts of `two_view_depth`,
    so `epipolar_score` is not for them. Device tensors go through libatdn_hip's kernels on the current stream and the results
    stay on the device (no synchronisation); CPU tensors go through the library's host form. The rule is float64, fixes the order
    of every sum and is stated in full in include/atdn_hip.h, atdn_epipolar_terms; the same inputs give the same bits on every
    call and on both paths."""
    single, keep, ptr, B, H, W = _epipolar_inputs(flow, pose, calib, mask, scale_px, inlier_px)
    dev = keep[0].device
    sums = torch.empty((B, 28), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.call("atdn_epipolar_terms", dev, *ptr, _ptr(sums), _ptr(counts),
              workspace=_lib.workspace("atdn_epipolar_workspace_bytes", dev, B, H, W))
    return (sums[0], counts[0]) if single else (sums, counts)


def pose_from_flow(flow, pose_init, calib, mask=None, iters=16, scale_px=2.0, inlier_px=1.0):
    """The relative pose refined on the flow alone: `iters` Levenberg-Marquardt steps from `pose_init` on the terms of
    `epipolar_terms`, every problem of the batch on its own, all on the device. Arguments as for `epipolar_terms`. Returns
    `(pose, cost, counts)` on the flow's device: `pose` float32 [B,4,4] ([4,4] for a 3-d flow) with X1 = R X2 + t — the rotation
    and the DIRECTION of t are refined, |t| is `pose_init`'s up to float32 rounding —, `cost` float64 [B] and `counts` int32 [B,4]
    = (candidates, used, inliers, accepted steps) at it; `counts[:, 2] / counts[:, 0]` is the share of inliers. Where no step was
    accepted — t = 0, an all-zero mask, a NaN in the pose — `pose` holds the bits of `pose_init`. This is a refinement from a pose
    that is near (the pose head's), not a global solver: the cost is blind to the sign of t and to the twisted pair. Small images
    with many outliers converge slowly (the rotation/translation valley of a forward motion is flat under a redescending loss):
    give them more `iters`. 2 * (iters + 1) launches on the current stream and no synchronisation; CPU tensors go through the
    library's host form. The rule is stated in full in include/atdn_hip.h, atdn_epipolar_solve; the same inputs give the same
    bits on every call and on both paths."""
    single, keep, ptr, B, H, W = _epipolar_inputs(flow, pose_init, calib, mask, scale_px, inlier_px)
    dev = keep[0].device
    rows = torch.empty((B, 12), dtype=torch.float32, device=dev)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call("atdn_epipolar_solve", dev, *ptr, int(iters), _ptr(rows), _ptr(cost), _ptr(counts),
              workspace=_lib.workspace("atdn_epipolar_workspace_bytes", dev, B, H, W))
    pose = _pose_matrices(rows)
    return (pose[0], cost[0], counts[0]) if single else (pose, cost, counts)


# The defaults of the ground-plane fit ("Ground plane"): choices, not measurements.
GROUND_DEFAULTS = dict(scale_rel=0.05, inlier_rel=0.05, min_z=0.1, max_depth=80.0, min_votes=64)


def ground_rows(calib, H):
    """The default row band of the ground-plane functions: the rows below the principal point, `(floor(cy) + 1, H)` — a level
    camera sees the road only there. (A principal point below the image leaves no row: the library refuses the band.)"""
    from .depth import intrinsics
    cy = intrinsics(calib)[3]
    return max(int(math.floor(cy)) + 1, 0), H


def _ground_inputs(depth, calib, mask, rows, q=None):
    """The checked, contiguous inputs of the ground-plane functions, with the batch axis added to an [H,W] depth: (single, kept
    tensors, leading ctypes arguments up to cy, B, H, W, (y0, y1))."""
    from .depth import intrinsics
    d = torch.as_tensor(depth)
    if d.dim() not in (2, 3, 4) or (d.dim() == 4 and d.shape[1] != 1):
        raise RuntimeError("expected a depth [H,W], [B,H,W] or [B,1,H,W], got %s" % (tuple(d.shape),))
    single = d.dim() == 2
    H, W = (int(v) for v in d.shape[-2:])
    B = 1 if single else int(d.shape[0])
    d = d.detach().float().contiguous()
    m = None
    if mask is not None:
        m = _byte_plane(torch.as_tensor(mask), "a mask", B, H, W)
        if m.device != d.device:
            raise RuntimeError("depth on %s but mask on %s" % (d.device, m.device))
    qq = None
    if q is not None:
        qq = torch.as_tensor(q)
        if qq.numel() != 3 * B or qq.shape[-1] != 3:
            raise RuntimeError("expected q of %d x 3 values, got %s" % (B, tuple(qq.shape)))
        if qq.device != d.device:
            raise RuntimeError("depth on %s but q on %s" % (d.device, qq.device))
        qq = qq.detach().to(torch.float64).contiguous()
    y0, y1 = ground_rows(calib, H) if rows is None else (int(rows[0]), int(rows[1]))
    ptr = (_ptr(d), _ptr(m), _ptr(qq), B, H, W, y0, y1) + tuple(intrinsics(calib))
    return single, (d, m, qq), ptr, B, H, W, (y0, y1)


def ground_terms(depth, q, calib, mask=None, rows=None, scale_rel=GROUND_DEFAULTS["scale_rel"],
                 inlier_rel=GROUND_DEFAULTS["inlier_rel"], min_z=GROUND_DEFAULTS["min_z"], max_depth=GROUND_DEFAULTS["max_depth"]):
    """How well a plane explains the lower part of a depth map. `depth` [B,H,W] ([B,1,H,W] or [H,W]) as a keyframe depth map holds
    it, `q` [B,3] ([3]) float64 = normal / height of the plane n . X = height in the camera frame (y down: a level camera 1.65 m
    over the road has q = (0, 1/1.65, 0)), `calib` and `mask` as for `two_view_depth`, `rows` = (y0, y1) the band of image rows
    to look at (None: `ground_rows`, the rows below the principal point). A pixel of the band that the mask keeps is a candidate;
    it is used if its depth is finite and in [min_z, max_depth]. Its residual is the RELATIVE depth error e = z (q . ray) - 1.
    Returns `(sums, counts)` on the depth's device: `sums` float64 [B,10] ([10]) = the 6 upper-triangle entries of the 3 x 3
    Gauss-Newton Hessian, the 3 gradient entries and the cost of e under the Geman-McClure loss of scale `scale_rel`; `counts`
    int32 [B,3] ([3]) = (candidates, used, those with |e| <= inlier_rel). Device tensors go through libatdn_hip's kernels on the
    current stream (no synchronisation); CPU tensors go through the library's host form. The rule is float64, fixes the order of
    every sum and is stated in full in include/atdn_hip.h, atdn_ground_terms; the same bits on every call and on both paths."""
    if q is None:
        raise RuntimeError("ground_terms needs q")
    single, keep, ptr, B, H, W, _ = _ground_inputs(depth, calib, mask, rows, q)
    dev = keep[0].device
    sums = torch.empty((B, 10), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int32, device=dev)
    _lib.call("atdn_ground_terms", dev, *ptr, float(scale_rel), float(inlier_rel), float(min_z), float(max_depth), _ptr(sums),
              _ptr(counts), workspace=_lib.workspace("atdn_ground_workspace_bytes", dev, B, H, W))
    return (sums[0], counts[0]) if single else (sums, counts)


def ground_plane(depth, calib, normal_prior=(0.0, 1.0, 0.0), q_init=None, mask=None, rows=None, iters=8,
                 scale_rel=GROUND_DEFAULTS["scale_rel"], inlier_rel=GROUND_DEFAULTS["inlier_rel"], min_z=GROUND_DEFAULTS["min_z"],
                 max_depth=GROUND_DEFAULTS["max_depth"], min_votes=GROUND_DEFAULTS["min_votes"]):
    """The ground plane of a depth map: a start from a vote, then `iters` Levenberg-Marquardt steps on the terms of `ground_terms`,
    every problem of the batch on its own, all on the device. Arguments as for `ground_terms`. The vote: nothing lies below the
    road, so under `normal_prior` (the road's normal in the camera frame, y down; any length) the ground pixels share one height
    and everything else spreads over smaller ones; the mode of a histogram of these heights (320 bins of 1.6 .. 3.1 % over
    [1/16, 64), smoothed over three bins) starts the solve, and a mode of fewer than `min_votes` pixels means there is no plane. A
    robust fit alone, started from least squares, settles between the road and what stands on it; from the mode it does not.
    `q_init` [B,3] float64 replaces the vote. Returns `(q, sums, counts)` on the depth's device: `q` float64 [B,3] = normal /
    height (`ground_height` splits it), `sums` float64 [B,10] the terms at it, `counts` int32 [B,6] = (candidates, used, inliers,
    accepted steps, votes of the mode, mode bin; the bin is -1 with `q_init`). No plane: q = 0, sums = 0 and all counts 0.
    2 + 2 * (iters + 1) launches on the current stream and no synchronisation; CPU tensors go through the library's host form.
    The rule is stated in full in include/atdn_hip.h, atdn_ground_solve; the same bits on every call and on both paths."""
    single, keep, ptr, B, H, W, _ = _ground_inputs(depth, calib, mask, rows, q_init)
    dev = keep[0].device
    n0 = [float(v) for v in torch.as_tensor(normal_prior, dtype=torch.float64).reshape(-1).tolist()]
    if len(n0) != 3:
        raise RuntimeError("expected a prior normal of 3 values, got %d" % len(n0))
    q = torch.empty((B, 3), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 10), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 6), dtype=torch.int32, device=dev)
    _lib.call("atdn_ground_solve", dev, *ptr, *n0, float(scale_rel), float(inlier_rel), float(min_z), float(max_depth),
              int(min_votes), int(iters), _ptr(q), _ptr(sums), _ptr(counts),
              workspace=_lib.workspace("atdn_ground_workspace_bytes", dev, B, H, W))
    return (q[0], sums[0], counts[0]) if single else (q, sums, counts)


def ground_classify(depth, q, calib, mask=None, rows=None, inlier_rel=GROUND_DEFAULTS["inlier_rel"],
                    min_z=GROUND_DEFAULTS["min_z"], max_depth=GROUND_DEFAULTS["max_depth"]):
    """The road map of a depth map under the plane `q`: `(residual, on_ground)` on the depth's device, `residual` float32
    [B,1,H,W] ([1,H,W] for an [H,W] depth) = e of `ground_terms` at every used pixel of the band, 0 elsewhere — the pixel stands
    -height * e above the road —, `on_ground` uint8 [B,H,W] ([H,W]) = 1 where |e| <= inlier_rel. Both are zero outside the band.
    One launch on the current stream; CPU tensors go through the library's host form (include/atdn_hip.h, atdn_ground_classify)."""
    if q is None:
        raise RuntimeError("ground_classify needs q")
    single, keep, ptr, B, H, W, _ = _ground_inputs(depth, calib, mask, rows, q)
    dev = keep[0].device
    residual = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    on_ground = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    _lib.call("atdn_ground_classify", dev, *ptr, float(inlier_rel), float(min_z), float(max_depth), _ptr(residual), _ptr(on_ground))
    return (residual[0], on_ground[0]) if single else (residual, on_ground)


def ground_height(q):
    """`(normal, height)` of `q` [B,3] (or [3]) = normal / height: normal = q / |q| float64 [B,3], height = 1 / |q| float64 [B]; both
    0 where q = 0 (no plane). Stays on q's device."""
    q = torch.as_tensor(q).to(torch.float64)
    norm = torch.sqrt((q * q).sum(-1))
    some = norm > 0
    safe = torch.where(some, norm, torch.ones_like(norm))
    return torch.where(some[..., None], q / safe[..., None], torch.zeros_like(q)), torch.where(some, 1.0 / safe, torch.zeros_like(norm))


def ground_sigma(q, sums):
    """The relative standard deviation of the fitted height per unit of relative depth noise: with H the 3 x 3 Hessian of `sums`
    [B,10] (or [10]) at `q`, height = 1 / |q| moves by -height (q . dq) / |q|^2, so sigma = sqrt(u^T H^-1 u) with u = q / |q|^2.
    A depth whose relative noise is s gives the height to s * sigma (relative). float64 [B]; inf where q = 0 or H is singular."""
    q = torch.as_tensor(q).to(torch.float64)
    S = torch.as_tensor(sums).to(torch.float64)
    a, b, c, d, e, f = (S[..., i] for i in range(6))                     # H = [[a, b, c], [b, d, e], [c, e, f]]
    co = torch.stack([d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b], -1)   # adj(H), upper
    det = a * co[..., 0] + b * co[..., 1] + c * co[..., 2]
    n2 = (q * q).sum(-1)
    ok = (det > 0) & (n2 > 0)
    u = q / torch.where(ok, n2, torch.ones_like(n2))[..., None]
    quad = (co[..., 0] * u[..., 0] ** 2 + co[..., 3] * u[..., 1] ** 2 + co[..., 5] * u[..., 2] ** 2 +
            2.0 * (co[..., 1] * u[..., 0] * u[..., 1] + co[..., 2] * u[..., 0] * u[..., 2] + co[..., 4] * u[..., 1] * u[..., 2]))
    var = quad / torch.where(ok, det, torch.ones_like(det))
    return torch.where(ok & (var >= 0), torch.sqrt(var.clamp(min=0.0)), torch.full_like(var, float("inf")))


def ground_accept(q, counts, normal_prior=(0.0, 1.0, 0.0), min_inlier_share=0.2, max_tilt_deg=10.0):
    """Whether a fitted plane is believed (bool [B], or a scalar tensor for one plane): there is one, the share of inliers among
    the used pixels (`counts` of `ground_plane`) is at least `min_inlier_share`, and its normal is within `max_tilt_deg` degrees
    of `normal_prior`. float64 on q's device."""
    normal, _ = ground_height(q)
    c = torch.as_tensor(counts)
    n0 = torch.as_tensor(normal_prior, dtype=torch.float64, device=normal.device).reshape(3)
    cos = (normal * (n0 / torch.sqrt((n0 * n0).sum()))).sum(-1)
    used, inliers = c[..., 1].double(), c[..., 2].double()
    share = torch.where(used > 0, inliers / used.clamp(min=1.0), torch.zeros_like(used))
    return (used > 0) & (share >= float(min_inlier_share)) & (cos >= math.cos(math.radians(float(max_tilt_deg))))


def ground_record(depth, calib, options=None, accept=None, camera_height=None):
    """The ground of one depth image [1,1,H,W], as a keyframe's `ground/%06d.pth` holds it: `ground_plane` (`options` its keyword
    arguments) on the depth's device, then on the host `q`, `sums`, `counts` of the one image, `normal` and `height`
    (`ground_height`), `accepted` (bool: `ground_accept`, `accept` its thresholds) and `scale` (float: `camera_height` / height
    when accepted and a `camera_height` is given, 1.0 otherwise)."""
    options = dict(options or {})
    q, sums, counts = ground_plane(depth, calib, **options)
    q, sums, counts = q[0].to("cpu"), sums[0].to("cpu"), counts[0].to("cpu")
    normal, height = ground_height(q)
    accepted = bool(ground_accept(q, counts, options.get("normal_prior", (0.0, 1.0, 0.0)), **(accept or {})))
    scale = float(camera_height) / float(height) if accepted and camera_height is not None else 1.0
    return dict(q=q, normal=normal, height=height, sums=sums, counts=counts, accepted=accepted, scale=scale)


def flow_track_step(flow, acc, alive, pose=None, calib=None, mask=None, depth=None, max_epipolar=1.0, min_parallax_deg=0.05,
                    max_depth=80.0, out=None):
    """One step of a flow track: the correspondences of an anchor frame's pixels carried one frame further and, given a pose,
    triangulated over the whole interval. `acc` [B,2,H,W] (or [2,H,W]) is the flow from the anchor to frame k on the anchor's grid
    (zeros at the start of a track), `alive` (uint8 or bool, [B,H,W], [B,1,H,W] or [H,W]) says which pixels still have a track,
    `flow` [B,2,H,W] (or [2,H,W]) is the flow from frame k to frame k+1, channel 0 = x. The step reads `flow` bilinearly where each
    track stands and adds it: acc(k+1) = acc(k) + flow(p + acc(k)). A track dies — for good — when it leaves the image, meets a
    NaN or an infinity, or stands (nearest pixel) where `mask` (as for `two_view_depth`, on frame k's grid; e.g. the mask of
    `flow_consistency` of that pair) is 0; a dead pixel keeps its `acc`. With `pose` — anchor <- frame k+1, X_anchor = R X + t, in
    any form `two_view_depth` takes, the product of the pairs' relative poses — and `calib`, the new `acc` is triangulated by the
    two-view rule and the depth is written where it is valid; elsewhere `depth` keeps what it had, so after several steps every
    pixel carries the triangulation of the last step at which it was valid. `depth` (float32 contiguous [B,1,H,W], or [1,H,W]) is
    updated in place; None starts from zeros. Without `pose` the chain alone is advanced (`depth` and `calib` must be None).
    Returns `(acc, alive, depth or None, counts)`: acc float32, alive uint8 [B,H,W] of 0 and 1, counts int32 [B,4] = (alive,
    inside, inliers, valid), the last three as in `two_view_depth` (0 without a pose); a 3-d flow gives [2,H,W], [H,W], [1,H,W], [4].
    `out=(acc_out, alive_out)` or `(acc_out, alive_out, counts_out)` names the tensors to write (float32 / uint8 / int32,
    contiguous); `out=(acc, alive)` updates the state in place. Device tensors go through libatdn_hip's kernel on the current stream
    and the results stay on the device (no synchronisation); CPU tensors go through the library's host form. The rule is float64
    and stated in full in include/atdn_hip.h, atdn_flow_track_step; the same inputs give the same bits on every call and on
    both paths."""
    from .depth import intrinsics
    if flow.dim() not in (3, 4) or flow.shape[-3] != 2:
        raise RuntimeError("expected a flow [2,H,W] or [B,2,H,W], got %s" % (tuple(flow.shape),))
    single = flow.dim() == 3
    f = (flow[None] if single else flow).detach().float().contiguous()
    B, _, H, W = f.shape
    dev = f.device

    def same_device(t, what):
        if t.device != dev:
            raise RuntimeError("flow on %s but %s on %s" % (dev, what, t.device))
        return t

    def bytes_of(t, what):
        return _byte_plane(same_device(torch.as_tensor(t), what), what, B, H, W)

    a = same_device(torch.as_tensor(acc), "acc")
    if tuple(a.shape) != ((2, H, W) if single else (B, 2, H, W)):
        raise RuntimeError("expected acc of the flow's shape %s, got %s" % (tuple(flow.shape), tuple(a.shape)))
    a = a.detach().float().contiguous()
    live = bytes_of(alive, "alive")
    m = None if mask is None else bytes_of(mask, "a mask")
    if pose is None:
        if depth is not None or calib is not None:
            raise RuntimeError("depth and calib need a pose: without one only the chain is advanced")
        p, d = None, None
        fx = fy = cx = cy = min_sin2 = 0.0
    else:
        if calib is None:
            raise RuntimeError("a pose needs the calibration")
        p = _pose_rows(pose, B, dev)
        fx, fy, cx, cy = intrinsics(calib)
        min_sin2 = _min_sin2(min_parallax_deg)
        if depth is None:
            d = torch.zeros((B, 1, H, W), dtype=torch.float32, device=dev)
        else:
            d = same_device(depth, "depth")
            if d.dtype != torch.float32 or not d.is_contiguous() or d.numel() != B * H * W or tuple(d.shape[-2:]) != (H, W):
                raise RuntimeError("depth is updated in place: expected contiguous float32 [%d,1,%d,%d], got %s %s"
                                   % (B, H, W, d.dtype, tuple(d.shape)))
    if out is None:
        a_out = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        l_out = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    else:
        if len(out) not in (2, 3):
            raise RuntimeError("out is (acc_out, alive_out) or (acc_out, alive_out, counts_out)")
        a_out, l_out = out[0], out[1]
        counts = out[2] if len(out) == 3 else torch.empty((B, 4), dtype=torch.int32, device=dev)
        for t, dt, count, what in ((a_out, torch.float32, B * 2 * H * W, "acc_out"), (l_out, torch.uint8, B * H * W, "alive_out"),
                                   (counts, torch.int32, B * 4, "counts_out")):
            same_device(t, what)
            if t.dtype != dt or not t.is_contiguous() or t.numel() != count:
                raise RuntimeError("%s must be contiguous %s of %d values, got %s %s" % (what, dt, count, t.dtype, tuple(t.shape)))
    _lib.call("atdn_flow_track_step", dev, _ptr(f), _ptr(m), _ptr(a), _ptr(live), B, H, W, _ptr(a_out), _ptr(l_out), _ptr(p), fx, fy,
              cx, cy, float(max_epipolar), min_sin2, float(max_depth), _ptr(d), _ptr(counts))
    d_ret = depth if depth is not None else (None if d is None else (d[0] if single else d))
    if out is not None:
        return a_out, l_out, d_ret, counts
    if single:
        return a_out[0], l_out[0], d_ret, counts[0]
    return a_out, l_out, d_ret, counts


def _graph_rows(x, what):
    """Poses [n,4,4], [n,3,4] or [n,12], or those with a batch axis in front -> (float32 [B,n,12] on x's device, batched)."""
    p = torch.as_tensor(x)
    if p.dim() >= 3 and tuple(p.shape[-2:]) in ((4, 4), (3, 4)):
        p = p[..., :3, :].reshape(tuple(p.shape[:-2]) + (12,))
    if p.dim() not in (2, 3) or p.shape[-1] != 12:
        raise RuntimeError("expected %s [n,4,4], [n,3,4] or [n,12], or batched, got %s" % (what, tuple(torch.as_tensor(x).shape)))
    batched = p.dim() == 3
    return (p if batched else p[None]).detach().float().contiguous(), batched


def _pose_graph_inputs(poses, edge_index, edge_pose, edge_weight, edge_robust, fixed, robust_scale):
    """The checked, contiguous inputs of `pose_graph_terms` and `pose_graph_optimize`, with the batch axis added."""
    p, batched = _graph_rows(poses, "poses")
    dev = p.device
    B, N = p.shape[:2]
    z, zb = _graph_rows(edge_pose, "edge poses")
    E = z.shape[1]

    def arg(t, shape, dtype, what):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.device != dev:
            raise RuntimeError("poses on %s but %s on %s" % (dev, what, t.device))
        if t.dim() == len(shape) - 1:
            t = t[None]
        if tuple(t.shape) != shape:
            raise RuntimeError("expected %s of shape %s, got %s" % (what, shape, tuple(t.shape)))
        if dtype == torch.uint8 and t.dtype != torch.uint8:
            t = t != 0
        return t.detach().to(dtype).contiguous()

    if z.device != dev or z.shape[0] != B or zb != batched:
        raise RuntimeError("expected edge poses [%s%d,12] on %s" % ("%d," % B if batched else "", E, dev))
    idx = arg(edge_index, (B, 2, E), torch.int32, "edge_index")
    w = arg(edge_weight, (B, E, 2), torch.float64, "edge_weight")
    if idx is None or w is None:
        raise RuntimeError("edge_index and edge_weight are required")
    rob = arg(edge_robust, (B, E), torch.uint8, "edge_robust")
    fix = arg(fixed, (B, N), torch.uint8, "fixed")
    return batched, dev, (B, N, E), (p, idx, z, w, rob, fix)


def pose_graph_terms(poses, edge_index, edge_pose, edge_weight, edge_robust=None, robust_scale=None):
    """The cost of a pose graph at given poses. `poses` [N,4,4], [N,3,4] or [N,12] (or with a batch axis in front: B graphs of the
    same N and E, each on its own) are the nodes, world <- camera, as `KeyframeMap.poses` holds them. `edge_index` [2,E] integers:
    edge e joins node i = edge_index[0,e] and j = edge_index[1,e]; `edge_pose` [E,4,4] (or [E,12]) its measurement of
    T_i^-1 T_j — what `transform(rot, tr)` of the pair (image i, image j) and `pose_from_depth` return; `edge_weight` [E,2] =
    (w_rot, w_tr) >= 0, 1/sigma^2 in rad^-2 and m^-2; `edge_robust` [E] marks the edges under the Geman-McClure loss of scale
    `robust_scale` (in sigmas; None = 1). Returns `(cost, edge_chi2, counts)` on the poses' device: `cost` float64 [B] (or a
    scalar), `edge_chi2` float64 [B,E] = w_rot |a|^2 + w_tr |te|^2 of every edge (a: the chordal rotation error, te: the
    translation error; +0.0 for an absent edge) and `counts` int32 [B,2] = (valid edges, absent ones: an index outside [0, N),
    i == j or a weight that is not >= 0). Device tensors go through libatdn_hip's kernel on the current stream (one launch, no
    synchronisation), CPU tensors through the library's host form. The rule is float64, fixes the order of every sum and is
    stated in full in include/atdn_hip.h, atdn_pose_graph_terms; the same bits on every call and on both paths."""
    batched, dev, (B, N, E), t = _pose_graph_inputs(poses, edge_index, edge_pose, edge_weight, edge_robust, None, robust_scale)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    chi2 = torch.empty((B, E), dtype=torch.float64, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    _lib.call("atdn_pose_graph_terms", dev, *(_ptr(x) for x in t[:5]), B, N, E, 1.0 if robust_scale is None else float(robust_scale),
              _ptr(cost), _ptr(chi2), _ptr(counts), workspace=_lib.workspace("atdn_pose_graph_workspace_bytes", dev, B, N, E))
    return (cost, chi2, counts) if batched else (cost[0], chi2[0], counts[0])


def pose_graph_optimize(poses, edge_index, edge_pose, edge_weight, edge_robust=None, robust_scale=None, fixed=None, iters=10,
                        cg_iters=64, cg_tol=1e-8):
    """The poses that agree best with the edges of a pose graph (loop closure): `iters` Levenberg-Marquardt steps from `poses`,
    each a conjugate-gradient solve (at most `cg_iters` iterations, to a relative residual `cg_tol`) preconditioned by the
    block-tridiagonal part of the system, every graph of the batch in its own workgroup, all in one launch. Arguments as for
    `pose_graph_terms`; `fixed` [N] marks the nodes that are held (default: node 0, the gauge). `robust_scale` may be a sequence,
    large to small: the graph is solved with each scale in turn, each from the last result — the Geman-McClure loss only works
    when the drift at a loop is within its scale; far beyond it every robust edge saturates and nothing moves.
    Returns `(poses, cost, edge_chi2, counts)` on the poses' device: `poses` float32 in the shape of the input (4 x 4 inputs come
    back 4 x 4 with the last row copied), `cost` float64 [B,2] ([2]) = (the cost at the input — of the last scale —, the cost
    reached), `edge_chi2` float64 [B,E] at the returned poses, `counts` int32 [B,4] = (valid edges, absent edges, accepted
    steps, CG iterations; the last two summed over a sequence of scales). A held node, and one without an edge of positive weight,
    comes back with its input bits; so does every node when no step is accepted. An edge of weight (0, 0) gives the same bits as
    the list without it. CPU tensors go through the library's host form. The rule is stated in full in include/atdn_hip.h,
    atdn_pose_graph_solve; the same inputs give the same bits on every call and on both paths."""
    batched, dev, (B, N, E), t = _pose_graph_inputs(poses, edge_index, edge_pose, edge_weight, edge_robust, fixed, robust_scale)
    p, idx, z, w, rob, fix = t
    if fix is None:
        fix = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        fix[:, 0] = 1
    scales = [1.0] if robust_scale is None else [float(s) for s in (robust_scale if isinstance(robust_scale, (list, tuple))
                                                                    else [robust_scale])]
    if not scales:
        raise RuntimeError("robust_scale is an empty sequence")
    total = None
    for scale in scales:
        rows = torch.empty((B, N, 12), dtype=torch.float32, device=dev)
        cost = torch.empty((B, 2), dtype=torch.float64, device=dev)
        chi2 = torch.empty((B, E), dtype=torch.float64, device=dev)
        counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
        _lib.call("atdn_pose_graph_solve", dev, _ptr(p), _ptr(idx), _ptr(z), _ptr(w), _ptr(rob), _ptr(fix), B, N, E, scale, int(iters),
                  int(cg_iters), float(cg_tol), _ptr(rows), _ptr(cost), _ptr(chi2), _ptr(counts),
                  workspace=_lib.workspace("atdn_pose_graph_workspace_bytes", dev, B, N, E))
        if total is not None:
            counts[:, 2:] += total[:, 2:]
        total = counts
        p = rows
    src = torch.as_tensor(poses)
    if src.shape[-1] == 12:
        out = rows.view(src.shape)
    else:
        out = src.detach().float().clone()
        out[..., :3, :] = rows.view(tuple(src.shape[:-2]) + (3, 4))
    return (out, cost, chi2, total) if batched else (out, cost[0], chi2[0], total[0])


def voxel_map(depth, poses, calib, images=None, mask=None, indices=None, stride=1, min_count=1, **options):
    """Depth maps and their cameras as ONE voxel-hashed point cloud, in one call: `voxel_map.VoxelMap(depth.device, **options)`
    (voxel, origin, min_z, max_z, capacity), its `integrate(depth, poses, calib, images, mask, indices, stride)` and its
    `extract(min_count)`, where the arguments are described. Returns `(points [M,3] float32, colors [M,3] uint8 or None, counts
    [M] int32, keys [M] int64)` on the depth's device, in ascending key order. Device tensors go through libatdn_hip's kernels,
    CPU tensors through the library's host form; the rule is integer and float64 and stated in full in include/atdn_hip.h: the
    same inputs give the same bits on every call and on both paths."""
    from .voxel_map import VoxelMap
    if not isinstance(depth, torch.Tensor):
        raise RuntimeError("expected a depth bank [N,H,W], got %s" % (type(depth).__name__,))
    m = VoxelMap(depth.device, **options)
    m.integrate(depth, poses, calib, images=images, mask=mask, indices=indices, stride=stride)
    return m.extract(min_count)


def render_points(points, colors, counts, poses, calib, hw, size, splat=1.0, max_splat=64, near=0.5, far=40.0, min_count=1):
    """A point cloud seen from B cameras, with a z-buffer: the inverse of `voxel_map`. `points` [M,3] float32, `colors` [M,3]
    uint8 or None and `counts` [M] int32 are what `VoxelMap.extract` returns or `VoxelMap.load_ply` reads (M = 0 is fine);
    `poses` ([B,12], [B,3,4] or [B,4,4]; rows of [R|t], world <- camera) the cameras, `calib` (fx, fy, cx, cy) or a calibration
    matrix without skew, `hw` = (H, W) the image size. A point with at least `min_count` support and near <= z <= far is a flat
    square splat of `splat` voxel edges of `size` (at least one pixel, at most `max_splat` pixels a side); a pixel shows the
    nearest splat that covers it, among equal depths the better supported one. Returns `(depth [B,H,W] float32, colors
    [B,3,H,W] uint8 or None, support [B,H,W] uint8 = min(count, 255) of the winner, counts [B,3] int64 = candidates, visible
    points, covered pixels)` on the points' device, zeros at empty pixels. Device tensors go through libatdn_hip's kernels on the
    current stream (no synchronisation), CPU tensors through the library's host form. The rule is float64 and an integer
    minimum, stated in full in include/atdn_hip.h, atdn_view_render: the same bits on every call and on both paths."""
    from .depth import intrinsics
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("expected points [M,3], got %s" % (tuple(getattr(points, "shape", ())),))
    dev = points.device
    M = int(points.shape[0])
    pts = points.detach().to(torch.float32).contiguous()
    if not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (M,) or counts.device != dev:
        raise RuntimeError("expected counts [%d] on %s" % (M, dev))
    cnt = counts.detach().to(torch.int32).contiguous()
    col = None
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or colors.dtype != torch.uint8 or tuple(colors.shape) != (M, 3) or colors.device != dev:
            raise RuntimeError("expected colors [%d,3] uint8 on %s" % (M, dev))
        col = colors.detach().contiguous()
    p = torch.as_tensor(poses)
    if p.device != dev and isinstance(poses, torch.Tensor):
        raise RuntimeError("points on %s but poses on %s" % (dev, p.device))
    B = 1 if tuple(p.shape) in ((4, 4), (3, 4), (12,)) else int(p.shape[0])
    p = _pose_rows(p, B, dev)
    H, W = int(hw[0]), int(hw[1])
    work = _lib.workspace("atdn_view_workspace_bytes", dev, B, H, W,
                          message="render_points: B, H, W must be >= 1, B <= 65535 and B * H * W < 2^31")
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    out_colors = None if col is None else torch.empty((B, 3, H, W), dtype=torch.uint8, device=dev)
    support = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    out_counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
    _lib.call("atdn_view_render", dev, _ptr(pts) if M else None, _ptr(col) if M else None, _ptr(cnt) if M else None, M, _ptr(p), B,
              H, W, *intrinsics(calib), float(size), float(splat), int(max_splat), float(near), float(far), int(min_count),
              _ptr(depth), _ptr(out_colors), _ptr(support), _ptr(out_counts), workspace=work)
    return depth, out_colors, support, out_counts


def visibility_votes(points, depth, poses, calib, indices=None, near=0.5, far=40.0, rel=0.05, abs_tol=0.25, radius=1, out=None):
    """Per point of a cloud, how many keyframes have it in view, confirm it and see straight through it. `points` [M,3] float32 is
    what `VoxelMap.extract` returns or `VoxelMap.load_ply` reads (M = 0 is fine); `depth` [N,H,W] float32 and `poses` ([N,12],
    [N,3,4] or [N,4,4]; rows of [R|t], world <- camera) are banks of N keyframes, `calib` (fx, fy, cx, cy) or a calibration
    matrix without skew. `indices` (integers, host or on the device) lists the keyframes that vote — the whole bank by default;
    an index outside the bank casts no vote, a repeat votes again. A point with near <= z <= far in a keyframe whose pixel lies
    at least `radius` pixels inside the image is IN VIEW; with band = rel * z + abs_tol it has SUPPORT where the pixel's depth
    lies within z -+ band, and is FREE where every depth of the (2 radius + 1)^2 window is measured (within [near, far]) and
    beyond z + band; anything else is occluded or unknown. Returns `votes` [M,3] int32 = (in view, support, free) on the
    points' device; `out=` (an earlier result) is added to and returned. Device tensors go through libatdn_hip's kernel on the
    current stream (no synchronisation), CPU tensors through the library's host form. The rule is float64 and integer sums,
    stated in full in include/atdn_hip.h, atdn_voxel_votes: the same bits on every call, on both paths and however the
    keyframes are split over calls."""
    from .depth import intrinsics
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("expected points [M,3], got %s" % (tuple(getattr(points, "shape", ())),))
    dev = points.device
    M = int(points.shape[0])
    pts = points.detach().to(torch.float32).contiguous()
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
        raise RuntimeError("expected a depth bank [N,H,W], got %s" % (tuple(getattr(depth, "shape", ())),))
    if depth.device != dev:
        raise RuntimeError("points on %s but depth on %s" % (dev, depth.device))
    if depth.dtype != torch.float32 or not depth.is_contiguous():
        depth = depth.detach().float().contiguous()
    N, H, W = (int(v) for v in depth.shape)
    if isinstance(poses, torch.Tensor) and poses.device != dev:
        raise RuntimeError("points on %s but poses on %s" % (dev, poses.device))
    p = _pose_rows(poses, N, dev)
    ix = None if indices is None else _index_tensor(indices, "indices", dev).reshape(-1)
    K = N if ix is None else int(ix.shape[0])
    if out is None:
        votes, accumulate = torch.empty((M, 3), dtype=torch.int32, device=dev), 0
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != (M, 3) or out.device != dev or \
                not out.is_contiguous():
            raise RuntimeError("expected out [%d,3] int32, contiguous, on %s" % (M, dev))
        votes, accumulate = out, 1
    if K < 1:
        return votes if accumulate else votes.zero_()
    _lib.call("atdn_voxel_votes", dev, _ptr(pts) if M else None, M, _ptr(depth), _ptr(p), _ptr(ix), N, K, H, W, *intrinsics(calib),
              float(near), float(far), float(rel), float(abs_tol), int(radius), accumulate, _ptr(votes) if M else None)
    return votes


class InputPadder:
    """Replicate-pads frames to multiples of 8 ('sintel' mode splits the padding on both sides)."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = dims[-2:]
        ph = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pw = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]
        else:
            self._pad = [pw // 2, pw - pw // 2, 0, ph]

    def pad(self, *inputs):
        if not any(self._pad):  # 376x1232: nothing to pad (neural_slam.py:54) — skip the copy
            return list(inputs)
        return [self._pad_one(x) for x in inputs]

    def _pad_one(self, x):
        """F.pad(x, pad, mode="replicate") (utils.py:19-20). Device tensors go through libatdn_hip's pad kernel; host
        tensors (the reference pads on whatever device the frame is on) use torch."""
        if not x.is_cuda:
            return torch.nn.functional.pad(x, self._pad, mode="replicate")
        l, r, t, b = self._pad
        src = x.float().contiguous()
        H, W = src.shape[-2:]
        out = torch.empty(tuple(src.shape[:-2]) + (H + t + b, W + l + r), dtype=torch.float32, device=src.device)
        planes = int(src.numel() // (H * W))
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().atdn_pad_frames(_ptr(src), planes, H, W, l, r, t, b, _ptr(out), _lib.stream()))
        return out

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        return x[..., self._pad[2]:ht - self._pad[3], self._pad[0]:wd - self._pad[1]]
