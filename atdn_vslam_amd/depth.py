"""Calibration and depth helpers (atdn_vslam/utils/depth.py): `read_calib` and `project_depth` with the reference's call contracts,
plus what the odometry path needs to use a calibration on its own grid: `intrinsics` and `resize_calib`. Depth itself comes from
`transforms.two_view_depth` (a flow, a relative pose and a calibration); the reference has no producer of it."""
import numpy as np
import torch

from . import _lib


def read_calib(path, include_rect=False):
    """The calibration matrix of a KITTI calibration file (depth.py:5-20): row 1 of the file (the line after the first), its
    twelve numbers as a float32 [3,4] matrix; `include_rect=True` appends the row (0, 0, 0, 1) -> [4,4], otherwise the last
    column is dropped -> [3,3]."""
    rows = np.loadtxt(path, dtype=str)
    calib = torch.from_numpy(rows[1][1:].astype(np.float32)).view(3, 4)
    if include_rect:
        return torch.cat([calib, torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
    return calib[:, :-1]


def intrinsics(calib):
    """(fx, fy, cx, cy) as Python floats from (fx, fy, cx, cy) itself or from a 3x3 / 3x4 (or 4x4) calibration matrix
    [[fx,0,cx,..],[0,fy,cy,..],[0,0,1,..]]. A matrix with skew, or whose left 3x3 block has any other entry off that pattern,
    raises ValueError: the two-view rule and the back-projection kernel are those of a pinhole camera without skew."""
    k = torch.as_tensor(calib, dtype=torch.float64).detach().cpu()
    if k.dim() == 1 and k.numel() == 4:
        fx, fy, cx, cy = (float(v) for v in k)
    elif k.dim() == 2 and tuple(k.shape) in ((3, 3), (3, 4), (4, 4)):
        if float(k[0, 1]) != 0.0:
            raise ValueError("calibration with skew (%g): not supported" % float(k[0, 1]))
        if float(k[1, 0]) != 0.0 or float(k[2, 0]) != 0.0 or float(k[2, 1]) != 0.0 or float(k[2, 2]) != 1.0:
            raise ValueError("calibration matrix is not [[fx,0,cx],[0,fy,cy],[0,0,1]]")
        fx, fy, cx, cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    else:
        raise ValueError("expected (fx, fy, cx, cy) or a 3x3 / 3x4 calibration matrix, got shape %s" % (tuple(k.shape),))
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx > 0 and fy > 0):
        raise ValueError("calibration needs finite values and fx, fy > 0, got %r" % ((fx, fy, cx, cy),))
    return fx, fy, cx, cy


def resize_calib(calib, from_hw, to_hw):
    """(fx, fy, cx, cy) of a frame resized from `from_hw` to `to_hw` = (H, W) the way the frame front-end resizes (half-pixel
    centres, align_corners=False): with sx = W'/W, fx' = fx*sx and cx' = (cx + 0.5)*sx - 0.5; likewise y. Takes a KITTI
    calibration at 376 x 1241 to the 376 x 1232 grid the flow lives on."""
    fx, fy, cx, cy = intrinsics(calib)
    sy, sx = float(to_hw[0]) / float(from_hw[0]), float(to_hw[1]) / float(from_hw[1])
    return fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5


def project_depth(depth, calib, device=None):
    """Depth image [H,W] (or [1,H,W]) -> points [3,H,W] float32 in the camera frame (depth.py:23-46): for z = depth[y,x],
    X = z*(x - cx)/fx, Y = z*(y - cy)/fy, Z = z, each formed in float64 and rounded once (the reference inverts the float32
    matrix and multiplies in float32). `device` (default: the depth's own) is where the result is computed and returned. Device
    tensors go through libatdn_hip's kernel on the current stream, CPU tensors through the same expression in torch. A
    calibration with skew raises ValueError (`intrinsics`)."""
    fx, fy, cx, cy = intrinsics(calib)
    d = torch.as_tensor(depth)
    if device is not None:
        d = d.to(device)
    H, W = d.shape[-2], d.shape[-1]
    if d.numel() != H * W:
        raise RuntimeError("expected one depth image [H,W] or [1,H,W], got %s" % (tuple(d.shape),))
    d = d.detach().float().contiguous()
    if d.is_cuda:
        points = torch.empty((3, H, W), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            _lib.check(_lib.lib().atdn_depth_backproject(_lib.ptr(d), 1, H, W, fx, fy, cx, cy, _lib.ptr(points), _lib.stream()))
        return points
    z = d.reshape(H, W).double()
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    return torch.stack([(z * (x - cx)) / fx, (z * (y - cy)) / fy, z]).float()


class FlowTrack:
    """The state of one anchor frame's flow track (transforms.flow_track_step) on the device: `acc` [B,2,H,W] float32, the flow
    from the anchor to the latest frame on the anchor's grid; `alive` [B,H,W] uint8; `depth` [B,1,H,W] float32, at every pixel the
    triangulation of the last step at which it was valid (0 = none yet); `counts` [B,4] int32 of the last step = (alive, inside,
    inliers, valid); `pose` [B,4,4] float64 on the host, anchor <- latest frame; `steps`, the number of pairs since the anchor.
    `calib` is that of the grid the flows live on (`resize_calib`); `thresholds` are max_epipolar, min_parallax_deg and max_depth
    of `transforms.two_view_depth`. `start()` begins a track at a new anchor, `extend(flow, pred_mat)` carries it over one pair.
    The pose goes to the device as 12 float32 through pinned memory, asynchronously; no call synchronises with the host.
    `history=K` (1 <= K <= 16, transforms.multiview_depth's limit) also keeps `acc`, `alive` and the pose row of the last K steps
    in preallocated device banks [K * B, ...] (`hist_acc`, `hist_alive`, `hist_pose`; ring position r of image b is slot r * B + b):
    a ring, filled after every step by device copies of `acc` and `alive` on the same stream — the pose row is uploaded straight
    into its ring slot —, still without a host synchronisation. `multiview()` solves the depth over the stored steps, `bundle()`
    first refines their poses jointly with the depth (transforms.bundle_adjust). With
    `history=0` (the default) nothing is allocated and `extend` does what it always did."""

    def __init__(self, hw, calib, device, batch=1, history=0, **thresholds):
        unknown = set(thresholds) - {"max_epipolar", "min_parallax_deg", "max_depth"}
        if unknown:
            raise TypeError("unknown threshold(s): %s" % ", ".join(sorted(unknown)))
        H, W = int(hw[0]), int(hw[1])
        B = int(batch)
        K = int(history)
        if not 0 <= K <= 16:
            raise ValueError("history must be in [0, 16], got %r" % (history,))
        self.history = K
        self.hist_acc = self.hist_alive = self.hist_pose = None
        if K:
            self.hist_acc = torch.zeros((K * B, 2, H, W), dtype=torch.float32, device=device)
            self.hist_alive = torch.zeros((K * B, H, W), dtype=torch.uint8, device=device)
            self.hist_pose = torch.zeros((K * B, 12), dtype=torch.float32, device=device)
        self.calib = intrinsics(calib)
        self.device = torch.device(device)
        self.thresholds = dict(thresholds)
        self.acc = torch.zeros((B, 2, H, W), dtype=torch.float32, device=self.device)
        self.alive = torch.ones((B, H, W), dtype=torch.uint8, device=self.device)
        self.depth = torch.zeros((B, 1, H, W), dtype=torch.float32, device=self.device)
        self.counts = torch.zeros((B, 4), dtype=torch.int32, device=self.device)
        self._pose_dev = torch.zeros((B, 12), dtype=torch.float32, device=self.device)
        self.pose = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
        self.steps = 0

    def to(self, device):
        """Move the device state, a running track included; the pose and `steps` stay on the host. Returns self."""
        self.device = torch.device(device)
        for name in ("acc", "alive", "depth", "counts", "_pose_dev") + (("hist_acc", "hist_alive", "hist_pose") if self.history else ()):
            setattr(self, name, getattr(self, name).to(self.device))
        return self

    def start(self):
        """Begin a track at a new anchor: acc and depth zero, every pixel alive, identity pose."""
        self.acc.zero_()
        self.depth.zero_()
        self.alive.fill_(1)
        self.counts.zero_()
        self.pose = torch.eye(4, dtype=torch.float64).repeat(self.pose.shape[0], 1, 1)
        self.steps = 0

    def extend(self, flow, pred_mat, mask=None):
        """Carry the track over the pair frame k -> k+1: `flow` [B,2,H,W] on the track's device, `pred_mat` [4,4] or [B,4,4] the
        pair's relative pose (X_k = R X_k+1 + t, what `transforms.transform` returns), `mask` as for `transforms.flow_track_step`.
        pose <- pose @ pred_mat in float64, then one in-place step. Returns `counts`."""
        from . import transforms
        B = self.pose.shape[0]
        step = torch.as_tensor(pred_mat).detach().to("cpu", torch.float64)
        if tuple(step.shape) not in ((4, 4), (B, 4, 4)):
            raise RuntimeError("expected a relative pose [4,4] or [%d,4,4], got %s" % (B, tuple(step.shape)))
        self.pose = self.pose @ step
        # a pinned buffer of the caching host allocator per step: it is handed out again only after the copy that reads it is done
        rows = torch.empty((B, 12), dtype=torch.float32, pin_memory=self.device.type == "cuda")
        rows.copy_(self.pose[:, :3, :].reshape(B, 12))
        ring = None
        if self.history:
            r = self.steps % self.history
            ring = slice(r * B, (r + 1) * B)
        pose_dev = self._pose_dev if ring is None else self.hist_pose[ring]
        pose_dev.copy_(rows, non_blocking=True)
        transforms.flow_track_step(flow, self.acc, self.alive, pose=pose_dev, calib=self.calib, mask=mask, depth=self.depth,
                                   out=(self.acc, self.alive, self.counts), **self.thresholds)
        if ring is not None:
            self.hist_acc[ring].copy_(self.acc)
            self.hist_alive[ring].copy_(self.alive)
        self.steps += 1
        return self.counts

    def history_slots(self):
        """[B,S] int64 on the host: the bank slots of the stored steps of every image, oldest first (S = min(steps, history))."""
        B, K = self.pose.shape[0], self.history
        S = min(self.steps, K)
        first = self.steps - S
        return torch.tensor([[((first + i) % K) * B + b for i in range(S)] for b in range(B)], dtype=torch.int64).reshape(B, S)

    def multiview(self, **options):
        """`transforms.multiview_depth` over the stored steps in time order (oldest first), started from `depth`: returns
        `(depth, info, views, counts)`; `options` are its keyword arguments (iters, scale_px, inlier_px, min_z, min_views,
        max_rel_sigma, max_depth). Needs `history` > 0 and at least one step since `start()`; the track's own state is untouched."""
        from . import transforms
        if not self.history:
            raise RuntimeError("FlowTrack.multiview needs a track created with history > 0")
        if self.steps < 1:
            raise RuntimeError("FlowTrack.multiview: no step since start()")
        return transforms.multiview_depth(self.hist_acc, self.hist_alive, self.hist_pose, self.history_slots().tolist(), self.calib,
                                          depth_init=self.depth, **options)

    def bundle(self, multiview_options=None, **options):
        """Windowed bundle adjustment of the stored steps, then the multi-view depth against the refined poses:
        `transforms.bundle_adjust` over `history_slots()` started from `depth` (`options` are its keyword arguments: stride, iters,
        scale_px, inlier_px, min_z, min_views, mask), the refined rows scattered into a COPY of `hist_pose` on the device, and
        `transforms.multiview_depth` (`multiview_options`) with that copy. Returns `(poses, depth, info, views, mv_counts, cost,
        ba_counts)`: `poses` [B,S,12] the refined poses anchor <- step, oldest first; `depth`, `info`, `views`, `mv_counts` as
        `multiview()` returns them; `cost` [B,2] and `ba_counts` [B,4] of the adjustment. Needs `history` > 0 and at least one
        step since `start()`; the track's own state, its banks included, is untouched."""
        from . import transforms
        if not self.history:
            raise RuntimeError("FlowTrack.bundle needs a track created with history > 0")
        if self.steps < 1:
            raise RuntimeError("FlowTrack.bundle: no step since start()")
        slots = self.history_slots()
        poses, _, cost, ba_counts = transforms.bundle_adjust(self.hist_acc, self.hist_alive, self.hist_pose, slots.tolist(),
                                                             self.calib, self.depth, **options)
        refined = self.hist_pose.clone()
        refined.index_copy_(0, slots.reshape(-1).to(self.device), poses.reshape(-1, 12))
        depth, info, views, mv_counts = transforms.multiview_depth(self.hist_acc, self.hist_alive, refined, slots.tolist(), self.calib,
                                                                   depth_init=self.depth, **(multiview_options or {}))
        return poses, depth, info, views, mv_counts, cost, ba_counts
