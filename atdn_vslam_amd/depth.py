"""Calibration and depth helpers (atdn_vslam/utils/depth.py): `read_calib` and `project_depth` with the reference's call contracts,
plus what the odometry path needs to use a calibration on its own grid: `intrinsics` and `resize_calib`. Depth itself comes from
`transforms.two_view_depth` (a flow, a relative pose and a calibration); the reference has no producer of it."""
import ctypes as C

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
            _lib.check(_lib.lib().atdn_depth_backproject(C.c_void_p(d.data_ptr()), 1, H, W, fx, fy, cx, cy,
                                                         C.c_void_p(points.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return points
    z = d.reshape(H, W).double()
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    return torch.stack([(z * (x - cx)) / fx, (z * (y - cy)) / fy, z]).float()
