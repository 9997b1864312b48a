"""Pose algebra of the odometry path (atdn_vslam/utils/transforms.py) and the frame padder
(whl:GMA/core/utils/utils.py:8-25), host side of libatdn_hip."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _np32(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().to("cpu")
        x = x.numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


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
    if src.is_cuda:
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().atdn_flow_forward_interpolate(C.c_void_p(src.data_ptr()), B, h, w, C.c_void_p(out.data_ptr()),
                                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    else:
        _lib.check(_lib.lib().atdn_flow_forward_interpolate_host(C.c_void_p(src.data_ptr()), B, h, w, C.c_void_p(out.data_ptr())))
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
    L = _lib.lib()
    if fw.is_cuda:
        with torch.cuda.device(fw.device):
            _lib.check(L.atdn_flow_consistency(C.c_void_p(fw.data_ptr()), C.c_void_p(bw.data_ptr()), B, H, W, float(alpha1),
                                               float(alpha2), C.c_void_p(mask.data_ptr()), C.c_void_p(count.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    else:
        _lib.check(L.atdn_flow_consistency_host(C.c_void_p(fw.data_ptr()), C.c_void_p(bw.data_ptr()), B, H, W, float(alpha1),
                                                float(alpha2), C.c_void_p(mask.data_ptr()), C.c_void_p(count.data_ptr())))
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
        import ctypes as C
        from . import _lib
        l, r, t, b = self._pad
        src = x.float().contiguous()
        H, W = src.shape[-2:]
        out = torch.empty(tuple(src.shape[:-2]) + (H + t + b, W + l + r), dtype=torch.float32, device=src.device)
        planes = int(src.numel() // (H * W))
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().atdn_pad_frames(C.c_void_p(src.data_ptr()), planes, H, W, l, r, t, b,
                                                  C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        return x[..., self._pad[2]:ht - self._pad[3], self._pad[0]:wd - self._pad[1]]
