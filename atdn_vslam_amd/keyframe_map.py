"""The relocalisation map of NeuralSLAM kept in HBM: keyframe images, their MappingVAE embeddings and a one-launch search.

The reference keeps a Python list of `Frame`s (slam_framework/frame.py): an image file per keyframe, a pose and a latent
embedding, and answers a relocalisation query with a loop of `torch.norm(kf.embedding - mu, p=2)` over that list, an
`argmin`, a `torch.load` of the winner's image and a batch-1 odometry step (slam_framework/neural_slam.py:355-399). Here:

* the image bank is one uint8 device buffer [capacity,3,H,W]; `images(indices)` is `atdn_map_gather_images_u8`, the fp32
  batch the encoder and the flow network read;
* the embedding bank is one fp32 device buffer [capacity, D], D = h * w * 128, a row being exactly what `atdn_vae_encode`
  writes for one image (CHANNELS-LAST: element (y * w + x) * 128 + c of a row is `MappingVAE(image)[0][0, c, y, x]`), so
  `embed` lets the encoder write straight into the rows of a batch of keyframes. The L2 norm does not care about element
  order, as long as the queries are in the same one;
* `search` is `atdn_map_search`: every distance of every query in one pass over the bank, and the top_k nearest keyframes
  per query;
* `relocalize` answers a batch of queries: one encoder call, one search, one image gather, the flow network and the pose
  head at batch Q;
* the depth bank is one fp32 device buffer [capacity,H,W] (allocated by the first `set_depth`; zeros = no depth): with
  `relocalize(geometric=True)` the keyframe's depth and the keyframe -> query flow give a second, geometric pose
  (`transforms.pose_from_depth`) next to the pose head's.

Poses live on the host ([K,4,4] float32), as in the reference.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, transforms
from . import keyframe_dir as kd
from .keyframe_dir import KeyframeDir
from ._lib import ptr as _ptr, stream as _stream

MAX_TOP_K = 16


def embedding_hw(hw):
    """Size of the MappingVAE embedding map of an H x W image: six stride-2 blocks (3x3, padding 1), 376x1232 -> 6x20."""
    h, w = int(hw[0]), int(hw[1])
    for _ in range(6):
        h, w = (h + 1) // 2, (w + 1) // 2
    return h, w


def _homogeneous(poses):
    p = torch.as_tensor(poses, dtype=torch.float32)
    if p.dim() == 2 and p.shape[1] == 12:
        p = p.view(-1, 3, 4)
    if p.dim() == 3 and tuple(p.shape[1:]) == (3, 4):
        last = torch.tensor([0.0, 0.0, 0.0, 1.0]).view(1, 1, 4).repeat(len(p), 1, 1)
        p = torch.cat([p, last], dim=1)
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
        raise ValueError("poses must be [K,12], [K,3,4] or [K,4,4], got %s" % (tuple(p.shape),))
    return p


def gather_images(bank, indices):
    """bank [K,3,H,W] uint8 (device) -> fp32 [n,3,H,W] with out[j] = bank[indices[j]].float() (atdn_map_gather_images_u8; the
    indices are a host array, each checked against [0, K) before anything is launched)."""
    K = int(bank.shape[0])
    if isinstance(indices, torch.Tensor):
        indices = indices.detach().cpu().numpy()
    ix = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if ix.size == 0:
        raise RuntimeError("gather_images: no index")
    if ix.min() < -2 ** 31 or ix.max() >= 2 ** 31:
        raise RuntimeError("gather_images: index outside the int range")
    ix = ix.astype(np.int32)
    if bank.dtype != torch.uint8 or not bank.is_contiguous():
        raise RuntimeError("gather_images: the bank must be a contiguous uint8 tensor")
    shape = (ix.size,) + tuple(bank.shape[1:])
    out = torch.empty(shape, dtype=torch.float32, device=bank.device)
    plane = int(np.prod(bank.shape[1:]))
    with torch.cuda.device(bank.device):
        _lib.check(_lib.lib().atdn_map_gather_images_u8(_ptr(bank), K, plane, ix.ctypes.data_as(C.c_void_p), int(ix.size),
                                                        _ptr(out), _stream()))
    return out


def search_bank(bank, queries, top_k=1):
    """bank [K,D], queries [Q,D] fp32 on one device -> (distances [Q,K] fp32, indices [Q,top_k] int32), device tensors
    (atdn_map_search)."""
    K, D = int(bank.shape[0]), int(bank.shape[1])
    if queries.dim() != 2 or int(queries.shape[1]) != D:
        raise RuntimeError("search: queries must be [Q,%d], got %s" % (D, tuple(queries.shape)))
    if queries.device != bank.device:
        raise RuntimeError("search: queries on %s but the map is on %s" % (queries.device, bank.device))
    q = queries.float().contiguous()
    Q = int(q.shape[0])
    dist = torch.empty((Q, K), dtype=torch.float32, device=bank.device)
    idx = torch.empty((Q, int(top_k)), dtype=torch.int32, device=bank.device)
    with torch.cuda.device(bank.device):
        _lib.check(_lib.lib().atdn_map_search(_ptr(bank), K, D, _ptr(q), Q, int(top_k), _ptr(dist), _ptr(idx), _stream()))
    return dist, idx


class KeyframeMap:
    """Keyframe images (uint8), embeddings (fp32, channels-last rows) and poses of one map; the first two in device memory."""

    def __init__(self, device, hw=(376, 1232), capacity=256):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("KeyframeMap lives in device memory: there is no CPU fallback")
        self.hw = (int(hw[0]), int(hw[1]))
        if (3 * self.hw[0] * self.hw[1]) % 16 != 0:
            raise ValueError("3 * H * W must be a multiple of 16 (16-byte image rows in the bank), got %dx%d" % self.hw)
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("KeyframeMap needs room for at least one keyframe")
        self.embedding_hw = embedding_hw(self.hw)
        self.D = self.embedding_hw[0] * self.embedding_hw[1] * 128
        self.image_bank = torch.empty((self.capacity, 3) + self.hw, dtype=torch.uint8, device=self.device)
        self.embedding_bank = None          # [capacity, D] fp32, allocated by the first embed()
        self.depth_bank = None              # [capacity, H, W] fp32, allocated by the first set_depth(); zeros = no depth
        self._poses = torch.zeros((self.capacity, 4, 4), dtype=torch.float32)
        self.n = 0
        self.n_embedded = 0
        self._embed_fp = None               # (module, its parameter fingerprint) of the rows embedded so far

    def __len__(self):
        return self.n

    @property
    def poses(self):
        """[K,4,4] float32, host."""
        return self._poses[:self.n]

    # ------------------------------------------------------------------ filling
    def _grow(self):
        cap = self.capacity * 2
        images = torch.empty((cap, 3) + self.hw, dtype=torch.uint8, device=self.device)
        images[:self.n].copy_(self.image_bank[:self.n])
        self.image_bank = images
        if self.embedding_bank is not None:
            emb = torch.empty((cap, self.D), dtype=torch.float32, device=self.device)
            emb[:self.n_embedded].copy_(self.embedding_bank[:self.n_embedded])
            self.embedding_bank = emb
        if self.depth_bank is not None:
            depth = torch.zeros((cap,) + self.hw, dtype=torch.float32, device=self.device)
            depth[:self.n].copy_(self.depth_bank[:self.n])
            self.depth_bank = depth
        poses = torch.zeros((cap, 4, 4), dtype=torch.float32)
        poses[:self.n] = self._poses[:self.n]
        self._poses = poses
        self.capacity = cap

    def append(self, image, pose):
        """Store one keyframe: image [3,H,W] (or [1,3,H,W]) uint8, or float with values 0..255 (`.byte()` of it is stored:
        what the reference writes to rgb/%06d.pth), on any device; pose [4,4]. The copy into the bank runs on the device.
        A full map doubles its capacity (new buffers, device-to-device copies). Returns the keyframe's index."""
        im = image[0] if image.dim() == 4 and image.shape[0] == 1 else image
        if tuple(im.shape) != (3,) + self.hw:
            raise ValueError("keyframe image must be [3,%d,%d], got %s" % (self.hw + (tuple(image.shape),)))
        pose = torch.as_tensor(pose, dtype=torch.float32).cpu()
        if tuple(pose.shape) != (4, 4):
            raise ValueError("keyframe pose must be [4,4], got %s" % (tuple(pose.shape),))
        if self.n == self.capacity:
            self._grow()
        im = im.to(self.device)
        self.image_bank[self.n].copy_(im if im.dtype == torch.uint8 else im.byte())
        self._poses[self.n] = pose
        self.n += 1
        return self.n - 1

    def set_depth(self, k, depth):
        """Give keyframe k its depth map: [H,W] or [1,H,W] float32 in the map's own scale, 0 = no depth (what
        `transforms.two_view_depth` and `depth.FlowTrack` produce), on any device; it replaces an earlier one. The bank is
        allocated, as zeros, by the first call; a keyframe that never got a depth holds zeros."""
        if not 0 <= int(k) < self.n:
            raise IndexError("keyframe %d of %d" % (k, self.n))
        d = torch.as_tensor(depth)
        d = d[0] if d.dim() == 3 and d.shape[0] == 1 else d
        if tuple(d.shape) != self.hw:
            raise ValueError("keyframe depth must be [%d,%d] or [1,%d,%d], got %s" % (self.hw + self.hw + (tuple(depth.shape),)))
        if self.depth_bank is None:
            self.depth_bank = torch.zeros((self.capacity,) + self.hw, dtype=torch.float32, device=self.device)
        self.depth_bank[int(k)].copy_(d.detach().to(self.device, torch.float32))

    def depths(self, indices):
        """fp32 [n,H,W] on the device: the depth maps of the keyframes `indices` (a host sequence), zeros where there is none."""
        ix = [int(i) for i in indices]
        if any(not 0 <= i < self.n for i in ix):
            raise IndexError("keyframe index outside [0, %d)" % self.n)
        if self.depth_bank is None:
            return torch.zeros((len(ix),) + self.hw, dtype=torch.float32, device=self.device)
        return self.depth_bank.index_select(0, torch.tensor(ix, dtype=torch.int64).to(self.device, non_blocking=True))

    @torch.no_grad()
    def fuse_depths(self, calib, window=2, sources=None, replace=False, batch=16, **thresholds):
        """Multi-view consistency filter of the keyframe depths (`transforms.fuse_depths`, where the rule and the `thresholds`
        max_reproj, max_rel_depth, min_views, min_z, average are described) over the whole map, straight from the depth bank and
        the poses: no copy of the bank, `batch` targets per launch. The sources of keyframe k are `sources[k]` ([n,S] integers,
        host; an entry < 0, >= n or == k is an empty slot) or, by default, its neighbours k-window .. k+window without k, with
        empty slots where the map ends. Returns device tensors `(fused [n,H,W] float32, views [n,H,W] uint8, counts [n,3] int32)`,
        counts = (pixels with a depth, pixels some source saw, pixels kept). The fusion is Jacobi: every target reads the
        unfused bank; `replace=True` then puts the fused depths into the bank (relocalisation's PnP leg and a second call
        see them). `calib` is the calibration of the map's grid. A map without a depth bank raises."""
        if self.depth_bank is None or self.n == 0:
            raise RuntimeError("fuse_depths: the map holds no depth (set_depth gives a keyframe its depth map)")
        n = self.n
        if sources is None:
            w = int(window)
            if w < 0:
                raise ValueError("window must be >= 0, got %d" % w)
            offsets = [d for d in range(-w, w + 1) if d != 0]
            src = np.array([[k + d if 0 <= k + d < n else -1 for d in offsets] for k in range(n)], dtype=np.int32).reshape(n, len(offsets))
        else:
            src = np.asarray(sources.cpu() if isinstance(sources, torch.Tensor) else sources, dtype=np.int64)
            if src.ndim != 2 or src.shape[0] != n:
                raise ValueError("sources must be [%d,S], got %s" % (n, src.shape))
            src = np.clip(src, -1, 2 ** 31 - 1).astype(np.int32)
        batch = max(1, int(batch))
        bank = self.depth_bank[:n]                                    # a view of the bank's first n planes
        poses = self._poses[:n, :3, :].reshape(n, 12).to(self.device)
        fused, views, counts = [], [], []
        with torch.cuda.device(self.device):
            for a in range(0, n, batch):
                b = min(batch, n - a)
                f, v, c = transforms.fuse_depths(bank, poses, np.arange(a, a + b), src[a:a + b], calib, **thresholds)
                fused.append(f[:, 0])
                views.append(v)
                counts.append(c)
            fused, views, counts = torch.cat(fused), torch.cat(views), torch.cat(counts)
            if replace:
                bank.copy_(fused)                                     # after the last target has read the unfused bank
        return fused, views, counts

    @torch.no_grad()
    def voxel_map(self, calib, fused=None, batch=8, stride=1, **options):
        """The map as one coloured point cloud (`voxel_map.VoxelMap`; `options`: voxel, origin, min_z, max_z, capacity): the
        depth bank, the poses and the image bank integrated straight out of device memory, `batch` keyframes per launch through
        an index list (no gather copy), every `stride`-th pixel. `fused` ([n,H,W] float32 on the map's device, what
        `fuse_depths` returns) replaces the depth bank. A keyframe without a depth holds zeros and adds nothing. `calib` is the
        calibration of the map's grid. Returns the VoxelMap; a map without a depth bank raises."""
        from .voxel_map import VoxelMap
        n = self.n
        if fused is None:
            if self.depth_bank is None or n == 0:
                raise RuntimeError("voxel_map: the map holds no depth (set_depth gives a keyframe its depth map)")
            depth = self.depth_bank[:n]
        else:
            depth = torch.as_tensor(fused)
            if tuple(depth.shape) != (n,) + self.hw or depth.device != self.device:
                raise ValueError("fused must be [%d,%d,%d] on %s, got %s on %s" %
                                 ((n,) + self.hw + (self.device, tuple(depth.shape), depth.device)))
        vm = VoxelMap(self.device, **options)
        poses = self._poses[:n, :3, :].reshape(n, 12).to(self.device)
        batch = max(1, int(batch))
        with torch.cuda.device(self.device):
            for a in range(0, n, batch):
                vm.integrate(depth, poses, calib, images=self.image_bank[:n], indices=np.arange(a, min(a + batch, n)), stride=stride)
        return vm

    @torch.no_grad()
    def carve(self, voxel_map, calib, fused=None, batch=8, **options):
        """Free-space carving of `voxel_map` (a `voxel_map.VoxelMap` on the map's device) against every keyframe of this map:
        `VoxelMap.carve` (`options`: its keyword arguments — min_free, ratio, min_support, near, far, rel, abs_tol, radius)
        straight from the depth bank and the poses, `batch` keyframes per launch through an index list (no gather copy).
        `fused` ([n,H,W] float32 on the map's device, what `fuse_depths` returns) replaces the depth bank — pass what the
        voxel map was integrated from. `calib` is the calibration of the map's grid. Returns `VoxelMap.carve`'s report; a map
        without a depth bank raises."""
        n = self.n
        if voxel_map.device != self.device:
            raise ValueError("the voxel map is on %s but the keyframe map on %s" % (voxel_map.device, self.device))
        if fused is None:
            if self.depth_bank is None or n == 0:
                raise RuntimeError("carve: the map holds no depth (set_depth gives a keyframe its depth map)")
            depth = self.depth_bank[:n]
        else:
            depth = torch.as_tensor(fused)
            if tuple(depth.shape) != (n,) + self.hw or depth.device != self.device:
                raise ValueError("fused must be [%d,%d,%d] on %s, got %s on %s" %
                                 ((n,) + self.hw + (self.device, tuple(depth.shape), depth.device)))
        poses = self._poses[:n, :3, :].reshape(n, 12).to(self.device)
        with torch.cuda.device(self.device):
            return voxel_map.carve(depth, poses, calib, batch=batch, **options)

    @torch.no_grad()
    def render_depths(self, cloud, calib, indices=None, fill=False, batch=8, **options):
        """The map's cloud seen from the keyframes' own poses: the depth every keyframe would have measured had it seen what all
        of them saw. `cloud` is a `voxel_map.VoxelMap` on the map's device (`options`: the keyword arguments of its `render` —
        min_count, splat, max_splat, near, far) or a tuple `(points, colors, counts)` of device tensors, e.g. a cloud read with
        `VoxelMap.load_ply` (`options`: those of `transforms.render_points`, `size` among them). `indices` (a host sequence; all
        keyframes by default) names the keyframes, `batch` of them are rendered per call, `calib` is the calibration of the
        map's grid. Returns the rendered depths, float32 [len(indices),H,W] on the device, 0 = nothing rendered. `fill=True`
        also writes the rendered depth into the depth bank at exactly the pixels that hold 0 (a keyframe's own measurements
        stay); with False nothing in the map changes."""
        from .transforms import render_points
        n = self.n
        ix = list(range(n)) if indices is None else [int(i) for i in indices]
        if any(not 0 <= i < n for i in ix):
            raise IndexError("keyframe index outside [0, %d)" % n)
        if isinstance(cloud, (tuple, list)):
            points, colors, counts = cloud[:3]
            if "size" not in options:
                raise ValueError("render_depths of a bare cloud needs size=, the edge of its voxels")
            size = options.pop("size")

            def render(poses):
                return render_points(points, colors, counts, poses, calib, self.hw, size, **options)[0]
        else:
            if cloud.device != self.device:
                raise ValueError("the voxel map is on %s but the keyframe map on %s" % (cloud.device, self.device))

            def render(poses):
                return cloud.render(poses, calib, self.hw, **options)[0]
        poses = self._poses[:n, :3, :].reshape(n, 12).to(self.device)
        batch = max(1, int(batch))
        out = torch.zeros((len(ix),) + self.hw, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for a in range(0, len(ix), batch):
                sel = torch.tensor(ix[a:a + batch], dtype=torch.int64).to(self.device, non_blocking=True)
                out[a:a + len(sel)] = render(poses.index_select(0, sel))
            if fill and ix:
                if self.depth_bank is None:
                    self.depth_bank = torch.zeros((self.capacity,) + self.hw, dtype=torch.float32, device=self.device)
                sel = torch.tensor(ix, dtype=torch.int64).to(self.device, non_blocking=True)
                own = self.depth_bank.index_select(0, sel)
                self.depth_bank.index_copy_(0, sel, torch.where(own == 0, out, own))
        return out

    @classmethod
    def from_directory(cls, keyframes_path, device, mapping_net=None):
        """The map of a keyframe directory as the reference and slam.NeuralSLAM write it: `rgb/*.pth` (sorted; uint8
        [3,H,W]), `poses.pth` ([K,12]) and, where a keyframe has one, `depth/<the frame's name>` (float32 [1,H,W]). Every file is read once; the directory is validated (poses.pth present, as many
        poses as frames, all frames of the first one's size) before anything touches the device.
        With `mapping_net` the keyframes are embedded too."""
        directory = KeyframeDir(keyframes_path)
        if not directory.exists(kd.POSES):
            raise FileNotFoundError("%s is missing: not a keyframe directory (end_odometry() writes it)" % directory.path(kd.POSES))
        files = directory.frames()
        if not files:
            raise ValueError("%s holds no keyframe (rgb/*.pth)" % keyframes_path)
        poses = _homogeneous(directory.load(kd.POSES, map_location="cpu"))
        if len(poses) != len(files):
            raise ValueError("%s: %d poses in poses.pth but %d frames under rgb/" % (keyframes_path, len(poses), len(files)))
        frames, hw = [], None
        for f in files:
            im = torch.load(f, map_location="cpu")
            if im.dim() == 4 and im.shape[0] == 1:
                im = im[0]
            if hw is None:
                if im.dim() != 3 or im.shape[0] != 3:
                    raise ValueError("%s: expected a [3,H,W] frame, got %s" % (f, tuple(im.shape)))
                hw = (int(im.shape[1]), int(im.shape[2]))
            if tuple(im.shape) != (3,) + hw:
                raise ValueError("%s: frame of size %s in a map of %dx%d frames" % (f, tuple(im.shape), hw[0], hw[1]))
            frames.append(im if im.dtype == torch.uint8 else im.byte())
        m = cls(device, hw=hw, capacity=len(files))
        for im, pose in zip(frames, poses):
            m.append(im, pose)
        for k, f in enumerate(files):
            if directory.exists(kd.DEPTH, f):
                m.set_depth(k, directory.load(kd.DEPTH, f, map_location="cpu"))
        if mapping_net is not None:
            m.embed(mapping_net)
        return m

    @torch.no_grad()
    def embed(self, mapping_net, batch=16):
        """Embed the keyframes that are not embedded yet, `batch` at a time: one image gather and one `atdn_vae_encode`
        whose output is the bank row of the first of them (no copy, no permute). Everything is embedded again when
        `mapping_net` is another module or its weights changed since the last call (the modules' `_fingerprint()`)."""
        fp = (id(mapping_net), mapping_net._fingerprint())
        if self._embed_fp != fp:
            self.n_embedded = 0
        if self.embedding_bank is None:
            self.embedding_bank = torch.empty((self.capacity, self.D), dtype=torch.float32, device=self.device)
        batch = max(1, int(batch))
        with torch.cuda.device(self.device):
            while self.n_embedded < self.n:
                first, b = self.n_embedded, min(batch, self.n - self.n_embedded)
                images = gather_images(self.image_bank[:self.n], np.arange(first, first + b))
                mapping_net.encode_rows(images, out=self.embedding_bank[first:first + b])
                self.n_embedded = first + b
        self._embed_fp = (id(mapping_net), mapping_net._fingerprint())   # (a handle built above does not touch the weights)
        return self

    # ------------------------------------------------------------------ reading
    def embedding(self, k):
        """Keyframe k's embedding as `Frame.embedding` holds it: [1,128,h,w], a (permuted) VIEW of the bank row."""
        if not 0 <= k < self.n_embedded:
            raise IndexError("keyframe %d is not embedded (%d of %d are)" % (k, self.n_embedded, self.n))
        h, w = self.embedding_hw
        return self.embedding_bank[k].view(1, h, w, 128).permute(0, 3, 1, 2)

    def images(self, indices):
        """fp32 [n,3,H,W]: `image_bank[indices].float()`, any order, repeats allowed."""
        if self.n == 0:
            raise RuntimeError("the map holds no keyframe")
        return gather_images(self.image_bank[:self.n], indices)

    def rows(self, mu):
        """Queries in the bank's row order: `mu` as MappingVAE returns it, [Q,128,h,w], is permuted to channels-last
        (`mu.permute(0, 2, 3, 1)`, then flattened); a [Q,D] tensor is taken as channels-last already (what
        `MappingVAE.encode_rows` returns)."""
        if mu.dim() == 4:
            h, w = self.embedding_hw
            if tuple(mu.shape[1:]) != (128, h, w):
                raise RuntimeError("expected mu [Q,128,%d,%d], got %s" % (h, w, tuple(mu.shape)))
            return mu.permute(0, 2, 3, 1).contiguous().view(mu.shape[0], self.D)
        if mu.dim() != 2 or mu.shape[1] != self.D:
            raise RuntimeError("expected mu [Q,128,%d,%d] or channels-last rows [Q,%d], got %s"
                               % (self.embedding_hw + (self.D, tuple(mu.shape))))
        return mu

    def search(self, queries_mu, top_k=1):
        """(distances [Q,K] fp32, indices [Q,top_k] int32), device tensors: distances[q, k] = torch.norm(embedding(k) - mu[q]),
        indices[q] = the top_k nearest keyframes, ascending, equal distances by the lower index (indices[q, 0] is the
        reference's argmin). `queries_mu`: see `rows`. 1 <= top_k <= min(K, 16)."""
        if self.n == 0 or self.n_embedded < self.n:
            raise RuntimeError("search: %d of %d keyframes are embedded (call embed(mapping_net) first)" % (self.n_embedded, self.n))
        if not 1 <= int(top_k) <= min(self.n, MAX_TOP_K):
            raise ValueError("top_k must be in [1, min(K, %d)] (K = %d), got %d" % (MAX_TOP_K, self.n, top_k))
        return search_bank(self.embedding_bank[:self.n], self.rows(queries_mu), top_k)

    @torch.no_grad()
    def relocalize(self, images, flow_net, odometry_net, mapping_net, top_k=1, refine=True, verify=False, geometric=False,
                   calib=None):
        """Answer Q relocalisation queries at once (neural_slam.py:355-399 for a batch). images [Q,3,H,W] (or [3,H,W]),
        values 0..255. Returns host tensors `distances` [Q,K], `indices` [Q,top_k] (int64), `initial` [Q,4,4] (the pose of
        the nearest keyframe) and `refined` [Q,4,4] (= initial @ the odometry step from that keyframe's image to the query;
        = initial when `refine` is False): one encoder call, one search, one image gather, the flow network on the Q
        (keyframe, query) pairs in chunks of its `max_batch` (at most 16), the pose head's encoder per chunk and ONE
        recurrent step with Q independent sequences.

        Pose-head state: every query is evaluated from the reset (zero) LSTM state, and the state `odometry_net` carries
        between its own calls is neither read nor changed. The reference's single-query call starts from whatever state
        earlier calls left behind (neural_slam.py:396); a batch has no such order. `NeuralSLAM.__call__` keeps the
        reference's semantics.

        `verify=True` (needs `refine`; ValueError otherwise) puts evidence behind the answer: ALL Q * top_k candidates are
        refined, pair p = q * top_k + r being (keyframe indices[q, r], query q). The pairs go through
        `flow_net.forward_backward` in chunks of max(1, max_batch // 2) pairs, `transforms.flow_consistency` (alpha1 = 0.01,
        alpha2 = 0.5) scores each chunk, the pose head's encoder runs on the forward flows, and ONE recurrent step runs with
        Q * top_k independent sequences from the reset state (the carried state is untouched, as above). Returns the 6-tuple
        `(distances, indices, initial, refined, scores, chosen)`: `scores` [Q,top_k] float32 (host), the share of pixels whose
        forward and backward flow agree — near 0 when the two images show different places; `chosen` [Q] int64, the rank r
        with the largest integer count of such pixels, ties to the lower rank; `initial` and `refined` are those of the chosen
        candidate. With top_k = 1 the poses are those of verify=False (the flows come from batches of another composition:
        equal within rounding, not bit for bit) and `scores` is the confidence. With verify=False the code path, the 4-tuple
        and its bits are unchanged.

        `geometric=True` (needs `refine` and `calib`, the calibration of the map's grid; ValueError otherwise) adds a pose from
        geometry: for every refined pair, `transforms.pose_from_depth` on the keyframe's depth (`set_depth`; zeros where it
        has none) and the forward flow, started at the pose head's relative pose, with the consistency mask as its mask when
        `verify` is on; all pairs of a flow chunk in one batch, nothing synchronises until the results are fetched. Two items
        are appended to the tuple: `refined_geo` [Q,4,4] = initial @ that pose and `geo_counts` [Q,4] int32 = (candidates,
        used, inliers, accepted steps), both of the chosen candidate with `verify`. A keyframe without depth gives
        refined_geo == refined and zero counts. With geometric=False the code paths, the tuples and their bits are unchanged."""
        if verify and not refine:
            raise ValueError("verify=True scores the flows of the refinement: it needs refine=True")
        if geometric and not refine:
            raise ValueError("geometric=True solves for the pose of the refinement's flow: it needs refine=True")
        if geometric and calib is None:
            raise ValueError("geometric=True needs the calibration of the map's grid: pass calib=")
        q = images.to(self.device)
        if q.dim() == 3:
            q = q.unsqueeze(0)
        if q.dim() != 4 or tuple(q.shape[1:]) != (3,) + self.hw:
            raise RuntimeError("expected queries [Q,3,%d,%d], got %s" % (self.hw + (tuple(images.shape),)))
        q = q.float().contiguous()
        Q = int(q.shape[0])
        with torch.cuda.device(self.device):
            mu, _ = mapping_net.encode_rows(q)
            dist, idx = self.search(mu, top_k)
            indices = idx.cpu().long()
            if verify:
                return self._relocalize_verified(q, dist, indices, flow_net, odometry_net, calib if geometric else None)
            best = indices[:, 0]
            initial = self.poses[best].clone()
            if not refine:
                return dist.cpu(), indices, initial, initial.clone()
            keyframes = self.images(best)
            chunk = max(1, min(int(getattr(flow_net, "max_batch", 1)), 16))
            feats, flows = [], []
            for a in range(0, Q, chunk):
                _, flow = flow_net(keyframes[a:a + chunk], q[a:a + chunk], iters=12, test_mode=True)
                feats.append(odometry_net.encode(flow))
                if geometric:
                    flows.append(flow)
            rot, tr, _ = odometry_net.scan(torch.cat(feats, dim=0)[None], state=None, hw=self.hw)
            rot, tr = rot[0].cpu(), tr[0].cpu()
            if geometric:
                geo, geo_counts = self._geometric(best.tolist(), flows, None, rot, tr, calib)
        refined = torch.stack([initial[i] @ transforms.transform(rot[i], tr[i]) for i in range(Q)], dim=0)
        if geometric:
            return dist.cpu(), indices, initial, refined, torch.stack([initial[i] @ geo[i] for i in range(Q)], dim=0), geo_counts
        return dist.cpu(), indices, initial, refined

    def _geometric(self, keyframe_indices, flows, masks, rot, tr, calib):
        """The geometric leg of `relocalize`: `flows` (and `masks`, or None) are the forward flows (consistency masks) of the
        pairs, chunk by chunk, `keyframe_indices` the keyframe of every pair, `rot` / `tr` the pose head's answers on the host.
        Returns host tensors: the PnP poses [P,4,4] and counts [P,4]."""
        head = torch.stack([transforms.transform(rot[p], tr[p]) for p in range(len(keyframe_indices))], dim=0)
        poses, counts, a = [], [], 0
        for c, flow in enumerate(flows):
            b = int(flow.shape[0])
            pose, _, cnt = transforms.pose_from_depth(self.depths(keyframe_indices[a:a + b]), flow, head[a:a + b], calib,
                                                      mask=None if masks is None else masks[c])
            poses.append(pose)
            counts.append(cnt)
            a += b
        return torch.cat(poses).cpu(), torch.cat(counts).cpu()

    def _evaluate_pairs(self, keyframe_indices, images, flow_net, odometry_net, calib=None):
        """The evidence for P pairs (keyframe keyframe_indices[p], images[p]) — shared by `_relocalize_verified` and
        `loop_closure.find_loops`, called under the map's device and no_grad: `flow_net.forward_backward` in chunks of
        max(1, max_batch // 2) pairs, the consistency mask and count of each chunk (alpha1 = 0.01, alpha2 = 0.5), the pose head's
        encoder on the forward flows and ONE recurrent step with P independent sequences from the reset state; with `calib`
        the PnP pose of every pair from the keyframe's depth under the consistency mask. `images` [P,3,H,W] fp32 on the device.
        Returns host tensors (rot [P,3], tr [P,3], counts [P] int64, geo [P,4,4] or None, geo_counts [P,4] or None)."""
        P = len(keyframe_indices)
        keyframes = self.images(keyframe_indices)
        chunk = max(1, int(getattr(flow_net, "max_batch", 1)) // 2)     # 2 * chunk images per flow call
        feats, counts, flows, masks = [], [], [], []
        for a in range(0, P, chunk):
            fw, bw = flow_net.forward_backward(keyframes[a:a + chunk], images[a:a + chunk], iters=12)
            mask, count = transforms._flow_consistency_counts(fw, bw, 0.01, 0.5)
            counts.append(count)
            feats.append(odometry_net.encode(fw))
            if calib is not None:
                flows.append(fw)
                masks.append(mask)
        rot, tr, _ = odometry_net.scan(torch.cat(feats, dim=0)[None], state=None, hw=self.hw)
        rot, tr = rot[0].cpu(), tr[0].cpu()
        geo = geo_counts = None
        if calib is not None:
            geo, geo_counts = self._geometric(list(keyframe_indices), flows, masks, rot, tr, calib)
        return rot, tr, torch.cat(counts).cpu().long(), geo, geo_counts

    def update_poses(self, poses):
        """Replace the poses of all keyframes (after a loop closure): [K,4,4], [K,3,4] or [K,12]; the only writer of the
        map's poses besides `append`. Images, embeddings and depth maps stay: depth lives in the keyframe's own camera."""
        p = _homogeneous(torch.as_tensor(poses).detach().cpu())
        if p.shape[0] != self.n:
            raise ValueError("expected %d poses, got %d" % (self.n, p.shape[0]))
        self._poses[:self.n] = p

    def _relocalize_verified(self, q, dist, indices, flow_net, odometry_net, calib=None):
        """The verify=True half of `relocalize` (called under its device and no_grad): q [Q,3,H,W] fp32 on the device, `dist`
        the device distances, `indices` [Q,top_k] int64 on the host; `calib` not None: with the geometric leg."""
        Q, top_k = int(indices.shape[0]), int(indices.shape[1])
        n = self.hw[0] * self.hw[1]
        flat = indices.reshape(-1)                                   # pair p = q * top_k + r
        queries = q.repeat_interleave(top_k, dim=0) if top_k > 1 else q
        rot, tr, counts, geo, geo_counts = self._evaluate_pairs(flat.tolist(), queries, flow_net, odometry_net, calib)
        counts = counts.view(Q, top_k)
        scores = (counts.double() / float(n)).float()
        chosen = torch.tensor([row.index(max(row)) for row in counts.tolist()], dtype=torch.int64)   # ties: the lower rank
        rows = torch.arange(Q)
        initial = self.poses[indices[rows, chosen]].clone()
        pick = (rows * top_k + chosen).tolist()
        refined = torch.stack([initial[i] @ transforms.transform(rot[p], tr[p]) for i, p in enumerate(pick)], dim=0)
        if calib is not None:
            refined_geo = torch.stack([initial[i] @ geo[p] for i, p in enumerate(pick)], dim=0)
            return dist.cpu(), indices, initial, refined, scores, chosen, refined_geo, geo_counts[pick]
        return dist.cpu(), indices, initial, refined, scores, chosen
