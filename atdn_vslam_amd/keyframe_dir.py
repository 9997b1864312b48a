"""The keyframe directory, `<keyframes_path>`, as the reference and `slam.NeuralSLAM` write it: one table of its outputs, the name
of a keyframe's file in each, save / load, and what a cold start does to each. Nothing here touches a device."""
import glob
import os

import torch

# per-keyframe directories (one `%06d.pth` per keyframe) ...
RGB, DEPTH, DEPTH_FUSED, DEPTH_VIEWS = "rgb", "depth", "depth_fused", "depth_views"
DEPTH_INFO, DEPTH_MV_VIEWS, BUNDLE, GROUND, MAP_DEPTH = "depth_info", "depth_mv_views", "bundle", "ground", "map_depth"
# ... and the files of the whole map
POSES, POSES_CLOSED, POSES_SCALED, WEIGHTS, MAP_PLY = "poses.pth", "poses_closed.pth", "poses_scaled.pth", "MappingVAE_weights.pth", "map.ply"

ALWAYS = "always"
# output -> (what a cold start needs to create the directory, what it needs to remove the output's files): ALWAYS, None (never)
# or the name of an option in `prepare_cold_start(enabled)`. An output that can be created is a directory, the others are files.
# Whatever is not listed (mapping_loss.pth, ...) is never touched.
OUTPUTS = {
    RGB: (ALWAYS, ALWAYS),
    DEPTH: ("calib", ALWAYS),                    # depths of an earlier session go like its frames, calibration or not
    DEPTH_FUSED: ("fuse_depth", "fuse_depth"),   # (without the option nothing is cleared: stale files stay)
    DEPTH_VIEWS: ("fuse_depth", "fuse_depth"),
    DEPTH_INFO: ("multiview", "multiview"),
    DEPTH_MV_VIEWS: ("multiview", "multiview"),
    BUNDLE: ("bundle", "bundle"),
    GROUND: ("ground", "ground"),
    MAP_DEPTH: ("map_depth", "map_depth"),
    POSES_SCALED: (None, "ground"),
    MAP_PLY: (None, "voxel_map"),
    POSES: (None, ALWAYS),                       # a cold start owns the directory: poses and map weights of an earlier session go
    POSES_CLOSED: (None, ALWAYS),
    WEIGHTS: (None, ALWAYS),
}


class KeyframeDir:
    """`base` and the paths under it. `key` names a keyframe's file in a per-keyframe directory: an index (`%06d.pth`, the name
    the odometry gives) or a frame's file name (the same base name, `.pth`)."""

    def __init__(self, base):
        self.base = base

    def path(self, output, key=None):
        if output not in OUTPUTS:
            raise KeyError("%r is no output of a keyframe directory" % (output,))
        if key is None:
            return os.path.join(self.base, output)
        name = os.path.splitext(os.path.basename(key))[0] + ".pth" if isinstance(key, (str, os.PathLike)) else "%06d.pth" % key
        return os.path.join(self.base, output, name)

    def exists(self, output, key=None):
        return os.path.exists(self.path(output, key))

    def save(self, obj, output, key=None):
        torch.save(obj, self.path(output, key))

    def load(self, output, key=None, **options):
        return torch.load(self.path(output, key), **options)

    def frames(self, pattern="*.pth"):
        """The stored frames' files, sorted."""
        return sorted(glob.glob(os.path.join(self.path(RGB), pattern)))

    def create(self, *outputs):
        for output in outputs:
            os.makedirs(self.path(output), exist_ok=True)

    def prepare_cold_start(self, enabled=()):
        """What a session that starts from nothing does to the directory, by `OUTPUTS`. `enabled`: the options that are on, of
        "calib", "fuse_depth", "multiview", "bundle", "ground", "map_depth", "voxel_map"."""
        on = set(enabled) | {ALWAYS}
        unknown = on - {rule for rules in OUTPUTS.values() for rule in rules}
        if unknown:
            raise ValueError("unknown option(s): %s" % ", ".join(sorted(unknown)))
        for output, (create, clear) in OUTPUTS.items():
            if create in on:
                self.create(output)
            if clear in on:
                target = self.path(output)
                for f in glob.glob(os.path.join(target, "*") if create is not None else target):
                    os.remove(f)
