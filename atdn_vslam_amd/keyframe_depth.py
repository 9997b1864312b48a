"""Which keyframe gets its depth from which pairs, and when: the one state machine behind `NeuralSLAM(keyframe_depth=...)`. It
holds no network, no path and no map, and every function it calls has a host form, so it runs on CPU tensors as it does on the
device."""
import collections

from . import transforms
from .depth import FlowTrack, intrinsics

MODES = ("pair", "track", "multiview", "bundle")
HISTORY = 16   # the steps a "multiview" / "bundle" track keeps (transforms.multiview_depth's limit)

# What one keyframe's interval gave. `index`: the keyframe; `depth` [1,1,H,W] on the device ("track": the track's own tensor, which
# the next anchor() clears). "multiview" and "bundle" add `info`,
# `views` and `multiview_counts` (FlowTrack.multiview), "bundle" also `poses` [1,S,12], `cost` [1,2] and `counts` [1,4]
# (FlowTrack.bundle); all on the device. `complete`: the track's window held every step of the interval; `new_keyframe`: the
# interval was closed by the next keyframe, whose frame is then the last step.
KeyframeDepth = collections.namedtuple("KeyframeDepth", "index depth info views multiview_counts poses cost counts complete new_keyframe",
                                       defaults=(None,) * 6 + (False, False))


class KeyframeDepthRecorder:
    """`anchor(index)`: keyframe `index` was just registered, its depth comes from the pairs that follow. `pair(flow, pred_mat)`:
    the next pair of the sequence, `pred_mat` [4,4] its relative pose on the host. `close(new_keyframe)`: the anchor's interval is
    over. `pair` and `close` return a `KeyframeDepth` or None:

    * "pair": the two-view depth (transforms.two_view_depth) of the first pair after `anchor`, from that `pair` call;
    * "track": a FlowTrack is started by `anchor` and extended by every `pair`; `close` returns its depth;
    * "multiview": the track keeps its last 16 steps and `close` returns FlowTrack.multiview (`multiview_options`);
    * "bundle": `close` returns FlowTrack.bundle (`bundle_options`, `multiview_options`).

    `close` returns None when no pair followed the anchor, and always with "pair". Without a calibration (`calib=None`, "pair"
    only) nothing is ever returned. The track (`self.track`) is created by the first `anchor`."""

    def __init__(self, mode, hw, calib, device, multiview_options=None, bundle_options=None):
        if mode not in MODES:
            raise ValueError("mode is one of %s, got %r" % (", ".join(MODES), mode))
        if mode != "pair" and calib is None:
            raise ValueError('mode "%s" needs the calibration' % mode)
        self.mode = mode
        self.hw = hw
        self.calib = None if calib is None else intrinsics(calib)
        self.device = device
        self.multiview_options = dict(multiview_options or {})
        self.bundle_options = dict(bundle_options or {})
        self.track = None
        self._index = None   # the keyframe whose depth is still to come

    def to(self, device):
        """Later pairs arrive on `device`; a running track goes along."""
        self.device = device
        if self.track is not None:
            self.track.to(device)

    def anchor(self, index):
        if self.calib is None:
            return
        if self.mode != "pair":
            if self.track is None:
                self.track = FlowTrack(self.hw, self.calib, self.device, history=HISTORY if self.mode in ("multiview", "bundle") else 0)
            self.track.start()
        self._index = index

    def pair(self, flow, pred_mat):
        if self._index is None:
            return None
        if self.mode != "pair":
            self.track.extend(flow, pred_mat)
            return None
        # the pair's first frame is the keyframe: the flow starts at its pixels, so the depth is the keyframe's
        depth, _ = transforms.two_view_depth(flow, pred_mat[None].to(self.device), self.calib)
        index, self._index = self._index, None
        return KeyframeDepth(index, depth)

    def close(self, new_keyframe=False):
        if self.mode == "pair":
            return None
        index, self._index = self._index, None
        track = self.track
        if index is None or track.steps == 0:
            return None
        if self.mode == "track":
            return KeyframeDepth(index, track.depth, new_keyframe=new_keyframe)
        complete = track.steps <= track.history
        if self.mode == "multiview":
            depth, info, views, counts = track.multiview(**self.multiview_options)
            return KeyframeDepth(index, depth, info, views, counts, complete=complete, new_keyframe=new_keyframe)
        poses, depth, info, views, mv_counts, cost, counts = track.bundle(multiview_options=self.multiview_options, **self.bundle_options)
        return KeyframeDepth(index, depth, info, views, mv_counts, poses, cost, counts, complete, new_keyframe)
