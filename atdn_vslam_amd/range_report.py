"""Range report: how far a checkpoint's activations are from the limit of the split-f16 format, before it clamps.

The default arithmetic of the flow network stores activations as f16 pairs and is fp32-grade only while |activation| <= 65504
(csrc/sf.h). `RAFTGMA.range_report` runs a pair of frames once through a private exact-fp32 handle with the library's range
probe on (csrc/range_probe.hip: per written tensor the largest magnitude, the finite values beyond 65504 and the non-finite
values, reduced on the device) and once through a private split-f16 handle whose clamp count it reads; this module holds what
happens after the rows have been read back — plain host Python, usable from a list of rows without a GPU — and the driver:

    python -m atdn_vslam_amd.range_report --flow-weights gma-kitti.pth --kitti DATA_PATH --sequence 00 --pairs 8
    python -m atdn_vslam_amd.range_report --synthetic [--json]

Exit status 0: in range; 3: out of range, or the default path clamped.
"""
import argparse
import collections
import json
import math
import os
import sys

LIMIT = 65504.0   # largest finite f16: the range of the split-f16 storage format (csrc/sf.h)

IN_RANGE = "in range"
OUT_OF_RANGE = "out of range"
CLAMPS_OUTSIDE = "clamps outside the stored activations"
EXIT_OUT_OF_RANGE = 3


class Row(collections.namedtuple("Row", "name iteration limited max_abs over nonfinite")):
    """One probed tensor. `iteration`: 0-based refinement iteration, -1 for tensors written outside the loop. `limited`: the
    default path keeps this tensor (or values that are its, one to one) in the range-limited format. `max_abs`: largest finite
    magnitude; `over`: finite values with |x| > 65504; `nonfinite`: infinities and NaNs."""
    __slots__ = ()

    @property
    def headroom(self):
        return LIMIT / self.max_abs if self.max_abs > 0 else math.inf

    @property
    def bad(self):
        return self.over + self.nonfinite > 0


def _row(r):
    if isinstance(r, Row):
        return r
    if isinstance(r, dict):
        r = [r[k] for k in Row._fields]
    name, it, limited, mx, over, nonf = r
    return Row(str(name), int(it), bool(limited), float(mx), int(over), int(nonf))


class RangeReport:
    """`rows` in execution order; `default_clamped`: what the default path's saturation counter read on the same frames (None:
    not run); `flow_diff`: max |flow_up(default) - flow_up(f32)| in px (None: not run); `seconds`: wall time of the call."""

    def __init__(self, rows, default_clamped=None, flow_diff=None, seconds=None, pairs=1):
        self.rows = [_row(r) for r in rows]
        self.default_clamped = None if default_clamped is None else int(default_clamped)
        self.flow_diff = None if flow_diff is None else float(flow_diff)
        self.seconds = None if seconds is None else float(seconds)
        self.pairs = int(pairs)

    # ---- what the rows say
    @property
    def worst(self):
        """The limited row with the largest magnitude, over all iterations (the first one on a tie); None without limited rows."""
        best = None
        for r in self.rows:
            if r.limited and (best is None or r.max_abs > best.max_abs):
                best = r
        return best

    @property
    def headroom(self):
        w = self.worst
        return w.headroom if w is not None else math.inf

    @property
    def first_over(self):
        """The first limited row, in execution order, that holds a value beyond the limit or a non-finite one."""
        for r in self.rows:
            if r.limited and r.bad:
                return r
        return None

    @property
    def verdict(self):
        if self.first_over is not None:
            return OUT_OF_RANGE
        if self.default_clamped:
            return CLAMPS_OUTSIDE
        return IN_RANGE

    @property
    def exit_status(self):
        return 0 if self.verdict == IN_RANGE else EXIT_OUT_OF_RANGE

    def find(self, name, iteration=None):
        """Rows of that name (all iterations), or the one row of that iteration."""
        hit = [r for r in self.rows if r.name == name and (iteration is None or r.iteration == iteration)]
        if iteration is None:
            return hit
        if len(hit) != 1:
            raise KeyError("%d rows named %r at iteration %r" % (len(hit), name, iteration))
        return hit[0]

    def folded(self):
        """Per-iteration rows folded into one per name, in order of first appearance: (Row with the maximum of the maxima and
        the sums of the counts, its `iteration` = the one where the maximum occurred — the first on a tie — or -1; number of
        rows folded)."""
        order, acc = [], {}
        for r in self.rows:
            if r.name not in acc:
                order.append(r.name)
                acc[r.name] = [r, 1]
                continue
            a = acc[r.name]
            best = a[0]
            it = r.iteration if r.max_abs > best.max_abs else best.iteration
            a[0] = Row(r.name, it, best.limited or r.limited, max(best.max_abs, r.max_abs), best.over + r.over,
                       best.nonfinite + r.nonfinite)
            a[1] += 1
        return [(acc[n][0], acc[n][1]) for n in order]

    # ---- presentation
    def table(self):
        lines = ["%-30s %5s %8s %13s %10s %9s %9s" % ("tensor", "iter", "limited", "max |x|", "headroom", "> 65504", "non-fin")]
        for r, n in self.folded():
            it = "-" if r.iteration < 0 else ("%d/%d" % (r.iteration, n))
            head = "inf" if math.isinf(r.headroom) else "%.3g" % r.headroom
            lines.append("%-30s %5s %8s %13.6g %10s %9d %9d%s" % (r.name, it, "yes" if r.limited else "no", r.max_abs, head, r.over,
                                                                 r.nonfinite, "  <-- over" if r.limited and r.bad else ""))
        w = self.worst
        lines.append("")
        if w is not None:
            lines.append("worst limited tensor: %s%s  max |x| = %.6g  headroom to 65504 = %.4gx"
                         % (w.name, "" if w.iteration < 0 else " (iteration %d)" % w.iteration, w.max_abs, w.headroom))
        f = self.first_over
        if f is not None:
            lines.append("first limited tensor over the limit: %s%s  (%d over, %d non-finite)"
                         % (f.name, "" if f.iteration < 0 else " (iteration %d)" % f.iteration, f.over, f.nonfinite))
        if self.default_clamped is not None:
            lines.append("default (split-f16) path on the same frames: %d value(s) clamped%s"
                         % (self.default_clamped, "" if self.flow_diff is None else "; max |flow_up - flow_up(f32)| = %.3g px" % self.flow_diff))
        lines.append("pairs: %d%s" % (self.pairs, "" if self.seconds is None else "; %.2f s" % self.seconds))
        lines.append("verdict: %s" % self.verdict)
        return "\n".join(lines)

    __str__ = table

    def to_dict(self):
        w, f = self.worst, self.first_over

        def num(x):   # JSON has no infinity
            return None if x is None or math.isinf(x) or math.isnan(x) else x
        return {"verdict": self.verdict, "headroom": num(self.headroom), "worst": None if w is None else w._asdict(),
                "first_over": None if f is None else f._asdict(), "default_clamped": self.default_clamped,
                "flow_diff": num(self.flow_diff), "seconds": self.seconds, "pairs": self.pairs, "limit": LIMIT,
                "rows": [r._asdict() for r in self.rows]}

    def to_json(self, **kw):
        return json.dumps(self.to_dict(), **kw)

    @classmethod
    def from_json(cls, text):
        d = json.loads(text) if isinstance(text, str) else text
        return cls(d["rows"], d.get("default_clamped"), d.get("flow_diff"), d.get("seconds"), d.get("pairs", 1))

    @classmethod
    def merge(cls, reports):
        """Several pairs as one report, row by row (the rows of a forward do not depend on the frames: same names, same order):
        maxima of the maxima, sums of the counts and of the clamp counts, the largest flow difference, the total time."""
        reports = list(reports)
        if not reports:
            raise ValueError("nothing to merge")
        keys = [(r.name, r.iteration) for r in reports[0].rows]
        rows = list(reports[0].rows)
        for rep in reports[1:]:
            if [(r.name, r.iteration) for r in rep.rows] != keys:
                raise ValueError("reports with different rows cannot be merged (another frame size or iteration count?)")
            rows = [Row(a.name, a.iteration, a.limited or b.limited, max(a.max_abs, b.max_abs), a.over + b.over,
                        a.nonfinite + b.nonfinite) for a, b in zip(rows, rep.rows)]

        def total(vals, fn):
            vals = [v for v in vals if v is not None]
            return fn(vals) if vals else None
        return cls(rows, total([r.default_clamped for r in reports], sum), total([r.flow_diff for r in reports], max),
                   total([r.seconds for r in reports], sum), sum(r.pairs for r in reports))


# ------------------------------------------------------------------------------------------------ driver
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m atdn_vslam_amd.range_report", description=__doc__.split("\n\n")[0])
    ap.add_argument("--flow-weights", help="GMA checkpoint (torch.load; with or without the DataParallel prefix)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--frames", metavar="DIR", help="directory of frames (*.png / *.jpg), taken in sorted order")
    src.add_argument("--kitti", metavar="DATA_PATH", help="KITTI odometry root: <DATA_PATH>/dataset/sequences/<seq>/image_2")
    src.add_argument("--synthetic", action="store_true", help="seeded synthetic frames (and checkpoint, without --flow-weights)")
    ap.add_argument("--sequence", default="00")
    ap.add_argument("--pairs", type=int, default=1, help="consecutive frame pairs to run (merged row by row)")
    ap.add_argument("--size", default="376x1232", help="HxW the frames are resized to, as NeuralSLAM does")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--json", action="store_true", help="print the merged report as one JSON document instead of the table")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    try:
        h, w = (int(v) for v in a.size.lower().split("x"))
    except ValueError:
        ap.error("--size must look like 376x1232")
    if h < 128 or w < 128:
        ap.error("--size: frames must be at least 128x128 (level 3 of the correlation pyramid needs at least 2x2 cells)")
    a.size = (h, w)
    if a.pairs < 1:
        ap.error("--pairs must be at least 1")
    if not 1 <= a.iters <= 64:
        ap.error("--iters must be in 1..64")
    if not a.synthetic and not a.flow_weights:
        ap.error("--flow-weights is required unless --synthetic")
    return a


def _load_frames(a):
    """uint8 / float frames [pairs + 1, 3, H, W] in host memory."""
    import torch
    n = a.pairs + 1
    if a.synthetic:
        from . import synthetic
        return torch.from_numpy(synthetic.make_frames(n, a.size[0], a.size[1], seed=3))
    from . import flowbank
    if a.kitti:
        seq = flowbank.KittiSequence(a.kitti, a.sequence)
        try:
            if len(seq) < n:
                raise SystemExit("sequence %s has %d frames, %d pairs need %d" % (a.sequence, len(seq), a.pairs, n))
            return seq[0:n].clone()
        finally:
            seq.close()
    files = sorted(f for f in os.listdir(a.frames) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    if len(files) < n:
        raise SystemExit("%s holds %d frames, %d pairs need %d" % (a.frames, len(files), a.pairs, n))
    return torch.stack([flowbank._decode_png(os.path.join(a.frames, f)) for f in files[:n]])


def _gpu_reports(a):
    """One RangeReport per pair: frames through resize_frames / InputPadder as NeuralSLAM feeds the flow network."""
    import torch
    from . import synthetic, transforms
    from .modules import RAFTGMA
    from .pipeline import resize_frames
    if a.flow_weights:
        state = torch.load(a.flow_weights, map_location="cpu")
        state = state.get("state_dict", state) if isinstance(state, dict) else state
    else:
        state = synthetic.to_torch(synthetic.make_gma_state(seed=1))
    net = RAFTGMA()
    net.load_state_dict(state)
    net = net.to(a.device).eval()
    frames = _load_frames(a).to(a.device)
    frames = resize_frames(frames if frames.dtype == torch.uint8 else frames.float(), a.size).float()
    frames = transforms.InputPadder((3,) + tuple(a.size)).pad(frames)[0]
    return [net.range_report(frames[i:i + 1], frames[i + 1:i + 2], iters=a.iters) for i in range(a.pairs)]


def main(argv=None, report_fn=None, out=None):
    """`report_fn(args) -> [RangeReport per pair]` replaces the GPU run (tests)."""
    a = parse_args(argv)
    out = out or sys.stdout
    rep = RangeReport.merge((report_fn or _gpu_reports)(a))
    out.write((rep.to_json() if a.json else rep.table()) + "\n")
    return rep.exit_status


if __name__ == "__main__":
    sys.exit(main())
