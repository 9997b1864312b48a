"""Range report, host side (no GPU): the walker that the GPU tests measure the report against, and the report's own logic.

The WALKER restates the flow network's forward from `oracle.gma_ref`'s building blocks and torch ops, in the dtype it is given,
and records for every tensor the exact-fp32 GPU path writes — under the row names of the report — the largest finite magnitude,
the finite values beyond 65504 and the non-finite values. It proves itself first: in fp32 its flow equals
`gma_ref.gma_forward`'s bit for bit."""
import io
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from atdn_vslam_amd import synthetic as syn
from oracle import gma_ref
from oracle.gma_ref import _norm, _w

LIMIT = 65504.0

# rows every report must hold: one per tensor outside the loop ...
_FNET_BLOCKS = [("fnet.layer%d.%d" % (l, k), l > 1 and k == 0) for l in (1, 2, 3) for k in (0, 1)]
_CNET_BLOCKS = [("cnet.layer%d.%d" % (l, k), l > 1 and k == 0) for l in (1, 2, 3) for k in (0, 1)]
REQUIRED_ONCE = (
    ["fnet.conv1.raw", "fnet.conv1.out"]
    + [b + s for b, ds in _FNET_BLOCKS for s in [".conv1.raw", ".conv1.out", ".conv2.raw"] + ([".downsample.raw"] if ds else []) + [""]]
    + ["fnet.conv2", "cnet.conv1.out"]
    + [b + s for b, ds in _CNET_BLOCKS for s in [".conv1.out"] + ([".downsample.out"] if ds else []) + [""]]
    + ["net0", "inp", "corr.0", "corr.1", "corr.2", "corr.3", "att.qk", "att.logits", "att.attn", "mask.0", "mask", "flow_up"])
# ... and one per iteration for those written inside it
REQUIRED_PER_ITERATION = ["corr_lookup", "encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv",
                          "aggregator.to_v", "aggregator.out", "gru.z1", "gru.rh1", "gru.h1", "gru.z2", "gru.rh2", "gru.h2",
                          "flow_head.conv1", "flow"]


def scaled_state(scales, seed=1):
    """Synthetic GMA checkpoint with the weights (and biases) of the named layers multiplied by a factor (the construction of
    tests/test_gpu_round3.py::_scaled_state)."""
    sd = syn.make_gma_state(seed=seed)
    for prefix, f in scales.items():
        hit = False
        for k in sd:
            if k.startswith(prefix) and (k.endswith(".weight") or k.endswith(".bias")) and "norm" not in k:
                sd[k] = (sd[k] * f).astype(sd[k].dtype)
                hit = True
        assert hit, prefix
    return syn.to_torch(sd)


class Walk:
    """rows: {(name, iteration): (max_abs, over, nonfinite, {threshold: count of finite |x| > threshold})} in execution order."""

    def __init__(self, thresholds=()):
        self.rows = {}
        self.thresholds = tuple(thresholds)
        self.it = -1
        self.flow_low = self.flow_up = None

    def rec(self, name, t):
        a = t.detach().abs().reshape(-1)
        fin = torch.isfinite(a)
        af = a[fin]
        mx = float(af.max()) if af.numel() else 0.0
        self.rows[(name, self.it)] = (mx, int((af > LIMIT).sum()), int((~fin).sum()),
                                      {th: int((af > th).sum()) for th in self.thresholds})
        return t

    def names(self):
        return [k[0] for k in self.rows]


def _walk_encoder(x, sd, p, kind, rec):
    inst = kind == "instance"
    y = F.conv2d(x, *_w(sd, p + "conv1"), stride=2, padding=3)
    if inst:
        rec(p + "conv1.raw", y)
    x = rec(p + "conv1.out", F.relu(_norm(y, sd, p + "norm1", kind)))
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        for k, s in ((0, stride), (1, 1)):
            q = "%slayer%d.%d." % (p, li, k)
            y = F.conv2d(x, *_w(sd, q + "conv1"), stride=s, padding=1)
            if inst:
                rec(q + "conv1.raw", y)
            y = rec(q + "conv1.out", F.relu(_norm(y, sd, q + "norm1", kind)))
            y = F.conv2d(y, *_w(sd, q + "conv2"), padding=1)
            if inst:
                rec(q + "conv2.raw", y)
            y = F.relu(_norm(y, sd, q + "norm2", kind))
            if s != 1:
                d = F.conv2d(x, *_w(sd, q + "downsample.0"), stride=s)
                if inst:
                    rec(q + "downsample.raw", d)
                x = _norm(d, sd, q + "norm3", kind)
                if not inst:
                    rec(q + "downsample.out", x)
            x = rec(q[:-1], F.relu(x + y))
    return F.conv2d(x, *_w(sd, p + "conv2"))


@torch.no_grad()
def walk(sd, image1, image2, iters, dtype=torch.float32, thresholds=(), flow_init=None):
    sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in gma_ref.strip_prefix(sd).items()}
    W = Walk(thresholds)
    rec = W.rec
    im1 = (2 * (image1.to(dtype) / 255.0) - 1.0).contiguous()
    im2 = (2 * (image2.to(dtype) / 255.0) - 1.0).contiguous()
    rec("image", torch.cat([im1, im2], 0))
    b = im1.shape[0]
    fmaps = rec("fnet.conv2", _walk_encoder(torch.cat([im1, im2], 0), sd, "fnet.", "instance", rec))
    pyr = gma_ref.corr_pyramid(fmaps[:b], fmaps[b:])
    for l, c in enumerate(pyr):
        rec("corr.%d" % l, c)
    cnet = _walk_encoder(im1, sd, "cnet.", "batch", rec)
    net, inp = torch.split(cnet, [128, 128], dim=1)
    net = rec("net0", torch.tanh(net))
    inp = rec("inp", torch.relu(inp))
    # gma_ref.attention, with its intermediates
    _, c, h8, w8 = inp.shape
    qk = F.conv2d(inp, sd["att.to_qk.weight"])
    q, k = qk.chunk(2, dim=1)
    q = q.reshape(b, c, h8 * w8).transpose(1, 2) * (c ** -0.5)
    k = k.reshape(b, c, h8 * w8)
    rec("att.qk", torch.cat([q.reshape(-1), k.reshape(-1)]))
    attn = rec("att.attn", torch.softmax(rec("att.logits", torch.matmul(q, k)), dim=-1))
    coords0 = gma_ref.coords_grid(b, h8, w8, dtype)
    coords1 = gma_ref.coords_grid(b, h8, w8, dtype)
    if flow_init is not None:
        coords1 = coords1 + flow_init.to(dtype)
    rec("flow_init", coords1 - coords0)
    e, g, u = "update_block.encoder.", "update_block.gru.", "update_block."
    for it in range(iters):
        W.it = it
        corr = rec("corr_lookup", gma_ref.corr_lookup(pyr, coords1))
        flow = coords1 - coords0
        # gma_ref.motion_encoder
        cor = rec("encoder.convc1", F.relu(F.conv2d(corr, *_w(sd, e + "convc1"))))
        cor = rec("encoder.convc2", F.relu(F.conv2d(cor, *_w(sd, e + "convc2"), padding=1)))
        flo = rec("encoder.convf1", F.relu(F.conv2d(flow, *_w(sd, e + "convf1"), padding=3)))
        flo = rec("encoder.convf2", F.relu(F.conv2d(flo, *_w(sd, e + "convf2"), padding=1)))
        out = rec("encoder.conv", F.relu(F.conv2d(torch.cat([cor, flo], 1), *_w(sd, e + "conv"), padding=1)))
        mf = torch.cat([out, flow], 1)
        # gma_ref.aggregate
        v = rec("aggregator.to_v", F.conv2d(mf, sd[u + "aggregator.to_v.weight"])).reshape(b, c, h8 * w8)
        agg = torch.matmul(attn, v.transpose(1, 2)).transpose(1, 2).reshape(b, c, h8, w8)
        mfg = rec("aggregator.out", mf + sd[u + "aggregator.gamma"] * agg)
        # gma_ref.sep_conv_gru
        x = torch.cat([inp, mf, mfg], 1)
        for tag, pad in (("1", (0, 2)), ("2", (2, 0))):
            hx = torch.cat([net, x], 1)
            z = rec("gru.z" + tag, torch.sigmoid(F.conv2d(hx, *_w(sd, g + "convz" + tag), padding=pad)))
            r = torch.sigmoid(F.conv2d(hx, *_w(sd, g + "convr" + tag), padding=pad))
            rh = rec("gru.rh" + tag, r * net)
            qq = torch.tanh(F.conv2d(torch.cat([rh, x], 1), *_w(sd, g + "convq" + tag), padding=pad))
            net = rec("gru.h" + tag, (1 - z) * net + z * qq)
        # gma_ref.flow_head
        f1 = rec("flow_head.conv1", F.relu(F.conv2d(net, *_w(sd, u + "flow_head.conv1"), padding=1)))
        coords1 = coords1 + F.conv2d(f1, *_w(sd, u + "flow_head.conv2"), padding=1)
        rec("flow", coords1 - coords0)
        rec("coords1", coords1)
    W.it = -1
    # gma_ref.up_mask
    m0 = rec("mask.0", F.relu(F.conv2d(net, *_w(sd, u + "mask.0"), padding=1)))
    mask = rec("mask", 0.25 * F.conv2d(m0, *_w(sd, u + "mask.2")))
    W.flow_low = rec("flow_low", coords1 - coords0)
    W.flow_up = rec("flow_up", gma_ref.convex_upsample(W.flow_low, mask))
    return W


def test_walker_reproduces_the_oracle_bit_for_bit():
    sd = syn.to_torch(syn.make_gma_state(seed=1))
    fr = torch.from_numpy(syn.make_frames(2, 160, 512, seed=3))
    low, up = gma_ref.gma_forward(sd, fr[0:1], fr[1:2], iters=2)
    W = walk(sd, fr[0:1], fr[1:2], 2)
    assert W.flow_low.dtype == torch.float32
    assert torch.equal(W.flow_low, low) and torch.equal(W.flow_up, up)
    names = W.names()
    for n in REQUIRED_ONCE:
        assert names.count(n) == 1, n
    for n in REQUIRED_PER_ITERATION:
        assert [k[1] for k in W.rows if k[0] == n] == [0, 1], n
    assert all(v[1] == 0 and v[2] == 0 for v in W.rows.values())
    # the counting itself: strict "> 65504", non-finite values counted apart and kept out of the maximum
    W2 = Walk(thresholds=(1.0,))
    W2.rec("t", torch.tensor([0.0, -0.0, 65504.0, -np.nextafter(np.float32(65504), np.float32(np.inf)), np.inf, -np.inf, np.nan, -3.0]))
    assert W2.rows[("t", -1)] == (float(np.nextafter(np.float32(65504), np.float32(np.inf))), 1, 3, {1.0: 3})


# ------------------------------------------------------------------------------------------------ RangeReport logic
def _rr():
    from atdn_vslam_amd import range_report
    return range_report


def _rows(**over):
    """A small forward: two tensors outside the loop, two inside it for three iterations, one after."""
    rows = [("fnet.conv2", -1, True, 40.0, 0, 0), ("corr.0", -1, False, 9.0e4, 12, 0), ("att.logits", -1, False, 2.6e6, 900, 0)]
    for it, (a, b) in enumerate([(5.0e3, 10.0), (6.0e3, 30.0), (5.5e3, 20.0)]):
        rows += [("corr_lookup", it, True, a, 0, 0), ("gru.h2", it, True, b, 0, 0)]
    rows.append(("mask", -1, False, 7.0e4, 3, 0))
    rows = [list(r) for r in rows]
    for (name, it), (mx, ov, nf) in over.get("set", {}).items():
        for r in rows:
            if r[0] == name and r[1] == it:
                r[3], r[4], r[5] = mx, ov, nf
    return [tuple(r) for r in rows]


def test_verdicts_worst_and_first_over():
    rr = _rr()
    rep = rr.RangeReport(_rows(), default_clamped=0, flow_diff=2e-5)
    # unlimited rows are far over the limit and count for nothing
    assert rep.verdict == rr.IN_RANGE == "in range" and rep.exit_status == 0
    assert rep.first_over is None
    assert (rep.worst.name, rep.worst.iteration, rep.worst.max_abs) == ("corr_lookup", 1, 6.0e3)
    assert rep.headroom == pytest.approx(65504.0 / 6.0e3)
    assert rep.rows[0].headroom == pytest.approx(65504.0 / 40.0)
    # no limited row over, yet the default path clamped
    rep = rr.RangeReport(_rows(), default_clamped=17)
    assert rep.verdict == rr.CLAMPS_OUTSIDE == "clamps outside the stored activations" and rep.exit_status == 3
    # not run: nothing known against the checkpoint
    assert rr.RangeReport(_rows()).verdict == rr.IN_RANGE and rr.RangeReport(_rows()).default_clamped is None
    # first_over is by execution order, not by magnitude
    rep = rr.RangeReport(_rows(set={("gru.h2", 0): (7.0e4, 2, 0), ("corr_lookup", 2): (9.0e9, 50, 0)}), default_clamped=52)
    assert (rep.first_over.name, rep.first_over.iteration) == ("gru.h2", 0)
    assert (rep.worst.name, rep.worst.iteration) == ("corr_lookup", 2)
    assert rep.verdict == rr.OUT_OF_RANGE == "out of range" and rep.exit_status == 3 and rep.headroom < 1
    # a limited row over decides, whatever the counter says
    assert rr.RangeReport(rep.rows, default_clamped=0).verdict == rr.OUT_OF_RANGE
    # non-finite values count as over although they do not enter the maximum
    rep = rr.RangeReport(_rows(set={("gru.h2", 1): (1.0, 0, 4)}))
    assert (rep.first_over.name, rep.first_over.iteration) == ("gru.h2", 1) and rep.verdict == rr.OUT_OF_RANGE
    assert rep.worst.name == "corr_lookup"
    # an all-zero tensor has infinite headroom
    assert math.isinf(rr.Row("flow_init", -1, True, 0.0, 0, 0).headroom)
    assert rr.RangeReport([]).worst is None and rr.RangeReport([]).verdict == rr.IN_RANGE


def test_folding_table_and_json_round_trip():
    rr = _rr()
    rep = rr.RangeReport(_rows(set={("gru.h2", 2): (7.0e4, 2, 1)}), default_clamped=3, flow_diff=0.5, seconds=1.25)
    folded = rep.folded()
    assert [r.name for r, _ in folded] == ["fnet.conv2", "corr.0", "att.logits", "corr_lookup", "gru.h2", "mask"]
    by = {r.name: (r, n) for r, n in folded}
    assert by["corr_lookup"][1] == 3 and (by["corr_lookup"][0].iteration, by["corr_lookup"][0].max_abs) == (1, 6.0e3)
    assert (by["gru.h2"][0].iteration, by["gru.h2"][0].max_abs, by["gru.h2"][0].over, by["gru.h2"][0].nonfinite) == (2, 7.0e4, 2, 1)
    assert by["fnet.conv2"][1] == 1 and by["fnet.conv2"][0].iteration == -1
    text = str(rep)
    assert text == rep.table()
    lines = text.splitlines()
    assert len([l for l in lines if l.startswith("gru.h2")]) == 1 and "<-- over" in [l for l in lines if l.startswith("gru.h2")][0]
    assert "<-- over" not in [l for l in lines if l.startswith("corr.0")][0]      # over, but not limited
    assert "verdict: out of range" in text and "3 value(s) clamped" in text and "gru.h2 (iteration 2)" in text
    d = json.loads(rep.to_json())
    assert d["verdict"] == "out of range" and d["worst"]["name"] == "gru.h2" and d["first_over"]["iteration"] == 2
    assert d["default_clamped"] == 3 and d["limit"] == 65504.0 and len(d["rows"]) == len(rep.rows)
    back = rr.RangeReport.from_json(rep.to_json())
    assert back.rows == rep.rows and back.default_clamped == 3 and back.flow_diff == 0.5 and back.seconds == 1.25
    assert back.to_json() == rep.to_json()
    assert json.loads(rr.RangeReport([("flow_init", -1, True, 0.0, 0, 0)]).to_json())["headroom"] is None   # no infinity in JSON


def test_merging_of_pairs():
    rr = _rr()
    a = rr.RangeReport(_rows(), default_clamped=0, flow_diff=1e-5, seconds=1.0)
    b = rr.RangeReport(_rows(set={("gru.h2", 1): (7.0e4, 2, 1), ("fnet.conv2", -1): (35.0, 0, 0)}), default_clamped=5, flow_diff=3e-5,
                       seconds=2.0)
    m = rr.RangeReport.merge([a, b])
    assert m.pairs == 2 and m.default_clamped == 5 and m.flow_diff == 3e-5 and m.seconds == 3.0
    assert m.find("fnet.conv2", -1).max_abs == 40.0                      # maximum of the maxima
    h = m.find("gru.h2", 1)
    assert (h.max_abs, h.over, h.nonfinite) == (7.0e4, 2, 1)
    assert m.find("corr.0", -1).over == 24                               # sums of the counts
    assert m.verdict == rr.OUT_OF_RANGE and [r.iteration for r in m.find("gru.h2")] == [0, 1, 2]
    assert rr.RangeReport.merge([a]).rows == a.rows
    assert rr.RangeReport.merge([a, rr.RangeReport(_rows())]).default_clamped == 0      # None: that pair did not run the default path
    with pytest.raises(ValueError):
        rr.RangeReport.merge([a, rr.RangeReport(_rows()[:-1])])
    with pytest.raises(ValueError):
        rr.RangeReport.merge([])


def test_driver_arguments_merge_and_exit_status(capsys):
    rr = _rr()
    a = rr.parse_args(["--synthetic"])
    assert a.synthetic and a.size == (376, 1232) and a.iters == 12 and a.pairs == 1 and not a.json and a.flow_weights is None
    a = rr.parse_args(["--flow-weights", "w.pth", "--kitti", "/data", "--sequence", "05", "--pairs", "4", "--size", "160x512",
                       "--iters", "8", "--json"])
    assert (a.kitti, a.sequence, a.pairs, a.size, a.iters, a.json, a.flow_weights) == ("/data", "05", 4, (160, 512), 8, True, "w.pth")
    for bad in (["--frames", "d"],                                        # real frames need a checkpoint
                ["--synthetic", "--kitti", "/data"],                      # one source of frames
                [],                                                       # ... and at least one
                ["--synthetic", "--size", "376"], ["--synthetic", "--pairs", "0"], ["--synthetic", "--iters", "65"]):
        with pytest.raises(SystemExit) as ei:
            rr.parse_args(bad)
        assert ei.value.code == 2
    capsys.readouterr()

    seen = {}

    def fake(args, bad=False):
        seen["args"] = args
        reps = [rr.RangeReport(_rows(), default_clamped=0, flow_diff=1e-5, seconds=0.5) for _ in range(args.pairs)]
        if bad:
            reps[-1] = rr.RangeReport(_rows(set={("corr_lookup", 0): (8.2e4, 7, 0)}), default_clamped=7, seconds=0.5)
        return reps
    out = io.StringIO()
    assert rr.main(["--synthetic", "--pairs", "3"], report_fn=fake, out=out) == 0
    assert seen["args"].pairs == 3 and "verdict: in range" in out.getvalue() and "pairs: 3" in out.getvalue()
    out = io.StringIO()
    assert rr.main(["--synthetic", "--pairs", "2", "--json"], report_fn=lambda a: fake(a, bad=True), out=out) == 3
    d = json.loads(out.getvalue())
    assert d["verdict"] == "out of range" and d["pairs"] == 2 and d["first_over"]["name"] == "corr_lookup"
    assert d["first_over"]["over"] == 7 and d["default_clamped"] == 7
    out = io.StringIO()
    assert rr.main(["--synthetic"], report_fn=lambda a: [rr.RangeReport(_rows(), default_clamped=9)], out=out) == 3
    assert "clamps outside the stored activations" in out.getvalue()


def test_the_report_is_wired_through_every_layer():
    """The entry points the GPU tests go through exist and agree: C ABI table, module method, row names."""
    import inspect
    from atdn_vslam_amd import _lib
    from atdn_vslam_amd.modules import RAFTGMA
    for n in ("atdn_gma_set_range_probe", "atdn_gma_range_rows", "atdn_gma_range_row", "atdn_range_probe", "atdn_range_probe_launch"):
        assert n in _lib.SIGNATURES
    sig = inspect.signature(RAFTGMA.range_report)
    assert list(sig.parameters) == ["self", "image1", "image2", "iters", "flow_init", "check_default"]
    assert sig.parameters["iters"].default == 12 and sig.parameters["check_default"].default is True
    assert len(set(REQUIRED_ONCE)) == len(REQUIRED_ONCE) == 56
