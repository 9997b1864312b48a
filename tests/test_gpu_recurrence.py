"""The pose head's recurrence (ClvoNet::step: lstm1 -> lstm_linear + Mish -> lstm2 -> regressors) against the fp64 oracle on EVERY
route a scan can take — per-step kernel launched eagerly (1), the same launches replayed from a hipGraph (2), the persistent
one-launch scan (3) — with batched rows, a non-zero initial state, row counts around the input-projection GEMM's tile edges,
graphs re-captured after a buffer growth or a cache eviction, the state carried from one route to the next, and inputs that
saturate the gates and both branches of Mish. Every test first proves its route through ATDNVO.last_scan_path.

Yardstick (tests/parity_check.py, as tests/test_gpu_train_geometry.py): rot, tr, h1, c1, h2, c2 each within
M_ENC x the fp32 CPU oracle's own error on that tensor + 1e-6 of its largest magnitude; tests/test_recurrence_oracle.py shows
on the CPU that this flags a one-unit error by >= 38x. `pytest -s` prints every comparison ("PARITY" / "PARITY-WORST" lines)."""
import contextlib
import os
import sys

import pytest
import torch

from atdn_vslam_amd import synthetic as syn
from atdn_vslam_amd.modules import ATDNVO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recurrence_ref as rr  # noqa: E402
from parity_check import Checker  # noqa: E402
from recurrence_ref import MISH, SAT30, SAT1000, mish_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

M_ENC, FLOOR_ENC = 2.5, 1e-6      # ordinary-scale inputs, as tests/test_gpu_train_geometry.py (observed 0.107 eager, 0.269 graph
                                  # replay: graph/T1024/B1 rot, 0.376 persistent: persistent/T130/B1 rot, 0.307 carried across routes)
M_SAT = 5.0                       # saturated gates and Mish extremes (observed 1.48: sat/persistent/amp1000/T24/B1 c2; per-step kernel
                                  # 1.44: sat/per_step/amp1000/T24/B1 c2; Mish 1.37: mish/persistent/T24/B1 rot). Calibrated with M = 20:
                                  # 3x the worst need_m (a maximum of a rounding-noise ratio over a few thousand values moves by ~2x
                                  # between seeds), rounded up to one digit, never below M_ENC, never above 20 (M_ITER)

EAGER, GRAPH, PERSISTENT, GAVE_UP = 1, 2, 3, 4
SWITCHES = ("ATDN_SCAN_PERSISTENT", "ATDN_NO_GRAPH")
PER_STEP_EAGER = {"ATDN_SCAN_PERSISTENT": "0", "ATDN_NO_GRAPH": "1"}
PER_STEP_GRAPHED = {"ATDN_SCAN_PERSISTENT": "0"}
DEFAULT = {}

ORDINARY = dict(amp=1.0, s=0.2)
# the longest sequence each batch-row count of the ordinary family is asked for: ONE oracle run per (Bs, dtype) serves them all
TMAX = {1: 1025, 2: 1026, 3: 43, 4: 600, 5: 20, 64: 1}


@contextlib.contextmanager
def _env(switches):
    """Both scan switches as given (absent = unset) for the duration; they are read when a handle is finalized."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        if k in switches:
            os.environ[k] = switches[k]
        else:
            os.environ.pop(k, None)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _head(sd, switches, max_bs=1):
    """A fresh module whose handle (wide enough for max_bs rows: a wider scan later would rebuild it under another environment)
    was finalized under `switches`."""
    with _env(switches):
        h = ATDNVO()
        h.load_state_dict(sd)
        h = h.to(DEV).eval()
        h.scan(torch.zeros(2, max_bs, 512, device=DEV))   # the handle exists now (T = 2 is never graphed, never persistent)
    assert h.last_scan_path == EAGER
    return h


@pytest.fixture(scope="module")
def sd():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return syn.to_torch(syn.make_clvo_state(seed=1))


@pytest.fixture(scope="module")
def sd_mish(sd):
    return mish_state(sd)


def _inputs(T, Bs, fam):
    st = rr.make_state(Bs, fam["s"], fam["seed"])
    return rr.make_feats(T, Bs, fam["amp"], fam["seed"]).to(DEV), None if st is None else st.to(DEV)


def _want(tag, sd, T, Bs, fam, tmax=None):
    """(fp32, fp64) oracle results of the first T steps of the family, from the module's cache."""
    return tuple(rr.prefix(rr.cached_oracle(tag, sd, max(T, tmax or T), Bs, fam["amp"], fam["s"], fam["seed"], dt), T)
                 for dt in (torch.float32, torch.float64))


def _ordinary(Bs):
    return dict(ORDINARY, seed=1000 + Bs)


def _check(case, got, want, m=M_ENC):
    """rot, tr and the four state tensors SEPARATELY against both oracles; a violation names the first bad step and batch row."""
    rot, tr, st = got
    o32, o64 = want
    chk = Checker(case, m, FLOOR_ENC)
    have = {"rot": rot, "tr": tr, "h1": st[0], "c1": st[1], "h2": st[2], "c2": st[3]}
    for k in ("rot", "tr") + rr.STATE_NAMES:
        chk(k, have[k], o32[k], o64[k])
    for line in chk.bad:
        k = line.split(":")[0]
        err = (have[k].detach().cpu().double() - o64[k]).abs()
        if k in ("rot", "tr"):
            per_step = err.amax(dim=(1, 2))
            first = int((per_step > 0.5 * float(per_step.max())).nonzero()[0])
            print("LOCALISE %s %s: first step at half the worst error %d of %d; worst batch row %d" % (
                case, k, first, err.shape[0], int(err.amax(dim=(0, 2)).argmax())))
        else:
            print("LOCALISE %s %s: worst batch row %d, unit %d" % (case, k, int(err.amax(dim=1).argmax()), int(err.amax(dim=0).argmax())))
    chk.finish()


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ a. the per-step kernel, launched eagerly
@pytest.fixture(scope="module")
def eager_head(sd):
    return _head(sd, PER_STEP_EAGER, max_bs=64)


EAGER_SHAPES = [(1, 1), (1, 2), (3, 1), (1, 64),          # T < 4: never graphed
                (4, 2), (5, 3),                            # the smallest graphable lengths
                (31, 1), (16, 2), (11, 3),                 # 31 / 32 / 33 rows of the input-projection GEMM
                (127, 1), (64, 2), (43, 3),                # 127 / 128 / 129 rows
                (20, 5),                                   # 100 rows
                (1026, 2)]                                 # T > kMaxGraphedSteps


@pytest.mark.parametrize("T,Bs", EAGER_SHAPES, ids=["T%d-B%d" % s for s in EAGER_SHAPES])
def test_per_step_kernel_batched_rows_and_gemm_tails(sd, eager_head, T, Bs):
    """ATDN_NO_GRAPH=1, ATDN_SCAN_PERSISTENT=0: every call is T + 2 eager launches behind one GEMM of T * Bs rows, from a
    non-zero state. A second call of the same shape stays eager and gives the same bits."""
    fam = _ordinary(Bs)
    f, st = _inputs(T, Bs, fam)
    a = eager_head.scan(f, state=st)
    assert eager_head.last_scan_path == EAGER
    b = eager_head.scan(f, state=st)
    assert eager_head.last_scan_path == EAGER
    torch.cuda.synchronize()
    assert _same_bits(a, b)
    _check("eager/T%d/B%d" % (T, Bs), a, _want("seed1", sd, T, Bs, fam, TMAX.get(Bs)))


def test_per_step_kernel_relocalisation_pattern_of_33_candidates(sd, eager_head):
    """keyframe_map's batched relocalisation: scan(feats[None]) with one row per candidate and no state given."""
    fam = dict(amp=1.0, s=None, seed=1033)
    f, _ = _inputs(1, 33, fam)
    got = eager_head.scan(f)
    assert eager_head.last_scan_path == EAGER
    _check("eager/reloc/T1/B33", got, _want("seed1", sd, 1, 33, fam))


# ------------------------------------------------------------------ b. the same launches replayed from a graph
GRAPHED_SHAPES = [(4, 2), (17, 1), (43, 3), (1024, 1)]


@pytest.mark.parametrize("T,Bs", GRAPHED_SHAPES, ids=["T%d-B%d" % s for s in GRAPHED_SHAPES])
def test_graph_replay_has_the_bits_of_the_eager_launches(sd, T, Bs):
    """First sight runs eagerly, second sight captures and replays, the third replays: three results with the same bits, each
    within the bound (the graph reads library-owned buffers only; the caller's state is copied in and out around it)."""
    head = _head(sd, PER_STEP_GRAPHED, max_bs=Bs)
    fam = _ordinary(Bs)
    f, st = _inputs(T, Bs, fam)
    outs, routes = [], []
    for _ in range(3):
        outs.append(head.scan(f, state=st))
        routes.append(head.last_scan_path)
    assert routes == [EAGER, GRAPH, GRAPH]
    torch.cuda.synchronize()
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    want = _want("seed1", sd, T, Bs, fam, TMAX.get(Bs))
    for i, o in enumerate(outs):
        _check("graph/T%d/B%d/call%d" % (T, Bs, i), o, want)


def test_a_sequence_longer_than_the_graph_limit_stays_eager(sd):
    head = _head(sd, PER_STEP_GRAPHED)
    fam = _ordinary(1)
    f, st = _inputs(1025, 1, fam)
    outs = []
    for _ in range(3):
        outs.append(head.scan(f, state=st))
        assert head.last_scan_path == EAGER
    torch.cuda.synchronize()
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    _check("graph/T1025/B1", outs[2], _want("seed1", sd, 1025, 1, fam, TMAX[1]))


def test_graphs_are_recaptured_after_the_scan_buffers_grow(sd):
    """A graph holds the addresses it was captured with. (600, 4) grows every sequence buffer of the handle: the (8, 2) graph is
    dropped, the next (8, 2) captures again and gives the bits it gave before."""
    head = _head(sd, PER_STEP_GRAPHED, max_bs=4)
    f2, st2 = _inputs(8, 2, _ordinary(2))
    f4, st4 = _inputs(600, 4, _ordinary(4))
    head.scan(f2, state=st2)
    before = head.scan(f2, state=st2)
    assert head.last_scan_path == GRAPH
    big = head.scan(f4, state=st4)
    assert head.last_scan_path == EAGER
    after = []
    for _ in range(2):
        after.append(head.scan(f2, state=st2))
        assert head.last_scan_path == GRAPH
    torch.cuda.synchronize()
    assert _same_bits(before, after[0]) and _same_bits(before, after[1])
    want = _want("seed1", sd, 8, 2, _ordinary(2), TMAX[2])
    _check("graph/growth/T8/B2/before", before, want)
    _check("graph/growth/T8/B2/after", after[1], want)
    _check("graph/growth/T600/B4", big, _want("seed1", sd, 600, 4, _ordinary(4), TMAX[4]))


def test_graphs_are_recaptured_after_the_cache_of_16_is_cleared(sd):
    """17 lengths, two calls each: the 17th capture clears the cache. T = 4 comes back through a new capture with its first bits."""
    head = _head(sd, PER_STEP_GRAPHED)
    fam = _ordinary(1)
    f, st = _inputs(20, 1, fam)
    first = {}
    for T in range(4, 21):
        first[T] = head.scan(f[:T], state=st)
        assert head.last_scan_path == EAGER, T
        again = head.scan(f[:T], state=st)
        assert head.last_scan_path == GRAPH, T
        assert _same_bits(first[T], again), T
    for _ in range(2):
        back = head.scan(f[:4], state=st)
        assert head.last_scan_path == GRAPH
        assert _same_bits(first[4], back)
    torch.cuda.synchronize()
    for T in range(4, 21):
        _check("graph/eviction/T%d/B1" % T, first[T], _want("seed1", sd, T, 1, fam, TMAX[1]))


def test_a_wider_batch_rebuilds_the_handle_and_a_narrower_one_reuses_it(sd):
    """Bs = 2, then Bs = 5 (the module builds a wider handle), then Bs = 2 on that handle: first sight there (eager), then replayed."""
    with _env(PER_STEP_GRAPHED):
        head = _head(sd, PER_STEP_GRAPHED, max_bs=2)
        f2, st2 = _inputs(5, 2, _ordinary(2))
        f5, st5 = _inputs(5, 5, _ordinary(5))
        outs, routes = [], []
        for f, st in ((f2, st2), (f2, st2), (f5, st5), (f2, st2), (f2, st2)):
            outs.append(head.scan(f, state=st))
            routes.append(head.last_scan_path)
    assert routes == [EAGER, GRAPH, EAGER, EAGER, GRAPH]   # the fourth call is a first sight again: the handle is new
    torch.cuda.synchronize()
    want2, want5 = _want("seed1", sd, 5, 2, _ordinary(2), TMAX[2]), _want("seed1", sd, 5, 5, _ordinary(5), TMAX[5])
    for i, (o, w) in enumerate(zip(outs, (want2, want2, want5, want2, want2))):
        _check("graph/resize/call%d" % i, o, w)
    assert _same_bits(outs[0], outs[3]) and _same_bits(outs[0], outs[4])


# ------------------------------------------------------------------ c. the persistent scan
def _require_persistent(head):
    """After a scan with Bs = 1 and T >= 16 on a default handle."""
    if head.last_scan_path in (EAGER, GRAPH):
        pytest.skip("the persistent scan's 128 workgroups cannot be resident together on this device: the handle keeps the per-step kernel")
    assert head.last_scan_path == PERSISTENT, "route %d: the persistent launch gave up" % head.last_scan_path


@pytest.fixture(scope="module")
def persistent_head(sd):
    return _head(sd, DEFAULT)


@pytest.mark.parametrize("T", [16, 17, 22, 23, 130])
def test_persistent_scan_from_a_nonzero_state(sd, persistent_head, T):
    """T = 16 is the shortest persistent sequence; at 22 / 23 the six-tick prefetch ring wraps its 8 slots while the pipeline drains."""
    fam = _ordinary(1)
    f, st = _inputs(T, 1, fam)
    got = persistent_head.scan(f, state=st)
    _require_persistent(persistent_head)
    _check("persistent/T%d/B1" % T, got, _want("seed1", sd, T, 1, fam, TMAX[1]))


def test_state_carried_across_routes_follows_the_single_fp64_run(sd):
    """47 steps cut into 20 (persistent) + 3 (eager, T < 4) + 8 (eager, first sight) + 8 + 8 (replayed), each piece starting from the
    state the previous one returned, against ONE 47-step oracle run. (No bits are asserted across routes: the persistent kernel's
    gate functions round differently.)"""
    head = _head(sd, DEFAULT)
    fam = _ordinary(1)
    f, st = _inputs(47, 1, fam)
    rots, trs, at = [], [], 0
    for n, route in ((20, PERSISTENT), (3, EAGER), (8, EAGER), (8, GRAPH), (8, GRAPH)):
        r, x, st = head.scan(f[at:at + n], state=st)
        if route == PERSISTENT:
            _require_persistent(head)
        assert head.last_scan_path == route, (at, n)
        rots.append(r)
        trs.append(x)
        at += n
    _check("carried/T47/B1", (torch.cat(rots), torch.cat(trs), st), _want("seed1", sd, 47, 1, fam, TMAX[1]))


def _saturated(case, head, route, tag, sdx, T, Bs, fam):
    f, st = _inputs(T, Bs, fam)
    got = head.scan(f, state=st)
    if route == PERSISTENT:
        _require_persistent(head)
    assert head.last_scan_path == route
    _check(case, got, _want(tag, sdx, T, Bs, fam), M_SAT)


@pytest.fixture(scope="module")
def per_step_head(sd):
    return _head(sd, PER_STEP_GRAPHED, max_bs=5)


def test_saturated_gates_on_the_persistent_kernel(sd, persistent_head):
    """amp 30: gate pre-activations around +-22, |c1| beyond 100, h1 pinned at +-1; amp 1000: pre-activations of several hundred, where
    exp2 overflows to inf and rcp(inf) must give 0 (tests/test_recurrence_oracle.py asserts that the inputs reach this)."""
    _saturated("sat/persistent/amp30/T130/B1", persistent_head, PERSISTENT, "seed1", sd, 130, 1, SAT30)
    _saturated("sat/persistent/amp1000/T24/B1", persistent_head, PERSISTENT, "seed1", sd, 24, 1, SAT1000)


@pytest.mark.parametrize("case,T,Bs", [("amp30", 130, 5), ("amp30", 130, 1), ("amp1000", 24, 1), ("amp1000", 24, 2)],
                         ids=["amp30-B5", "amp30-B1", "amp1000-B1", "amp1000-B2"])
def test_saturated_gates_on_the_per_step_kernel(sd, per_step_head, case, T, Bs):
    """The same inputs through expf / tanhf and an IEEE division (ATDN_SCAN_PERSISTENT=0), batched rows included."""
    _saturated("sat/per_step/%s/T%d/B%d" % (case, T, Bs), per_step_head, EAGER, "seed1", sd, T, Bs, SAT30 if case == "amp30" else SAT1000)


def test_mish_extremes_on_both_kernels(sd_mish):
    """lstm_linear x 100: more than 2 % of its pre-activations above +20 (Mish returns x) and below -20 (e^x underflows towards 0),
    the rest across the fminf(x, 20) clamp. Bs = 1 takes the persistent kernel, Bs = 2 the per-step kernel."""
    head = _head(sd_mish, DEFAULT, max_bs=2)
    _saturated("mish/per_step/T24/B2", head, EAGER, "mish100", sd_mish, 24, 2, MISH)
    _saturated("mish/persistent/T24/B1", head, PERSISTENT, "mish100", sd_mish, 24, 1, MISH)
