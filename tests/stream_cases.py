"""Seeded delta rows for the C5 stream detector (csrc/stream.hip, meteorgpu/stream.py) and their
references from the oracle.

No GPU here.  The rows of tests/detector_cases.py describe the same two detectors and every class of
them applies to the stream (DETECTOR_CLASSES; the histogram rows do not).  This module adds the
stream's own classes in the same Case shape (frames are the detector's blocks, block_sec = 1.0):

window_tree             W chosen by what numpy's pairwise tree over a W-frame window makes of it in
                        fresh_kernel's leaf program (np_program.h; build_program below restates it)
huge_window             more than 4096 leaf records; 64 chunks and 65 chunks + 3 in fresh_list_kernel
tile_and_segment_edges  events and freeze ends on the 512-frame tile edge of fresh_kernel
shard_cuts              one adaptive and one global row with cut sets for world sizes 2 .. 5
long_runs_sharded       the long_runs rows of detector_cases, cut inside the run
freeze_before           one row under four (Fb, Fa): main.py:491-493 is max(i + Fa, max(0, i - Fb))
nonfinite_stream        NaN, +inf, -inf far ahead of the events of a 5000-frame stream

Unless a class says otherwise a row is bounded quiet noise plus planted bursts, k = 4 and Fa = 30, so
that most frames read a fresh threshold.  reference(name) gives thresholds, detections, margin and
status of any row of any class, as detector_cases.reference does; cuts(name) gives a row's shard cut
sets.  tests/test_stream_cases.py holds the generators to their promises with the oracle alone;
tests/test_gpu_stream_contract.py holds the kernels to the references.
"""
import functools
import warnings

import numpy as np

from oracle import dsp_oracle as O
from tests import detector_cases as D
from tests.detector_cases import Case, Ref, _case, _plant, _quiet

DETECTOR_CLASSES = ("config_sweep", "window_sizes", "ties", "lane_and_chunk_edges", "long_runs", "nonfinite",
                    "mixed")
STREAM_CLASSES = ("window_tree", "huge_window", "tile_and_segment_edges", "shard_cuts", "long_runs_sharded",
                  "freeze_before", "nonfinite_stream")
CLASSES = DETECTOR_CLASSES + STREAM_CLASSES

K, FA = 4.0, 30
same_floats = D.same_floats

# 2: the shortest window with a spread; 15 .. 17: one leaf, scalar tail of 7, none, 1; 136: the first
# split (128 + 8); 255 .. 257: two leaves, the last with a scalar tail / without / three leaves;
# 7689: the first length with 8 pending partial sums; 8191: the last, the whole stack; 8192: one
# whole chunk (7 pending); 8193, 8195, 8199: a scalar leaf of 1, 3, 7 after a chunk end; 8200: a
# second chunk that is one leaf of 8; 16383: two chunks, the second with the full stack; 65536: 512
# records, the last count kept in LDS; 65537: 513 records, read from HBM; 73727 = 8 * 8192 + 8191:
# HBM records and the full stack
TREE_W = (2, 15, 16, 17, 136, 255, 256, 257, 7689, 8191, 8192, 8193, 8195, 8199, 8200, 16383, 65536, 65537, 73727)
TREE_TAIL = 1100  # frames past W: the tile that straddles i = W, two tiles of full windows, a ragged tail
TREE_LEAD = 700   # frames below W that are past F0: fresh_short_kernel's share

HUGE_W = (524288, 532483)  # 64 chunks: the last count on four waves; 65 chunks + 3: wave 0 alone
HUGE_TAIL, HUGE_LEAD = 300, 100

TILE_NB = 3000
TILE_CFG = (50, 0, 3, 10)
TILE_FA = (11, 12, 13)  # event at 500: the freeze ends on 511 .. 513, the next burst right behind it

CUT_NB = 6000
CUT_CFG = (600, 0, 100, 50)
CUT_RUNS = ((1000, 1020), (2500, 2501), (4000, 4040))
_FZ = CUT_RUNS[0][1] - 1 + CUT_CFG[2]  # the freeze of the first run ends here (adaptive row)
CUT_SETS = (
    # world 2: at a run's start, one frame inside, at its stop and past it; at fz and fz + 1; at F0; at W;
    # the first and the last shard empty
    (1000,), (1001,), (1020,), (1021,), (_FZ,), (_FZ + 1,), (CUT_CFG[3],), (CUT_CFG[0],), (0,), (CUT_NB,),
    # world 3: an empty shard, a one-frame shard that is a whole run, empty ends
    (2500, 2500), (2500, 2501), (0, 1010), (4020, CUT_NB),
    # world 4
    (1000, 1020, _FZ), (CUT_CFG[3], CUT_CFG[0], 4001),
    # world 5
    (0, 1001, 1001, CUT_NB), (1020, 1021, _FZ, _FZ + 1), (2500, 2501, 4000, 4039),
)

FB_NB = 1500
FB_PAIRS = ((15, 5), (55, 5), (-40, 5), (-3, 5))  # (Fb, Fa)
FB_W, FB_F0 = 100, 10

NONFINITE_NB, NONFINITE_W = 5000, 100


# ------------------------------------------------------------------ np_program.h in Python
def np_tree_records(base, m, rec):
    if m <= 128:
        rec.append([base, m, 0, 0])
        return
    m2 = m // 2
    m2 -= m2 % 8
    np_tree_records(base, m2, rec)
    np_tree_records(base + m2, m - m2, rec)
    rec[-1][2] += 1  # the add combining the two halves follows the right half's last leaf


def build_program(n):
    """np_program.h build_program: the leaf records [offset, length, adds, chunk_end] of numpy's
    np.sum over n elements, and the largest number of pending partial sums while they run"""
    rec, depth, sp = [], 0, 0
    for c in range(0, n, 8192):
        first = len(rec)
        np_tree_records(c, min(8192, n - c), rec)
        rec[-1][3] = 1
        for _, _, adds, end in rec[first:]:
            sp += 1
            depth = max(depth, sp)
            sp -= adds + end
    assert sp == 0
    return rec, depth


def leaf_sum(a):
    """numpy's pairwise_sum on a leaf of at most 128 elements: eight accumulators, their tree, a tail"""
    n = len(a)
    if n < 8:
        res = np.float64(-0.0)
        for v in a:
            res = res + v
        return res
    lim = n - n % 8
    r = np.array(a[:8], np.float64)
    for i in range(8, lim, 8):
        r = r + a[i:i + 8]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[lim:]:
        res = res + v
    return res


def run_program(rec, x):
    """the records over x as fresh_pass runs them: a stack of partial sums, s += chunk sum"""
    stk, acc = [], np.float64(0.0)
    for off, m, adds, end in rec:
        stk.append(leaf_sum(x[off:off + m]))
        for _ in range(adds):
            top = stk.pop()
            stk[-1] = stk[-1] + top
        if end:
            acc = acc + stk.pop()
    assert not stk
    return acc


# ------------------------------------------------------------------ the classes
def _ramp(rng, nb):
    """falling noise: every frame lies below the two before it, so a window of two never fires"""
    return -0.3 * np.arange(nb) + rng.uniform(-0.1, 0.1, nb)


def _lead_in(d, nb=20):
    """the first frames fall onto the noise: with F0 = 0 the windows of one, two, ... frames would
    otherwise fire at random (the spread of two bounded values bounds nothing)"""
    d[:nb] += 0.3 * (nb - np.arange(nb))
    return d


def _window_tree():
    out = []
    for W in TREE_W:
        rng = np.random.default_rng(9100 + W)
        nb = W + TREE_TAIL
        F0 = max(0, W - TREE_LEAD)
        base = max(F0, 20)
        # 3-frame bursts keep the threshold of any window that holds them below the next burst;
        # the last run is Fa + 1 frames, held by its own freeze, and ends with the stream
        runs = tuple(sorted({(base + 150, base + 153), (W - 1, W + 2), (W + 400, W + 403), (W + 700, W + 703),
                             (nb - FA - 1, nb)}))
        noise = _ramp(rng, nb) if W < 9 else _quiet(rng, nb)
        d = _plant(rng, _lead_in(noise) if W >= 9 and F0 == 0 else noise, runs)
        out.append(_case(f"window_tree/W{W}", d, K, (W, 0, FA, F0), runs))
    return out


def _huge_window():
    out = []
    for W in HUGE_W:
        rng = np.random.default_rng(9200 + W % 1000)
        nb = W + HUGE_TAIL
        runs = ((W - 50, W - 47), (W + 100, W + 103), (nb - 20, nb))
        out.append(_case(f"huge_window/W{W}", _plant(rng, _quiet(rng, nb), runs), K, (W, 0, FA, W - HUGE_LEAD), runs))
    return out


def _tile_edges():
    out = []

    def row(name, runs, cfg=TILE_CFG, seed=0):
        rng = np.random.default_rng(9300 + seed)
        out.append(_case(f"tile_and_segment_edges/{name}", _plant(rng, _quiet(rng, TILE_NB), runs), K, cfg, runs))

    # neighbours go to different rows: side by side they would be one run
    row("singles_511_513", ((511, 512), (513, 514), (1535, 1536), (1537, 1538)), seed=1)
    row("single_512", ((512, 513), (1536, 1537), (2560, 2561)), seed=2)
    row("run_510_514", ((510, 515),), seed=3)
    row("run_to_511", ((500, 512),), seed=4)
    row("run_from_512", ((512, 524),), seed=5)
    for fa in TILE_FA:
        row(f"freeze_ends_{500 + fa}", ((500, 501), (500 + fa + 1, 500 + fa + 3)), cfg=(50, 0, fa, 10), seed=10 + fa)
    row("global_single_512", ((512, 513), (1536, 1537)), cfg=None, seed=40)
    row("global_run_510_514", ((510, 515),), cfg=None, seed=41)
    return out


def _shard_cuts():
    rng = np.random.default_rng(9400)
    a = _case("shard_cuts/adaptive", _plant(rng, _quiet(rng, CUT_NB), CUT_RUNS), K, CUT_CFG, CUT_RUNS)
    rng = np.random.default_rng(9401)
    g = _case("shard_cuts/global", _plant(rng, _quiet(rng, CUT_NB), CUT_RUNS), K, None, CUT_RUNS)
    return [a, g]


def _long_runs_sharded():
    out = []
    for c in D.cases("long_runs"):
        out.append(Case(c.name.replace("long_runs/", "long_runs_sharded/"), c.delta, c.k, c.cfg, c.expect))
    return out


def _freeze_before():
    # bursts at 500 and 520 fire under every pair; the low plateau at 530 .. 532 stays below a fresh
    # threshold (its window holds both bursts) and above a held one: it fires only while a freeze of
    # 40 frames still holds the threshold that frame 500 fired under
    out = []
    for Fb, Fa in FB_PAIRS:
        rng = np.random.default_rng(9500)
        runs = ((500, 503), (520, 523), (1000, 1003))
        d = _plant(rng, _quiet(rng, FB_NB), runs)
        d[530:533] += 5.0
        frozen = max(Fa, -Fb)
        expect = runs + (((530, 533),) if 520 + 2 + frozen >= 532 else ())
        out.append(_case(f"freeze_before/Fb{Fb}_Fa{Fa}", d, K, (FB_W, Fb, Fa, FB_F0), sorted(expect)))
    return out


def _nonfinite_stream():
    out = []
    runs = ((1000, 1003), (2047, 2050), (4000, 4000 + FA + 1))
    for name, at, v in (("nan", 100, np.nan), ("posinf", 100, np.inf), ("neginf", 100, -np.inf),
                        ("nan_first", 0, np.nan)):
        for F0 in (0, 10):
            rng = np.random.default_rng(9600 + len(out))
            d = _plant(rng, _quiet(rng, NONFINITE_NB), runs)
            if F0 == 0 and at:
                _lead_in(d)
            d[at] = v
            out.append(_case(f"nonfinite_stream/{name}-f0_{F0}", d, K, (NONFINITE_W, 0, FA, F0), runs))
    return out


_GENERATORS = {"window_tree": _window_tree, "huge_window": _huge_window, "tile_and_segment_edges": _tile_edges,
               "shard_cuts": _shard_cuts, "long_runs_sharded": _long_runs_sharded, "freeze_before": _freeze_before,
               "nonfinite_stream": _nonfinite_stream}


@functools.lru_cache(maxsize=None)
def cases(cls):
    """the rows of one class, in a fixed order; read-only"""
    return D.cases(cls) if cls in DETECTOR_CLASSES else tuple(_GENERATORS[cls]())


@functools.lru_cache(maxsize=None)
def _by_name(cls):
    return {c.name: c for c in cases(cls)}


def case(name):
    return _by_name(name.split("/")[0])[name]


def cuts(name):
    """the shard cut sets of a row: tuples of world - 1 cut frames"""
    cls, rest = name.split("/")
    if cls == "shard_cuts":
        return CUT_SETS
    if cls == "long_runs_sharded":  # 10 frames after the run's start, and in its middle
        (s, e), = case(name).expect
        return ((s + 10, (s + e) // 2),)
    raise KeyError(name)


def margin_of(delta, thr):
    """min |delta - threshold used|, NaN terms ignored, +inf if none is left"""
    with np.errstate(all="ignore"):
        terms = np.abs(delta - thr)
    terms = terms[~np.isnan(terms)]
    return float(terms.min()) if terms.size else D.INF


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle on row `name` of any class, as detector_cases.reference"""
    cls = name.split("/")[0]
    if cls in DETECTOR_CLASSES:
        return D.reference(name)
    if cls == "long_runs_sharded":
        return D.reference(name.replace("long_runs_sharded/", "long_runs/"))
    c = case(name)
    d = c.delta
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # mean of an empty window, inf - inf: the reference's own NaNs
        if c.cfg is None:
            rdets, thr = O.get_detections_ref(d, c.k, 1.0)
            thr = np.array([thr], np.float64)
        else:
            rdets, thr = O.get_detections_adaptive_ref(d, c.k, 1.0, *c.cfg)
            thr = np.array(thr, np.float64).reshape(len(d))
        ties = int(np.count_nonzero(d == thr))
    dets = np.zeros(len(rdets), D.DET)
    for i, r in enumerate(rdets):
        dets[i] = (int(round(r[0])), int(round(r[1])), r[3])
    for a in (thr, dets):
        a.setflags(write=False)
    return Ref(thr, dets, margin_of(d, thr), 0, ties, ())


def fresh_full(c):
    """frames of an adaptive row whose threshold is a fresh full-window one: at or past W and F0, not
    frozen (the freeze state replayed from the reference's detections' frames)"""
    W, Fb, Fa, F0 = c.cfg
    r = reference(c.name)
    d, thr = c.delta, r.thr
    with np.errstate(invalid="ignore"):
        fired = np.flatnonzero(d > thr)
    frozen = np.zeros(len(d), bool)
    for i in fired:
        frozen[i + 1: max(i + Fa, max(0, i - Fb)) + 1] = True
    ok = ~frozen
    ok[:max(W, F0)] = False
    return np.flatnonzero(ok)
