"""Seeded delta rows for detect_kernel (csrc/detect.hip) and their references from the oracle.

No GPU here.  Everything is in block units: block_sec = 1.0 keeps t = index, as detector_kats.py does.
A case is (name, delta row, k, (W, Fb, Fa, F0) in blocks or None for the global detector), plus the
runs [start, stop) a generator plants where it promises them (tests/test_detector_cases.py holds the
generators to those promises with the oracle alone; tests/test_gpu_detect_contract.py holds the
kernel to the references).

reference(name) is oracle/dsp_oracle.py's get_detections_ref / get_detections_adaptive_ref on the
row: thresholds, detections, the margin min |delta - threshold used| (NaN terms ignored, +inf if
none is left) and the status word of include/msdsp.h.  Rows and references are cached and
read-only.
"""
import datetime
import functools
import warnings
from collections import Counter
from typing import NamedTuple

import numpy as np

from oracle import dsp_oracle as O

DET = np.dtype([("start", np.int64), ("stop", np.int64), ("db", np.float64)])  # msd_det
INF = float("inf")


class Case(NamedTuple):
    name: str
    delta: np.ndarray
    k: float
    cfg: tuple | None            # (W, Fb, Fa, F0) in blocks; None: the global detector
    expect: tuple | None = None  # planted runs ((start, stop), ...) where the generator promises them


class Ref(NamedTuple):
    thr: np.ndarray   # adaptive: the thresholds list [nb]; global: the single threshold [1]
    dets: np.ndarray  # DET; empty where status is 1 or 2 (the reference raises there)
    margin: float
    status: int       # 0; 1: zero-duration global detection (main.py:437); 2: empty global input (:412)
    ties: int         # blocks with delta == threshold used, bit for bit
    utc: tuple        # utc_start of every detection when a start time was given


CLASSES = ("config_sweep", "window_sizes", "ties", "lane_and_chunk_edges", "long_runs", "nonfinite")

# ------------------------------------------------------------------ building blocks
SWEEP_W = (0, 1, 7, 8, 9, 127, 128, 129, 600)
SWEEP_FA = (0, 1, 5, 100)
SWEEP_FB = (0, 15, "Fa+50")
SWEEP_F0 = (0, 1, 50, "nb", "nb+7")
SWEEP_K = (0.0, 0.5, 4.0)
SWEEP_GLOBAL_K = (0.0, 1.0, 3.5)
SWEEP_N = 150

EDGE_NB = 3000
EDGE_CFG = (50, 0, 3, 10)  # W = 50: an event 64 blocks after another meets a clean window
EDGE_K = 4.0
EDGE_SINGLES = (0, 62, 63, 64, 65, 127, 128, 1022, 1023, 1024, 1025, 2047, 2048, EDGE_NB - 2, EDGE_NB - 1)
EDGE_FA = (22, 23, 24, 25)  # event at 1000: the freeze ends on 1022 .. 1025, the next burst right behind it

LONG_RUNS = (129, 1000, 8193, 20000)

MIXED_NB = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 3000)
MIXED_CFG = (100, 3, 20, 10)
MIXED_K = 3.0
MIXED_GLOBAL_K = 1.0


def random_delta(seed, nb, bursts=None):
    """noise plus bursts, as test_gpu_parity._random_delta"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(nb) * 1.5 + rng.uniform(-3, 3)
    for _ in range(max(1, nb // 100) if bursts is None else bursts):
        i = rng.integers(0, max(1, nb))
        d[i:i + rng.integers(1, 30)] += rng.uniform(3, 25)
    return d


def _quiet(rng, nb, amp=0.1):
    """bounded noise: nothing in it is 4 sigma above its own mean, so only planted blocks fire"""
    return rng.uniform(-amp, amp, nb)


def _plant(rng, d, runs, height=30.0):
    for s, e in runs:
        d[s:e] += height + rng.uniform(-1.0, 1.0, e - s)
    return d


def _case(name, d, k, cfg, expect=None):
    d = np.ascontiguousarray(d, dtype=np.float64)
    d.setflags(write=False)
    return Case(name, d, float(k), None if cfg is None else tuple(int(v) for v in cfg),
                None if expect is None else tuple((int(s), int(e)) for s, e in expect))


def sweep_params():
    """SWEEP_N seeded (nb, W, Fb, Fa, F0, k): every column cycles through its values before it is
    shuffled, so each listed value of each parameter occurs; F0 and Fb are resolved per row"""
    rng = np.random.default_rng(2025_0625)

    def column(values):
        c = [values[i % len(values)] for i in range(SWEEP_N)]
        rng.shuffle(c)
        return c

    cols = [column(v) for v in (SWEEP_W, SWEEP_FB, SWEEP_FA, SWEEP_F0, SWEEP_K)]
    out = []
    for W, Fb, Fa, F0, k in zip(*cols):
        nb = 300 + int(1200 * rng.uniform() ** 2)  # 300 .. 1500, most of them short
        Fb = Fa + 50 if Fb == "Fa+50" else Fb
        F0 = {"nb": nb, "nb+7": nb + 7}.get(F0, F0)
        out.append((nb, W, Fb, Fa, F0, k))
    return tuple(out)


# ------------------------------------------------------------------ the classes
def _config_sweep():
    out = []
    for i, (nb, W, Fb, Fa, F0, k) in enumerate(sweep_params()):
        out.append(_case(f"config_sweep/{i:03d}", random_delta(7000 + i, nb), k, (W, Fb, Fa, F0)))
    for j, k in enumerate(SWEEP_GLOBAL_K):
        for m, nb in enumerate((300, 777, 1500)):
            d = random_delta(7500 + 10 * j + m, nb, bursts=max(1, nb // 50))
            d[-1] = -10.0  # the last block below: the reference asserts otherwise
            out.append(_case(f"config_sweep/global-k{k}-{nb}", d, k, None))
    return out


def _window_sizes():
    nb = 2100
    rng = np.random.default_rng(8100)
    d = rng.standard_normal(nb) * 1.5
    if d[1] > d[0]:  # the window of one block has std 0: its threshold is delta[0] itself
        d[0], d[1] = d[1], d[0]
    return [_case("window_sizes/nothing_fires", d, 1e9, (nb - 1, 0, 0, 0)),
            _case("window_sizes/bursts", random_delta(8101, nb), 0.5, (nb - 1, 0, 5, 0))]


def _ties():
    d = np.random.default_rng(8200).integers(0, 4, 3000).astype(np.float64)
    return [_case(f"ties/k{k}", d, k, (8, 0, 2, 0)) for k in (0, 1)]


def _edges():
    nb = EDGE_NB
    out = []

    def row(name, runs, cfg=EDGE_CFG, seed=0):
        rng = np.random.default_rng(8300 + seed)
        out.append(_case(f"lane_and_chunk_edges/{name}", _plant(rng, _quiet(rng, nb), runs), EDGE_K, cfg, runs))

    def single(*idx):
        return tuple((i, i + 1) for i in idx)

    # neighbours go to different rows: side by side they would be one run
    row("singles_a", single(0, 62, 64, 127, 1022, 1024, 2047, nb - 2), seed=1)
    row("singles_b", single(63, 65, 128, 1023, 1025, 2048, nb - 1), seed=2)
    row("pairs_64_65_run_across", single(200, 264, 400, 465) + ((1020, 1031),), seed=3)
    row("run_to_1023", ((1000, 1024),), seed=4)
    row("run_from_1024", ((1024, 1041),), seed=5)
    row("gap_at_1023", ((1020, 1023), (1024, 1031)), seed=6)
    row("gap_at_1024", ((1020, 1024), (1025, 1031)), seed=7)
    for fa in EDGE_FA:
        row(f"freeze_ends_{1000 + fa}", ((1000, 1001), (1000 + fa + 1, 1000 + fa + 3)), cfg=(50, 0, fa, 10),
            seed=10 + fa)
    row("global_singles_a", single(0, 62, 64, 127, 1022, 1024, 2047, nb - 2), cfg=None, seed=40)
    row("global_run_to_1023", ((1010, 1024),), cfg=None, seed=41)
    row("global_run_from_1024", ((1024, 1036),), cfg=None, seed=42)
    row("global_run_across", ((1020, 1031),), cfg=None, seed=43)
    return out


def _long_runs():
    out = []
    for L in LONG_RUNS:
        # adaptive: quiet bounded noise, the plateau starts at block 150 and Fa = 1 holds the threshold
        # it started under, so every plateau block fires again and the plateau is one run.  The row of
        # the 129-block plateau fits one LDS chunk (nb <= 1024), the others do not.
        rng = np.random.default_rng(8400 + L)
        nb = 400 if L == 129 else L + 600
        d = _quiet(rng, nb)
        d[150:150 + L] += 30.0 + 0.5 * rng.standard_normal(L)
        out.append(_case(f"long_runs/adaptive-{L}", d, 4.0, (100, 0, 1, 10), ((150, 150 + L),)))
        # global: the plateau is two thirds of the row, so mean + 0.25 std is about 23 dB, far from the
        # quiet blocks and from the plateau (a short plateau at k = 1 leaves the threshold inside it)
        nb = L + L // 2
        s = L // 4
        d = 0.5 * rng.standard_normal(nb)
        d[s:s + L] += 30.0
        out.append(_case(f"long_runs/global-{L}", d, 0.25, None, ((s, s + L),)))
    return out


def _nonfinite():
    out = []
    for name, v in (("posinf", np.inf), ("neginf", -np.inf), ("nan", np.nan)):
        for mode, k, cfg in (("adaptive", 4.0, (100, 3, 20, 10)), ("adaptive_f0_0", 4.0, (100, 3, 20, 0)),
                             ("global", 1.0, None)):
            d = random_delta(8500 + len(out), 500)
            d[-1] = -10.0
            d[250] = v
            out.append(_case(f"nonfinite/{name}-{mode}", d, k, cfg))
    return out


def _mixed():
    """files that fit the LDS chunk and files that do not, for one launch; the global rows keep their
    last block low, and two more global rows carry status 2 (empty) and status 1 (only the last block
    above the threshold)"""
    out = []
    for i, nb in enumerate(MIXED_NB):
        d = random_delta(8600 + i, nb) if nb else np.zeros(0)
        out.append(_case(f"mixed/adaptive-{nb}", d, MIXED_K, MIXED_CFG))
    for i, nb in enumerate(MIXED_NB):
        if nb == 0:
            continue
        d = random_delta(8600 + i, nb, bursts=max(1, nb // 50))
        d[-1] = -10.0
        out.append(_case(f"mixed/global-{nb}", d, MIXED_GLOBAL_K, None))
    out.append(_case("mixed/global-empty", np.zeros(0), MIXED_GLOBAL_K, None))
    last = np.zeros(50)
    last[-1] = 100.0
    out.append(_case("mixed/global-last_block_only", last, MIXED_GLOBAL_K, None))
    return out


# histogram rows: 60 s files at block_sec = 0.2, the reference configuration (120, 3, 20, 10) s
HIST_BLOCK_SEC = 0.2
HIST_NB = 300
HIST_SEC = (120, 3, 20, 10)
HIST_CFG = tuple(int(s / HIST_BLOCK_SEC) for s in HIST_SEC)  # the oracle's own int(sec / bs)
HIST_K = 4.0
HIST_NBUCKETS = 6
HIST_BASE = datetime.datetime(2025, 6, 25, 3, 0, 0)
HIST_FILES = ("on_boundary", "before_boundary", "before_base", "far_before_base", "past_end", "across_bucket",
              "across_end", "across_base")


def _histogram():
    out = []
    planted = {"on_boundary": (35, 120, 250), "before_boundary": (34, 121, 251)}
    for i, name in enumerate(HIST_FILES):
        rng = np.random.default_rng(8700 + i)
        starts = planted.get(name, (20 + 7 * i, 90 + i, 148, 150, 210 + 3 * i, 297))
        runs = tuple((s, s + 1) for s in starts)
        out.append(_case(f"histogram/{name}", _plant(rng, _quiet(rng, HIST_NB), runs), HIST_K, HIST_CFG, runs))
    for i, name in enumerate(HIST_FILES):
        d = np.array(out[i].delta)
        d[-1] = -10.0
        out.append(_case(f"histogram/global-{name}", d, 2.0, None))
    return out


def hist_starts(bucket_us):
    """file start times for the histogram rows, for buckets of bucket_us from HIST_BASE:
    a detection at block 35 (7.0 s) starts exactly on the first bucket boundary and belongs to the later
    bucket, the one at block 34 of the next file starts 0.2 s before it; one file ends before the
    base (negative buckets, on a start that is no multiple of the bucket or of a second), one lies
    several buckets before it, one starts past the last bucket; the others straddle a boundary, the
    end of the histogram and the base"""
    B = datetime.timedelta(microseconds=bucket_us)
    s = lambda x: datetime.timedelta(seconds=x)  # noqa: E731
    return {
        "on_boundary": HIST_BASE + B - s(7),
        "before_boundary": HIST_BASE + B - s(7),
        "before_base": HIST_BASE - s(90.5),
        "far_before_base": HIST_BASE - 3 * B - s(123.456789),
        "past_end": HIST_BASE + HIST_NBUCKETS * B + s(5),
        "across_bucket": HIST_BASE + 3 * B - s(30),
        "across_end": HIST_BASE + HIST_NBUCKETS * B - s(30),
        "across_base": HIST_BASE - s(30),
    }


def bucket_counts_ref(utc_starts, base, bucket_us, nbuckets):
    """count_per_hour_ref (main.py:687-696) for buckets of bucket_us counted from base: datetime
    arithmetic on the oracle's utc_start, buckets outside [0, nbuckets) dropped"""
    width = datetime.timedelta(microseconds=bucket_us)
    c = Counter((u - base) // width for u in utc_starts)
    return np.array([c.get(b, 0) for b in range(nbuckets)], np.int64)


_GENERATORS = {"config_sweep": _config_sweep, "window_sizes": _window_sizes, "ties": _ties,
               "lane_and_chunk_edges": _edges, "long_runs": _long_runs, "nonfinite": _nonfinite,
               "mixed": _mixed, "histogram": _histogram}


@functools.lru_cache(maxsize=None)
def cases(cls):
    """the rows of one class, in a fixed order; read-only"""
    return tuple(_GENERATORS[cls]())


@functools.lru_cache(maxsize=None)
def _by_name(cls):
    return {c.name: c for c in cases(cls)}


def case(name):
    return _by_name(name.split("/")[0])[name]


def seconds_for(blocks, block_sec):
    """a duration the oracle's int(sec / block_sec) turns into `blocks`"""
    s = blocks * block_sec
    while int(s / block_sec) < blocks:
        s = float(np.nextafter(s, np.inf))
    assert int(s / block_sec) == blocks
    return s


@functools.lru_cache(maxsize=None)
def reference(name, block_sec=1.0, start=None):
    """the oracle on case `name` (block_sec and a file start time only move the time stamps)"""
    c = case(name)
    d = c.delta
    status, rdets = 0, []
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # mean of an empty window, inf - inf: the reference's own NaNs
        if c.cfg is None:
            try:
                rdets, thr = O.get_detections_ref(d, c.k, block_sec, start)
            except IndexError:        # above_thresh[0] on an empty array (main.py:412)
                status = 2
            except AssertionError:    # t_dur == 0 (main.py:437)
                status = 1
            if status:
                thr = np.mean(d) + c.k * np.std(d)  # main.py:399-400, evaluated before either error
            thr = np.array([thr], np.float64)
        else:
            secs = [seconds_for(v, block_sec) for v in c.cfg]
            rdets, thr = O.get_detections_adaptive_ref(d, c.k, block_sec, *secs, wav_start_date_time=start)
            thr = np.array(thr, np.float64).reshape(len(d))
        terms = np.abs(d - thr)
        ties = int(np.count_nonzero(d == thr))
    terms = terms[~np.isnan(terms)]
    dets = np.zeros(len(rdets), DET)
    for i, r in enumerate(rdets):
        dets[i] = (int(round(r[0] / block_sec)), int(round(r[1] / block_sec)), r[3])
    for a in (thr, dets):
        a.setflags(write=False)
    return Ref(thr, dets, float(terms.min()) if terms.size else INF, status, ties, tuple(r[4] for r in rdets))


def same_floats(a, b):
    """bit-exact equality of float64 arrays, except that any NaN equals any NaN at the same position"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and
                np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))
