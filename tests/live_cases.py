"""Seeded band-dB rows for the phase-2 live detector (csrc/live.hip) and their references from the oracle.

No GPU here.  A case is (name, band dB rows [3][nb] = signal, noise 1, noise 2, a ConfigDetectionRef,
fs, block_size, the one-shot capacity or None for ample room), plus what its generator promises
(tests/test_live_cases.py holds the generators to those promises with the oracle alone;
tests/test_gpu_live_contract.py holds both device implementations to the references).

reference(name) is oracle/live_oracle.live_detect_ref on the rows: meteors, thresholds used, over-noise
values, and from them the state after every block (replay), the block indices of every meteor, the
events (Init end, trigger, close, lock expiry) and the state a live session carries after the last
block.  Rows and references are cached and read-only.

Where a class needs the over-noise value to take an exact value it keeps both noise rows at 0.0
(over = sig - np.mean([0.0, 0.0]) = sig) and builds the signal row block by block with _Builder, which
steps the oracle's own numpy arithmetic over the history so far.
"""
import functools
import warnings
from contextlib import contextmanager
from typing import NamedTuple

import numpy as np

from oracle import live_oracle as L
from tests.detector_cases import same_floats, seconds_for  # noqa: F401  (same_floats: re-exported)

METEOR = np.dtype([("start_block", np.int64), ("stop_block", np.int64), ("time_start", np.float64),
                   ("time_stop", np.float64), ("duration", np.float64), ("db_min", np.float64),
                   ("db_max", np.float64), ("db_mean", np.float64), ("db_std", np.float64)])  # msd_meteor
STATS = ("time_start", "time_stop", "duration", "db_min", "db_max", "db_mean", "db_std")
INF = float("inf")
RATES = ((4000, 800), (8000, 800), (4000, 200), (44100, 4410))
CFG_FIELDS = tuple(L.ConfigDetectionRef.__dataclass_fields__)

CLASSES = ("config_sweep", "value_ties", "time_ties", "lane_and_segment_edges", "long_histories", "nonfinite",
           "capacity")


class Case(NamedTuple):
    name: str
    rows: np.ndarray             # [3][nb], read-only
    cfg: L.ConfigDetectionRef
    fs: int
    bs: int
    cap: int | None = None       # meteor capacity of the one-shot forms; None: ample
    expect: dict | None = None   # what the generator planted


class Ref(NamedTuple):
    meteors: np.ndarray  # METEOR, block indices from the replayed states
    thr: np.ndarray      # thresholds used [nb]
    over: np.ndarray     # over-noise values [nb]
    states: tuple        # replay(): the state after every block
    events: tuple        # ((block, kind), ...), kind in init_end / trigger / close / expiry
    final: tuple         # (state, trig, lock, until, t_start): msd_live_stream_state after the last block
    ties: int            # decisions met with equality: over == thr, until == block end, t0 == init wait, dur == min
    longest: int         # the longest history read: a threshold window or a tracking run
    nonfinite: int       # blocks whose over-noise value is not finite


@contextmanager
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # mean of an empty window, inf - inf: the reference's own NaNs
        yield


def config(fs, bs, W=40, k=4.0, init=8.0, wait=0.0, min_db=-1.0, min_dur=-1.0):
    """(Init lasts 8 s unless asked otherwise: quiet rows then meet a filled window.)  A ConfigDetectionRef whose int(proc_block_sec * fs) is bs and whose int(avg_win_sec / proc_block_sec) is W"""
    pbs = bs / fs
    assert int(pbs * fs) == bs
    return L.ConfigDetectionRef(proc_block_sec=pbs, avg_win_sec=seconds_for(W, pbs), init_detection_wait_sec=init,
                                after_tracking_wait_sec=wait, threshold_std_factor=k,
                                detection_db_over_noise_mean_min=min_db, detection_dur_min_sec=min_dur)


def win_blocks(cfg):
    return int(cfg.avg_win_sec / cfg.proc_block_sec)  # processor.py:58


def cfg_key(c):
    """cases with the same key share a launch / a session"""
    return (c.fs, c.bs) + tuple(getattr(c.cfg, f) for f in CFG_FIELDS)


def t_start_of(b, fs, bs):
    return (b * bs) / fs          # processor.py:181


def t_end_of(b, fs, bs):
    return (b * bs + bs) / fs     # processor.py:182


def ulps(x, n):
    x = np.float64(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, INF if n > 0 else -INF)
    return x


def replay(thr, over, cfg, fs=4000, bs=800):
    """The oracle's state after each block, replayed from its thresholds used and over-noise values
    (processor.py:448-504): ('init',) / ('detection', lock, until) / ('tracking', lock, t_start, trig).
    The lock is thr + 0 * std of the fresh window (processor.py:466): NaN where that std is not finite."""
    W = int(cfg.avg_win_sec / cfg.proc_block_sec)
    state, out = ("init",), []
    for b in range(len(over)):
        t0 = (b * bs) / fs
        if state[0] == "init":
            if t0 >= cfg.init_detection_wait_sec:
                state = ("detection", -1.0, -1.0)
        elif state[0] == "detection":
            if over[b] > thr[b]:
                with _quiet():
                    h_std = np.std(over[b - W if W and b > W else 0:b])
                state = ("tracking", thr[b] + 0 * h_std, t0, b)
        elif over[b] < thr[b]:
            state = ("detection", state[1], t0 + cfg.after_tracking_wait_sec)
        out.append(state)
    return out


# ------------------------------------------------------------------ building blocks
class _Builder:
    """live_detect_ref's loop (processor.py:391-504) one block at a time over noise rows of 0.0, so that a
    generator can read the threshold the next block will meet before it chooses that block's value"""

    def __init__(self, cfg, fs=4000, bs=800):
        self.cfg, self.fs, self.bs, self.W = cfg, fs, bs, win_blocks(cfg)
        self.over, self.thr, self.state = [], [], ("init",)

    @property
    def b(self):
        return len(self.over)

    def fresh(self):
        hist = self.over[-self.W:]
        with _quiet():
            h_mean, h_std = np.mean(hist), np.std(hist)
        return h_mean + self.cfg.threshold_std_factor * h_std, h_std

    def used(self):
        """the threshold the next block is compared with"""
        thr = self.fresh()[0]
        if self.state[0] == "tracking":
            thr = self.state[1]
        elif self.state[0] == "detection" and self.state[2] > t_end_of(self.b, self.fs, self.bs):
            thr = self.state[1]
        return thr

    def push(self, v):
        cfg = self.cfg
        t0 = t_start_of(self.b, self.fs, self.bs)
        db2 = np.float64(v) - np.mean([0.0, 0.0])
        thr, h_std = self.used(), self.fresh()[1]
        self.over.append(db2)
        self.thr.append(thr)
        st = self.state
        if st[0] == "init":
            if t0 >= cfg.init_detection_wait_sec:
                self.state = ("detection", -1.0, -1.0)
        elif st[0] == "detection":
            if db2 > thr:
                self.state = ("tracking", thr + 0 * h_std, t0, [])
        else:
            st[3].append(db2)
            if db2 < thr:
                self.state = ("detection", st[1], t0 + cfg.after_tracking_wait_sec)
        return self

    def rows(self):
        sig = np.array(self.over, np.float64)
        return np.stack([sig, np.zeros_like(sig), np.zeros_like(sig)])


def _case(name, rows, cfg, fs=4000, bs=800, cap=None, expect=None):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    rows = rows.reshape(3, rows.size // 3)
    rows.setflags(write=False)
    return Case(name, rows, cfg, int(fs), int(bs), cap, expect)


def random_rows(seed, nb):
    """Gaussian rows plus bursts, the recipe of test_gpu_live.py::test_state_machine_random_rows at any nb"""
    rng = np.random.default_rng(seed)
    sig = rng.normal(0, 1, nb)
    if nb > 70:
        for s in rng.integers(50, nb - 10, max(3, nb // 50)):
            sig[s:s + rng.integers(1, 8)] += rng.uniform(5, 30)
    elif nb > 4:
        sig[nb // 2:nb // 2 + 2] += 20.0
    return np.stack([sig, rng.normal(0, 0.5, nb), rng.normal(0, 0.5, nb)])


def quiet_rows(rng, nb):
    """bounded noise: |over| <= 0.15, below mean + 4 std of any window of it; only planted blocks fire at k = 4"""
    return np.stack([rng.uniform(-0.1, 0.1, nb), rng.uniform(-0.05, 0.05, nb), rng.uniform(-0.05, 0.05, nb)])


# ------------------------------------------------------------------ config_sweep
SWEEP_N = 150
SWEEP_W = (0, 1, 7, 8, 9, 40, 127, 128, 129, 300)
SWEEP_K = (0.0, 0.5, 4.0)
SWEEP_INIT = ("0", "block", "8s", "60s", "file")
SWEEP_WAIT = (0.0, 0.2, 0.4, 0.6, 12.0, 200.0)
SWEEP_MIN_DB = (-1.0, 4.0)
SWEEP_MIN_DUR = (-1.0, 0.4, 0.6)


def sweep_params():
    """SWEEP_N seeded (nb, (fs, bs), W, k, init tag, wait, min dB, min dur): every column cycles through its
    values before it is shuffled, so each listed value of each parameter occurs"""
    rng = np.random.default_rng(2025_1020)

    def column(values):
        c = [values[i % len(values)] for i in range(SWEEP_N)]
        idx = rng.permutation(SWEEP_N)
        return [c[i] for i in idx]

    cols = [column(v) for v in (RATES, SWEEP_W, SWEEP_K, SWEEP_INIT, SWEEP_WAIT, SWEEP_MIN_DB, SWEEP_MIN_DUR)]
    return tuple((150 + int(551 * rng.uniform()),) + p for p in zip(*cols))


def init_wait(tag, nb, fs, bs):
    return {"0": 0.0, "block": bs / fs, "8s": 8.0, "60s": 60.0, "file": (nb * bs) / fs + 1.0}[tag]


def _config_sweep():
    out = []
    for i, (nb, (fs, bs), W, k, tag, wait, min_db, min_dur) in enumerate(sweep_params()):
        cfg = config(fs, bs, W, k, init_wait(tag, nb, fs, bs), wait, min_db, min_dur)
        out.append(_case(f"config_sweep/{i:03d}", random_rows(9000 + i, nb), cfg, fs, bs))
    return out


# ------------------------------------------------------------------ value_ties
def _probe_kinds():
    return {k: [] for k in ("det_tie", "det_below", "det_above", "trk_tie", "trk_above", "trk_below")}


def _dyadic_ties(k, wait, tag):
    """a history of 2.5 only: every sum is exact, mean 2.5, std 0, thr == 2.5 bit for bit.  wait 0: the
    fresh threshold decides; wait 12 s: after the first close the lock (also 2.5) does"""
    cfg = config(4000, 800, W=8, k=k, init=0.0, wait=wait)
    B, ex, c = _Builder(cfg), _probe_kinds(), 2.5

    def pad(n=10):
        for _ in range(n):
            B.push(c)
            assert B.state[0] == "detection"

    def probe(kind, step):
        t = B.used()
        assert t == c
        ex[kind].append(B.b)
        B.push(ulps(t, step))

    pad(12)
    for _ in range(2):  # the second pass of the 12 s rows runs under the lock
        for kind, step in (("det_tie", 0), ("det_below", -1)):
            pad()
            probe(kind, step)
            assert B.state[0] == "detection"
        pad()
        probe("det_above", +1)
        for kind, step in (("trk_tie", 0), ("trk_above", +1), ("trk_below", -1)):
            assert B.state[0] == "tracking" and B.state[1] == c
            probe(kind, step)
        assert B.state[0] == "detection"
    pad()
    return _case(f"value_ties/dyadic-k{k:g}-{tag}", B.rows(), cfg, expect=ex)


def _rounded_ties(k):
    """thresholds with real rounding: uniform history, W = 40; every seventh Detection block is the
    threshold it meets, or one ulp either side; the first three Tracking blocks are the lock, one ulp
    above it and one ulp below it (which closes)"""
    cfg = config(4000, 800, W=40, k=k)
    B, ex = _Builder(cfg), _probe_kinds()
    rng = np.random.default_rng(9200 + int(k))
    turn = 0
    for b in range(600):
        st = B.state
        if st[0] == "tracking":
            kind, step = (("trk_tie", 0), ("trk_above", +1), ("trk_below", -1))[min(len(st[3]), 2)]
            ex[kind].append(b)
            B.push(ulps(st[1], step))
        elif st[0] == "detection" and b > 45 and b % 7 == 0:
            kind, step = (("det_tie", 0), ("det_below", -1), ("det_above", +1))[turn % 3]
            turn += 1
            ex[kind].append(b)
            B.push(ulps(B.used(), step))
        else:
            B.push(rng.uniform(-1, 1))
    return _case(f"value_ties/rounded-k{k:g}", B.rows(), cfg, expect=ex)


MEAN_TIE_HISTORIES = ((4.0,), (5.0, 5.0, 2.0), (4.5, 4.5, 4.5, 4.5, 2.0), (float(ulps(4.0, 1)),),
                      (float(ulps(4.0, -1)),), (8.0, 0.0))


def _mean_ties(k, tag, min_db):
    """tracking histories of dyadic values whose mean is 4.0 exactly, and single-element ones one ulp off,
    against min_db_mean 4.0 and its two neighbours.  The history is 4.5 (the lock); the 12 s wait keeps the
    lock in use between the events, whatever the closed bursts do to the window"""
    cfg = config(4000, 800, W=8, k=k, init=0.0, wait=12.0, min_db=min_db)
    B, closes = _Builder(cfg), []
    for _ in range(12):
        B.push(4.5)
    for h in MEAN_TIE_HISTORIES:
        assert B.state[0] == "detection" and B.used() == 4.5
        B.push(9.0)
        for v in h:
            assert B.state[0] == "tracking" and B.state[1] == 4.5
            B.push(v)
        assert B.state[0] == "detection"
        closes.append((B.b - 1, float(np.mean(h)) >= min_db))
        for _ in range(12):
            B.push(4.5)
    return _case(f"value_ties/mean-k{k:g}-{tag}", B.rows(), cfg, expect={"closes": closes})


def _value_ties():
    out = []
    for k in (0.0, 4.0):
        out += [_dyadic_ties(k, 0.0, "fresh"), _dyadic_ties(k, 12.0, "locked"), _rounded_ties(k)]
        out += [_mean_ties(k, tag, float(ulps(4.0, s))) for tag, s in (("eq", 0), ("up", 1), ("down", -1))]
    return out


# ------------------------------------------------------------------ time_ties
TT_FS, TT_BS, TT_NB = 4000, 800, 700
TT_WAITS = ((0.2, 1), (0.4, 2), (0.6, 3))  # (wait, wait / block_sec)


def until_vs_end(c, wait, n):
    """'gt' / 'lt' / 'eq': until = t0(c) + wait against the end of block c + n - 1, the one block where the
    two are a rounding apart"""
    until, t1 = t_start_of(c, TT_FS, TT_BS) + wait, t_end_of(c + n - 1, TT_FS, TT_BS)
    return "gt" if until > t1 else ("lt" if until < t1 else "eq")


def _spaced(first, pick, gap=60, last=TT_NB - 12):
    """block indices >= first, at least gap apart, the i-th one accepted by pick(i, block)"""
    out, b = [], first
    while b <= last:
        if pick(len(out), b):
            out.append(b)
            b += gap
        else:
            b += 1
    return out


def _balanced_closes(first, wait, n, gap=50, last=TT_NB - 12):
    """close blocks at least gap apart, each the nearest block of the set that has had the fewest so far"""
    out, count, b = [], {"gt": 0, "lt": 0, "eq": 0}, first
    while True:
        nxt = {rel: next((c for c in range(b, last + 1) if until_vs_end(c, wait, n) == rel), None) for rel in count}
        nxt = {rel: c for rel, c in nxt.items() if c is not None}
        if not nxt:
            return out
        rel = min(nxt, key=lambda r: (count[r] * 40 + nxt[r] - b, r))
        out.append(nxt[rel])
        count[rel] += 1
        b = nxt[rel] + gap


def _lock_row(wait, n, offset, first, seed):
    """closes at blocks drawn in turn from the three sets; on block c + n - 1 + offset a value above the
    lock and below the fresh threshold (the burst just closed is inside the window): Tracking starts
    there exactly when the lock is still in use"""
    cfg = config(TT_FS, TT_BS, W=40, k=4.0, wait=wait)
    rng = np.random.default_rng(seed)
    B, ev = _Builder(cfg), []
    for c in _balanced_closes(first, wait, n):
        while B.b < c - 2:
            B.push(rng.uniform(-0.1, 0.1))
        assert B.state[0] == "detection"
        B.push(30.0).push(30.0).push(rng.uniform(-0.1, 0.1))
        assert B.state[0] == "detection" and B.b == c + 1
        lock = B.state[1]
        p = c + n - 1 + offset
        while B.b < p:
            B.push(rng.uniform(-0.1, 0.1))
        assert lock < lock + 1.0 < B.fresh()[0] and B.state[0] == "detection"
        B.push(lock + 1.0)
        ev.append((c, p, until_vs_end(c, wait, n)))
    while B.b < TT_NB:
        B.push(rng.uniform(-0.1, 0.1))
    return _case(f"time_ties/lock-{wait}-{offset:+d}-{first}", B.rows(), cfg, expect={"lock": ev, "offset": offset})


def _dur_row(n, min_dur, first, seed):
    """tracking runs of exactly n blocks (trigger s, close s + n) against min_dur = n block lengths: the
    duration (s + n) bs / fs - s bs / fs rounds to either side of it"""
    cfg = config(TT_FS, TT_BS, W=40, k=4.0, min_dur=min_dur)
    rng = np.random.default_rng(seed)
    rows = quiet_rows(rng, TT_NB)
    dur = lambda s: t_start_of(s + n, TT_FS, TT_BS) - t_start_of(s, TT_FS, TT_BS)  # noqa: E731
    ev = []
    for s in _spaced(first, lambda i, s: (dur(s) >= min_dur) == (i % 2 == 0)):
        rows[0, s:s + n] += 30.0
        ev.append((s, s + n, bool(dur(s) >= min_dur)))
    return _case(f"time_ties/dur-{n}-{min_dur}-{first}", rows, cfg, expect={"dur": ev})


def _dur_exact(n, min_dur, s):
    """the only runs whose duration is min_dur bit for bit start on blocks 0, 2 and 3 (later block starts are
    too coarse): a history of 2.5, a trigger on block s, a close on block s + n; emitted, as >= says"""
    cfg = config(TT_FS, TT_BS, W=8, k=4.0, init=0.0, min_dur=min_dur)
    B = _Builder(cfg)
    for v in [2.5] * s + [9.0] * n + [2.0] + [2.5] * 12:
        B.push(v)
    assert t_start_of(s + n, TT_FS, TT_BS) - t_start_of(s, TT_FS, TT_BS) == min_dur and B.state[0] == "detection"
    return _case(f"time_ties/dur_exact-{n}-{s}", B.rows(), cfg, expect={"dur_exact": (s, s + n)})


def _init_rows():
    """init_wait equal to a block start and one ulp either side; the block after it fires if Init is over"""
    out = []
    for fs, bs in ((4000, 800), (44100, 4410)):
        for b0 in (7, 41):
            for s in (-1, 0, 1):
                wait = float(ulps(t_start_of(b0, fs, bs), s))
                rows = quiet_rows(np.random.default_rng(9400 + b0), 80)
                rows[0, b0 + 1] += 30.0
                out.append(_case(f"time_ties/init-{fs}-{b0}{s:+d}", rows, config(fs, bs, W=8, init=wait), fs, bs,
                                 expect={"init_end": b0 + (s > 0), "burst": b0 + 1}))
    return out


def _time_ties():
    out = [_lock_row(0.2, 1, +1, 60, 9300)]
    for j, (wait, n) in enumerate(TT_WAITS[1:]):
        out += [_lock_row(wait, n, 0, 60, 9310 + j), _lock_row(wait, n, 0, 75, 9320 + j),
                _lock_row(wait, n, +1, 65, 9330 + j)]
    out.append(_lock_row(0.6, 3, -1, 70, 9340))  # (wait 0.4: the block before is the closing block itself)
    for j, (n, md) in enumerate(((2, 0.4), (3, 0.6))):
        out += [_dur_row(n, md, 60, 9350 + j), _dur_row(n, md, 85, 9360 + j)]
    out += [_dur_row(3, 0.4, 60, 9370), _dur_row(2, 0.6, 60, 9371)]  # clear of the tie: always / never
    out += [_dur_exact(n, md, s) for n, md in ((2, 0.4), (3, 0.6)) for s in (2, 3)]
    return out + _init_rows()


# ------------------------------------------------------------------ lane_and_segment_edges
EDGE_NB = 600
EDGE_BLOCKS = (0, 1, 62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 258, 511, 512, 513, EDGE_NB - 2, EDGE_NB - 1)
EDGE_GROUPS = ((63, 127, 255, 511, EDGE_NB - 2), (62, 128, 256, 512, EDGE_NB - 1), (64, 254, 513), (65, 257),
               (258,))
EDGE_MIXED_NB = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 3000)
EDGE_WAIT = 1.0  # s: five blocks


def expiry_block(c, wait, fs=4000, bs=800):
    """the first block after a close at c that no longer meets the lock (until > block end fails)"""
    until, b = t_start_of(c, fs, bs) + wait, c + 1
    while until > t_end_of(b, fs, bs):
        b += 1
    return b


def _edges():
    out = []
    for X in EDGE_BLOCKS:  # Init ends on X
        out.append(_case(f"lane_and_segment_edges/init_end-{X}", random_rows(9500 + X, EDGE_NB),
                         config(4000, 800, init=t_start_of(X, 4000, 800), wait=0.4), expect={"init_end": (X,)}))
    for g, group in enumerate(EDGE_GROUPS):
        rng = np.random.default_rng(9520 + g)
        trig, close, exp = (quiet_rows(rng, EDGE_NB) for _ in range(3))
        ge = tuple(X for X in group if X >= 62)
        for X in group:
            trig[0, X:X + 3] += 30.0   # a trigger on X (the run of the last two stays open at the end)
        for X in ge:
            close[0, X - 3:X] += 30.0  # a close on X
            c = next(c for c in range(X - 8, X) if expiry_block(c, EDGE_WAIT) == X)
            exp[0, c - 3:c] += 30.0    # a lock that runs out on X, where a value above it no longer fires
            exp[0, X] += 1.0
        out.append(_case(f"lane_and_segment_edges/trigger-g{g}", trig, config(4000, 800), expect={"trigger": group}))
        out.append(_case(f"lane_and_segment_edges/close-g{g}", close, config(4000, 800), expect={"close": ge}))
        out.append(_case(f"lane_and_segment_edges/expiry-g{g}", exp, config(4000, 800, wait=EDGE_WAIT),
                         expect={"expiry": ge}))
    rows = quiet_rows(np.random.default_rng(9530), EDGE_NB)  # Init ends on block 0, block 1 fires
    rows[0, 1:4] += 30.0
    out.append(_case("lane_and_segment_edges/trigger-1", rows, config(4000, 800, init=0.0), expect={"trigger": (1,)}))
    for nb in EDGE_MIXED_NB:  # one configuration: files of every length in one launch
        out.append(_case(f"lane_and_segment_edges/mixed-{nb}", random_rows(9540 + nb, nb),
                         config(4000, 800, W=8, k=2.0, init=0.0, wait=0.4)))
    for edges, stop, nb in ((1, 260, 400), (2, 520, 700), (5, 1290, 1400)):  # a run across segment edges
        rows = quiet_rows(np.random.default_rng(9560 + edges), nb)
        rows[0, 250:stop] += 30.0
        out.append(_case(f"lane_and_segment_edges/run_across-{edges}", rows, config(4000, 800),
                         expect={"run": (250, stop)}))
    rows = quiet_rows(np.random.default_rng(9570), 1400)  # a 200 s lock across four segment edges, then met
    rows[0, 247:250] += 30.0
    rows[0, 1100:1102] += 1.0
    rows[0, 1300:1302] += 1.0
    out.append(_case("lane_and_segment_edges/lock_200s", rows, config(4000, 800, wait=200.0),
                     expect={"close": (250,), "trigger": (1100, 1300)}))
    out.append(_case("lane_and_segment_edges/init_300", random_rows(9580, 700), config(4000, 800, init=60.0),
                     expect={"init_end": (300,)}))
    return out


# ------------------------------------------------------------------ long_histories
LONG_RUNS_SHORT = (1, 2, 7, 8, 9, 127, 128, 129, 255, 256, 257)
LONG_RUNS = LONG_RUNS_SHORT + (1000, 8193)
LONG_W0_NB = 8192 + 200


def _plateaus(seed, lengths, tail=150):
    rng = np.random.default_rng(seed)
    nb = 60 + sum(n + 60 for n in lengths) + tail
    rows, s, runs = quiet_rows(rng, nb), 60, []
    for n in lengths:
        rows[0, s:s + n] += 30.0 + rng.uniform(-1, 1, n)
        runs.append((s, s + n))  # trigger s, close s + n: a history of n values
        s += n + 60
    return rows, tuple(runs)


def _long_histories():
    out = [_case("long_histories/w0", random_rows(9600, LONG_W0_NB), config(4000, 800, W=0, init=8.0, wait=12.0))]
    for name, lengths in (("short", LONG_RUNS_SHORT), ("1000", (1000,)), ("8193", (8193,))):
        rows, runs = _plateaus(9610 + len(out), lengths)
        out.append(_case(f"long_histories/runs-{name}", rows, config(4000, 800), expect={"runs": runs}))
    return out


# ------------------------------------------------------------------ nonfinite
NF_KINDS = {"neginf_sig": (-INF, None, None), "all_neginf": (-INF, -INF, -INF), "posinf_sig": (INF, None, None),
            "nan_sig": (np.nan, None, None), "neginf_noise": (None, -INF, None), "nan_noise": (None, None, np.nan)}
NF_PLACES = {"window": 80, "trigger": 200, "first": 201, "later": 203}
NF_NB = 300


def _nf_base(seed):
    rows = quiet_rows(np.random.default_rng(seed), NF_NB)
    rows[0, 100:106] += 30.0
    rows[0, 200:206] += 30.0
    return rows


def _zero_rows():
    """+0.0 and -0.0 in every combination of the three rows, a burst whose history opens with -0.0, +0.0,
    -0.0, and histories of a single -0.0"""
    z = (0.0, -0.0)
    combos = [(a, b, c) for a in z for b in z for c in z] * 2
    sig = [c[0] for c in combos] + [5.0, -0.0, 0.0, -0.0, -1.0] + [2.0] * 9 + [-0.0] + [2.0] * 3 + [9.0, -0.0] + \
        [c[0] for c in combos]
    n1 = [c[1] for c in combos] + [-0.0, -0.0, 0.0, -0.0, 0.0] + [-0.0] * 15 + [c[1] for c in combos]
    n2 = [c[2] for c in combos] + [-0.0, -0.0, -0.0, 0.0, 0.0] + [-0.0] * 15 + [c[2] for c in combos]
    return np.array([sig, n1, n2], np.float64)


def _nonfinite():
    out = []
    for kind, vals in NF_KINDS.items():
        for place, b in NF_PLACES.items():
            rows = _nf_base(9700 + len(out))
            for j, v in enumerate(vals):
                if v is not None:
                    rows[j, b] = v
            out.append(_case(f"nonfinite/{kind}-{place}", rows, config(4000, 800, wait=0.4), expect={"block": b}))
    rows = _nf_base(9790)  # a trigger under a lock while the fresh window holds -inf: the new lock is NaN
    rows[0, 110] = -INF
    rows[0, 120:123] += 30.0
    out.append(_case("nonfinite/lock_becomes_nan", rows, config(4000, 800, wait=12.0), expect={"block": 110}))
    for k in (0.0, 4.0):
        out.append(_case(f"nonfinite/signed_zeros-k{k:g}", _zero_rows(), config(4000, 800, W=8, k=k, init=0.0)))
    return out


# ------------------------------------------------------------------ capacity
CAP_COUNT = 12


def _capacity():
    out = []
    rows = []
    for r in range(2):
        rng = np.random.default_rng(9800 + r)
        q = quiet_rows(rng, 700)
        for i in range(CAP_COUNT):
            s = 55 + 25 * r + 50 * i
            q[0, s:s + 1 + int(rng.integers(0, 5))] += 30.0
        rows.append(q)
    for cap in (0, 1, CAP_COUNT - 1, CAP_COUNT, CAP_COUNT + 1):
        for r in range(2):
            out.append(_case(f"capacity/cap{cap}-row{r}", rows[r], config(4000, 800), cap=cap,
                             expect={"count": CAP_COUNT}))
    return out


_GENERATORS = {"config_sweep": _config_sweep, "value_ties": _value_ties, "time_ties": _time_ties,
               "lane_and_segment_edges": _edges, "long_histories": _long_histories, "nonfinite": _nonfinite,
               "capacity": _capacity}


@functools.lru_cache(maxsize=None)
def cases(cls):
    """the cases of one class, in a fixed order; read-only"""
    return tuple(_GENERATORS[cls]())


@functools.lru_cache(maxsize=None)
def _by_name(cls):
    return {c.name: c for c in cases(cls)}


def case(name):
    return _by_name(name.split("/")[0])[name]


def groups(rows, with_cap=True):
    """cases of one configuration (and capacity), in order of first appearance"""
    g = {}
    for c in rows:
        g.setdefault(cfg_key(c) + ((c.cap,) if with_cap else ()), []).append(c)
    return list(g.values())


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle on case `name`"""
    c = case(name)
    nb = c.rows.shape[1]
    with _quiet():
        rm, thr, over = L.live_detect_ref(c.rows, c.fs, c.bs, c.cfg)
    thr, over = thr.reshape(nb), over.reshape(nb)
    states = tuple(replay(thr, over, c.cfg, c.fs, c.bs))
    W = win_blocks(c.cfg)
    events, closes = [], []
    trig, lock, until, t_start, locked = 0, -1.0, -1.0, 0.0, False
    ties, longest, prev = 0, 0, ("init",)
    for b, s in enumerate(states):
        t0, t1 = t_start_of(b, c.fs, c.bs), t_end_of(b, c.fs, c.bs)
        if prev[0] == "init":
            ties += int(t0 == c.cfg.init_detection_wait_sec)
        else:
            ties += int(over[b] == thr[b]) + int(prev[0] == "detection" and prev[2] == t1)
        longest = max(longest, min(W, b) if W else b)
        if locked and prev[0] == "detection" and not prev[2] > t1:
            events.append((b, "expiry"))
            locked = False
        if s[0] != prev[0]:
            if prev[0] == "init":
                events.append((b, "init_end"))
                lock, until = s[1], s[2]
            elif s[0] == "tracking":
                events.append((b, "trigger"))
                lock, t_start, trig, locked = s[1], s[2], s[3], False
            else:
                events.append((b, "close"))
                closes.append((prev[3], b))
                ties += int(t0 - prev[2] == c.cfg.detection_dur_min_sec)
                longest = max(longest, b - prev[3])
                lock, until, locked = s[1], s[2], True
        prev = s
    final = ({"init": 0, "detection": 1, "tracking": 2}[prev[0]], trig, lock, until, t_start)
    meteors = np.zeros(len(rm), METEOR)
    it = iter(closes)
    for i, m in enumerate(rm):  # a meteor's closing block is the close whose block start is its time_stop
        a, e = next((a, e) for a, e in it if t_start_of(e, c.fs, c.bs) == m.time_stop)
        meteors[i] = (a, e) + tuple(getattr(m, f) for f in STATS)
    for a in (thr, over, meteors):
        a.setflags(write=False)
    return Ref(meteors, thr, over, states, tuple(events), final, ties, longest,
               int(np.count_nonzero(~np.isfinite(over))))


def summary_line(cls, rows=None):
    rows = cases(cls) if rows is None else rows
    refs = [reference(c.name) for c in rows]
    return (f"LIVE {cls}: files {len(rows)}, blocks {sum(c.rows.shape[1] for c in rows)}, meteors "
            f"{sum(len(r.meteors) for r in refs)}, exact ties {sum(r.ties for r in refs)}, longest history "
            f"{max(r.longest for r in refs)}, non-finite blocks {sum(r.nonfinite for r in refs)}")
