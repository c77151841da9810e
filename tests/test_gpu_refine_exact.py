"""GPU: the exact C5 delta step (msd_iq_delta64_dev: csrc/refine_i8.hip's block_i8_kernel, then
csrc/refine.hip's frame_kernel) held to tests/refine_exact.py's restatement of its own arithmetic, on
every path of the tile pipeline, the compact block map and the bin layouts -- where the other tests hold
it to |delta - oracle| <= ed with ed read from the device (200-400 times loose).  Driven through
_lib.iq_delta64_dev alone; samples at a 16-byte-aligned base; delta, ed and frame_sums pre-filled with a
NaN of a recognisable payload and 64 guard entries past the last frame.

Bars (none reads the device's ed; u = 2^-53; own / combine / reference from msd_iq_delta64_chain; amp
= frame_kernel's from the exact integer sums):
 1 model        |delta - delta_truth| <= db_bound(E_b, n_b, d) + db_bound(E_n, n_n, d) + 1e-13 with d =
                (own + combine) u amp + N 2^-63 amp, truth in long double ("truth" cases); on the three
                whole-grid pipeline cases truth is too slow and the float64 scipy oracle stands in with d =
                (own + combine + reference) u amp ("oracle" cases).
 2 restatement  (int8 path) |sqrt E_gpu - sqrt E_quantised| <= sqrt n (own - 91 + combine) u amp + 3 u
                sqrt E per band where the other band is empty (its dB is exactly 10 log10(1e-12), so E_gpu
                = 10^(dB / 10) - 1e-12; the recovery's own error, 8 u (|dB| + 1) (ln 10 / 10) (E + 1e-12) in
                E, is added: it dominates below E ~ 1e-24); elsewhere |delta - delta_quantised| within the
                same d carried through db_bound.
 3 precision    (noise-like input) rms over the frames of delta_gpu - delta_quantised <= 4 x the float64
                yardstick's.
 4 exact        frame_sums bit-equal to the integer sums; MSD_ERR_UNSUPPORTED with nothing written where
                the block step carries no sums (int8, <= 8 bins); ed within 1e-9 of its restatement (from
                l1_device on the int8 path) wherever the band energies it was formed from are known to
                1e-10 of themselves (ed moves by at most half an energy's relative change) -- recovered
                from delta where a band is empty, else the reference's where 2 sqrt n d / sqrt E <= 1e-10;
                the count of frames this covers is recorded -- and ed >= |delta - delta_truth|; every frame inside the
                ranges written, every other entry and the guards bit for bit the payload; all-zero input
                exactly 0.
 5 invariance   delta, ed and sums bit-equal in one range, alone in [t, t + 1), in a many-range list, on a
                second call, on a fresh context and on a context that has just run other geometries.

The largest ratio to each bar per case goes to the file REFINE_EXACT_RATIO_FILE names
(profiles/refine_exact_mi355x.txt); no measured ratio is asserted back."""
import math
import os

import numpy as np
import pytest

import refine_exact as X
from band_signals import LD_OK, LD_REASON
from meteorgpu import _lib
from oracle import iq_oracle as Q

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not LD_OK, reason=LD_REASON)]

FS = 192000.0
GUARD = 64
CI16, CF32 = _lib.MSD_CI16, _lib.MSD_CF32
PAY = {"delta": 0x7FF8DE17A0000001, "ed": 0x7FF80ED000000002, "sums": 0x7FF85A3500000003}
C5_BAND, C5_NOISE = (21, 22), (-65, -63)


def _f(v):
    return np.asarray(v, dtype=np.float64)


def _cus():
    """the device's compute units (launch_refine_i8 sizes its grid from them)"""
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256  # MI355X


@pytest.fixture(scope="module")
def ctx():
    from meteorgpu import dsp
    return dsp.context(0)


def _note(case, ratios):
    line = f"{case}: " + ", ".join(f"{k} {v:.4g}" for k, v in ratios.items())
    print(line)
    path = os.environ.get("REFINE_EXACT_RATIO_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ----------------------------------------------------------------------------- launching
class Samples:
    """int16 (or float32 = int16 / 32768: every sum stays exact) interleaved I/Q on the device at a
    16-byte-aligned base, and the values the references take"""

    def __init__(self, ctx, x16, f32=False):
        self.ctx = ctx
        self.x16 = np.ascontiguousarray(x16, dtype=np.int16).reshape(-1)
        self.code = CF32 if f32 else CI16
        self.unit = 2.0 ** -15 if f32 else 1.0
        raw = (self.x16.astype(np.float32) / np.float32(32768.0)) if f32 else self.x16
        self.n = self.x16.size // 2
        self.buf = ctx.alloc(raw.nbytes + 64)
        assert self.buf.ptr.value % 16 == 0
        self.buf.upload(raw)
        ctx.synchronize()
        self.ref = self.x16.astype(np.float64) * self.unit if f32 else self.x16  # what truth / amp take
        self.cache = {}

    def frames(self, P):
        return (self.n - P.N) // P.hop + 1 if self.n >= P.N else 0

    def free(self):
        self.buf.free()


class Out:
    def __init__(self, rc, delta, ed, sums):
        self.rc, self.delta, self.ed, self.sums = rc, delta, ed, sums  # uint64 bit patterns

    def f(self, name):
        return getattr(self, name).view(np.float64)

    def same(self, other, frames):
        """bit equality of delta, ed and sums on the frames"""
        fr = np.asarray(frames, np.int64)
        return (np.array_equal(self.delta[fr], other.delta[fr]) and np.array_equal(self.ed[fr], other.ed[fr])
                and np.array_equal(self.sums.reshape(-1, 2)[fr], other.sums.reshape(-1, 2)[fr]))


def _launch(ctx, S, P, ranges, sums=True):
    """one msd_iq_delta64_(sums_)dev call into freshly pre-filled buffers"""
    T = S.frames(P)
    n = T + GUARD
    bufs = [ctx.alloc(8 * n), ctx.alloc(8 * n), ctx.alloc(16 * n)]
    try:
        for b, k, m in zip(bufs, ("delta", "ed", "sums"), (n, n, 2 * n)):
            b.upload(np.full(m, PAY[k], np.uint64))
        rc = _lib.MSD_OK
        try:
            _lib.iq_delta64_dev(ctx, S.buf, S.code, S.n, P.N, P.hop, P.fs, P.band, P.noise,
                                np.asarray(ranges, np.int64).reshape(-1, 2), bufs[0], bufs[1],
                                frame_sums=bufs[2] if sums else None)
        except _lib.MsdError as e:
            rc = e.code
        ctx.synchronize()
        got = [b.download(np.empty(m, np.uint64)) for b, m in zip(bufs, (n, n, 2 * n))]
    finally:
        for b in bufs:
            b.free()
    return Out(rc, *got)


def _inside(ranges, T):
    m = np.zeros(T + GUARD, bool)
    for a, b in np.asarray(ranges, np.int64).reshape(-1, 2):
        m[a:b] = True
    return m


def _has_sums(P, code, goertzel):
    return not (code == CI16 and not goertzel and P.i8() and P.nk <= 8)


def _run(ctx, S, P, ranges, goertzel=False):
    """the call with sums where the block step carries them; where not, first the refusal with nothing
    written (bar 4), then the call without.  Checks what is written and what is not."""
    T = S.frames(P)
    ranges = np.asarray(ranges, np.int64).reshape(-1, 2)
    has = _has_sums(P, S.code, goertzel)
    if not has:
        o = _launch(ctx, S, P, ranges, sums=True)
        assert o.rc == _lib.MSD_ERR_UNSUPPORTED
        for k in PAY:
            assert (getattr(o, k) == PAY[k]).all(), k
    o = _launch(ctx, S, P, ranges, sums=has)
    assert o.rc == _lib.MSD_OK
    m = _inside(ranges, T)
    for k in ("delta", "ed"):
        v = getattr(o, k)
        assert (v[~m] == PAY[k]).all(), (k, "outside the ranges or in the guards")
        assert (v[m] != PAY[k]).all() and not np.isnan(o.f(k)[m]).any(), (k, "inside the ranges")
    s = o.sums.reshape(-1, 2)
    assert (s[~m] == PAY["sums"]).all()
    if has:
        assert (s[m] != PAY["sums"]).all()
    else:
        assert (s == PAY["sums"]).all()
    return o


def _cached(fn):
    def get(S, P, T):
        key = (fn.__name__, P.N, P.hop, T)
        if key not in S.cache:
            S.cache[key] = fn(S, P, T)
        return S.cache[key]
    return get


@_cached
def _int_sums(S, P, T):
    """every frame's (sum I, sum Q) as exact integers [T, 2], from block sums"""
    z = S.x16.reshape(-1, 2)
    nb = z.shape[0] // P.D
    bs = z[: nb * P.D].reshape(nb, P.D, 2).sum(axis=1, dtype=np.int64)
    cs = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(bs, axis=0)])
    m0 = np.arange(T) * (P.hop // P.D)
    return cs[m0 + P.R] - cs[m0]


@_cached
def _abs_sums(S, P, T):
    """every frame's sum (|I| + |Q|) as an exact integer [T]"""
    z = np.abs(S.x16.reshape(-1, 2).astype(np.int32)).sum(axis=1, dtype=np.int64)
    nb = z.shape[0] // P.D
    cs = np.concatenate([[0], np.cumsum(z[: nb * P.D].reshape(nb, P.D).sum(axis=1))])
    m0 = np.arange(T) * (P.hop // P.D)
    return cs[m0 + P.R] - cs[m0]


def _oracle(S, P, T, chunk=1024):
    """(delta, E_band, E_noise) of every frame from scipy.signal.spectrogram, in chunks of frames"""
    z = S.x16.reshape(-1, 2)
    f = FS / P.N
    fb, fn = [((lo - 0.3) * f, (hi + 0.3) * f) if hi >= lo else (1.0, 0.0) for lo, hi in (P.band, P.noise)]
    kb, kn = ([P.km[t[1]] for t in idx] for idx in (P.bidx, P.nidx))
    d, eb, en = [], [], []
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        seg = z[a * P.hop: (b - 1) * P.hop + P.N]
        _, _, Sx = Q.spectrogram_iq_ref(seg[:, 0], seg[:, 1], FS, P.N, P.N - P.hop)
        assert Sx.shape[1] == b - a
        d.append(Q.band_delta_iq_ref(Sx, FS, P.N, fb, fn)[2])
        eb.append(Sx[kb].sum(axis=0) if kb else np.zeros(b - a))
        en.append(Sx[kn].sum(axis=0) if kn else np.zeros(b - a))
    return np.concatenate(d), np.concatenate(eb), np.concatenate(en)


def _check(case, S, P, o, frames, *, goertzel=False, noise_like=False, oracle=None, all_frames=None):
    """bars 1-4 on `frames` (bar 1 in its truth form there; with oracle = (delta, Eb, En) of every frame
    also in its oracle form on all_frames); returns the largest ratios"""
    frames = [int(t) for t in frames]
    fr = np.asarray(frames, np.int64)
    T = S.frames(P)
    code = S.code
    own, combine, reference = X.chains(P, code, goertzel)
    i8 = code == CI16 and not goertzel and P.i8()
    assert (_lib.iq_delta64_path(P.N, P.hop, P.fs, P.band, P.noise, code) == _lib.REFINE_INT8_MFMA) == (
        code == CI16 and P.i8())
    delta, ed = o.f("delta"), o.f("ed")
    ratios = {}
    # bar 4: the sums, on every written frame
    m = np.flatnonzero(_inside_of(o, T))
    if _has_sums(P, code, goertzel):
        want = _int_sums(S, P, T).astype(np.float64) * S.unit
        assert np.array_equal(o.f("sums").reshape(-1, 2)[m], want[m]), "frame_sums against the integer sums"
    amp_all = X._amp(P, _abs_sums(S, P, T).astype(np.float64) * S.unit, _int_sums(S, P, T).astype(np.float64) * S.unit)
    amp = amp_all[fr]
    silent = amp_all == 0
    assert (delta[m][silent[m]] == 0.0).all(), "all-zero input"
    # bar 1, truth form
    dt, ebt, ent = X.truth(P, S.ref.reshape(-1, 2), frames)
    dtf = _f(dt)
    b1 = X.delta_bar(P, _f(ebt), _f(ent), (own + combine) * X.U * amp + X.truth_error(P, amp))
    r = np.abs(delta[fr] - dtf) / b1
    assert (r <= 1.0).all(), (case, "model", frames[int(np.argmax(r))], float(r.max()))
    ratios["model"] = float(r.max())
    assert (ed[fr] >= np.abs(delta[fr] - dtf)).all(), (case, "ed below the error")
    ratios["err/ed"] = float((np.abs(delta[fr] - dtf) / ed[fr]).max())
    if oracle is not None:
        od, oeb, oen = oracle
        af = np.asarray(all_frames, np.int64)
        bo = X.delta_bar(P, oeb[af], oen[af], (own + combine + reference) * X.U * amp_all[af])
        ro = np.abs(delta[af] - od[af]) / bo
        assert (ro <= 1.0).all(), (case, "model (oracle)", int(af[int(np.argmax(ro))]), float(ro.max()))
        assert (ed[af] >= np.abs(delta[af] - od[af])).all()
        ratios["model_oracle"] = float(ro.max())
    # the energies ed was formed from, and how well each is known (dE): recovered from delta where the other
    # band is empty (the recovery's own error), else the reference's (the kernel is within d of it per bin)
    E = [_f(ebt), _f(ent)]
    side = 0 if (P.nn == 0 and P.nb) else 1 if (P.nb == 0 and P.nn) else None
    if side is not None:
        Erec = np.maximum(X.recover_E(delta[fr], side), 0.0)
        db = delta[fr] + X.FLOOR_DB if side == 0 else X.FLOOR_DB - delta[fr]
        rec = 8.0 * X.U * (np.abs(db) + 1.0) * (math.log(10.0) / 10.0) * (Erec + X.FLOOR)
    if i8:
        dq, ebq, enq = X.quantised(P, S.x16, frames)
        dy, eby, eny = X.yardstick(P, S.x16, frames)
        E = [eby, eny]
        if side is not None:  # bar 2, per band
            n, eq = (P.nb, ebq) if side == 0 else (P.nn, enq)
            srec = np.minimum(np.sqrt(rec), rec / np.maximum(np.sqrt(Erec), 1e-300))
            bar = X.sqrtE_bar(P, n, Erec, amp, own, combine)
            err = np.abs(np.sqrt(Erec) - _f(np.sqrt(eq)))
            live = bar > 0
            r2 = err[live] / (bar + srec)[live]
            assert (r2 <= 1.0).all(), (case, "restatement", float(r2.max()))
            ratios["restatement"] = float(r2.max(initial=0.0))
            ratios["restatement_less_recovery"] = float((np.maximum(err - srec, 0.0)[live] / bar[live]).max(initial=0.0))
        else:
            b2 = X.delta_bar(P, _f(ebq), _f(enq), (own - _lib.REFINE_I8_CHAIN_QUANT + combine) * X.U * amp)
            r2 = np.abs(delta[fr] - _f(dq)) / b2
            assert (r2 <= 1.0).all(), (case, "restatement (delta)", float(r2.max()))
            ratios["restatement_delta"] = float(r2.max())
        if noise_like:  # bar 3
            rg, ry = X.rms_ld(delta[fr], dq), X.rms_ld(dy, dq)
            assert rg <= 4.0 * ry, (case, "precision", rg, ry)
            ratios["rms/yardstick"] = rg / ry if ry > 0 else 0.0
        amp_d = X.amp_device(P, S.x16, frames)
    else:
        amp_d = amp
    # bar 4: ed restated wherever both energies are known to 1e-10 of themselves (ed moves by at most half
    # the relative change of an energy)
    chain = own + combine + reference
    d = chain * X.U * amp_d
    known = np.ones(len(fr), bool)
    for sd, n in ((0, P.nb), (1, P.nn)):
        if not n:
            continue
        if sd == side:
            E[sd] = Erec
            known &= rec <= 1e-10 * Erec
        else:
            known &= 2.0 * math.sqrt(n) * d * np.sqrt(E[sd]) + n * d * d <= 1e-10 * E[sd]
    want = X.ed(P, E[0], E[1], amp_d, chain)
    ok = known & np.isfinite(want)
    assert np.allclose(ed[fr][ok], want[ok], rtol=1e-9, atol=0.0), (case, "ed restated")
    assert not np.isinf(ed[fr][ok]).any()
    ratios["ed_restated_on"] = float(ok.sum())
    return ratios


def _inside_of(o, T):
    """the frames a run wrote (its delta no longer the payload); what lies inside the ranges is checked in _run"""
    return o.delta[:T] != PAY["delta"]


def _noise16(n, seed, sigma=300.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(0.0, sigma, 2 * n)), -32768, 32767).astype(np.int16)


def _fast16(n, seed, lim=2000):
    return np.random.default_rng(seed).integers(-lim, lim + 1, 2 * n, dtype=np.int16)


def _pick(T, k, seed):
    rng = np.random.default_rng(seed)
    return sorted({0, T - 1} | set(int(t) for t in rng.integers(0, T, k)))


# ----------------------------------------------------------------------------- the tile pipeline
def _pipeline_frames(nblk, T, seed):
    """the first and last frame of each pipeline position of the first wave, a middle wave and the last
    wave (block_i8_kernel: wave w takes tiles w + j nwaves of four blocks), plus 64 random frames"""
    ntiles = -(-nblk // 4)
    nwaves = 4 * ((min(4 * _cus(), ntiles) + 3) // 4)
    out = set(_pick(T, 64, seed))
    cnts = set()
    for w in (0, nwaves // 2, nwaves - 1):
        tiles = list(range(w, ntiles, nwaves))
        cnts.add(len(tiles))
        for tile in tiles:
            out.update(t for t in (4 * tile, 4 * tile + 3) if t < T)
    return sorted(out), cnts, nwaves


@pytest.mark.parametrize("mult,extra,cnts", [(6, 1, {1, 2}), (14, 3, {3, 4}), (18, 2, {4, 5})],
                         ids=["cnt1-2", "cnt3-4", "cnt4-5"])
def test_pipeline_many_tiles_per_wave(ctx, mult, extra, cnts):
    """4 W + 2 W + 1, 12 W + 2 W + 3 and 16 W + 2 W + 2 blocks (W = 4 CUs waves of 4 blocks): tile counts
    per wave 1 and 2 (no loop, the even tail), 3 and 4 (the paired loop body once, both tails), 4 and
    5; the prefetch of tile k + 2 clamped.  Bars 1 (oracle form), 4 and 5 on every frame; 1 (truth), 2
    and 3 on the pipeline positions of three waves and 64 random frames."""
    W = 4 * _cus()
    nblk = mult * W + extra
    P = X.Plan(4096, 1024, FS, C5_BAND, C5_NOISE)
    S = Samples(ctx, _fast16(nblk * 1024, seed=mult))
    try:
        T = S.frames(P)
        assert T == nblk - 3
        frames, seen, nwaves = _pipeline_frames(nblk, T, seed=mult)
        ntiles = -(-nblk // 4)
        assert {-(-(ntiles - w) // nwaves) for w in (0, nwaves - 1)} == cnts and seen <= cnts
        o = _run(ctx, S, P, [[0, T]])
        every = np.arange(T)
        ratios = _check(f"pipeline {nblk} blocks", S, P, o, frames, noise_like=True, oracle=_oracle(S, P, T),
                        all_frames=every)
        # bar 5 on every frame: a second call, a fresh context, a many-range list of adjacent ranges
        assert _run(ctx, S, P, [[0, T]]).same(o, every)
        other = _lib.Context(ctx.device)
        try:
            assert _run(other, S, P, [[0, T]]).same(o, every)
        finally:
            other.close()
        cuts = list(range(0, T, 97)) + [T]
        assert _run(ctx, S, P, [[a, b] for a, b in zip(cuts[:-1], cuts[1:])]).same(o, every)
        for t in frames[:: max(1, len(frames) // 6)]:
            assert _run(ctx, S, P, [[t, t + 1]]).same(o, [t]), t
        _note(f"pipeline {mult} W + {extra} blocks (tiles per wave {sorted(cnts)})", ratios)
    finally:
        S.free()


@pytest.mark.parametrize("nblk", [1, 2, 3, 4, 5, 7])
def test_pipeline_partial_tiles(ctx, nblk):
    """N 1024 / hop 1024 (one block is one frame): a partial only tile, a full one, a partial last tile"""
    P = X.Plan(1024, 1024, FS, (100, 101), (-200, -198))
    assert P.nk == 9
    S = Samples(ctx, _noise16(nblk * 1024, seed=nblk))
    try:
        T = S.frames(P)
        assert T == nblk
        o = _run(ctx, S, P, [[0, T]])
        ratios = _check(f"partial tiles {nblk}", S, P, o, range(T))  # too few frames for an rms (bar 3)
        for t in range(T):
            assert _run(ctx, S, P, [[t, t + 1]]).same(o, [t])
        _note(f"partial tiles: {nblk} blocks", ratios)
    finally:
        S.free()


def test_pipeline_idle_waves(ctx):
    """W - 3 blocks: fewer tiles than waves"""
    nblk = 4 * _cus() - 3
    P = X.Plan(4096, 1024, FS, C5_BAND, C5_NOISE)
    S = Samples(ctx, _noise16(nblk * 1024, seed=9))
    try:
        T = S.frames(P)
        o = _run(ctx, S, P, [[0, T]])
        ratios = _check("idle waves", S, P, o, _pick(T, 48, 9), noise_like=True)
        assert _run(ctx, S, P, [[0, T]]).same(o, np.arange(T))
        _note(f"idle waves: {nblk} blocks", ratios)
    finally:
        S.free()


# ----------------------------------------------------------------------------- geometry and bins
def _bands_for(N):
    return (N // 8, N // 8 + 1), (-(N // 4), -(N // 4) + 2)


GEOMETRY = [(1024, 1024), (2048, 1024), (3072, 1024), (4096, 1024), (5120, 1024), (8192, 1024), (4096, 2048),
            (4096, 3072), (4096, 5120)]


@pytest.mark.parametrize("N,hop", GEOMETRY, ids=[f"N{n}-hop{h}" for n, h in GEOMETRY])
def test_geometry(ctx, N, hop):
    """R = 1, 2, 3, 4, 5 and 8 blocks per frame on the int8 path (frame_kernel's runtime R beside the
    compiled R = 4), hop 3072, hop 5120 > N (blocks between the frames computed and unread) -- and hop
    2048, whose blocks are gcd(4096, 2048) = 2048 samples: that geometry takes the Goertzel rows and is
    held to bars 1, 4 and 5 with their chain.  n_samples is no multiple of the block."""
    band, noise = _bands_for(N)
    P = X.Plan(N, hop, FS, band, noise)
    assert P.nk == 9 and P.i8() == (hop != 2048) and P.R == N // math.gcd(N, hop)
    T0 = 23
    S = Samples(ctx, _noise16((T0 - 1) * hop + N + 517, seed=N + hop))
    try:
        T = S.frames(P)
        assert T == T0 and S.n % P.D
        o = _run(ctx, S, P, [[0, T]])
        ratios = _check(f"geometry N {N} hop {hop}", S, P, o, range(T), noise_like=True)
        cuts = [0, 1, 2, 7, 8, 16, T]
        assert _run(ctx, S, P, [[a, b] for a, b in zip(cuts[:-1], cuts[1:])]).same(o, np.arange(T))
        assert _run(ctx, S, P, [[5, 6]]).same(o, [5])
        _note(f"geometry N {N} hop {hop} R {P.R} D {P.D} path {'int8' if P.i8() else 'goertzel rows'}", ratios)
    finally:
        S.free()


# (band, noise) -> needed bins; N 4096 / hop 1024
BINS = [
    ((500, 500), (0, -1), 3),            # one band bin, an empty noise band
    ((0, -1), (-500, -500), 3),          # the reverse
    ((2046, 2047), (0, -1), 4),          # N/2 - 2 .. N/2 - 1: the neighbour wraps to -N/2
    ((2, 2), (4, 4), 5),                 # bin 2, whose neighbour is bin 1; band and noise share bin 3
    ((-2048, -2047), (-2045, -2045), 6), # -N/2 .. -N/2 + 1 (the neighbour N/2 - 1); a shared neighbour
    ((100, 102), (101, 104), 7),         # band and noise overlapping
    ((21, 22), (-65, -64), 8),           # the last layout without the digit-lane tile (no sums)
    ((21, 22), (-65, -63), 9),           # C5
    ((100, 102), (-300, -298), 10),      # both digit-lane tiles
    ((21, 24), (-65, -63), 11),          # too many bins: the Goertzel rows
    ((1, 1), (-65, -63), 8),             # needs bin 0: the Goertzel rows
]


@pytest.mark.parametrize("band,noise,nk", BINS, ids=[f"nk{c[2]}-b{c[0][0]}_{c[0][1]}-n{c[1][0]}_{c[1][1]}" for c in BINS])
def test_bin_layouts(ctx, band, noise, nk):
    """3 .. 10 needed bins, each once (NT 6, 7, 8), the wraps at +-N/2, shared and overlapping bins; 11
    bins and a band at bin 1 report the Goertzel rows and are held to bars 1, 4 and 5 with that chain"""
    P = X.Plan(4096, 1024, FS, band, noise)
    assert P.nk == nk
    i8 = nk <= 10 and band != (1, 1)
    assert P.i8() == i8
    want = _lib.REFINE_INT8_MFMA if i8 else _lib.REFINE_GOERTZEL_ROWS
    assert _lib.iq_delta64_path(4096, 1024, FS, band, noise, CI16) == want
    S = Samples(ctx, _noise16(22 * 1024 + 4096, seed=nk))
    try:
        T = S.frames(P)
        o = _run(ctx, S, P, [[0, T]])
        ratios = _check(f"bins {band} {noise}", S, P, o, range(T), noise_like=True)
        assert _run(ctx, S, P, [[3, 4]]).same(o, [3])
        _note(f"bins band {band} noise {noise}: {nk} needed, path {'int8' if i8 else 'goertzel rows'}", ratios)
    finally:
        S.free()


# ----------------------------------------------------------------------------- ranges
def test_ranges_compact_map(ctx):
    """64 two-frame ranges at hop 1024 (5 blocks each: every tile straddles two ranges), the first
    starting past 0; adjacent ranges (their shared blocks twice in the compact table) ending at the last
    frame the samples allow; no range at all"""
    P = X.Plan(4096, 1024, FS, C5_BAND, C5_NOISE)
    S = Samples(ctx, _noise16(400 * 1024 + 4096 + 100, seed=31))
    try:
        T = S.frames(P)
        assert T == 401
        whole = _run(ctx, S, P, [[0, T]])
        two = [[6 * i + 1, 6 * i + 3] for i in range(64)]
        o = _run(ctx, S, P, two)
        fr = [t for a, b in two for t in range(a, b)]
        assert o.same(whole, fr)
        ratios = _check("64 two-frame ranges", S, P, o, fr[::5] + fr[-2:], noise_like=True)
        adj = [[T - 40, T - 33], [T - 33, T - 32], [T - 32, T - 20], [T - 20, T]]
        oa = _run(ctx, S, P, adj)
        assert oa.same(whole, range(T - 40, T))
        _check("adjacent ranges", S, P, oa, range(T - 40, T, 3), noise_like=True)
        none = _launch(ctx, S, P, np.zeros((0, 2), np.int64), sums=True)
        assert none.rc == _lib.MSD_OK
        for k in PAY:
            assert (getattr(none, k) == PAY[k]).all()
        _note("ranges: 64 two-frame ranges, 4 adjacent ranges to the last frame, none", ratios)
    finally:
        S.free()


def test_ranges_one_frame_each(ctx):
    """200 one-frame ranges at N 1024 (one block each): every tile spans four ranges"""
    P = X.Plan(1024, 1024, FS, (100, 101), (-200, -198))
    S = Samples(ctx, _noise16(640 * 1024, seed=32))
    try:
        T = S.frames(P)
        whole = _run(ctx, S, P, [[0, T]])
        one = [[3 * i + 2, 3 * i + 3] for i in range(200)]
        o = _run(ctx, S, P, one)
        fr = [a for a, _ in one]
        assert o.same(whole, fr)
        ratios = _check("200 one-frame ranges", S, P, o, fr[::4], noise_like=True)
        _note("ranges: 200 one-frame ranges at N 1024", ratios)
    finally:
        S.free()


# ----------------------------------------------------------------------------- inputs
INPUT_BANDS = [(C5_BAND, (0, -1)), ((0, -1), C5_NOISE), (C5_BAND, C5_NOISE)]


@pytest.mark.parametrize("band,noise", INPUT_BANDS, ids=["noise_empty", "band_empty", "c5"])
def test_input_classes(ctx, band, noise):
    """every input class of refine_exact.signals (noise, +- full scale, |x| <= 3, the sample split's edge
    constants, unit impulses at the sub-block and block edges, tones on and beside a band bin, a weak
    tone beside a carrier, the digit-sign patterns that drive an accumulator to its extreme) in one stream, 8
    blocks each (32 for the noise-like ones, which bar 3 takes an rms over): each stretch's own 5 (29) frames
    and the 3 mixed frames into the next class alike.  With an empty band E_gpu is recovered and held per band (bar 2)."""
    P = X.Plan(4096, 1024, FS, band, noise)
    sig, long = X.signals(P, 5, seed=7), X.signals(P, 29, seed=8)  # 8 blocks each; 32 for the noise-like ones
    parts, at = [], 0
    for k in sig:
        x = long[k] if k in X.NOISE_LIKE else sig[k]
        parts.append((k, at, x.size // 2048, x))
        at += x.size // 2048
    S = Samples(ctx, np.concatenate([p[3] for p in parts]))
    try:
        T = S.frames(P)
        assert T == at - 3
        o = _run(ctx, S, P, [[0, T]])
        worst = {}
        for name, m0, nb, _ in parts:
            own_frames = list(range(m0, m0 + nb - 3))
            mixed = [t for t in range(m0 + nb - 3, m0 + nb) if t < T]
            r = _check(f"{name}", S, P, o, own_frames, noise_like=name in X.NOISE_LIKE)
            r2 = _check(f"{name} into the next class", S, P, o, mixed) if mixed else {}
            for k, v in list(r.items()) + list(r2.items()):
                if k != "ed_restated_on" and v >= worst.get(k, (0.0, ""))[0]:
                    worst[k] = (v, name)
        assert _run(ctx, S, P, [[0, T]]).same(o, np.arange(T))
        _note(f"inputs band {band} noise {noise} ({len(parts)} classes)",
              {f"{k} ({n})": v for k, (v, n) in worst.items()})
    finally:
        S.free()


# ----------------------------------------------------------------------------- the other paths
OTHER = [("int16-goertzel-option", 4096, 1024, False, True), ("f32-D1024", 4096, 1024, True, False),
         ("f32-D512", 4096, 512, True, False), ("f32-D64", 4096, 64, True, False),
         ("int16-direct", 1000, 500, False, False), ("f32-direct", 1000, 500, True, False)]


@pytest.mark.parametrize("name,N,hop,f32,goertzel", OTHER, ids=[c[0] for c in OTHER])
def test_other_paths(ctx, name, N, hop, f32, goertzel):
    """the same harness on the float64 Goertzel rows (int16 under MSD_OPT_REFINE_GOERTZEL; float32 at D
    1024, 512 and 64) and the direct step (N 1000 / hop 500): bars 1, 4 and 5 with each path's chain, with
    both bands and with an empty noise band (E_gpu recovered: ed restated on every frame)"""
    band, noise = ((21, 22), (-65, -63)) if N == 4096 else ((10, 12), (-9, -8))
    T0 = 21
    S = Samples(ctx, _noise16((T0 - 1) * hop + N + 3, seed=hop), f32=f32)
    try:
        if goertzel:
            ctx.set_option(_lib.OPT_REFINE_GOERTZEL, 1)
        for nz in (noise, (0, -1)):
            P = X.Plan(N, hop, FS, band, nz)
            path = _lib.iq_delta64_path(N, hop, FS, band, nz, S.code)
            assert path == (_lib.REFINE_DIRECT if N == 1000 else
                            _lib.REFINE_INT8_MFMA if not f32 else _lib.REFINE_GOERTZEL_ROWS)
            T = S.frames(P)
            assert T == T0
            o = _run(ctx, S, P, [[0, T]], goertzel=goertzel)
            ratios = _check(name, S, P, o, range(T), goertzel=goertzel)
            assert _run(ctx, S, P, [[0, T]], goertzel=goertzel).same(o, np.arange(T))
            assert _run(ctx, S, P, [[0, 2], [2, 9], [11, 12], [12, T]], goertzel=goertzel).same(
                o, [t for t in range(T) if t not in (9, 10)])
            assert _run(ctx, S, P, [[7, 8]], goertzel=goertzel).same(o, [7])
            _note(f"other paths: {name} noise {nz}", ratios)
    finally:
        ctx.set_option(_lib.OPT_REFINE_GOERTZEL, 0)
        S.free()


# ----------------------------------------------------------------------------- one context, many geometries
def test_context_that_ran_other_geometries(ctx):
    """NT 6 -> the same bins shifted by a multiple of R (the per-call rotation table and the ranges
    byte-identical: msd_iq_delta64_sums_dev skips their upload) -> NT 8 -> the Goertzel rows (option set,
    then cleared) -> NT 6 again, on one context with the same ranges: each call bit-equal to the same
    call on a fresh context"""
    steps = [((21, 22), (0, -1), False), ((25, 26), (0, -1), False), ((100, 102), (-300, -298), False),
             ((21, 22), (0, -1), True), ((21, 22), (0, -1), False), ((25, 26), (0, -1), False),
             (C5_BAND, C5_NOISE, False)]
    ranges = [[1, 9], [12, 30]]
    S = Samples(ctx, _noise16(40 * 1024, seed=41))
    seq = _lib.Context(ctx.device)
    try:
        fr = [t for a, b in ranges for t in range(a, b)]
        for i, (band, noise, goertzel) in enumerate(steps):
            P = X.Plan(4096, 1024, FS, band, noise)
            assert P.i8()
            outs = []
            for c in (seq, None):
                fresh = _lib.Context(ctx.device) if c is None else None
                cc = fresh or c
                try:
                    cc.set_option(_lib.OPT_REFINE_GOERTZEL, int(goertzel))
                    outs.append(_run(cc, S, P, ranges, goertzel=goertzel))
                finally:
                    cc.set_option(_lib.OPT_REFINE_GOERTZEL, 0)
                    if fresh:
                        fresh.close()
            assert outs[0].same(outs[1], fr), (i, band, noise, goertzel)
            _check(f"sequence step {i}", S, P, outs[0], fr[::3], goertzel=goertzel)
    finally:
        seq.close()
        S.free()
