"""GPU: the decimating down-converter (include/msdsp.h, msd_ddc_*) against its contract.

Bars, on every output of every case (u = 2^-53, S_m = sum_k |h_k| |x_{m D + c - k}|, chain = msd_ddc_chain, the
count of csrc/ddc_plan.h):
    |y_gpu - y_longdouble| <= chain u gain S_m
    |y_gpu - y_float64|    <= (chain + ntaps + 6) u gain S_m
zero input gives exactly zero; int16 output equals rint of the long-double value (the inputs are chosen, from
the reference alone, so that no value lies within the bound of a half-integer); pushes of any lengths
followed by flush, halo rows, reset streams and streams pushed together equal the batch row bit for bit.
The largest ratio of each case is printed (and appended to the file DDC_RATIO_FILE names, if set)."""
import os

import numpy as np
import pytest

import ddc_ref as R
from meteorgpu import _lib, ddc
from meteorgpu.dsp import context

pytestmark = pytest.mark.gpu

U = R.U
SHAPES = [(1, 1), (2, 3), (12, 5), (12, 97), (48, 385), (1024, 4095), (3, 4095)]
QS = [(0, 1), (1, 4), (3, 7), (5, 32), (12345, 192000), (1234567, (1 << 24) - 3)]
POS = [0, 1, None, (1 << 40) + 3, 1 << 62]  # None: D - 1


def _tile(D, ntaps):
    """outputs per tile, as csrc/ddc_plan.h chooses them (tests/test_ddc_abi.py holds the chain to this)"""
    def tile_bytes(tm):
        Uu = (-(-(tm * D + ntaps - 1) // D)) | 1
        return 8 * (2 * ((D * Uu + 1) & ~1) + 256)
    return next((tm for tm in (256, 128, 64, 32, 16, 8, 4, 2, 1) if tile_bytes(tm) <= 64 * 1024), None) \
        or next(tm for tm in (256, 128, 64, 32, 16, 8, 4, 2, 1) if tile_bytes(tm) <= 150 * 1024)


def _taps(D, ntaps, seed=0):
    if ntaps == 1:
        return np.array([0.75])
    if ntaps < 8 * D // 2:  # a filter much shorter than the decimation: random taps of both signs
        return np.random.default_rng(seed + ntaps).uniform(-1, 1, ntaps)
    return ddc.design_lowpass(ntaps, min(0.9 / D, 0.9))


def _cfg(ssb, D, ntaps, p=0, q=1, gain=1.0, out=np.float64):
    return _lib.MsdDdcCfg(_lib.DDC_SSB if ssb else _lib.DDC_REAL, D, ntaps,
                          _lib.MSD_I16 if np.dtype(out) == np.int16 else _lib.MSD_F64, p, q, gain)


def _noise(ssb, N, seed, f32=False):
    """(the array the library takes, its dtype code, the exact values for the references)"""
    rng = np.random.default_rng(seed)
    w = 2 if ssb else 1
    if f32:
        raw = (rng.standard_normal(w * N) * 8000).astype(np.float32)
        code = _lib.MSD_CF32 if ssb else _lib.MSD_F32
    else:
        raw = rng.integers(-32768, 32768, w * N).astype(np.int16)
        code = _lib.MSD_CI16 if ssb else _lib.MSD_I16
    val = raw.astype(np.float64)
    return raw, code, (val[0::2] + 1j * val[1::2]) if ssb else val


def _pack(val, ssb, f32=False):
    """exact integer (or float32) values back into the library's array"""
    dt = np.float32 if f32 else np.int16
    if not ssb:
        return np.asarray(val.real if np.iscomplexobj(val) else val).astype(dt)
    out = np.empty(2 * len(val), dt)
    out[0::2], out[1::2] = val.real, val.imag
    return out


def _note(case, ratio):
    line = f"{case}: largest |y - y_longdouble| / (chain u gain S_m) = {ratio:.4f}"
    print(line)
    path = os.environ.get("DDC_RATIO_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check(y, val, taps, cfg, pos0=0):
    """the two bars on every output; returns the largest ratio to the first"""
    ssb = cfg.mode == _lib.DDC_SSB
    D, ntaps, gain = int(cfg.decim), int(cfg.ntaps), float(cfg.gain)
    p, q = int(cfg.shift_num), int(cfg.shift_den)
    ld = R.ref_ld(val, taps, D, ssb, p, q, gain, pos0)
    f64 = R.ref_f64(val, taps, D, ssb, p, q, gain, pos0)
    S = R.abs_sum(val, taps, D, pos0)
    assert y.shape == ld.shape, (y.shape, ld.shape)
    if not len(y):
        return 0.0
    chain = _lib.ddc_chain(cfg)
    bar = chain * U * abs(gain) * S
    e1 = np.abs(y.astype(R.LD) - ld).astype(np.float64)
    e2 = np.abs(y - f64)
    assert np.all(e1 <= bar), (np.max(e1 / np.maximum(bar, 1e-300)), int(np.argmax(e1 - bar)))
    assert np.all(e2 <= (chain + ntaps + 6) * U * abs(gain) * S)
    assert np.all(y[S == 0] == 0)
    nz = bar > 0
    return float(np.max(e1[nz] / bar[nz])) if nz.any() else 0.0


@pytest.fixture(scope="module")
def ctx():
    return context(0)


@pytest.mark.parametrize("D,ntaps", SHAPES)
def test_shapes_lengths_positions(ctx, D, ntaps):
    """every N at which a path changes, every position class, every q class, REAL and SSB"""
    c, TM = (ntaps - 1) // 2, _tile(D, ntaps)
    taps = _taps(D, ntaps)
    Ns = sorted({0, 1, c, c + 1, max(D - 1, 0), D, D + 1, (TM - 1) * D, TM * D, (TM + 1) * D, (2 * TM + 1) * D})
    worst = 0.0
    real = _lib.DdcPlan(ctx, _cfg(False, D, ntaps, gain=1.5), taps, 0, 0)
    ssbs = [_lib.DdcPlan(ctx, _cfg(True, D, ntaps, p, q, gain=1.5), taps, 0, 0) for p, q in QS]
    k = 0
    for N in Ns:
        positions = POS if N == (TM + 1) * D else [POS[k % len(POS)]]
        for pos in positions:
            pos0 = D - 1 if pos is None else pos
            raw, code, val = _noise(False, N, 100 + k)
            worst = max(worst, _check(real.run(raw, code, N, pos0), val, taps, real.cfg, pos0))
            plan = ssbs[k % len(ssbs)]
            raw, code, val = _noise(True, N, 200 + k)
            worst = max(worst, _check(plan.run(raw, code, N, pos0), val, taps, plan.cfg, pos0))
            k += 1
    # every q at the two-tile length and the far position
    N, pos0 = (2 * TM + 1) * D, (1 << 40) + 3
    raw, code, val = _noise(True, N, 7)
    for plan in ssbs:
        worst = max(worst, _check(plan.run(raw, code, N, pos0), val, taps, plan.cfg, pos0))
    _note(f"shapes D {D} ntaps {ntaps}", worst)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ssb", [False, True])
def test_input_dtypes(ctx, ssb, f32):
    D, ntaps = (48, 385) if ssb else (12, 97)
    taps = _taps(D, ntaps)
    cfg = _cfg(ssb, D, ntaps, 5 if ssb else 0, 32 if ssb else 1, gain=0.5)
    plan = _lib.DdcPlan(ctx, cfg, taps, 0, 0)
    N = 40 * D + 17
    raw, code, val = _noise(ssb, N, 5, f32)
    _note(f"dtype code {code}", _check(plan.run(raw, code, N, 3), val, taps, cfg, 3))
    # a dtype that does not fit the mode is refused
    wrong = _lib.MSD_I16 if ssb else _lib.MSD_CI16
    with pytest.raises(_lib.MsdError) as e:
        plan.run(raw, wrong, 4, 0)
    assert e.value.code == _lib.MSD_ERR_INVALID and "msd_ddc_run" in e.value.msg


def test_special_inputs(ctx):
    """zeros, a constant, impulses at 0, c and N - 1, the accumulator's extreme, carriers on and off tune"""
    D, ntaps, p, q = 48, 385, 5, 32
    c = (ntaps - 1) // 2
    taps = _taps(D, ntaps)
    N = 30 * D + 5
    for ssb in (False, True):
        cfg = _cfg(ssb, D, ntaps, p if ssb else 0, q if ssb else 1, gain=2.0)
        plan = _lib.DdcPlan(ctx, cfg, taps, 0, 0)
        code = _lib.MSD_CI16 if ssb else _lib.MSD_I16
        y = plan.run(_pack(np.zeros(N), ssb), code, N, 0)
        assert y.shape == (-(-N // D),) and np.all(y == 0)
        worst = 0.0
        const = np.full(N, 12345.0) + (1j * -321.0 if ssb else 0)
        worst = max(worst, _check(plan.run(_pack(const, ssb), code, N, 0), const, taps, cfg, 0))
        for at in (0, c, N - 1):
            imp = np.zeros(N, np.complex128 if ssb else np.float64)
            imp[at] = 32767.0 - (32768.0j if ssb else 0)
            worst = max(worst, _check(plan.run(_pack(imp, ssb), code, N, 0), imp, taps, cfg, 0))
        # +- full scale following the sign of h around output m*: every product of that output has one sign
        ms = 12
        ext = np.zeros(N)
        n = ms * D + c - np.arange(ntaps)
        ext[n] = np.where(taps >= 0, 32767.0, -32768.0)
        if ssb:  # the mixed sample, not the raw one, must follow h: only REAL reaches the extreme exactly
            ext = ext + 1j * ext[::-1]
        worst = max(worst, _check(plan.run(_pack(ext, ssb), code, N, 0), ext, taps, cfg, 0))
        _note(f"special inputs ssb {ssb}", worst)
    # a carrier on the tuned frequency comes out as the 1 kHz tone; 1.5 kHz off it is in the transition band
    cfg, taps = ddc.weaver(192000, 30000, gain=1.0)
    plan = _lib.DdcPlan(ctx, cfg, taps, 0, 0)
    t = np.arange(192000 // 2)
    rms = []
    for f in (30000.0, 28500.0):
        z = np.round(1000 * np.exp(2j * np.pi * f * t / 192000))
        z = np.round(z.real) + 1j * np.round(z.imag)
        y = plan.run(_pack(z, True), _lib.MSD_CI16, len(t), 0)
        _check(y, z, taps, cfg, 0)
        rms.append(np.sqrt(np.mean(y[50:-50] ** 2)))
    tone = plan.run(_pack(np.round(1000 * np.exp(2j * np.pi * 30000.0 * t / 192000)), True), _lib.MSD_CI16, len(t), 0)
    spec = np.abs(np.fft.rfft(tone[48:48 + 1600] * np.hanning(1600)))
    assert np.argmax(spec) * 4000 / 1600 == 1000.0
    assert 650 < rms[0] < 760 and rms[1] < 0.1 * rms[0]


def test_int16_output_and_saturation(ctx):
    D, ntaps = 12, 97
    taps = _taps(D, ntaps)
    N = 60 * D + 1
    for ssb, p, q in ((False, 0, 1), (True, 5, 32)):
        cfg = _cfg(ssb, D, ntaps, p, q, gain=0.9, out=np.int16)
        chain = _lib.ddc_chain(cfg)
        for seed in range(40):  # the first seed whose reference has no output near a half-integer
            raw, code, val = _noise(ssb, N, 1000 + seed)
            ld = R.ref_ld(val, taps, D, ssb, p, q, 0.9, 0)
            bar = chain * U * 0.9 * R.abs_sum(val, taps, D, 0)
            frac = np.abs((ld - np.floor(ld)).astype(np.float64) - 0.5)
            if np.all(frac > bar) and np.all(np.abs(ld) < 32767):
                break
        else:
            raise AssertionError("no seed without a near-half-integer output")
        y = _lib.DdcPlan(ctx, cfg, taps, 0, 0).run(raw, code, N, 0)
        assert y.dtype == np.int16
        assert np.array_equal(y, np.rint(ld).astype(np.int64))
    # saturation at +- full scale with gain 4: a constant through a unit-gain low-pass
    lp = ddc.design_lowpass(ntaps, 0.05)
    plan = _lib.DdcPlan(ctx, _cfg(False, D, ntaps, gain=4.0, out=np.int16), lp, 0, 0)
    for v, want in ((32767, 32767), (-32768, -32768)):
        y = plan.run(np.full(N, v, np.int16), _lib.MSD_I16, N, 0)
        assert np.all(y[10:-10] == want) and y.min() >= -32768 and y.max() <= 32767
    # ties go to even: an impulse through taps of exact halves
    plan = _lib.DdcPlan(ctx, _cfg(False, 1, 1, gain=0.5, out=np.int16), np.array([1.0]), 0, 0)
    x = np.array([1, 3, 5, -1, -3, 2, 0, 32767, -32768], np.int16)
    assert plan.run(x, _lib.MSD_I16, len(x), 0).tolist() == [0, 2, 2, 0, -2, 1, 0, 16384, -16384]


def _dev(ctx, a):
    b = ctx.alloc(max(a.nbytes, 16))
    if a.nbytes:
        b.upload(a)
    return b


def test_ragged_batch_padding_and_many_tiles(ctx):
    """rows of one buffer side by side (a neighbour's samples, one past a row, contribute nothing), an empty
    row, ld_out larger than needed (the padding keeps its sentinel), more tiles than the grid has slots"""
    D, ntaps = 2, 3
    taps = _taps(D, ntaps)
    lens = [200001, 0, 199999, 1, 200000, 123457, 200003, 7]
    pos = [0, 5, 1, (1 << 40) + 3, 1 << 62, 3, 2, 9]
    for ssb, p, q in ((False, 0, 1), (True, 12345, 192000)):
        cfg = _cfg(ssb, D, ntaps, p, q, gain=1.25)
        plan = _lib.DdcPlan(ctx, cfg, taps, 0, 0)
        raw, code, val = _noise(ssb, sum(lens), 77)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        counts = [_lib.ddc_out_len(cfg, p0, n)[1] for p0, n in zip(pos, lens)]
        ld = max(counts) + 37
        y = np.full((len(lens), ld), -7.5)
        dy, dn = _dev(ctx, y), ctx.alloc(8 * len(lens))
        plan.run_dev(_dev(ctx, raw), code, _dev(ctx, off), _dev(ctx, np.array(lens, np.int64)),
                     _dev(ctx, np.array(pos, np.int64)), len(lens), dy, ld, dn)
        got_n = np.empty(len(lens), np.int64)
        dn.download(got_n)
        dy.download(y)
        assert got_n.tolist() == counts
        worst = 0.0
        for r, (o, n, p0) in enumerate(zip(off, lens, pos)):
            assert np.all(y[r, counts[r]:] == -7.5), r
            worst = max(worst, _check(y[r, : counts[r]], val[o: o + n], taps, cfg, p0))
        _note(f"ragged batch of {sum(counts)} outputs ssb {ssb}", worst)


def _chunks(N, D, ntaps, big):
    sizes = [0, 1, D - 1, ntaps - 2, 1, big, 0, 2, ntaps - 2, D + 1]
    out, at = [], 0
    for s in sizes:
        s = min(max(s, 0), N - at)
        out.append((at, at + s))
        at += s
    out.append((at, N))
    return out


@pytest.mark.parametrize("ssb,D,ntaps,p,q,out", [
    (True, 48, 385, 5, 32, np.float64), (True, 48, 385, 12345, 192000, np.int16), (False, 12, 97, 0, 1, np.float64),
    (False, 1024, 4095, 0, 1, np.float64), (True, 1, 1, 3, 7, np.float64)])
def test_pushes_then_flush_equal_run(ctx, ssb, D, ntaps, p, q, out):
    """chunks of 0, 1, D - 1 and ntaps - 2 samples (shorter than the history, which then spans several
    pushes), 30 s worth at once, then flush: bit for bit the batch row; from position 0 and after reset"""
    taps = _taps(D, ntaps)
    cfg = _cfg(ssb, D, ntaps, p, q, gain=0.8, out=out)
    big = {48: 30 * 192000, 1024: 180000}.get(D, 30 * 48000)  # 30 s of the rate the shape is meant for
    N = big + 3 * D + 2 * ntaps + 20
    w = 2 if ssb else 1
    raw, code, _ = _noise(ssb, N, 31)
    plan = _lib.DdcPlan(ctx, cfg, taps, 2, N)
    for pos0, stream in ((0, 0), ((1 << 40) + 3, 1), (D + 1, 0)):
        whole = plan.run(raw, code, N, pos0)
        if pos0:  # (a new plan's streams start at 0)
            plan.reset(stream, pos0)
        parts = [plan.push(stream, raw[w * a: w * b], code, b - a) for a, b in _chunks(N, D, ntaps, big)]
        parts.append(plan.flush(stream))
        got = np.concatenate(parts)
        assert got.dtype == whole.dtype and np.array_equal(got, whole), (pos0, len(got), len(whole))
        with pytest.raises(_lib.MsdError):  # a flushed stream must be reset first
            plan.push(stream, raw[: w], code, 1)
    # a row with c samples of halo on each side equals the whole on its interior
    c = (ntaps - 1) // 2
    whole = plan.run(raw, code, N, 0)
    a, b = 5 * D + 3 + c, min(N - c, 5 * D + 3 + c + 700 * D + 1)
    part = plan.run(raw[w * (a - c): w * (b + c)], code, b + c - (a - c), a - c)
    m_first = -(-(a - c) // D)
    lo, hi = -(-a // D), -(-b // D)
    assert hi > lo and np.array_equal(part[lo - m_first: hi - m_first], whole[lo:hi])


def test_two_streams_pushed_together_equal_each_alone(ctx):
    D, ntaps, p, q = 12, 97, 5, 32
    taps = _taps(D, ntaps)
    cfg = _cfg(True, D, ntaps, p, q)
    max_push = 5000
    plan = _lib.DdcPlan(ctx, cfg, taps, 2, max_push)
    rawA, code, _ = _noise(True, 9000, 1)
    rawB, _, _ = _noise(True, 7001, 2)
    alone = [plan.run(rawA, code, 9000, 0), plan.run(rawB, code, 7001, 0)]
    ld = -(-max_push // D) + 5
    cuts = [(0, 0), (4000, 17), (4001, 3000), (9000, 7001)]  # (samples of A, of B) pushed so far
    got = [[], []]
    dy, dn = ctx.alloc(2 * ld * 8), ctx.alloc(16)
    for (a0, b0), (a1, b1) in zip(cuts[:-1], cuts[1:]):
        x = np.concatenate([rawA[2 * a0: 2 * a1], rawB[2 * b0: 2 * b1]])
        lens = np.array([a1 - a0, b1 - b0], np.int64)
        y = np.full((2, ld), np.nan)
        dy.upload(y)
        plan.push_dev(_dev(ctx, x), code, _dev(ctx, np.array([0, a1 - a0], np.int64)), _dev(ctx, lens), dy, ld, dn)
        n = np.empty(2, np.int64)
        dn.download(n)
        dy.download(y)
        for s in range(2):
            assert np.all(np.isnan(y[s, n[s]:]))
            got[s].append(y[s, : n[s]].copy())
    for s in range(2):
        got[s].append(plan.flush(s))
        assert np.array_equal(np.concatenate(got[s]), alone[s]), s


def test_timing_id(ctx):
    D, ntaps = 12, 97
    plan = _lib.DdcPlan(ctx, _cfg(False, D, ntaps), _taps(D, ntaps), 0, 0)
    raw, code, _ = _noise(False, 5000, 1)
    ctx.timing(True)
    try:
        ctx.timing_reset()
        plan.run(raw, code, 5000, 0)
        ms, n = ctx.timing_get(_lib.K_DDC)
        assert n == 1 and ms > 0
    finally:
        ctx.timing(False)
