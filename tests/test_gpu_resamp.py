"""GPU: the rational-ratio resampler (include/msdsp.h, msd_resamp_*) against its contract.

Bars, on every output of every case (u = 2^-53, S_m = sum_i |h[phi + i L]| |x[n0 - i]|, chain = msd_resamp_chain,
the count of csrc/resamp_plan.h, I = ceil(ntaps / L)):
    |y_gpu - y_longdouble| <= chain u |gain| S_m
    |y_gpu - y_float64|    <= (chain + I + 6) u |gain| S_m
zero input and a branch without a tap give exactly zero; int16 output equals rint of the long-double value
(the inputs are chosen, from the reference alone, so that no value lies within the bound of a half-integer);
pushes of any lengths followed by flush, halo rows, reset streams and streams pushed together equal the
batch row bit for bit.  The largest ratio of each case is printed (and appended to the file
RESAMP_RATIO_FILE names, if set)."""
import os

import numpy as np
import pytest

import resamp_ref as R
from meteorgpu import _lib, ddc
from meteorgpu.dsp import context

pytestmark = pytest.mark.gpu

U = R.U
SHAPES = [(1, 1, 1), (2, 3, 1), (2, 3, 25), (3, 2, 25), (7, 5, 3), (2, 125, 1001), (40, 441, 3529), (160, 441, 4095),
          (256, 1, 4095), (255, 1024, 4095), (1, 12, 97)]
QS = [(0, 1), (1, 4), (3, 7), (5, 32), (12345, 192000), (1234567, (1 << 24) - 3)]  # test_gpu_ddc.py's classes
POS = [0, 1, "M-1", (1 << 40) + 3, "limit"]


def _taps(L, M, ntaps, seed=0):
    if ntaps == 1:
        return np.array([0.75])
    if ntaps < 4 * max(L, M):  # a filter much shorter than the ratio's period: random taps of both signs
        return np.random.default_rng(seed + ntaps).uniform(-1, 1, ntaps)
    return L * ddc.design_lowpass(ntaps, 0.9 / max(L, M))


def _cfg(ssb, L, M, ntaps, p=0, q=1, gain=1.0, out=np.float64):
    return _lib.MsdResampCfg(_lib.DDC_SSB if ssb else _lib.DDC_REAL, L, M, ntaps,
                             _lib.MSD_I16 if np.dtype(out) == np.int16 else _lib.MSD_F64, 0, p, q, gain)


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
    path = os.environ.get("RESAMP_RATIO_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _params(cfg):
    return (int(cfg.up), int(cfg.down), cfg.mode == _lib.DDC_SSB, int(cfg.shift_num), int(cfg.shift_den), float(cfg.gain))


def _check(y, val, taps, cfg, pos0=0):
    """the two bars on every output; returns the largest ratio to the first"""
    L, M, ssb, p, q, gain = _params(cfg)
    ld = R.ref_ld(val, taps, L, M, ssb, p, q, gain, pos0)
    f64 = R.ref_f64(val, taps, L, M, ssb, p, q, gain, pos0)
    S = R.abs_sum(val, taps, L, M, pos0)
    assert y.shape == ld.shape, (y.shape, ld.shape)
    if not len(y):
        return 0.0
    chain = _lib.resamp_chain(cfg)
    bar = chain * U * abs(gain) * S
    e1 = np.abs(y.astype(R.LD) - ld).astype(np.float64)
    e2 = np.abs(y - f64)
    assert np.all(e1 <= bar), (np.max(e1 / np.maximum(bar, 1e-300)), int(np.argmax(e1 - bar)))
    assert np.all(e2 <= (chain + -(-int(cfg.ntaps) // L) + 6) * U * abs(gain) * S)
    assert np.all(y[S == 0] == 0)
    nz = bar > 0
    return float(np.max(e1[nz] / bar[nz])) if nz.any() else 0.0


def _n_for(pos0, k, L, M):
    """the fewest samples from pos0 on that give k outputs (k >= 1)"""
    m_lo = -(-pos0 * L // M)
    return (m_lo + k - 1) * M // L + 1 - pos0


@pytest.fixture(scope="module")
def ctx():
    return context(0)


@pytest.mark.parametrize("L,M,ntaps", SHAPES)
def test_shapes_lengths_positions(ctx, L, M, ntaps):
    """every N at which a path changes, every position class, every q class, REAL and SSB"""
    TM, G, K, I = R.plan(L, M, ntaps)
    H = I - 1
    taps = _taps(L, M, ntaps)
    real = _lib.ResampPlan(ctx, _cfg(False, L, M, ntaps, gain=1.5), taps, 0, 0)
    ssbs = [_lib.ResampPlan(ctx, _cfg(True, L, M, ntaps, p, q, gain=1.5), taps, 0, 0) for p, q in QS]
    # (kind, value): a length, or a count of outputs whose fewest samples are taken at the case's position
    lengths = [("n", 0), ("n", 1), ("k", 1), ("n", max(H - 1, 0)), ("n", H), ("n", H + 1), ("k", TM - 1), ("k", TM),
               ("k", TM + 1), ("k", 2 * TM + 1)]
    worst, k = 0.0, 0
    for kind, v in lengths:
        positions = POS if (kind, v) == ("k", TM + 1) else [POS[k % len(POS)]]
        for pos in positions:
            far = pos == "limit"
            pos0 = M - 1 if pos == "M-1" else (0 if far else pos)
            N = v if kind == "n" else _n_for(pos0, max(v, 1), L, M)
            if far:  # the last samples the contract allows: (pos0 + N) L <= 2^62
                pos0 = (1 << 62) // L - N
            elif kind == "k" and v >= 1:  # (a sample brings ceil(L / M) outputs at the most)
                assert v <= R.out_range(pos0, N, L, M)[1] < v + -(-L // M) and R.out_range(pos0, N - 1, L, M)[1] < v
            raw, code, val = _noise(False, N, 100 + k)
            worst = max(worst, _check(real.run(raw, code, N, pos0), val, taps, real.cfg, pos0))
            plan = ssbs[k % len(ssbs)]
            raw, code, val = _noise(True, N, 200 + k)
            worst = max(worst, _check(plan.run(raw, code, N, pos0), val, taps, plan.cfg, pos0))
            k += 1
    # every q at the two-tile length and the far position
    pos0 = (1 << 40) + 3
    N = _n_for(pos0, 2 * TM + 1, L, M)
    raw, code, val = _noise(True, N, 7)
    for plan in ssbs:
        worst = max(worst, _check(plan.run(raw, code, N, pos0), val, taps, plan.cfg, pos0))
    if (L, M, ntaps) == (2, 3, 1):  # the branch without a tap gives exact zeros, every second output here
        raw, code, val = _noise(False, 300, 9)
        y = real.run(raw, code, 300, 0)
        assert len(y) == 200 and np.all(y[1::2] == 0) and np.all(y[0::2] == 1.5 * 0.75 * val[0::3][:100])
    _note(f"shapes {L}/{M} ntaps {ntaps}", worst)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ssb", [False, True])
def test_input_dtypes(ctx, ssb, f32):
    L, M, ntaps = (2, 125, 1001) if ssb else (40, 441, 3529)
    taps = _taps(L, M, ntaps)
    cfg = _cfg(ssb, L, M, ntaps, 5 if ssb else 0, 32 if ssb else 1, gain=0.5)
    plan = _lib.ResampPlan(ctx, cfg, taps, 0, 0)
    N = 40 * M // L + 17
    raw, code, val = _noise(ssb, N, 5, f32)
    _note(f"dtype code {code}", _check(plan.run(raw, code, N, 3), val, taps, cfg, 3))
    # a dtype that does not fit the mode is refused
    for wrong in ((_lib.MSD_I16, _lib.MSD_F32) if ssb else (_lib.MSD_CI16, _lib.MSD_CF32)) + (_lib.MSD_F64,):
        with pytest.raises(_lib.MsdError) as e:
            plan.run(raw, wrong, 4, 0)
        assert e.value.code == _lib.MSD_ERR_INVALID and "msd_resamp_run" in e.value.msg


def test_special_inputs(ctx):
    """zeros, a constant, impulses at 0, in the middle and at N - 1, the accumulator's extreme at full scale,
    and the 6 kHz archive's 1 kHz tone"""
    for ssb, L, M, ntaps, p, q in ((False, 2, 3, 25, 0, 1), (True, 2, 3, 25, 5, 32), (False, 40, 441, 3529, 0, 1),
                                   (True, 3, 2, 25, 12345, 192000)):
        taps = _taps(L, M, ntaps)
        I = -(-ntaps // L)
        cfg = _cfg(ssb, L, M, ntaps, p, q, gain=2.0)
        plan = _lib.ResampPlan(ctx, cfg, taps, 0, 0)
        code = _lib.MSD_CI16 if ssb else _lib.MSD_I16
        N = 30 * M // L + 3 * I + 5
        y = plan.run(_pack(np.zeros(N), ssb), code, N, 0)
        assert y.shape == (-(-N * L // M),) and np.all(y == 0)
        worst = 0.0
        const = np.full(N, 12345.0) + (1j * -321.0 if ssb else 0)
        worst = max(worst, _check(plan.run(_pack(const, ssb), code, N, 0), const, taps, cfg, 0))
        for at in (0, N // 2, N - 1):
            imp = np.zeros(N, np.complex128 if ssb else np.float64)
            imp[at] = 32767.0 - (32768.0j if ssb else 0)
            worst = max(worst, _check(plan.run(_pack(imp, ssb), code, N, 0), imp, taps, cfg, 0))
        # +- full scale following the sign of the taps of output m*'s branch: every product has one sign
        ms = -(-N * L // M) // 2
        t = ms * M + (ntaps - 1) // 2
        hb = taps[t % L:: L]
        ext = np.zeros(N)
        ext[t // L - np.arange(len(hb))] = np.where(hb >= 0, 32767.0, -32768.0)
        if ssb:  # the mixed sample, not the raw one, must follow h: only REAL reaches the extreme exactly
            ext = ext + 1j * ext[::-1]
        else:
            assert R.abs_sum(ext, taps, L, M)[ms] == pytest.approx(abs(float(R.ref_ld(ext, taps, L, M)[ms])), rel=1e-12)
        worst = max(worst, _check(plan.run(_pack(ext, ssb), code, N, 0), ext, taps, cfg, 0))
        full = np.full(N, -32768.0) + (-32768.0j if ssb else 0)
        worst = max(worst, _check(plan.run(_pack(full, ssb), code, N, 0), full, taps, cfg, 0))
        _note(f"special inputs {L}/{M} ssb {ssb}", worst)
    # a 1 kHz tone recorded at 6 kHz comes out at 1000.0 Hz of 4 kHz audio
    from meteorgpu import resample
    t = np.arange(3 * 6000)
    x = np.round(10000 * np.sin(2 * np.pi * 1000.0 * t / 6000)).astype(np.int16)
    y = resample.resample_audio(x, 6000)
    seg = y[200: 200 + 8000]
    assert len(y) == 3 * 4000 and np.argmax(np.abs(np.fft.rfft(seg * np.hanning(8000)))) * 4000 / 8000 == 1000.0


@pytest.mark.parametrize("ssb", [False, True])
def test_non_finite_float32_samples(ctx, ssb):
    """the header's statement: an output whose own window n0 - I_phi + 1 .. n0 holds no such sample is what it is
    with that sample replaced by 0, bit for bit; one whose window holds one is not finite (REAL, one inf: the
    sign of tap times gain times inf, NaN where the tap is 0); a branch without a tap still gives 0"""
    for L, M, ntaps in ((2, 3, 25), (2, 3, 1), (40, 441, 3529)):
        taps = _taps(L, M, ntaps).copy()
        if ntaps > 1:
            taps[ntaps // 2 + 3] = 0.0  # a tap that is exactly zero meets the inf in some output
        c, I = (ntaps - 1) // 2, -(-ntaps // L)
        N = 20 * M // L + 3 * I
        cfg = _cfg(ssb, L, M, ntaps, 3 if ssb else 0, 7 if ssb else 1, gain=-1.5)
        plan = _lib.ResampPlan(ctx, cfg, taps, 0, 0)
        raw, code, _ = _noise(ssb, N, 3, f32=True)
        w = 2 if ssb else 1
        # (at multiples of 3: with one tap at 2/3 no other sample is read at all)
        at = {3 * (N // 9): np.float32(np.inf), 3 * (N // 6): np.float32(np.nan), 3 * (2 * N // 9): np.float32(-np.inf)}
        bad = raw.copy()
        for n, v in at.items():
            bad[w * n] = v
            raw[w * n: w * n + w] = 0
        y0, y = plan.run(raw, code, N, 0), plan.run(bad, code, N, 0)
        m = np.arange(len(y))
        t = m * M + c
        n0, phi = t // L, t % L
        Iphi = np.where(phi < ntaps, -(-(ntaps - phi) // L), 0)
        hit = np.zeros(len(y), bool)
        for n in at:
            hit |= (n0 - Iphi < n) & (n <= n0)
        assert hit.any() and (~hit).any()
        assert np.array_equal(y[~hit], y0[~hit]) and np.all(np.isfinite(y0))
        assert not np.isfinite(y[hit]).any()
        assert np.all(y[Iphi == 0] == 0)
        if not ssb:  # the windows that hold the +inf alone: tap gain inf, by IEEE
            n = 3 * (N // 9)
            others = [k for k in at if k != n]
            only = (n0 - Iphi < n) & (n <= n0) & ~np.logical_or.reduce([(n0 - Iphi < k) & (k <= n0) for k in others])
            tap = taps[np.minimum(phi[only] + (n0[only] - n) * L, ntaps - 1)]
            want = np.where(tap == 0, np.nan, np.where(tap > 0, -np.inf, np.inf))  # (the gain is negative)
            assert only.any() and np.array_equal(y[only], want, equal_nan=True)


def test_int16_output_and_saturation(ctx):
    for ssb, L, M, ntaps, p, q in ((False, 2, 3, 25, 0, 1), (True, 40, 441, 3529, 5, 32)):
        taps = _taps(L, M, ntaps)
        N = 60 * M // L + 1
        cfg = _cfg(ssb, L, M, ntaps, p, q, gain=0.9, out=np.int16)
        chain = _lib.resamp_chain(cfg)
        for seed in range(40):  # the first seed whose reference has no output near a half-integer
            raw, code, val = _noise(ssb, N, 1000 + seed)
            ld = R.ref_ld(val, taps, L, M, ssb, p, q, 0.9, 0)
            bar = chain * U * 0.9 * R.abs_sum(val, taps, L, M, 0)
            frac = np.abs((ld - np.floor(ld)).astype(np.float64) - 0.5)
            if np.all(frac > bar) and np.all(np.abs(ld) < 32767):
                break
        else:
            raise AssertionError("no seed without a near-half-integer output")
        assert np.all(frac > bar) and np.all(np.abs(ld) < 32767)
        y = _lib.ResampPlan(ctx, cfg, taps, 0, 0).run(raw, code, N, 0)
        assert y.dtype == np.int16
        assert np.array_equal(y, np.rint(ld).astype(np.int64))
    # saturation at +- full scale with gain 4: a constant through a low-pass of gain L
    L, M, ntaps = 2, 3, 25
    lp = L * ddc.design_lowpass(ntaps, 0.3)
    plan = _lib.ResampPlan(ctx, _cfg(False, L, M, ntaps, gain=4.0, out=np.int16), lp, 0, 0)
    for v, want in ((32767, 32767), (-32768, -32768)):
        y = plan.run(np.full(600, v, np.int16), _lib.MSD_I16, 600, 0)
        assert len(y) == 400 and np.all(y[20:-20] == want) and y.min() >= -32768 and y.max() <= 32767
    # ties go to even: exact halves through one tap (3 / 1: the two other branches have no tap)
    plan = _lib.ResampPlan(ctx, _cfg(False, 3, 1, 1, gain=0.5, out=np.int16), np.array([1.0]), 0, 0)
    x = np.array([1, 3, 5, -1, -3, 2, 0, 32767, -32768], np.int16)
    y = plan.run(x, _lib.MSD_I16, len(x), 0)
    assert y[0::3].tolist() == [0, 2, 2, 0, -2, 1, 0, 16384, -16384] and not y[1::3].any() and not y[2::3].any()


def _dev(ctx, a):
    b = ctx.alloc(max(a.nbytes, 16))
    if a.nbytes:
        b.upload(a)
    return b


def test_ragged_batch_short_rows_and_many_tiles(ctx):
    """rows of one buffer side by side (a neighbour's samples, one past a row, contribute nothing), an empty
    row, ld_out smaller than some rows' counts (only ld_out outputs are written, out_len is the full count,
    the padding and the guard row keep their sentinel), more tiles than the grid has slots"""
    L, M, ntaps = 2, 3, 25
    taps = _taps(L, M, ntaps)
    lens = [300001, 0, 299999, 1, 300000, 123457, 300003, 7, 250000, 300002, 299998, 280000]
    pos = [0, 5, 1, (1 << 40) + 3, (1 << 62) // L - 300000, 3, 2, 9, 4, 6, 8, 10]
    for ssb, p, q, out in ((False, 0, 1, np.float64), (True, 12345, 192000, np.int16)):
        cfg = _cfg(ssb, L, M, ntaps, p, q, gain=1.25, out=out)
        plan = _lib.ResampPlan(ctx, cfg, taps, 0, 0)
        raw, code, val = _noise(ssb, sum(lens), 77)
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        counts = [_lib.resamp_out_len(cfg, p0, n)[1] for p0, n in zip(pos, lens)]
        ld = 190000  # below the long rows' 200000 or so, above the others'
        assert sum(c > ld for c in counts) >= 6 and sum(0 < c < ld for c in counts) >= 4
        sentinel = -7.5 if out == np.float64 else -12345
        y = np.full((len(lens) + 1, ld), sentinel, out)  # (the last row: a guard)
        dy, dn = _dev(ctx, y), ctx.alloc(8 * len(lens))
        plan.run_dev(_dev(ctx, raw), code, _dev(ctx, off), _dev(ctx, np.array(lens, np.int64)),
                     _dev(ctx, np.array(pos, np.int64)), len(lens), dy, ld, dn)
        got_n = np.empty(len(lens), np.int64)
        dn.download(got_n)
        dy.download(y)
        assert got_n.tolist() == counts
        assert np.all(y[-1] == sentinel)
        worst = 0.0
        for r, (o, n, p0) in enumerate(zip(off, lens, pos)):
            vis = min(counts[r], ld)
            assert np.all(y[r, vis:] == sentinel), r
            if out == np.float64:
                # the row alone, through the host form, is the same bits; its first ld outputs are checked
                alone = plan.run(raw[o: o + n], code, n, p0)
                assert np.array_equal(alone[:vis], y[r, :vis]), r
                if r in (0, 3, 4, 7):
                    worst = max(worst, _check(alone, val[o: o + n], taps, cfg, p0))
            else:
                w = 2
                alone = plan.run(raw[w * o: w * (o + n)], code, n, p0)
                assert np.array_equal(alone[:vis], y[r, :vis]), r
        _note(f"ragged batch of {sum(counts)} outputs ssb {ssb}", worst)


def _chunks(N, L, M, H, big):
    sizes = [0, 1, L, M - 1, 1, M, big, 0, M + 1, H + 1, 2, max(H - 1, 0)]
    out, at = [], 0
    for s in sizes:
        s = min(max(s, 0), N - at)
        out.append((at, at + s))
        at += s
    out.append((at, N))
    return out


@pytest.mark.parametrize("ssb,L,M,ntaps,p,q,out", [
    (False, 2, 3, 25, 0, 1, np.float64), (True, 2, 3, 25, 5, 32, np.int16),
    (False, 40, 441, 3529, 0, 1, np.int16), (True, 40, 441, 3529, 12345, 192000, np.float64),
    (False, 3, 2, 25, 0, 1, np.float64), (True, 3, 2, 25, 3, 7, np.int16)])
def test_pushes_then_flush_equal_run(ctx, ssb, L, M, ntaps, p, q, out):
    """chunks of 0, 1, L, M - 1, M, M + 1 and history + 1 samples, several tiles at once, then flush: bit for
    bit the batch row; from position 0 and after reset; a flushed stream refuses pushes; halo rows"""
    TM, G, K, I = R.plan(L, M, ntaps)
    H = I - 1
    taps = _taps(L, M, ntaps)
    cfg = _cfg(ssb, L, M, ntaps, p, q, gain=0.8, out=out)
    big = -(-5 * TM * M // L) + 3  # five tiles and a bit
    N = big + 4 * M + 3 * H + L + 40
    w = 2 if ssb else 1
    raw, code, _ = _noise(ssb, N, 31)
    plan = _lib.ResampPlan(ctx, cfg, taps, 2, N)
    for pos0, stream in ((0, 0), ((1 << 40) + 3, 1), (M + 1, 0)):
        whole = plan.run(raw, code, N, pos0)
        if pos0:  # (a new plan's streams start at 0)
            plan.reset(stream, pos0)
        parts = [plan.push(stream, raw[w * a: w * b], code, b - a) for a, b in _chunks(N, L, M, H, big)]
        parts.append(plan.flush(stream))
        assert len(parts[-1]) <= -(-((ntaps - 1) // 2) // M) + 1
        got = np.concatenate(parts)
        assert got.dtype == whole.dtype and np.array_equal(got, whole), (pos0, len(got), len(whole))
        with pytest.raises(_lib.MsdError) as e:  # a flushed stream must be reset first
            plan.push(stream, raw[: w], code, 1)
        assert e.value.code == _lib.MSD_ERR_INVALID and "msd_resamp_push" in e.value.msg
        with pytest.raises(_lib.MsdError):
            plan.flush(stream)
    # a row with I samples of halo on each side equals the whole on its interior
    whole = plan.run(raw, code, N, 0)
    a, b = 5 * M + 3 + I, min(N - I, 5 * M + 3 + I + -(-3 * TM * M // L) + 1)
    part = plan.run(raw[w * (a - I): w * (b + I)], code, b + I - (a - I), a - I)
    m_first = R.out_range(a - I, 1, L, M)[0]
    lo, hi = R.out_range(a, b - a, L, M)[0], R.out_range(b, 1, L, M)[0]
    assert hi - lo > 2 * TM and np.array_equal(part[lo - m_first: hi - m_first], whole[lo:hi])


def test_two_streams_pushed_together_equal_each_alone(ctx):
    L, M, ntaps, p, q = 40, 441, 3529, 5, 32
    taps = _taps(L, M, ntaps)
    cfg = _cfg(True, L, M, ntaps, p, q)
    max_push = 50000
    plan = _lib.ResampPlan(ctx, cfg, taps, 2, max_push)
    rawA, code, _ = _noise(True, 90000, 1)
    rawB, _, _ = _noise(True, 70001, 2)
    alone = [plan.run(rawA, code, 90000, 0), plan.run(rawB, code, 70001, 0)]
    ld = -(-max_push * L // M) + 1  # the least the contract takes
    cuts = [(0, 0), (40000, 17), (40001, 30000), (90000, 70001)]  # (samples of A, of B) pushed so far
    got = [[], []]
    dy, dn = ctx.alloc(2 * ld * 8), ctx.alloc(16)
    x0 = _dev(ctx, rawA[:2])
    with pytest.raises(_lib.MsdError) as e:  # one output less than ceil(max_push L / M) + 1 is refused
        plan.push_dev(x0, code, _dev(ctx, np.zeros(2, np.int64)), _dev(ctx, np.zeros(2, np.int64)), dy, ld - 1, dn)
    assert e.value.code == _lib.MSD_ERR_INVALID and "msd_resamp_push_dev" in e.value.msg
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


def test_host_forms_report_capacity(ctx):
    L, M, ntaps = 2, 3, 25
    plan = _lib.ResampPlan(ctx, _cfg(False, L, M, ntaps), _taps(L, M, ntaps), 1, 1000)
    raw, code, _ = _noise(False, 900, 1)
    y = np.full(10, -7.5)
    got = _lib.C.c_int64(0)
    rc = ctx.lib.msd_resamp_run(plan.h, _lib.ptr(raw), code, 900, 0, _lib.ptr(y), 10, _lib.C.byref(got))
    assert rc == _lib.MSD_ERR_CAPACITY and got.value == 600 and np.all(y == -7.5)
    rc = ctx.lib.msd_resamp_push(plan.h, 0, _lib.ptr(raw), code, 900, _lib.ptr(y), 10, _lib.C.byref(got))
    assert rc == _lib.MSD_ERR_CAPACITY and got.value == 596 and np.all(y == -7.5)  # 3 m + 12 < 1800
    with pytest.raises(_lib.MsdError):
        plan.push(0, raw[:1], _lib.MSD_F32, 1)  # the stream holds int16 samples


def test_timing_id(ctx):
    L, M, ntaps = 2, 3, 25
    plan = _lib.ResampPlan(ctx, _cfg(False, L, M, ntaps), _taps(L, M, ntaps), 0, 0)
    raw, code, _ = _noise(False, 5000, 1)
    ctx.timing(True)
    try:
        ctx.timing_reset()
        plan.run(raw, code, 5000, 0)
        ms, n = ctx.timing_get(_lib.K_RESAMP)
        assert n == 1 and ms > 0
        assert ctx.timing_get(_lib.K_DDC)[1] == 0
    finally:
        ctx.timing(False)
