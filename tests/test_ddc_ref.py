"""CPU: the down-converter's references (tests/ddc_ref.py) against scipy and against each other, the
Weaver example of the contract, meteorgpu.ddc's filter design against scipy.signal.firwin, and the proof
that the GPU test's error bar bites: each single mistake in the operation misses it by a stated factor."""
import numpy as np
import pytest
from scipy import signal

import ddc_ref as R
from meteorgpu import _lib, ddc

U = R.U


def _chain(mode, D, ntaps, p=0, q=1):
    return _lib.ddc_chain(_lib.MsdDdcCfg(mode, D, ntaps, _lib.MSD_F64, p, q, 1.0))


@pytest.mark.parametrize("N,D,ntaps", [(1000, 48, 385), (7, 2, 3), (1, 12, 5), (100, 12, 5), (4801, 48, 385)])
def test_real_is_resample_poly(N, D, ntaps):
    rng = np.random.default_rng(N + D)
    x = rng.integers(-32768, 32768, N).astype(np.float64)
    h = rng.standard_normal(ntaps)
    want = signal.resample_poly(x, 1, D, window=h)
    got = R.ref_f64(x, h, D)
    assert got.shape == want.shape == (-(-N // D),)
    assert np.max(np.abs(got - want)) == 0.0


def _weaver_case(f_carrier, seed=3, secs=4.0):
    fs, f_sig = 192000, 30000
    cfg, _ = ddc.weaver(fs, f_sig)
    assert (cfg.shift_num, cfg.shift_den, cfg.decim, cfg.ntaps) == (5, 32, 48, 385)
    h = signal.firwin(385, 0.9 * 1000 / 96000)
    rng = np.random.default_rng(seed)
    n = int(secs * fs)
    t = np.arange(n)
    x = 1000.0 * np.exp(2j * np.pi * f_carrier * t / fs) + 300.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.round(x.real) + 1j * np.round(x.imag)
    return R.ref_f64(x, h, 48, ssb=True, p=5, q=32)


def test_weaver_puts_the_carrier_on_1000_hz():
    y = _weaver_case(30000.0)
    f, P = signal.welch(y, 4000, nperseg=256, nfft=4096)
    assert f[np.argmax(P)] == 1000.0
    assert 10 * np.log10(P.max() / np.median(P)) > 45.0
    on = np.sqrt(np.mean(y ** 2))
    assert 600.0 < on < 800.0  # amplitude 1000: 707 rms
    # a carrier 1.5 kHz below the tuned centre (30 kHz here, as f_tone = fs_out / 4): the transition band
    off = np.sqrt(np.mean(_weaver_case(28500.0) ** 2))
    assert off < 0.1 * on


CASES = [  # (ssb, D, ntaps, p, q, N, pos0)
    (False, 12, 97, 0, 1, 3000, 0),
    (False, 3, 4095, 0, 1, 9000, 5),
    (True, 48, 385, 5, 32, 9000, 0),
    (True, 48, 385, 12345, 192000, 9000, (1 << 40) + 3),
    (True, 2, 3, 1234567, (1 << 24) - 3, 5000, 1 << 62),
    (True, 12, 5, 0, 1, 400, 1),
]


def _signal(ssb, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, N).astype(np.float64)
    return x + 1j * rng.integers(-32768, 32768, N) if ssb else x


@pytest.mark.parametrize("ssb,D,ntaps,p,q,N,pos0", CASES)
def test_float64_and_long_double_agree(ssb, D, ntaps, p, q, N, pos0):
    x = _signal(ssb, N, ntaps)
    h = ddc.design_lowpass(ntaps, 0.8 / D if D > 1 else 0.5)
    gain = 1.5
    a = R.ref_f64(x, h, D, ssb, p, q, gain, pos0)
    b = R.ref_ld(x, h, D, ssb, p, q, gain, pos0)
    S = R.abs_sum(x, h, D, pos0)
    assert a.shape == b.shape == S.shape and len(a) == R.out_range(pos0, N, D)[1]
    err = np.abs(a.astype(R.LD) - b).astype(np.float64)
    assert np.all(err <= (ntaps + 6) * U * gain * S)


# each corruption of the operation, on full-scale noise, misses the GPU test's bar chain u gain S_m by at
# least this factor on its worst output (all are first-order mistakes: their error is a fraction of S_m,
# against chain u ~ 1e-14; the float32 factors' is 2^-25 of it)
CORRUPTIONS = [
    (dict(drop_tap=100), 1e6),
    (dict(c_off=1), 1e9),
    # (p / q = 1 - 2 / q here: a sample late is a phase off by 4 pi / q = 7.5e-7 rad, 6e7 of chain u, on a
    # sum |v| that for noise is a few percent of S_m)
    (dict(phase_late=1), 1e5),
    (dict(im_off=1), 1e9),
    (dict(wrap64=True), 1e9),
    (dict(tw32=True), 1e3),
]


@pytest.mark.parametrize("kw,factor", CORRUPTIONS)
def test_the_bar_bites(kw, factor):
    # (q and p near 2^24: n p passes 2^63 at pos0 = 2^40 + 3, so the unreduced product wraps)
    D, ntaps, p, q, N, pos0 = 48, 385, (1 << 24) - 5, (1 << 24) - 3, 6000, (1 << 40) + 3
    x = _signal(True, N, 11)
    h = ddc.design_lowpass(ntaps, 0.9 * 1000 / 96000)
    good = R.ref_ld(x, h, D, True, p, q, 1.0, pos0)
    S = R.abs_sum(x, h, D, pos0)
    bar = _chain(_lib.DDC_SSB, D, ntaps, p, q) * U * S
    ok = np.abs(R.ref_f64(x, h, D, True, p, q, 1.0, pos0).astype(R.LD) - good).astype(np.float64)
    assert np.all(ok <= bar), "the uncorrupted float64 reference must pass the bar"
    bad = np.abs(R.ref_f64(x, h, D, True, p, q, 1.0, pos0, **kw).astype(R.LD) - good).astype(np.float64)
    worst = np.max(bad / bar)
    print(kw, f"misses the bar by {worst:.3g}")
    assert worst > factor


def test_phase_index_is_exact_at_2_62():
    q, p, n = (1 << 24) - 3, 1234567, 1 << 62
    r = R.phase_index(n, 4, p, q)
    assert [int(v) for v in r] == [((n + j) * p) % q for j in range(4)]
    assert [int(v) for v in R.phase_index(n, 4, p, q, wrap64=True)] != [int(v) for v in r]


def test_design_lowpass_is_firwin():
    # firwin evaluates the same formula in its own order (window by get_window, the sinc's argument
    # scaled differently): measured 0.125 .. 3 ulp of the largest tap over these lengths and cutoffs (3 at
    # ntaps 3, cutoff 0.5; 2 at 97 taps, 0.9 kHz of 96 kHz; 1 at 385 and 4095 taps); 8 ulp allowed
    for ntaps in (3, 97, 385, 4095):
        for cutoff in (0.9 * 1000 / 96000, 0.075, 0.5):
            a, b = ddc.design_lowpass(ntaps, cutoff), signal.firwin(ntaps, cutoff)
            tol = 8 * np.spacing(np.max(np.abs(b)))
            d = np.max(np.abs(a - b))
            print(ntaps, cutoff, d / np.spacing(np.max(np.abs(b))))
            assert d <= tol, (ntaps, cutoff, d, tol)


def test_weaver_and_decimator_configs():
    cfg, taps = ddc.weaver(192000, 30000)
    assert (cfg.mode, cfg.decim, cfg.ntaps, cfg.shift_num, cfg.shift_den) == (_lib.DDC_SSB, 48, 385, 5, 32)
    assert len(taps) == 385 and abs(taps.sum() - 1) < 1e-12
    cfg, _ = ddc.weaver(192000, -30000.5)  # a negative, half-hertz offset: still an exact fraction
    assert 0 <= cfg.shift_num < cfg.shift_den <= 1 << 24
    with pytest.raises(ValueError):
        ddc.weaver(192000, 30000, fs_out=4100)
    with pytest.raises(ValueError):
        ddc.weaver(192000, 0.1)  # 0.1 is not a short binary fraction
    cfg, taps = ddc.lowpass_decimator(48000)
    assert (cfg.mode, cfg.decim, cfg.ntaps, cfg.shift_num, cfg.shift_den) == (_lib.DDC_REAL, 12, 97, 0, 1)
