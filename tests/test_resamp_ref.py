"""CPU: the resampler's references (tests/resamp_ref.py) against scipy and against each other, the 6 kHz
archive example of the contract, meteorgpu.resample's designs, and the proof that the GPU test's error bar
bites: each single mistake in the operation misses it by at least a factor of ten on some output."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import signal

import resamp_ref as R
from meteorgpu import _lib, ddc, resample

U = R.U
SHAPES = [(2, 3, 25), (40, 441, 3529), (3, 2, 25), (2, 125, 1001), (1, 12, 97), (5, 7, 1), (7, 5, 3)]


def _chain(mode, L, M, ntaps, p=0, q=1):
    return _lib.resamp_chain(_lib.MsdResampCfg(mode, L, M, ntaps, _lib.MSD_F64, 0, p, q, 1.0))


@pytest.mark.parametrize("L,M,ntaps", SHAPES)
def test_real_is_resample_poly(L, M, ntaps):
    """resample_poly filters with (h / L) L, which is h to within an ulp per tap, in upfirdn's own order:
    the two differ by at most 2 u S_m from the taps and by the two sums' own rounding, I u S_m each"""
    rng = np.random.default_rng(L * 1000 + M)
    h = rng.standard_normal(ntaps)
    I = -(-ntaps // L)
    for N in (1, 7, 3 * M + 1, 40 * M + 5, 2 * ntaps // L + 17):
        x = rng.integers(-32768, 32768, N).astype(np.float64)
        want = signal.resample_poly(x, L, M, window=h / L)
        got = R.ref_f64(x, h, L, M)
        S = R.abs_sum(x, h, L, M)
        assert got.shape == want.shape == S.shape == (-(-N * L // M),), (N, got.shape, want.shape)
        assert np.all(np.abs(got - want) <= (2 * I + 4) * U * S), (N, np.max(np.abs(got - want)))
        if L & (L - 1) == 0:  # (h / L) L is h exactly
            assert np.array_equal(got, want)


def test_up_1_is_the_down_converters_reference():
    import ddc_ref
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 3000) + 1j * rng.integers(-32768, 32768, 3000)
    h = ddc.design_lowpass(97, 0.07)
    for pos0 in (0, 7, (1 << 40) + 3):
        assert np.array_equal(R.ref_f64(x.real, h, 1, 12, gain=1.5, pos0=pos0), ddc_ref.ref_f64(x.real, h, 12, gain=1.5, pos0=pos0))
        a, b = R.ref_ld(x, h, 1, 12, True, 5, 32, 1.5, pos0), ddc_ref.ref_ld(x, h, 12, True, 5, 32, 1.5, pos0)
        S = R.abs_sum(x, h, 1, 12, pos0)
        assert a.shape == b.shape and np.all(np.abs(a - b).astype(np.float64) <= 97 * 2.0 ** -63 * 1.5 * S)
        assert np.array_equal(R.abs_sum(x.real, h, 1, 12, pos0), ddc_ref.abs_sum(x.real, h, 12, pos0))


CASES = [  # (ssb, L, M, ntaps, p, q, N, pos0)
    (False, 2, 3, 25, 0, 1, 3000, 0),
    (False, 40, 441, 3529, 0, 1, 9000, 5),
    (False, 256, 1, 4095, 0, 1, 40, 1),
    (False, 2, 3, 1, 0, 1, 50, 0),
    (True, 2, 125, 1001, 5, 32, 9000, 0),
    (True, 3, 2, 25, 12345, 192000, 2000, (1 << 40) + 3),
    (True, 7, 5, 3, 1234567, (1 << 24) - 3, 3000, (1 << 62) // 7 - 3000),
    (True, 160, 441, 4095, 0, 1, 4000, 1),
]


def _signal(ssb, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, N).astype(np.float64)
    return x + 1j * rng.integers(-32768, 32768, N) if ssb else x


@pytest.mark.parametrize("ssb,L,M,ntaps,p,q,N,pos0", CASES)
def test_float64_and_long_double_agree(ssb, L, M, ntaps, p, q, N, pos0):
    x = _signal(ssb, N, ntaps)
    h = L * ddc.design_lowpass(ntaps, 0.8 / max(L, M)) if ntaps > 1 else np.array([0.75])
    gain = 1.5
    a = R.ref_f64(x, h, L, M, ssb, p, q, gain, pos0)
    b = R.ref_ld(x, h, L, M, ssb, p, q, gain, pos0)
    S = R.abs_sum(x, h, L, M, pos0)
    assert a.shape == b.shape == S.shape and len(a) == R.out_range(pos0, N, L, M)[1]
    err = np.abs(a.astype(R.LD) - b).astype(np.float64)
    assert np.all(err <= (-(-ntaps // L) + 6) * U * gain * S)
    assert np.all(b[S == 0] == 0)
    if ntaps < L:  # branches without a tap give exact zeros
        assert np.sum(S == 0) >= len(S) // L


def test_long_form_equals_the_whole():
    x = _signal(False, 20000, 3)
    h = 40 * ddc.design_lowpass(3529, 0.9 / 441)
    assert np.array_equal(R.ref_ld_long(x, h, 40, 441, gain=2.0, block=300), R.ref_ld(x, h, 40, 441, gain=2.0))
    x = _signal(True, 2000, 4)
    h = 3 * ddc.design_lowpass(25, 0.3)
    assert np.array_equal(R.ref_ld_long(x, h, 3, 2, True, 5, 32, block=77), R.ref_ld(x, h, 3, 2, True, 5, 32))


# each corruption of the operation, on full-scale noise, misses the GPU test's bar chain u gain S_m by at
# least a factor of ten on its worst output: all are first-order mistakes, whose error is a fraction of S_m
# (a dropped tap: about S_m / I) against chain u ~ 1e-14; the float32 factors' is 2^-25 of it
CORRUPTIONS = [dict(drop_tap=100), dict(c_off=1), dict(c_off=-1), dict(phi_off=1), dict(n_off=1), dict(swap=True),
               dict(phase_late=1), dict(im_off=1), dict(wrap64=True), dict(tw32=True)]


@pytest.mark.parametrize("kw", CORRUPTIONS, ids=lambda kw: next(iter(kw)) + str(next(iter(kw.values()))))
@pytest.mark.parametrize("L,M,ntaps", [(2, 3, 25), (40, 441, 3529)])
def test_the_bar_bites(L, M, ntaps, kw):
    # (q and p near 2^24: n p passes 2^63 at pos0 = 2^40 + 3, so the unreduced product wraps)
    p, q, N, pos0 = (1 << 24) - 5, (1 << 24) - 3, 6000, (1 << 40) + 3
    if "swap" in kw:
        pos0 = 0
    if "drop_tap" in kw:
        kw = dict(drop_tap=ntaps // 2 - 3)
    x = _signal(True, N, 11)
    h = L * ddc.design_lowpass(ntaps, 0.9 * min(1 / (2 * M), 1 / L))
    good = R.ref_ld(x, h, L, M, True, p, q, 1.0, pos0)
    S = R.abs_sum(x, h, L, M, pos0)
    bar = _chain(_lib.DDC_SSB, L, M, ntaps, p, q) * U * S
    ok = np.abs(R.ref_f64(x, h, L, M, True, p, q, 1.0, pos0).astype(R.LD) - good).astype(np.float64)
    assert np.all(ok <= bar), "the uncorrupted float64 reference must pass the bar"
    bad = np.abs(R.ref_f64(x, h, L, M, True, p, q, 1.0, pos0, **kw).astype(R.LD) - good).astype(np.float64)
    worst = np.max(bad[bar > 0] / bar[bar > 0])
    print(kw, f"misses the bar by {worst:.3g}")
    assert worst >= 10.0


def test_a_1_khz_tone_at_6_khz_stays_at_1000_hz():
    cfg, h = resample.lowpass_resampler(6000)
    assert (cfg.up, cfg.down, cfg.ntaps) == (2, 3, 25)
    t = np.arange(4 * 6000)
    x = np.round(10000 * np.sin(2 * np.pi * 1000.0 * t / 6000))
    y = R.ref_f64(x, h, 2, 3)
    assert len(y) == 4 * 4000
    seg = y[200: 200 + 8000]
    spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
    assert np.argmax(spec) * 4000 / len(seg) == 1000.0
    assert 0.95 * 10000 / np.sqrt(2) < np.sqrt(np.mean(seg ** 2)) < 1.05 * 10000 / np.sqrt(2)


def test_ratio_and_designs():
    assert resample.ratio(6000, 4000) == (2, 3) and resample.ratio(4000, 6000) == (3, 2)
    assert resample.ratio(44100, 4000) == (40, 441) and resample.ratio(22050, 4000) == (80, 441)
    assert resample.ratio(11025, 4000) == (160, 441) and resample.ratio(44100, 6000) == (20, 147)
    assert resample.ratio(250000, 4000) == (2, 125) and resample.ratio(48000, 4000) == (1, 12)
    assert resample.ratio(Fraction(44100), 4000.0) == (40, 441)
    with pytest.raises(ValueError):
        resample.ratio(4000, 4001)  # down 4000 and up 4001 are outside the limits
    for fs, (L, M) in ((6000, (2, 3)), (44100, (40, 441)), (11025, (160, 441))):
        cfg, h = resample.lowpass_resampler(fs, gain=2.0, out_dtype=np.int16)
        n = 8 * max(L, M) + 1
        assert (cfg.mode, cfg.up, cfg.down, cfg.ntaps, cfg.out_dtype, cfg.shift_num, cfg.shift_den, cfg.gain) == \
            (_lib.DDC_REAL, L, M, n, _lib.MSD_I16, 0, 1, 2.0)
        assert np.array_equal(h, L * ddc.design_lowpass(n, 0.9 / max(L, M)))
        tol = 8 * np.spacing(np.max(np.abs(h)))
        assert abs(h.sum() - L) < 1e-9 and np.max(np.abs(h - h[::-1])) <= tol
        assert np.max(np.abs(h - L * signal.firwin(n, 0.9 / max(L, M)))) <= L * tol
    cfg, h = resample.lowpass_resampler(4000, 6000)
    assert (cfg.up, cfg.down, cfg.ntaps) == (3, 2, 25)
    cfg, h = resample.lowpass_resampler(6000, ntaps=41)
    assert cfg.ntaps == 41 and len(h) == 41
    # the single-sideband form: 250 kHz I/Q
    cfg, h = resample.weaver_resampler(250000, 30000)
    assert (cfg.mode, cfg.up, cfg.down, cfg.ntaps) == (_lib.DDC_SSB, 2, 125, 1001)
    assert Fraction(cfg.shift_num, cfg.shift_den) == Fraction(30000 - 1000 + 1000, 250000)
    assert np.array_equal(h, 2 * ddc.design_lowpass(1001, 0.9 * min(1 / 250, 1 / 2)))
    cfg, h = resample.weaver_resampler(4000, 1200, fs_out=6000)  # upwards: the input's Nyquist bounds the filter
    assert (cfg.up, cfg.down) == (3, 2) and np.array_equal(h, 3 * ddc.design_lowpass(25, 0.9 * min(1 / 4, 1 / 3)))
    with pytest.raises(ValueError):
        resample.weaver_resampler(250000, 0.1)  # 0.1 is not a short binary fraction
    # a default filter above 4095 taps is refused with the ratio named; a given length is taken
    with pytest.raises(ValueError, match="600 / 1021"):  # 8 * 1021 + 1 = 8169 taps
        resample.lowpass_resampler(1021, 600)
    cfg, h = resample.lowpass_resampler(225000, 128000, ntaps=4095)
    assert (cfg.up, cfg.down, cfg.ntaps) == (128, 225, 4095)


def test_integer_ratios_take_the_down_converters_design():
    for fs in (48000, 8000, 4000):
        dcfg, dh = ddc.lowpass_decimator(fs)
        cfg, h = resample.lowpass_resampler(fs)
        assert (cfg.mode, cfg.up, cfg.down, cfg.ntaps) == (dcfg.mode, 1, dcfg.decim, dcfg.ntaps) and np.array_equal(h, dh)
    dcfg, dh = ddc.weaver(192000, 30000, gain=3.0)
    cfg, h = resample.weaver_resampler(192000, 30000, gain=3.0)
    assert (cfg.up, cfg.down, cfg.ntaps, cfg.shift_num, cfg.shift_den, cfg.gain) == (1, 48, 385, 5, 32, 3.0)
    assert np.array_equal(h, dh)


def test_the_down_converter_still_refuses_what_the_resampler_takes():
    with pytest.raises(ValueError):
        ddc.weaver(192000, 30000, fs_out=4100)
    # 4100 / 192000 = 41 / 1920: its down is above the resampler's limit of 1024 too, and it says so
    with pytest.raises(ValueError, match="41 / 1920"):
        resample.weaver_resampler(192000, 30000, fs_out=4100)
    # the neighbouring rates inside the limits, which ddc.weaver refuses as well, are taken
    for fs_out, (L, M) in ((4320, (9, 400)), (4500, (3, 128))):
        with pytest.raises(ValueError):
            ddc.weaver(192000, 30000, fs_out=fs_out)
        cfg, h = resample.weaver_resampler(192000, 30000, fs_out=fs_out)
        assert (cfg.mode, cfg.up, cfg.down, cfg.ntaps) == (_lib.DDC_SSB, L, M, 8 * M + 1) and len(h) == cfg.ntaps
        assert Fraction(cfg.shift_num, cfg.shift_den) == (Fraction(30000 - 1000) + Fraction(fs_out, 4)) / 192000
    with pytest.raises(ValueError):
        ddc.lowpass_decimator(6000)
    assert resample.lowpass_resampler(6000)[0].down == 3
