"""GPU: the whole-band Welch row (csrc/welch_fft.hip, msd_welch_spectrum / msd_welch_spectrum_dev) against
the long-double truth of tests/welch_fft_signals.py: every bin of every block within the per-bin
bound, the dB mean within its bound, on every shape of the table (the smallest that reach each path:
pruned, folded, one segment, step 1, the in-place sizes) and the classes carrier_weak,
fullscale_noise, nyquist_dc, dc_quiet, impulses, const; the rms error of the noise-like classes against
scipy's float64 pipeline; the band sums against msd_welch_bands; the batch layout; the shapes the
transform does not take."""
import ctypes as C

import numpy as np
import pytest

import spec_signals as ss
import welch_fft_signals as W
from meteorgpu import _lib, dsp, live

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ss.LD_OK, reason=ss.LD_REASON)]


def _cfg(shape, dtype, fs=W.FS, bands=((0, 0),)):
    bs, nper, nov, nfft = shape
    win = dsp.hann_periodic(nper)
    wc = win.astype(np.complex128)
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = bs, nper, nov, nfft
    c.sample_scale = W.sample_scale(dtype)
    c.scale = float(np.real(1.0 / (fs * (wc * wc).sum())))
    c.nbands = len(bands)
    for j, (lo, hi) in enumerate(bands):
        c.band_lo[j], c.band_hi[j] = lo, hi
    return c, win


def _plan(shape, dtype, **kw):
    c, win = _cfg(shape, dtype, **kw)
    return _lib.WelchPlan(dsp.context(0), c, win)


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_every_bin_within_the_bound(case):
    shape, dt = case
    chain = W.chain(shape[1], shape[3])
    plan = _plan(shape, dt)
    try:
        for cls in W.CLASSES:
            x = W.block_signal(cls, shape, dt)
            R, B = W.row_bound(W.truth(cls, shape, dt), chain)
            S, db = plan.spectrum(x)
            assert S.shape == R.shape and db.shape == (R.shape[0],)
            ratio, at = W.row_ratio(S, R, B)
            print(f"{W.case_id(case)} {cls}: per-bin ratio {ratio:.3g} at {at}")
            assert ratio <= 1.0, (cls, ratio, at)
            ref, bound = W.db_mean_ref(R), W.db_mean_bound(R, B)
            for b in range(len(ref)):
                if np.isfinite(bound[b]):
                    print(f"   block {b}: dB mean off by {abs(db[b] - float(ref[b])):.3g}, bound {float(bound[b]):.3g}")
                    assert abs(db[b] - float(ref[b])) <= float(bound[b]), (cls, b)
                else:
                    assert not np.isnan(db[b]) and not np.isposinf(db[b]), (cls, b)
                with np.errstate(divide="ignore"):  # the kernel's own mean of its own row
                    own = np.mean(10 * np.log10(S[b]))
                assert db[b] == own or abs(db[b] - own) <= 1e-12 * max(1.0, abs(own)), (cls, b, db[b], own)
            if cls == "const":
                assert not S.any() and np.all(np.isneginf(db))
            if cls in ss.NOISE_LIKE:
                mine, ref64 = W.rms_rows(S, R), W.rms_rows(W.scipy_rows(x, shape, dt), R)
                print(f"   rms error {mine.max():.3g}, scipy float64 {ref64.max():.3g}")
                assert np.all(mine <= ss.RMS_FACTOR * ref64), (cls, mine, ref64)
    finally:
        plan.close()


def test_band_sums_match_welch_bands():
    shape = W.SHAPES[0][0]
    cfg = live.ConfigDetection()
    c, win = live.welch_cfg(W.FS, cfg, W.sample_scale("int16"))
    assert (c.block_size, c.nperseg, c.noverlap, c.nfft) == shape
    x = W.block_signal("fullscale_noise", shape, "int16")
    plan = _lib.WelchPlan(dsp.context(0), c, win)
    try:
        bands = plan.run(x)
        S, _ = plan.spectrum(x)
    finally:
        plan.close()
    S2, _ = live.welch_spectrum(x, W.FS, cfg, W.sample_scale("int16"))
    assert np.array_equal(S, S2)
    for j in range(3):
        lo, hi = int(c.band_lo[j]), int(c.band_hi[j])
        mine = 10 * np.log10(np.array([np.sum(r[lo: hi + 1]) for r in S]))
        print(f"band {j}: max |dB difference| {np.abs(mine - bands[j]).max():.3g}")
        assert np.abs(mine - bands[j]).max() <= 1e-9


@pytest.mark.parametrize("dt", ["int16", "float64"])
def test_ragged_batch_layout_and_bit_identity(dt):
    shape = W.SHAPES[0][0]
    bs, K = shape[0], shape[3] // 2 + 1
    ctx = dsp.context(0)
    x = W.block_signal("fullscale_noise", shape, dt, 4)
    files = [x[:bs - 1], x[100: 100 + bs + 5], x[bs: 4 * bs + 7]]  # 0, 1 and 3 blocks
    nbs = [0, 1, 3]
    offs, pos = [], 0
    for f in files:
        offs.append(pos)
        pos += (len(f) + 63) // 64 * 64
    flat = np.zeros(pos, x.dtype)
    for o, f in zip(offs, files):
        flat[o: o + len(f)] = f
    ld, max_blocks, sentinel = 5, 3, -7.25
    plan = _plan(shape, dt)
    try:
        d_x, d_off, d_len = ctx.alloc(flat.nbytes), ctx.alloc(24), ctx.alloc(24)
        d_psd, d_db = ctx.alloc(3 * ld * K * 8), ctx.alloc(3 * ld * 8)
        d_x.upload(flat)
        d_off.upload(np.array(offs, np.int64))
        d_len.upload(np.array([len(f) for f in files], np.int64))
        d_psd.upload(np.full(3 * ld * K, sentinel))
        d_db.upload(np.full(3 * ld, sentinel))
        plan.spectrum_dev(d_x, x.dtype, d_off, d_len, 3, max_blocks, d_psd, ld, d_db)
        psd, db = np.empty((3, ld, K)), np.empty((3, ld))
        d_psd.download(psd)
        d_db.download(db)
        for f, (xf, nb) in enumerate(zip(files, nbs)):
            S, m = plan.spectrum(xf)
            assert S.shape == (nb, K)
            assert np.array_equal(psd[f, :nb], S) and np.array_equal(db[f, :nb], m)
            assert np.all(psd[f, nb:] == sentinel) and np.all(db[f, nb:] == sentinel)
        # no db_mean: the rows alone, the same
        d_psd.upload(np.full(3 * ld * K, sentinel))
        plan.spectrum_dev(d_x, x.dtype, d_off, d_len, 3, max_blocks, d_psd, ld, None)
        psd2 = np.empty((3, ld, K))
        d_psd.download(psd2)
        assert np.array_equal(psd, psd2)
        for b in (d_x, d_off, d_len, d_psd, d_db):
            b.free()
    finally:
        plan.close()


@pytest.mark.parametrize("nfft", [24, 32768])
def test_unsupported_shapes(nfft):
    plan = _plan((64, 16, 8, nfft), "int16")
    try:
        x = np.zeros(128, np.int16)
        out, db, got = np.full((2, nfft // 2 + 1), 3.0), np.full(2, 3.0), C.c_int64(-1)
        rc = plan.ctx.lib.msd_welch_spectrum(plan.h, _lib.ptr(x), _lib.dtype_code(x.dtype), 128, _lib.ptr(out), _lib.ptr(db),
                                             C.byref(got))
        assert rc == _lib.MSD_ERR_UNSUPPORTED
        assert np.all(out == 3.0) and np.all(db == 3.0)
        with pytest.raises(_lib.MsdError) as e:
            plan.spectrum(x)
        assert e.value.code == _lib.MSD_ERR_UNSUPPORTED
    finally:
        plan.close()


def test_timing_id():
    ctx = dsp.context(0)
    shape = W.SHAPES[0][0]
    plan = _plan(shape, "int16")
    try:
        ctx.timing(True)
        ctx.timing_reset()
        plan.spectrum(W.block_signal("fullscale_noise", shape, "int16"))
        ms, n = ctx.timing_get(_lib.K_WSPEC)
        assert n == 1 and ms > 0
    finally:
        ctx.timing(False)
        plan.close()
