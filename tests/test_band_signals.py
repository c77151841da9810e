"""CPU: the references, yardsticks, chains and inputs of tests/band_signals.py, before a GPU sees them.

* the float64 yardsticks (textbook Goertzel in the kernels' segmentation, the generic kernel's
  rotation recurrence) stay within a quarter of the model (within the counted chain for the generic
  one) on every class and shape that tests/test_gpu_band_bins.py runs;
* margin._chain covers the generic kernel's counted chain wherever that kernel can run;
* the long-double references agree with numpy's / scipy's own numbers where those are accurate;
* the assertions have teeth: a neighbouring bin, samples shifted by one, a dropped 16-sample
  segment and sample L leaking in each break the model bound; a twiddle four bits short passes it
  and breaks the precision bar (rounded to float32 it breaks both);
* the model's bound is finite on every block of every GPU case but the all-zero ones.
"""
import math

import numpy as np
import pytest

import band_signals as G
from meteorgpu import margin as M
from oracle import dsp_oracle as O

pytestmark = pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)

YARDSTICK_SHARE = 0.25  # of the model; the worst measured is 0.105 (300 / 1024, a constant, bin 1)


def _block_case_ratios(case):
    """per class of a case: (model ratio of the yardstick, every bound finite, all-zero input)"""
    kernel, B, nfft, dt, rect, band, noise, generic, classes = case
    out = {}
    for cls in classes:
        r = G.block_refs(cls, kernel, B, nfft, np.dtype(dt).name, rect, band, noise)
        worst, finite = 0.0, True
        for bd in r["bands"]:
            bound = G.model_bound(bd["db"], bd["n"], r["chain"], r["S"])
            finite &= bool(np.all(np.isfinite(bound)))
            ok = np.isfinite(bound)
            worst = max(worst, G.ratio(np.abs(G.db(bd["Ey"]) - bd["db"])[ok], bound[ok]))
        out[cls] = (worst, finite)
    return out


@pytest.mark.parametrize("case", [pytest.param(c, id=G.block_case_id(c)) for c in G.block_cases()])
def test_block_yardstick_within_model_and_bound_finite(case):
    kernel = case[0]
    for cls, (worst, finite) in _block_case_ratios(case).items():
        assert finite or cls == "zeros", f"{cls}: the model's bound is infinite on a block that is not all zero"
        assert worst <= (YARDSTICK_SHARE if kernel == "bd2" else 1.0), (cls, worst)


def test_zero_blocks_are_exactly_the_floor():
    r = G.block_refs("zeros", "bd2", 300, 1024, "int16", False, (1, 1), (511, 511))
    for bd in r["bands"]:
        assert (bd["db"] == -120.0).all() and not r["S"].any()


@pytest.mark.parametrize("case", [pytest.param(c, id=G.welch_case_id(c)) for c in G.welch_cases()])
def test_welch_yardstick_within_model(case):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    finite = total = 0
    for cls in G.WELCH_CLASSES:
        if cls == "tiny" and dt != G.F64:
            continue
        r = G.welch_refs(cls, case)
        bound = G.welch_bin_bound(r["P"], r["dx"], r["bins"], nfft, r["scale"])
        err = np.abs(np.sqrt(r["Y"].astype(G.LD)) - np.sqrt(r["P"])).astype(np.float64)
        if cls in ("zeros", "constant"):
            assert not r["P"].any() and not r["Y"].any()
        assert G.ratio(err, bound) <= YARDSTICK_SHARE, (cls, G.ratio(err, bound))
        # the band bound may be infinite where a band is empty by construction (the DC bin after the
        # detrend, a ramp's top band below the error floor): the per-bin bound above holds anyway
        ref_db = G.welch_band_db(r["P"], bands)
        for j, (lo, hi) in enumerate(bands):
            j0 = sum(h - l + 1 for l, h in bands[:j])
            dx = r["dx"][:, j0: j0 + hi - lo + 1].max(axis=1)
            e = M.welch_band_db_error(ref_db[j], hi - lo + 1, dx, r["scale"], nseg)
            finite += int(np.isfinite(e).sum())
            total += e.size
    assert finite > 0.5 * total, (finite, total)  # the band check is not vacuous


def test_margin_chain_covers_the_generic_kernel():
    """wherever block_delta_kernel can run (above 64 bins; under MSD_OPT_GENERIC_STFT any plan) the
    guard's device chain is at least the chain counted from that kernel's code, and at least the
    16-lane Goertzel's over the SPL samples a lane really runs (L < 256, L no multiple of 16)"""
    for case in G.block_cases():
        kernel, B, nfft, dt, rect, band, noise, generic, _ = case
        L = min(B, nfft)
        bins = np.array(G.plan_bins(band, noise))
        if not bins.size:
            continue
        w = G.block_window(B, L, rect)
        dev = M._chain(nfft, L, bins, float(w.sum())) - (4.0 * math.log2(nfft) + 8.0)
        assert dev >= G.chain_generic(L) - 1e-9, (B, nfft, dev, G.chain_generic(L))
        assert dev >= G.chain_goertzel16(L, bins, nfft) - 1e-9, (B, nfft, dev)


def test_block_reference_matches_numpy_on_a_synthetic_minute():
    from meteorgpu import dsp, synth
    fs, bs, n_fft, band, noise = 6000, 0.2, 512, (993, 1013), (690, 710)
    x, _ = synth.synth_real(seed=77, fs=fs, duration_s=60.0, f0=1000.0, rate_per_min=10)
    rb, rn, rd = O.block_powers_ref(x, fs, bs, band, noise, n_fft)
    B, nfft = int(fs * bs), 2 * n_fft
    w = G.block_window(B, min(B, nfft))
    for (lo, hi), ref in ((dsp.band_bins(nfft, fs, band), rb), (dsp.band_bins(nfft, fs, noise), rn)):
        got = G.db(G.band_energy(G.block_powers_ld(x, B, nfft, w, range(lo, hi + 1))))
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)


@pytest.mark.parametrize("nperseg,nfft,nov", [(256, 256, 128), (255, 1020, 0), (1000, 1000, 500)])
def test_welch_reference_matches_scipy_on_noise(nperseg, nfft, nov):
    from scipy.signal import welch
    rng = np.random.default_rng(3)
    block = nperseg + 2 * (nperseg - nov)
    x = rng.standard_normal(2 * block)
    w = G.welch_window(nperseg)
    bins = range(nfft // 2 + 1)
    P = G.welch_psd_ld(G.welch_segments(x, block, nperseg, nov, 1.0), w, nfft, bins, G.welch_scale(w))
    for b in range(2):
        _, R = welch(x[b * block: (b + 1) * block], G.FS, nperseg=nperseg, noverlap=nov, nfft=nfft)
        np.testing.assert_allclose(P[b].astype(np.float64), R, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------- teeth
TEETH = (9600, 1024, (170, 170), (511, 511))


def _teeth(cls, **corrupt):
    """(assertion 1 holds, assertion 3 holds) for a corrupted yardstick standing in for the device"""
    B, nfft, band, noise = TEETH
    bins = G.plan_bins(band, noise)
    r = G.block_refs(cls, "bd2", B, nfft, "int16", False, band, noise)
    read = [k + corrupt.pop("bin_shift", 0) for k in bins]
    x = r["x"]
    if corrupt.get("shift"):
        x = np.concatenate([x, np.zeros(1, x.dtype)])
    Y = G.goertzel16_powers(x, B, nfft, r["w"], read, **corrupt)
    model, prec = True, True
    for j, bd in enumerate(r["bands"]):
        E = G.band_energy(Y[:, j: j + 1])
        bound = G.model_bound(bd["db"], 1, r["chain"], r["S"])
        model &= bool(np.all(np.abs(G.db(E) - bd["db"]) <= bound))
        prec &= G.rms_amp(E, bd["E"]) <= G.RMS_FACTOR * G.rms_amp(bd["Ey"], bd["E"]) + G.db_floor(bd["db"], bd["E"])
    return model, prec


@pytest.mark.parametrize("cls", ["carrier_weak", "staircase"])
def test_teeth_structural_faults_break_the_model(cls):
    assert _teeth(cls) == (True, True)
    assert not _teeth(cls, bin_shift=1)[0]      # a neighbouring bin in place of the right one
    assert not _teeth(cls, shift=1)[0]          # samples shifted by one
    assert not _teeth(cls, drop_segment=3)[0]   # one dropped 16-sample segment
    assert not _teeth(cls, leak=True)[0]        # sample L leaking in


def test_teeth_lost_precision_breaks_the_rms_bar():
    """2 cos th four bits short of float64 stays inside the model and breaks the precision bar alone.
    Rounded to float32 it is 2^-24 SPL of S off, far more than chain u = 216 * 2^-53: that breaks
    the precision bar and the model as well"""
    for cls in G.NOISE_LIKE:
        assert _teeth(cls, twiddle=4) == (True, False), cls
        assert _teeth(cls, twiddle=np.float32) == (False, False), cls
