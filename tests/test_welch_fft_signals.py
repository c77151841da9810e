"""CPU: the inputs and bounds of tests/welch_fft_signals.py are ones the reference alone passes.
scipy.signal.welch in float64 (pocketfft, another FFT than the kernel's) on every case of the table and
every class stays within the per-bin bound and the dB-mean bound against the long-double truth; the
chain constants respect their cap.

scipy is held to the kernel's bound plus the one term the kernel's bound rightly lacks, the rounding
of scipy's own segment mean (welch_fft_signals.scipy_mean_allowance).  Without it two of the 72
(shape, class) pairs cannot pass, dc_quiet at the segment lengths that are no power of two:
200-200-100-256 (bin 0 off by 124 times the kernel's bound) and 4099-3000-1000-4096 (52.2 times);
`test_allowance_is_needed_only_there` pins that down, so the term hides nothing else."""
import numpy as np
import pytest

import spec_signals as ss
import welch_fft_signals as W

pytestmark = pytest.mark.skipif(not ss.LD_OK, reason=ss.LD_REASON)


def test_chain_constants_under_their_cap():
    got = {(s[1], s[3]): W.chain(s[1], s[3]) for s, _ in W.SHAPES}
    assert got[(256, 4096)] == 29 and got[(16, 16)] == 15 and got[(3000, 4096)] == 40 and got[(8192, 16384)] == 46
    for (nper, nfft), c in got.items():
        assert c <= ss.CHAIN_ANY[nfft] + 1, (nper, nfft, c)
    assert W.sub_length(256, 4096) == 256 and W.sub_length(3000, 4096) == 2048 and W.sub_length(200, 256) == 128
    assert W.sub_length(16, 16) == 8 and W.sub_length(1, 16) == 2


@pytest.mark.parametrize("cls", W.CLASSES)
@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_scipy_float64_within_the_bounds(case, cls):
    shape, dt = case
    c = W.chain(shape[1], shape[3])
    x = W.block_signal(cls, shape, dt)
    R, B = W.row_bound(W.truth(cls, shape, dt), c, W.scipy_mean_allowance(x, shape, dt))
    S = W.scipy_rows(x, shape, dt)
    assert S.shape == R.shape and S.shape[0] >= 1
    ratio, at = W.row_ratio(S, R, B)
    print(f"{W.case_id(case)} {cls}: scipy per-bin ratio {ratio:.3g} at {at}")
    assert ratio <= 1.0, (cls, ratio, at)
    ref, bound = W.db_mean_ref(R), W.db_mean_bound(R, B)
    with np.errstate(divide="ignore"):
        got = (10 * np.log10(S)).mean(axis=1)
    for b in range(len(ref)):
        if np.isfinite(bound[b]):
            print(f"   block {b}: dB mean off by {abs(got[b] - float(ref[b])):.3g}, bound {float(bound[b]):.3g}")
            assert abs(got[b] - float(ref[b])) <= float(bound[b]), (cls, b)
        else:
            assert not np.isnan(got[b]) and not np.isposinf(got[b]), (cls, b)
    if cls == "const":
        assert not S.any() and not R.any() and np.all(np.isneginf(got))


def test_allowance_is_needed_only_there():
    """against the kernel's own bound, without the allowance, scipy passes everywhere but on dc_quiet at
    nperseg 200 and 3000, and there it misses at bin 0, where the window's transform puts a mean error"""
    missed = {}
    for case in W.CASES:
        shape, dt = case
        for cls in W.CLASSES:
            R, B = W.row_bound(W.truth(cls, shape, dt), W.chain(shape[1], shape[3]))
            ratio, at = W.row_ratio(W.scipy_rows(W.block_signal(cls, shape, dt), shape, dt), R, B)
            if ratio > 1.0:
                missed[(shape[1], cls)] = at[1]
    assert missed == {(200, "dc_quiet"): 0, (3000, "dc_quiet"): 0}, missed


def test_noise_rms_yardstick_is_small():
    shape, dt = W.CASES[0]
    for cls in ss.NOISE_LIKE:
        R, _ = W.row_bound(W.truth(cls, shape, dt), W.chain(shape[1], shape[3]))
        r = W.rms_rows(W.scipy_rows(W.block_signal(cls, shape, dt), shape, dt), R)
        assert np.all(r > 0) and np.all(r < 1e-15)
