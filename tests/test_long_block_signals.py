"""CPU: the yardstick, chain and cases of tests/long_block_signals.py, before a GPU sees them.

* at every case that tests/test_gpu_long_blocks.py runs, the float64 yardstick in the long kernel's
  segmentation stays inside the model against the long-double exact DFT, and the
  model's bound is finite on every block that is not all zero;
* margin.delta_error_bound at L > 4096, called as dsp.process_samples calls it, bounds the
  yardstick's delta against numpy's;
* margin._block_spl and margin._chain agree with the helper, and are unchanged up to 4096;
* the bars bite at L = 9600: a neighbouring bin, samples shifted by one, one dropped lane segment and
  sample L leaking in each break the model; 2 cos th rounded to float32 breaks it too; four bits
  short of float64 it passes the model and breaks the rms bar;
* the flat 1e-9 dB bar of the older tests: where the yardstick alone meets it against numpy.
"""
import math

import numpy as np
import pytest

import band_signals as G
import long_block_signals as LB
from meteorgpu import margin as M

pytestmark = pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)


@pytest.mark.parametrize("case", [pytest.param(c, id=LB.case_id(c)) for c in LB.cases()])
def test_yardstick_within_model_bound_finite_and_guard_holds(case):
    B, nfft, dt, band, noise, classes = case
    L = min(B, nfft)
    for cls in classes:
        r = LB.case_refs(case, cls)
        for bd in r["bands"]:
            if cls == "zeros" or bd["n"] == 0:
                assert (bd["db"] == -120.0).all() and (G.db(bd["Ey"]) == -120.0).all(), cls
                continue
            bound = G.model_bound(bd["db"], bd["n"], r["chain"], r["S"])
            assert np.all(np.isfinite(bound)), f"{cls}: the model's bound is infinite on a block that is not all zero"
            q = G.ratio(np.abs(G.db(bd["Ey"]) - bd["db"]), bound)
            assert q <= 1.0, (cls, q)
        # the shipped guard against numpy, with the yardstick standing in for the device
        yb, yn = (G.db(bd["Ey"]) for bd in r["bands"])
        xmax = float(np.max(np.abs(np.asarray(r["x"], dtype=np.float64))))
        guard = M.delta_error_bound(yb, yn, nfft=nfft, L=L, window=r["w"], xmax=xmax, band=band, noise=noise)
        d_np = r["bands"][0]["db_np"] - r["bands"][1]["db_np"]
        ok = np.isfinite(guard)
        assert G.ratio(np.abs((yb - yn) - d_np)[ok], guard[ok]) <= 1.0, cls


def test_margin_agrees_with_the_helper_and_is_unchanged_below():
    for L in (4097, 4112, 6000, 8192, 9600, 9601, 32768, 65535, 65536):
        assert M._block_spl(L) == LB.long_spl(L), L
        assert LB.long_spl(L) % 8 == 0 and 256 * LB.long_spl(L) >= L > 256 * (LB.long_spl(L) - 8), L
    for L in (1, 256, 257, 1024, 2049, 4096):
        assert M._block_spl(L) == G.spl_of(L), L
    for B, nfft, _ in LB.SHAPES:
        L = min(B, nfft)
        bins = np.array(G.edge_bins(nfft))
        w = G.block_window(B, L)
        dev = M._chain(nfft, L, bins, float(w.sum())) - (4.0 * math.log2(nfft) + 8.0)
        assert dev == LB.chain_long(L, bins, nfft) == 3.0 * LB.long_spl(L) ** 2 + 28.0, (B, nfft)
    bins = np.array([170, 511])
    assert M._chain(1024, 1024, bins, 512.0) == 4.0 * 10 + 8.0 + M._goertzel_chain(64, bins, 1024)


# ------------------------------------------------------------------------------------- teeth
# L = 9600 cropped from B = 38400: the window's foot, whose last value is not the 0 of a whole Hann
TEETH_B, TEETH_NFFT = 38400, 9600


def _most_moved_bins(nfft, short, among=20, take=2):
    """of the `among` bins below Nyquist (G = SPL, |2 cos th| in [1, 2): the coarsest ulp), the `take`
    whose 2 cos th a mantissa `short` bits shorter moves most (the higher bin on a tie).  Four bits are
    16 roundings of one operation against a bar of RMS_FACTOR = 4 yardsticks plus the dB floor, and
    SPL is 40 here: a bin whose 2 cos th happens to lie on the shorter grid is not corrupted at all"""
    K = nfft // 2 + 1
    k = np.arange(K - 1 - among, K - 1)
    c2 = 2.0 * np.cos(2.0 * np.pi * k / nfft)
    moved = np.abs(G.round_twiddle(c2, short) - c2)
    order = sorted(range(len(k)), key=lambda i: (moved[i], k[i]), reverse=True)
    return sorted(int(k[i]) for i in order[:take])


_KB, _KN = _most_moved_bins(TEETH_NFFT, 4)
TEETH = (TEETH_B, TEETH_NFFT, (_KB, _KB), (_KN, _KN))


def _teeth(cls, **corrupt):
    """(assertion 1 holds, assertion 3 holds) for a corrupted yardstick standing in for the device"""
    B, nfft, band, noise = TEETH
    bins = G.plan_bins(band, noise)
    r = LB.refs(cls, B, nfft, "int16", band, noise, LB.NBLK_RMS)
    read = [k + corrupt.pop("bin_shift", 0) for k in bins]
    Y = LB.goertzel256_powers(r["x"], B, nfft, r["w"], read, **corrupt)
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
    assert not _teeth(cls, bin_shift=1)[0]        # a neighbouring bin in place of the right one
    assert not _teeth(cls, shift=1)[0]            # samples shifted by one
    assert not _teeth(cls, drop_segment=100)[0]   # one dropped lane segment
    assert not _teeth(cls, leak=True)[0]          # sample L leaking in


def test_teeth_lost_precision_breaks_the_rms_bar():
    """2 cos th four bits short of float64 stays inside the model and breaks the precision bar alone;
    rounded to float32 it breaks the model as well"""
    for cls in G.NOISE_LIKE:
        assert _teeth(cls, twiddle=4) == (True, False), cls
        assert _teeth(cls, twiddle=np.float32) == (False, False), cls


# ------------------------------------------------------------------------------------- flat bar
@pytest.mark.parametrize("B,nfft", LB.FLAT_SHAPES)
def test_flat_bar_yardstick_alone(B, nfft):
    """1e-9 dB against numpy is a condition, not a measurement: the GPU test asserts it on the shapes
    at which the float64 yardstick alone meets it on the same input"""
    worst = max(float(np.max(np.abs(y - n))) for y, n in zip(LB.flat_db_yardstick(B, nfft), LB.flat_db_numpy(B, nfft)))
    print(f"FLAT {B}/{nfft}: yardstick against numpy {worst:.3e} dB")
    assert worst <= LB.FLAT_DB
