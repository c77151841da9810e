"""CPU: the premises of the certificate stress classes (tests/iq_signals.py), pinned by the float64
oracle alone -- what each class is for (its delta range, band energy against frame energy, exact
zeros), that the classes with pings have oracle detections, and that the documented fp32 bound,
evaluated in numpy on the reference spectrum (iq_signals.model_ed), is finite where the GPU tests
(test_gpu_certify_stress.py) require the kernel's to be.

Two of the classes are not what one might take them for, and the oracle says so here: an impulse
train alone and noise below the 1e-12 floor do NOT have a constant delta (the impulses' delta moves
by +-0.05 dB with their position in the frame; 1e-12 + 1e-17 is not 1e-12 in float64), so only
`zeros` and `dc_only` are exact ties of delta and threshold."""
import numpy as np
import pytest

import iq_signals as G


def _energies(sg, o):
    bb, nb = G.bins(sg.band), G.bins(sg.noise)
    return o.S[G.band_rows(*bb)].sum(axis=0), o.S[G.band_rows(*nb)].sum(axis=0), o.S.sum(axis=0)


@pytest.mark.parametrize("name,kind", G.CASES, ids=G.CASE_IDS)
def test_class_premise(name, kind):
    sg, o = G.make(name, kind), G.oracle(name, kind)
    T = o.delta.size
    assert sg.i.dtype == (np.int16 if kind == "int16" else np.float32) and sg.i.shape == sg.q.shape
    assert 700 <= T <= 1100 and o.S.shape == (G.N, T)
    Eb, En, St = _energies(sg, o)
    with np.errstate(divide="ignore", invalid="ignore"):
        below = 10 * np.log10(St / Eb)  # dB of the signal band's energy below the frame's
    if sg.pings:
        assert len(o.dets) >= 1
        assert o.dets[0][0] >= 1.0  # nothing fires in the first second
    if name in ("white", "dropout"):
        assert abs(np.median(o.delta[o.delta != 0.0])) < 3.0  # 2 bins against 3 of the same noise: about -1.8 dB
    if name == "carrier_far":
        assert np.median(below) > 85.0
    if name == "carrier_far_quiet":
        assert np.median(below) > 110.0
    if name == "carrier_near":
        assert below.min() > 90.0
    if name == "lowpass":
        assert o.delta.min() >= 25.0 and o.delta.max() <= 70.0
    if name == "dropout":
        dead = St == 0.0
        assert dead.sum() >= 85 and np.all(o.delta[dead] == 0.0)
        partly = (St > 0.0) & (St < 0.5 * np.median(St))
        assert partly.sum() >= 4  # frames reaching into the gap from either side
    if name in ("zeros", "dc_only"):
        assert not o.S.any() and np.all(o.delta == 0.0) and len(o.dets) == 0
        assert np.all(o.thr[1:] == o.delta[1:])  # an exact tie at every decision (thr[0] is NaN)
    if name == "tiny":
        assert set(np.unique(sg.i)) <= {-1, 0, 1} and set(np.unique(sg.q)) <= {-1, 0, 1} and sg.i.any()
    if name == "tiny_f32":
        assert max(Eb.max(), En.max()) < 1e-14 and np.abs(o.delta).max() < 1e-3
        assert o.delta.std() > 0  # below the floor, yet not constant
    if name == "impulses":
        assert np.count_nonzero(sg.i) == -(-sg.i.size // 1000) and np.all(sg.i[::1000] == 32767)
        assert 0 < np.abs(o.delta).max() < 0.1 and len(o.dets) == 0
    if name == "clipped":
        assert np.mean(np.abs(sg.i.astype(np.int32)) >= 32767) > 0.3
    if name == "step":
        assert np.median(St[T // 2 + 8:]) > 1e6 * np.median(St[: T // 2 - 8])
    if name == "dc_band_2_4":
        assert G.bins(sg.band) == (2, 4) and abs(int(sg.i[0]) - 30000) < 30
    if name == "nyquist":
        assert G.bins(sg.band) == (2044, 2047) and G.bins(sg.noise) == (-2048, -2046)


@pytest.mark.parametrize("name,kind", G.CASES, ids=G.CASE_IDS)
def test_model_bound(name, kind):
    """the documented bound on the reference spectrum: finite on every frame of the classes the GPU
    test requires it on, a few 1e-3 dB on the white-like ones, and +inf throughout where a
    full-scale carrier stands over sigma-2 noise (there every frame has to be refined)"""
    sg, o = G.make(name, kind), G.oracle(name, kind)
    ed = G.model_ed(o.S, sg.band, sg.noise)
    assert ed.shape == o.delta.shape and not np.isnan(ed).any() and np.all(ed >= 1e-12)
    if name in G.ALL_FINITE:
        assert np.all(np.isfinite(ed))
    if name in G.TIGHT:
        assert np.median(ed) < 1e-2
    if name in ("zeros", "dc_only"):
        assert np.all(ed == 1e-12)
    if name in ("carrier_far_quiet", "carrier_near"):
        assert np.all(np.isinf(ed))
    if name == "lowpass":
        assert np.all(np.isfinite(ed))


def test_bins_match_the_package():
    from meteorgpu import iq
    for band in (G.BAND, G.NOISE, G.NYQ_BAND, G.NYQ_NOISE, (90.0, 190.0), (10.0, 20.0)):
        assert G.bins(band) == iq.iq_band_bins(G.N, G.FS, band)


def test_levels_signal_changes_every_three_frames():
    i, q = G.levels(72 * 1024, "int16", 1024, seed=1)
    p = (i.astype(np.float64) ** 2 + q.astype(np.float64) ** 2).reshape(-1, 3 * 1024).mean(axis=1)
    assert p.max() / p.min() > 1e4 and np.all(np.abs(np.diff(np.log10(p))) > 0)
