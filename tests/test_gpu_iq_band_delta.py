"""GPU: iq_band_delta_kernel by itself, over several streams (msd_iq_band_delta_bound_dev).

The detector only ever calls it with one stream and ld = max_frames.  Here: 3 streams of very
different level (x1, x1000, x0.001) and length in one spectrogram launch with energy partials,
ld = max_frames + 5, outputs prefilled with NaN.  The reference is numpy float64 on the DOWNLOADED
float32 spectrogram and partials, so only this kernel is under test:

* band_db, noise_db, delta: sums in ascending signed-bin order, 10 log10(E + 1e-12), within 1e-9 dB;
* everything outside [s*ld, s*ld + frames[s]) is still NaN (the detector points this output into
  the stream plan, between its halos);
* ed within 1e-9 relative of the documented formula (csrc/stream.hip above IQ_CHAIN) from the
  stream's own partials -- the levels are 10^6 apart, so another stream's partials cannot pass --
  and +inf exactly where a band touches bins -1..1;
* band pairs at the row ends, across 0 Hz (the scalar wrap-around loop), a single bin, an empty
  band, a wide unaligned one and lower edges of every residue mod 4 (the float4 head and tail);
* the optional outputs left out (band_db / noise_db; etot / ed) change no bit of delta.
"""
import numpy as np
import pytest

import iq_signals as G
from meteorgpu import _lib, iq
from meteorgpu.dsp import context

pytestmark = pytest.mark.gpu

FS, N, HOP = G.FS, G.N, G.HOP
DB_TOL = 1e-9
LEVELS = (1.0, 1000.0, 0.001)
PAD, GUARD = 5, 16

PAIRS = [
    ((21, 22), (-65, -63)),             # C5's own
    ((-2048, -2046), (2045, 2047)),     # the row's two ends (FFT order: its middle)
    ((-3, 2), (100, 103)),              # across 0 Hz: the wrap-around loop; bound +inf
    ((5, 5), (-5, -5)),                 # single bins
    ((3, 2), (10, 12)),                 # an empty band: exactly 10 log10(1e-12)
    ((1001, 1258), (-1258, -1001)),     # wide, unaligned at both ends
    ((41, 47), (-1006, -1001)),         # lower edges 1 and 2 mod 4
    ((43, 44), (-1005, -1000)),         # lower edges 3 mod 4 (rows 43 and 3091)
    ((2, 4), (-4, -2)),                 # next to the bins the bound excludes: finite
    ((1, 4), (10, 12)),                 # touching bin 1
    ((10, 12), (-9, -1)),               # the noise band touching bin -1
]


@pytest.fixture(scope="module")
def launch():
    """the spectrogram of the three streams with its partials, left on the device for every case"""
    rng = np.random.default_rng(2024)
    T = 41
    n = (T - 1) * HOP + N
    lens = [n, n - 5000, n - 20000]
    ctx = context(0).sibling()
    b = iq.IQBatch(ctx, 3, n, FS, N, N - HOP, dtype=np.float32)
    for s, lv in enumerate(LEVELS):
        z = G.cn(rng, n, 30.0) * lv
        z += 200.0 * lv * np.exp(2j * np.pi * 1000.0 * np.arange(n) / FS) * (np.arange(n) > n // 2)
        x = np.empty(2 * n, np.float32)
        x[0::2], x[1::2] = z.real, z.imag
        b.upload(s, x)
    b.d_len.upload(np.array(lens, np.int64))
    assert b.T == T
    nf = [(ln - N) // HOP + 1 for ln in lens]
    assert len(set(nf)) == 3 and max(nf) == T
    stride = int(ctx.lib.msd_cstft_energy_stride(3, T))
    etot = ctx.alloc(16 * 4 * stride)
    b.run(etot)
    frames = ctx.alloc(8 * 3)
    frames.upload(np.array(nf, np.int64))
    spec = np.empty((3, T, N), np.float32)
    b.d_out.download(spec)
    e = np.empty((16, stride), np.float32)
    etot.download(e)
    S = np.zeros((3, T))
    for q in range(16):  # the kernel's order
        S += e[q, : 3 * T].astype(np.float64).reshape(3, T)
    for s in range(3):
        assert S[s, : nf[s]].min() > 0
    # the premise of "another stream's partials cannot pass"
    assert S[1, : nf[1]].min() > 1e4 * S[0, : nf[0]].max() and S[0, : nf[0]].min() > 1e4 * S[2, : nf[2]].max()
    out = {k: ctx.alloc(8 * (3 * (T + PAD) + GUARD)) for k in ("band", "noise", "delta", "ed")}
    yield dict(ctx=ctx, b=b, T=T, nf=nf, etot=etot, frames=frames, spec=spec.astype(np.float64), S=S, out=out)
    for buf in (etot, frames, *out.values()):
        buf.free()
    b.close()
    ctx.close()


def _call(L, band, noise, band_db=True, bound=True):
    """one kernel launch into NaN-filled outputs; returns the four arrays [3 ld + GUARD] (None: not asked)"""
    ld = L["T"] + PAD
    m = 3 * ld + GUARD
    for buf in L["out"].values():
        buf.upload(np.full(m, np.nan))
    o = L["out"]
    _lib.iq_band_delta_dev(L["ctx"], L["b"].d_out, 3, L["T"], L["frames"], N, band, noise, o["delta"], ld,
                           band_db=o["band"] if band_db else None, noise_db=o["noise"] if band_db else None,
                           etot=L["etot"] if bound else None, ed=o["ed"] if bound else None)
    got = {k: buf.download(np.empty(m)) for k, buf in o.items()}
    return got, ld


def _energy(spec, lo, hi):
    """sum of rows' bins lo..hi in ascending signed order, sequentially, float64; spec [T][N]"""
    if hi < lo:
        return np.zeros(spec.shape[0])
    return np.cumsum(spec[:, G.band_rows(lo, hi)], axis=1)[:, -1]


@pytest.mark.parametrize("band,noise", PAIRS, ids=[f"{b[0]}_{b[1]}__{n[0]}_{n[1]}" for b, n in PAIRS])
def test_band_delta_multi_stream(launch, band, noise):
    L = launch
    got, ld = _call(L, band, noise)
    valid = np.zeros(3 * ld + GUARD, bool)
    for s in range(3):
        k = L["nf"][s]
        valid[s * ld: s * ld + k] = True
        Eb, En = _energy(L["spec"][s, :k], *band), _energy(L["spec"][s, :k], *noise)
        bd, nd = 10 * np.log10(Eb + 1e-12), 10 * np.log10(En + 1e-12)
        sl = slice(s * ld, s * ld + k)
        assert np.abs(got["band"][sl] - bd).max() <= DB_TOL
        assert np.abs(got["noise"][sl] - nd).max() <= DB_TOL
        assert np.abs(got["delta"][sl] - (bd - nd)).max() <= DB_TOL
        np.testing.assert_array_equal(got["delta"][sl], got["band"][sl] - got["noise"][sl])
        want = G.ed_formula(L["S"][s, :k], Eb, En, band, noise)
        touches = G.near_dc(*band) or G.near_dc(*noise)
        assert touches == any(lo <= c <= hi for lo, hi in (band, noise) for c in (-1, 0, 1))
        if touches:
            assert np.all(np.isposinf(got["ed"][sl]))
        else:
            assert np.all(np.isfinite(want)), "the case is meant to have a finite bound"
            np.testing.assert_allclose(got["ed"][sl], want, rtol=1e-9, atol=0)
        if band[1] < band[0]:  # the empty band: E = 0 exactly
            assert np.all(got["band"][sl] == 10 * np.log10(1e-12))
    for k_, a in got.items():
        assert np.all(np.isnan(a[~valid])), f"{k_}: written outside the streams' frames"
        assert not np.isnan(a[valid]).any()


def test_optional_outputs_change_nothing(launch):
    L = launch
    band, noise = PAIRS[0]
    full, ld = _call(L, band, noise)
    no_db, _ = _call(L, band, noise, band_db=False)
    no_ed, _ = _call(L, band, noise, bound=False)
    for other in (no_db, no_ed):
        np.testing.assert_array_equal(other["delta"].view(np.uint64), full["delta"].view(np.uint64))
    np.testing.assert_array_equal(no_db["ed"].view(np.uint64), full["ed"].view(np.uint64))
    assert np.all(np.isnan(no_db["band"])) and np.all(np.isnan(no_db["noise"])) and np.all(np.isnan(no_ed["ed"]))
    np.testing.assert_array_equal(no_ed["band"].view(np.uint64), full["band"].view(np.uint64))
