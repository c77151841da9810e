"""CPU: the premises of the any-frame-length I/Q spectrogram tests (tests/iq_any_signals.py), no GPU.

1. ABI: msd_cstft_chain is host only -- fails cleanly on null and unsupported shapes, returns 37 at
   4096 / 4096 and for every nfft in 16 .. 8192 the Python recount of the documented per-pass table, so
   narrowing the C++ constant fails here; msd_cstft_plan_create_ex and msd_cstft_nfft are exported and bound.
2. The yardstick -- a float32 numpy pipeline -- stays inside the per-frame and per-bin bars on every case
   of the GPU list: the bars are attainable from the references alone.
3. The bars bite: 5e-6 of the peak added to a -80 dB bin, that bin swapped with its neighbour, the samples
   shifted by one each break the per-bin bar; a frame's energy replaced by its neighbour's breaks the
   energy bars; detrending after the zero padding breaks the per-bin bar at 1000 / 1024.
4. For the white class the documented delta bound with the generic chain is finite on every frame of
   every shape, so the GPU tests can demand a finite bound everywhere.
"""
import ctypes

import numpy as np
import pytest

import iq_any_signals as A
from meteorgpu import _lib


# ------------------------------------------------------------------------------- 1. ABI
def test_chain_abi_fails_cleanly_without_gpu():
    lib = _lib.load()
    v = ctypes.c_double(-1.0)
    assert lib.msd_cstft_chain(1024, 1024, None) == _lib.MSD_ERR_INVALID
    assert b"msd_cstft_chain" in lib.msd_last_error()
    for nperseg, nfft in ((1024, 16384), (8, 8), (24, 24), (1000, 1000), (16, 0), (16, -16)):
        assert lib.msd_cstft_chain(nperseg, nfft, ctypes.byref(v)) == _lib.MSD_ERR_UNSUPPORTED, (nperseg, nfft)
        assert v.value == 0.0 and b"8192" in lib.msd_last_error()
    for nperseg, nfft in ((0, 16), (17, 16), (-1, 1024)):
        assert lib.msd_cstft_chain(nperseg, nfft, ctypes.byref(v)) == _lib.MSD_ERR_INVALID, (nperseg, nfft)
    with pytest.raises(_lib.MsdError) as ei:
        _lib.cstft_chain(1024, 16384)
    assert ei.value.code == _lib.MSD_ERR_UNSUPPORTED


def test_chain_values_match_the_documented_table():
    assert _lib.cstft_chain(4096, 4096) == 37.0 == _lib.cstft_chain(4096)
    table = {16: 12, 32: 17, 64: 18, 128: 23, 256: 24, 512: 29, 1024: 30, 2048: 36, 4096: 37, 8192: 42}
    for L in range(4, 14):
        nfft = 1 << L
        for nperseg in {1, 3, nfft // 2 + 1, nfft - 1, nfft}:
            if nperseg == nfft == 4096:
                continue
            got = _lib.cstft_chain(nperseg, nfft)
            assert got == A.chain_recount(nperseg, nfft) == table[nfft], (nperseg, nfft, got)
    # the generic kernel at 4096 counts the same three radix-16 passes as cstft4096_kernel
    assert _lib.cstft_chain(4000, 4096) == 37.0


def test_new_entry_points_exported_and_bound():
    lib = _lib.load()
    for name in ("msd_cstft_plan_create_ex", "msd_cstft_nfft", "msd_cstft_chain"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.OPT_GENERIC_CSTFT == 12
    out = ctypes.c_void_p()
    assert lib.msd_cstft_plan_create_ex(None, 1024, 1024, 256, None, 1.0, ctypes.byref(out)) == _lib.MSD_ERR_INVALID
    assert lib.msd_cstft_nfft(None) == 0


# ------------------------------------------------------------------------------- 2. the yardstick
@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_yardstick_inside_the_bars(case):
    nperseg, nfft, hop, kind = case
    chain = A.chain_recount(nperseg, nfft)
    worst_bin = worst_frame = 0.0
    for nm in A.classes(kind):
        i, q, R = A.case_data(nperseg, nfft, hop, kind, nm)
        Y = A.yardstick(A.as_complex(i, q), A.FS, nperseg, nfft, hop).astype(np.float64)
        assert Y.shape == R.shape == (A.FRAMES, nfft)
        worst_bin = max(worst_bin, A.bin_ratio(Y, R, chain).max())
        worst_frame = max(worst_frame, A.frame_err(Y, R).max())
        assert not Y[~R.any(axis=1)].any(), nm
    print(f"{A.case_id(case)}: yardstick per-bin ratio {worst_bin:.3f} (margin {1 / max(worst_bin, 1e-300):.1f}x), "
          f"per-frame {worst_frame:.2e}")
    assert worst_bin <= 1.0 and worst_frame <= A.FRAME_TOL


# ------------------------------------------------------------------------------- 3. the bars bite
BITE = (1024, 1024, 256, "int16")


def test_per_bin_bar_catches_a_small_bin_error():
    nperseg, nfft, hop, kind = BITE
    _, _, R = A.case_data(nperseg, nfft, hop, kind, "tone80")
    chain = A.chain_recount(nperseg, nfft)
    kt = nfft // 8 + 3
    peak = R.max(axis=1)
    assert np.all(R[:, kt] < 2e-8 * peak) and np.all(R[:, kt] > 0.5e-8 * peak)  # the -80 dB bin
    S = R.copy()
    S[:, kt] += 5e-6 * peak
    assert A.frame_err(S, R).max() <= A.FRAME_TOL        # the per-frame bar does not see it
    assert A.bin_ratio(S, R, chain)[:, kt].min() > 1.0   # the per-bin bar does, on every frame
    S = R.copy()
    S[:, [kt, kt + 1]] = S[:, [kt + 1, kt]]
    assert A.frame_err(S, R).max() <= A.FRAME_TOL
    assert A.bin_ratio(S, R, chain).max(axis=1).min() > 1.0


def test_bars_catch_a_one_sample_shift():
    nperseg, nfft, hop, kind = BITE
    i, q, R = A.case_data(nperseg, nfft, hop, kind, "white")
    z = A.as_complex(i, q)
    S = A.reference(np.concatenate([z[1:], z[:1]]), A.FS, nperseg, nfft, hop)
    assert A.bin_ratio(S, R, A.chain_recount(nperseg, nfft)).max(axis=1).min() > 1.0
    assert A.frame_err(S, R).min() > A.FRAME_TOL


def test_energy_bars_catch_a_neighbours_partials():
    nperseg, nfft, hop, kind = BITE
    i, q, _ = A.case_data(nperseg, nfft, hop, kind, "levels")
    e = A.energy_ref(A.as_complex(i, q), A.FS, nperseg, nfft, hop)
    assert A.energy_ok(e, e).all() and A.energy_ok(e * 1.0005, e).all() and A.energy_ok(e / 1.0005, e).all()
    assert not A.energy_ok(e * 1.002, e).any() and not A.energy_ok(e / 1.002, e).any()
    for shift in (1, -1):  # every level step (every 3 hops) shows
        bad = ~A.energy_ok(np.roll(e, shift), e)
        assert bad.sum() >= A.FRAMES // 3 - 1, bad.sum()


@pytest.mark.parametrize("kind,name", [("int16", "dc_noise"), ("float32", "f32_dc"), ("int16", "impulses")])
def test_per_bin_bar_catches_detrend_after_padding(kind, name):
    nperseg, nfft, hop = 1000, 1024, 250
    i, q, R = A.case_data(nperseg, nfft, hop, kind, name)
    z = A.as_complex(i, q)
    chain = A.chain_recount(nperseg, nfft)
    good = A.yardstick(z, A.FS, nperseg, nfft, hop).astype(np.float64)
    slip = A.yardstick(z, A.FS, nperseg, nfft, hop, detrend_after_padding=True).astype(np.float64)
    assert A.bin_ratio(good, R, chain).max() <= 1.0
    nz = R.any(axis=1)
    assert A.bin_ratio(slip, R, chain)[nz].max(axis=1).min() > 1.0


# ------------------------------------------------------------------------------- 4. ed stays finite
def _bands(nfft):
    w = nfft // 64
    return max(2, nfft // 8), max(2, nfft // 8) + w, -(nfft // 4) - w, -(nfft // 4)


@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_white_delta_bound_is_finite(case):
    nperseg, nfft, hop, kind = case
    _, _, R = A.case_data(nperseg, nfft, hop, kind, "white")
    chain = max(_lib.cstft_chain(nperseg, nfft), A.chain_recount(min(nperseg, nfft - 1), nfft))
    ed = A.model_ed(R, nfft, chain, *_bands(nfft))
    print(f"{A.case_id(case)}: chain {chain:g}, ed max {ed.max():.3e} dB "
          f"(2 chain u sqrt(nfft) = {2 * chain * A.U32 * np.sqrt(nfft):.2e})")
    assert np.isfinite(ed).all() and ed.max() < 0.5
