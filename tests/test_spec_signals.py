"""CPU: the spectrogram signal classes, references and metrics of tests/spec_signals.py keep their
conditions -- what tests/test_gpu_spectrogram_bins.py relies on and cannot check on the device:

* the float32 CPU pipeline (ref32_cpu, pocketfft in single precision) stays far inside the per-bin
  bound on every class, at a chain of 33 (below every kernel's derived chain): the inputs leave the
  bound to the kernel under test;
* the per-bin bound has teeth where the older normwise bar has none: two corruptions of a -80 dB bin
  pass 1e-5 normwise and miss the bound, by 627 times (5e-6 of the peak added) and by 29 times (the
  bin swapped with its neighbour two bins away: the whole tone's amplitude over the bound);
* carrier_weak's weak tone is 79-81 dB under the carrier in the float64 reference;
* the long-double reference of the float64 plans agrees with scipy's float64 spectrogram;
* the chain constants are the documented counts.
"""
import numpy as np
import pytest

import spec_signals as G

SIZES = [16, 64, 1024, 4096]
FRAMES = 5


def _case(cls, N, dtype=np.int16):
    if cls in ("f32_dc", "f64_dc"):
        dtype = np.float32 if cls == "f32_dc" else np.float64
    x = G.signal(cls, N, N // 2, FRAMES, dtype)
    return x, (G.FS, N, N // 2, N)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("cls", G.CLASSES)
def test_cpu_float32_pipeline_far_inside_the_bound(cls, N):
    x, shape = _case(cls, N)
    R, S = G.ref64(x, *shape), G.ref32_cpu(x, *shape)
    assert S.shape == R.shape == (N // 2 + 1, (len(x) - N) // (N // 2) + 1) and S.dtype == np.float32
    ratio, at = G.bound_ratio(S, R, 33, G.U32)
    print(f"ref32_cpu {cls} N={N}: bound ratio {ratio:.4f} at (bin, frame) {at}")
    assert ratio <= 0.1
    if cls == "const":
        assert not R.any() and not S.any() and ratio == 0.0


def test_weak_tone_is_80_db_down():
    for N in (1024, 4096):
        x, shape = _case("carrier_weak", N)
        R = G.ref64(x, *shape)
        db = 10 * np.log10(R[G.weak_bin(N)] / R[G.carrier_bin(N)])
        print(f"carrier_weak N={N}: weak bin {db.min():.2f} .. {db.max():.2f} dB under the carrier")
        assert np.all((db >= -81.0) & (db <= -79.0))
        assert np.array_equal(np.argmax(R, axis=0), np.full(R.shape[1], G.carrier_bin(N)))


@pytest.mark.parametrize("corruption", ["add", "swap"])
def test_bound_sees_what_the_normwise_bar_does_not(corruption):
    N = 1024
    x, shape = _case("carrier_weak", N)
    R = G.ref64(x, *shape)
    S = G.ref32_cpu(x, *shape).copy()
    k = G.weak_bin(N)
    clean, _ = G.bound_ratio(S, R, 33, G.U32)
    if corruption == "add":
        S[k] += np.float32(5e-6) * S.max(axis=0)
    else:
        S[[k, k + 2]] = S[[k + 2, k]]
    old = G.normwise(S, R)
    ratio, at = G.bound_ratio(S, R, 33, G.U32)
    print(f"{corruption}: normwise {old:.3e}, bound ratio {ratio:.1f} at (bin, frame) {at} (clean {clean:.4f})")
    assert old <= 1e-5  # the older bar passes it
    # the per-bin bound does not.  The swap moves the whole weak tone: an amplitude error of
    # (3 / 30000) sqrt(2/3) of the frame's 2-norm (2/3 of a Hann-windowed bin-centred tone's power sits
    # in its peak bin) against sqrt 2 * 33 u sqrt 1.001 = 2.78e-6 of it: 29.3 times the bound, the
    # most this corruption can reach at chain 33
    assert ratio > (100.0 if corruption == "add" else 25.0)
    assert clean <= 0.1


@pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)
@pytest.mark.parametrize("N", [16, 1024])
def test_long_double_reference_agrees_with_scipy(N):
    for dtype in (np.int32, np.float64):
        x, shape = _case("fullscale_noise", N, dtype)
        R, L = G.ref64(x, *shape), G.ref_ld(x, *shape)
        assert L.dtype == np.longdouble and L.shape == R.shape
        err = G.normwise(R, L)
        ratio, _ = G.bound_ratio(R, L, G.chain_any(N), G.U64)
        print(f"ref_ld N={N} {np.dtype(dtype).name}: scipy float64 normwise {err:.3e}, bound ratio {ratio:.4f}")
        assert err <= 1e-12
        assert ratio <= 0.5  # scipy's float64 pipeline is itself inside the float64 plans' bound


def test_metrics_on_zero_frames():
    R = np.zeros((9, 3))
    R[:, 1] = 1.0
    S = R.copy()
    assert G.bound_ratio(S, R, 33, G.U32)[0] == 0.0 and not G.rms_err(S, R).any()
    S[4, 2] = 1e-30  # power where the reference has none
    ratio, at = G.bound_ratio(S, R, 33, G.U32)
    assert ratio == np.inf and at == (4, 2)
    S[4, 2] = np.nan
    assert G.bound_ratio(S, R, 33, G.U32)[0] == np.inf


def test_chain_constants_are_the_documented_counts():
    assert G.CHAIN_STFT1024 == 35
    assert G.CHAIN_TILED == {256: 31, 512: 32, 1024: 36, 2048: 41}
    assert G.CHAIN_ANY == {16: 17, 32: 18, 64: 23, 128: 24, 256: 29, 512: 30, 1024: 36, 2048: 37, 4096: 42, 8192: 43,
                           16384: 48}
