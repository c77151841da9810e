"""stft1024_kernel after the sqrt(1/2) multiplies of its DFT8 butterflies were folded into FMAs
(csrc/fft_butterfly.h): spectrograms against scipy (oracle.dsp_oracle.spectrogram_ref)
at the project's bar, 1e-5 normwise per frame, at the frame counts where the kernel changes path --
a single frame, an odd last frame pair, one frame either side of the 32-frame tile edge, a third
tile -- for every sample type, with a DC offset (the mean's fractional part comes off bins 0 and 1
after the FFT), and over a ragged batch (the per-file tile walk).  The butterflies themselves are
checked on the CPU (tests/test_butterfly_host.py)."""
import numpy as np
import pytest

from meteorgpu import _lib, dsp
from oracle import dsp_oracle as O

pytestmark = pytest.mark.gpu

FS = 48000
N, HOP = 1024, 512
TOL = 1e-5
FRAMES = [1, 2, 3, 31, 32, 33, 65]


def _frame_err(S, ref):
    return (np.abs(S.astype(np.float64) - ref.astype(np.float64)).max(axis=0) /
            np.maximum(np.abs(ref).max(axis=0), 1e-30)).max()


def _samples(T, seed, dc=0.0, sigma=1000.0, extra=0):
    """int16 noise + a 1 kHz tone, 1024 + 512 (T - 1) (+ extra) samples: exactly T frames"""
    n = N + HOP * (T - 1) + extra
    rng = np.random.default_rng(seed)
    x = dc + sigma * rng.standard_normal(n) + 0.8 * sigma * np.sin(2 * np.pi * 1000.0 * np.arange(n) / FS)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def _as(x, dt):
    if np.dtype(dt) == np.float32:
        return (x / 32768.0).astype(np.float32)
    if np.dtype(dt) == np.uint8:
        return ((x.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return x


def _check(x, T):
    _, _, R = O.spectrogram_ref(x, FS, N)
    _, _, S = dsp.spectrogram(x, fs=FS, nperseg=N, noverlap=N - HOP)
    assert S.shape == R.shape == (N // 2 + 1, T) and S.dtype == np.float32
    err = _frame_err(S, R)
    print(f"T={T} {x.dtype.name}: per-frame error {err:.3e}")
    assert err <= TOL
    return S, R


@pytest.mark.parametrize("dt", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("T", FRAMES)
def test_edge_frame_counts(T, dt):
    _check(_as(_samples(T, seed=100 + T), dt), T)


def test_uint8_across_the_tile_edge():
    _check(_as(_samples(33, seed=7), np.uint8), 33)


@pytest.mark.parametrize("dc", [30000, -30000])
def test_dc_offset(dc):
    """a large offset over quiet noise: per frame, and bins 0 and 1 (where a residual of the mean
    would land) against each frame's mean power"""
    S, R = _check(_samples(33, seed=abs(dc) + (dc < 0), dc=dc, sigma=30.0), 33)
    mean = R.astype(np.float64).mean(axis=0)
    for k in (0, 1):
        e = np.max(np.abs(S[k].astype(np.float64) - R[k]) / mean)
        print(f"dc={dc} bin {k}: error over the frame's mean power {e:.3e}")
        assert e <= TOL, k


def test_ragged_batch():
    """three files of 33, 2 and 65 frames (the second with a tail short of a hop) in one launch: the
    workgroups walk from file to file over full, partial and empty tiles; padding columns are zero"""
    ctx = dsp.context(0)
    xs = [_samples(33, seed=1), _samples(2, seed=2, extra=100), _samples(65, seed=3)]
    lens = [len(x) for x in xs]
    F = len(xs)
    offs = np.cumsum([0] + [(m + 7) // 8 * 8 for m in lens[:-1]]).astype(np.int64)
    host = np.zeros(int(offs[-1] + lens[-1] + 8), np.int16)
    for o, x in zip(offs, xs):
        host[o:o + len(x)] = x
    bufs = []
    w = dsp.hann_periodic(N).astype(np.complex64)
    scale = float(np.real(1.0 / (FS * (w * w).sum())))
    plan = _lib.StftPlan(ctx, N, HOP, w.real.astype(np.float32), scale)
    try:
        d_x, d_off, d_len = ctx.alloc(host.nbytes), ctx.alloc(F * 8), ctx.alloc(F * 8)
        bufs += [d_x, d_off, d_len]
        d_x.upload(host)
        d_off.upload(offs)
        d_len.upload(np.array(lens, np.int64))
        T = [plan.frames(m) for m in lens]
        assert T == [33, 2, 65]
        K, ld = N // 2 + 1, 96
        d_spec = ctx.alloc(F * K * ld * 4)
        bufs.append(d_spec)
        d_spec.upload(np.full(F * K * ld, np.nan, np.float32))
        plan.run_dev(d_x, np.int16, d_off, d_len, F, max(T), d_spec, ld)
        spec = np.empty((F, K, ld), np.float32)
        d_spec.download(spec)
    finally:
        plan.close()
        for b in bufs:
            b.free()
    for i in range(F):
        _, _, R = O.spectrogram_ref(xs[i], FS, N)
        err = _frame_err(spec[i, :, :T[i]], R)
        print(f"file {i} ({T[i]} frames): per-frame error {err:.3e}")
        assert err <= TOL
        assert not spec[i, :, T[i]:].any()
