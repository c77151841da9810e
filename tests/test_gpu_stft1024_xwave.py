"""GPU: stft1024_kernel's pass 3 by bin (a half-wave owns a conjugate pair of pass-3 butterflies for
the tile's 32 frames and stores its 16 or 17 rows from registers), called the way BatchPipeline calls
it -- _lib.StftPlan.run_dev with offsets, lengths and ld -- so that batches dsp.spectrogram never
builds are reached: files that end inside a tile, on its edge, or before their first frame.

Every file of every launch is held to scipy's float64 spectrogram of the same samples under the
suite's two bars: max_k |S - R| / max_k |R| <= 1e-5 per frame, and on every bin of every frame the
per-bin bound of tests/spec_signals.py with CHAIN_STFT1024.  Every column in [frames, ld) must be
exactly zero (the output buffer is filled with 0xff bytes before each launch).
"""
import functools

import numpy as np
import pytest

import spec_signals as G
from meteorgpu import _lib, dsp

pytestmark = pytest.mark.gpu

N, K = 1024, 513
ROW_BINS = (0, 1, 31, 32, 33, 63, 64, 96, 255, 256, 257, 448, 480, 511, 512)


def _launch(files, hop, dtype, sched=1):
    """one launch over `files` (1-D sample arrays of `dtype`); returns S [F][K][ld] and the frame counts"""
    F = len(files)
    n_pad = (max(max(len(x) for x in files), 8) + 7) // 8 * 8
    frames = [(len(x) - N) // hop + 1 if len(x) >= N else 0 for x in files]
    ld = max(32, (max(frames) + 31) // 32 * 32)
    es = np.dtype(dtype).itemsize
    ctx = dsp.context(0).sibling()
    try:
        ctx.set_option(_lib.OPT_STFT_SCHED, sched)
        w = dsp.hann_periodic(N).astype(np.float32)
        plan = _lib.StftPlan(ctx, N, hop, w, float(1.0 / (G.FS * (w.astype(np.float64) ** 2).sum())))
        d_x, d_off, d_len, d_out = ctx.alloc(es * F * n_pad), ctx.alloc(8 * F), ctx.alloc(8 * F), ctx.alloc(4 * F * K * ld)
        buf = np.zeros((F, n_pad), dtype)
        for i, x in enumerate(files):
            buf[i, :len(x)] = x
        d_x.upload(buf)
        d_off.upload(np.arange(F, dtype=np.int64) * n_pad)
        d_len.upload(np.array([len(x) for x in files], np.int64))
        d_out.memset(0xff)
        plan.run_dev(d_x, dtype, d_off, d_len, F, max(frames), d_out, ld)
        S = np.empty((F, K, ld), np.float32)
        d_out.download(S)
        plan.close()
    finally:
        ctx.close()
    return S, frames


def _hold(tag, S, x, T, hop):
    """file spectrogram S [K][ld] of samples x with T frames: the pad columns zero, the rest within both bars"""
    assert not S[:, T:].view(np.uint32).any(), f"{tag}: a column in [frames, ld) is not exactly zero"
    if T == 0:
        return
    R = G.ref64(x, G.FS, N, N - hop, N)
    assert R.shape == (K, T)
    old = G.normwise(S[:, :T], R)
    ratio, at = G.bound_ratio(S[:, :T], R, G.CHAIN_STFT1024, G.U32)
    print(f"XWAVE {tag}: frames {T} normwise {old:.3e} bound ratio {ratio:.4f} at {at}")
    assert old <= 1e-5, f"{tag}: per-frame error {old:.3g}"
    assert ratio <= 1.0, f"{tag}: per-bin bound exceeded {ratio:.3g} times at (bin, frame) {at}"


@pytest.mark.parametrize("cls", G.NOISE_LIKE)
@pytest.mark.parametrize("frames", [1, 2, 31, 32, 33, 64, 65])
def test_tile_edges(frames, cls):
    x = G.signal(cls, N, 512, frames, np.int16)
    S, fr = _launch([x], 512, np.int16)
    assert fr == [frames]
    _hold(f"edges {cls} {frames}", S[0], x, frames, 512)


@functools.lru_cache(maxsize=None)
def _unequal(hop, dtname):
    """four files in one launch: shorter than one frame, 37 frames (ends inside the second tile, its last
    pair without a second frame), 64 frames (ends on a tile edge), 65 frames; read-only"""
    dt = np.dtype(dtname)
    files = [G.cast(G.samples("fullscale_noise", N, 1000), dt),
             G.signal("fullscale_noise", N, hop, 37, dt),
             G.signal("carrier_weak", N, hop, 64, dt),
             G.signal("fullscale_noise", N, hop, 65, dt)]
    for f in files:
        f.setflags(write=False)
    return tuple(files)


@pytest.mark.parametrize("hop,dtype,sched", [(512, np.int16, 1), (256, np.int16, 1), (768, np.int16, 1),
                                             (512, np.float32, 1), (512, np.uint8, 1), (512, np.int16, 2)],
                         ids=["h512-int16", "h256-int16", "h768-int16", "h512-float32", "h512-uint8", "h512-int16-chunked"])
def test_unequal_files(hop, dtype, sched):
    files = _unequal(hop, np.dtype(dtype).name)
    S, fr = _launch(list(files), hop, dtype, sched)
    assert fr == [0, 37, 64, 65] and S.shape == (4, K, 96)
    for i, (x, T) in enumerate(zip(files, fr)):
        _hold(f"unequal hop {hop} {np.dtype(dtype).name} sched {sched} file {i}", S[i], x, T, hop)
    if sched == 2:  # the chunked schedule: bit-identical to the default one
        S1, _ = _launch(list(files), hop, dtype, 1)
        np.testing.assert_array_equal(S.view(np.uint32), S1.view(np.uint32))


def test_every_row_lands_in_its_row():
    """one tone per file, its amplitude ramped over the 33 frames: the rows of slot 0 (0, 32, 64, 96, 256,
    448, 480, 512), both members of ordinary pairs (1 / 511 and 63, 31 / 33 / 255 / 257) and bin 256"""
    frames = 33
    n = G.length(N, 512, frames)
    i = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(256)
    files = [np.round((400.0 + 24000.0 * i / n) * np.cos(2 * np.pi * k * i / N + (0.0 if k in (0, 512) else rng.uniform(0, 2 * np.pi)))
                      ).astype(np.int16) for k in ROW_BINS]
    S, fr = _launch(files, 512, np.int16)
    assert fr == [frames] * len(ROW_BINS)
    for f, k in enumerate(ROW_BINS):
        _hold(f"row {k}", S[f], files[f], frames, 512)
        if k:  # bin 0's tone is what the detrend removes
            assert (S[f, :, :frames].argmax(axis=0) == k).all(), f"the tone at bin {k} peaks elsewhere"
            assert (np.diff(S[f, k, :frames]) > 0).all(), f"row {k} does not follow the ramp frame by frame"
