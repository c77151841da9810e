"""GPU: stft1024_kernel when a workgroup walks from one tile into the next across a file boundary while the
two files' means differ.  The next tile's samples are prefetched into registers one tile ahead, and a variant
of the kernel also makes their frame sums ahead and carries them over the loop's back edge
(tools/experiments/stft1024_presum_barrier_window.patch; measured slower and not shipped).
Whatever crosses the back edge, a sum taken from the wrong pair, tile, file or chunk shifts a frame's mean and
shows at bins 0 and 1.

Launches go through _lib.StftPlan.run_dev with ld = 96 (3 tiles per file) and more tiles than the device has
compute units, since below that every workgroup gets a single tile:
  static schedule   170 files = 510 tiles, 2 per workgroup on 256 CUs: every second workgroup crosses a file
                    boundary;
  chunked schedule  200 files = 300 two-tile chunks for at most 256 workgroups: some workgroups jump into
                    another chunk.  Bit-equal to the static schedule's result of the same files.
Files cycle through 65, 37, 64 and 0 frames (the last one shorter than a frame) and through five DC offsets
under Gaussian noise of sigma 30.

Every file is held to scipy's float64 spectrogram under the suite's two bars: max_k |S - R| / max_k |R| <= 1e-5
per frame, and the per-bin bound of tests/spec_signals.py with CHAIN_STFT1024 on every bin (0 and 1 included).
Every column in [frames, ld) must be exactly zero after a 0xff fill.  The float32 launch is the control: its
float sums always stay inside the loop.
"""
import functools

import numpy as np
import pytest

import spec_signals as G
from meteorgpu import _lib, dsp

pytestmark = pytest.mark.gpu

N, K, LD = 1024, 513, 96
FRAMES = (65, 37, 64, 0)
SIGMA = 30.0
DC16 = (20000.0, -15000.0, 0.0, 31000.0, -32000.0 + 4 * SIGMA)
DC8 = (200.0, 40.0, 128.0, 230.0, 25.0)  # inside 0..255; the noise clips at the ends
N_STATIC, N_CHUNKED = 170, 200

FORMS = [(512, np.int16), (256, np.int16), (768, np.int16), (512, np.uint8), (512, np.float32)]
IDS = ["h512-int16", "h256-int16", "h768-int16", "h512-uint8", "h512-float32"]


@functools.lru_cache(maxsize=None)
def _files(hop, dtname):
    """N_CHUNKED files (the static launches take the first N_STATIC); read-only"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng([1024, hop, dt.itemsize])
    out = []
    for i in range(N_CHUNKED):
        T = FRAMES[i % len(FRAMES)]
        n = G.length(N, hop, T) if T else 1000
        noise = SIGMA * rng.standard_normal(n)
        if dt == np.uint8:
            x = np.clip(np.round(noise + DC8[i % len(DC8)]), 0, 255).astype(np.uint8)
        else:
            x = np.clip(np.round(noise + DC16[i % len(DC16)]), -32768, 32767).astype(np.int16)
            if dt == np.float32:
                x = (x / 32768.0).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _refs(hop, dtname):
    """scipy's float64 spectrogram of every file that has a frame (None otherwise); read-only"""
    out = []
    for x in _files(hop, dtname):
        R = G.ref64(x, G.FS, N, N - hop, N) if len(x) >= N else None
        if R is not None:
            R.setflags(write=False)
        out.append(R)
    return tuple(out)


def _launch(files, hop, dtype, sched):
    """one launch over `files`; returns S [F][K][LD]"""
    F = len(files)
    n_pad = (max(len(x) for x in files) + 7) // 8 * 8
    frames = [(len(x) - N) // hop + 1 if len(x) >= N else 0 for x in files]
    assert max(frames) == 65 and LD == (max(frames) + 31) // 32 * 32
    es = np.dtype(dtype).itemsize
    ctx = dsp.context(0).sibling()
    try:
        ctx.set_option(_lib.OPT_STFT_SCHED, sched)
        w = dsp.hann_periodic(N).astype(np.float32)
        plan = _lib.StftPlan(ctx, N, hop, w, float(1.0 / (G.FS * (w.astype(np.float64) ** 2).sum())))
        d_x, d_off, d_len, d_out = ctx.alloc(es * F * n_pad), ctx.alloc(8 * F), ctx.alloc(8 * F), ctx.alloc(4 * F * K * LD)
        buf = np.zeros((F, n_pad), dtype)
        for i, x in enumerate(files):
            buf[i, :len(x)] = x
        d_x.upload(buf)
        d_off.upload(np.arange(F, dtype=np.int64) * n_pad)
        d_len.upload(np.array([len(x) for x in files], np.int64))
        d_out.memset(0xff)
        plan.run_dev(d_x, dtype, d_off, d_len, F, max(frames), d_out, LD)
        S = np.empty((F, K, LD), np.float32)
        d_out.download(S)
        plan.close()
    finally:
        ctx.close()
    return S


def _hold_all(tag, S, hop, dtype):
    files, refs = _files(hop, np.dtype(dtype).name), _refs(hop, np.dtype(dtype).name)
    worst_n, worst_r, at_r = 0.0, 0.0, None
    for f in range(S.shape[0]):
        T = FRAMES[f % len(FRAMES)]
        assert not S[f, :, T:].view(np.uint32).any(), f"{tag} file {f}: a column in [frames, ld) is not exactly zero"
        if T == 0:
            assert refs[f] is None
            continue
        R = refs[f]
        assert R.shape == (K, T)
        nw = G.normwise(S[f, :, :T], R)
        ratio, at = G.bound_ratio(S[f, :, :T], R, G.CHAIN_STFT1024, G.U32)
        if nw > worst_n:
            worst_n = nw
        if ratio > worst_r:
            worst_r, at_r = ratio, (f,) + at
        assert nw <= 1e-5, f"{tag} file {f} ({T} frames, {len(files[f])} samples): per-frame error {nw:.3g}"
        assert ratio <= 1.0, f"{tag} file {f}: per-bin bound exceeded {ratio:.3g} times at (bin, frame) {at}"
    print(f"PRESUM {tag}: {S.shape[0]} files, normwise {worst_n:.3e}, bound ratio {worst_r:.4f} at (file, bin, frame) {at_r}")


@pytest.mark.parametrize("hop,dtype", FORMS, ids=IDS)
def test_static_walk_crosses_files(hop, dtype):
    files = _files(hop, np.dtype(dtype).name)[:N_STATIC]
    S = _launch(list(files), hop, dtype, 1)
    _hold_all(f"static hop {hop} {np.dtype(dtype).name}", S, hop, dtype)


@pytest.mark.parametrize("hop,dtype", FORMS[:4], ids=IDS[:4])
def test_chunked_walk_equals_static(hop, dtype):
    files = list(_files(hop, np.dtype(dtype).name))
    S = _launch(files, hop, dtype, 2)
    _hold_all(f"chunked hop {hop} {np.dtype(dtype).name}", S, hop, dtype)
    S1 = _launch(files, hop, dtype, 1)
    np.testing.assert_array_equal(S.view(np.uint32), S1.view(np.uint32))
