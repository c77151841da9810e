"""GPU: the spectrogram kernel's energy partials (cstft4096_kernel<EN>, `etot`) against Parseval.

The fp32 delta bound of the C5 certificate takes each frame's total power from 16 partials the
spectrogram kernel writes beside the spectrogram; csrc/cstft.hip claims their sum, times 1.001, is
an upper bound of the frame's total power.  The reference needs no FFT:

    S_ref[t] = N * sum_n |(z_n - mean) w_n|^2 / (fs * sum w^2)          (float64, time domain)

* lower bound (the kernel's claim):  1.001 * sum_i etot[i][s*max_frames + t] >= S_ref[s][t];
* upper bound:  sum_i etot[i][...] <= 1.001 * sum of S_ref over the same stream's frames within 3 of
  t.  It holds for any scheme that bounds a frame by a group of at most 4 consecutive frames (the
  kernel's earlier form: per-thread maxima over such a group), wherever the scheduler started the
  group; a stale or foreign value (another stream's, a frame further away) fails it;
* the partials are the frame's own:  sum_i etot[i][...] <= 1.001 * S_ref[s][t].  With a group's
  maximum instead, a silent frame beside a loud one gets ed = +inf, and every threshold whose
  window reads it turns uncertain (test_gpu_certify_stress.py, `dropout`).

The input changes level by up to 10^4 every 3 hops (iq_signals.levels), so a partial stored for the
wrong frame of a group shows in one direction or the other.  Ragged batches (61, 56, 0, 2 and 1
frames in one launch), hops 1024 (the guided schedule, also with workgroup slots reserved, also with
the frame sums given), 2048 and 1096, int16 and float32; one launch of ~9000 frames in which every
workgroup owns several groups and the guided schedule reaches its 16-frame chunks.
"""
import numpy as np
import pytest

import iq_signals as G
from meteorgpu import _lib, iq
from meteorgpu.dsp import context

pytestmark = pytest.mark.gpu

FS, N = G.FS, G.N


def frame_power_ref(z, hop):
    """S_ref of every frame of the complex128 stream z"""
    T = (len(z) - N) // hop + 1 if len(z) >= N else 0
    k = np.arange(N)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / N)
    c = N / (FS * np.sum(w * w))
    out = np.empty(T, np.float64)
    if T:
        V = np.lib.stride_tricks.sliding_window_view(z, N)[::hop]
        for a in range(0, T, 256):
            v = V[a: a + 256]
            v = (v - v.mean(axis=1, keepdims=True)) * w
            out[a: a + 256] = c * (v.real ** 2 + v.imag ** 2).sum(axis=1)
    return out


def _run(kind, hop, lens, n, seed, reserve=0, given_sums=False, spec_rows=None):
    """one launch over len(lens) streams of capacity n; returns (etot sums [ns][T], S_ref list,
    frames list, spectrogram [ns][T][N] or None)"""
    ns = len(lens)
    dt = np.int16 if kind == "int16" else np.float32
    streams = [G.levels(n, kind, hop, seed + s) for s in range(ns)]
    ctx = context(0).sibling()
    try:
        if reserve:
            ctx.set_option(_lib.OPT_CSTFT_RESERVE, reserve)
        b = iq.IQBatch(ctx, ns, n, FS, N, N - hop, dtype=dt)
        for s, (i, q) in enumerate(streams):
            x = np.empty(2 * n, dt)
            x[0::2], x[1::2] = i, q
            b.upload(s, x)
        b.d_len.upload(np.array(lens, np.int64))
        T = b.T
        nf = [(ln - N) // hop + 1 if ln >= N else 0 for ln in lens]
        stride = int(ctx.lib.msd_cstft_energy_stride(ns, T))
        assert stride >= ns * T and stride % 4 == 0
        etot = ctx.alloc(16 * 4 * stride)
        etot.upload(np.full(16 * stride, np.nan, np.float32))  # a frame the kernel skips stays NaN
        bufs = [etot]
        fsum = None
        if given_sums:  # the exact delta step's frame sums, stream by stream (as test_iq.py takes them)
            fsum, d, e = ctx.alloc(16 * ns * T), ctx.alloc(8 * ns * T), ctx.alloc(8 * ns * T)
            bufs += [fsum, d, e]
            es = dt().itemsize
            for s in range(ns):
                if nf[s]:
                    _lib.iq_delta64_dev(ctx, b.d_x.at(s * 2 * b.n_pad * es), b.code, lens[s], N, hop, float(FS),
                                        G.bins(G.BAND), G.bins(G.NOISE), np.array([[0, nf[s]]], np.int64),
                                        d.at(8 * s * T), e.at(8 * s * T), frame_sums=fsum.at(16 * s * T))
        b.run(etot, fsums=fsum)
        e = np.empty((16, stride), np.float32)
        etot.download(e)
        spec = None
        if spec_rows is None:
            spec = np.empty((ns, T, N), np.float32)
            b.d_out.download(spec)
        else:  # a large launch: only the first frames past each stream's end
            spec = [b.frames(s, nf[s], min(spec_rows, T - nf[s])) for s in range(ns)]
        for buf in bufs:
            buf.free()
        b.close()
    finally:
        ctx.close()
    esum = e.astype(np.float64).sum(axis=0)[: ns * T].reshape(ns, T)
    ref = [frame_power_ref((i[:ln].astype(np.float64) + 1j * q[:ln].astype(np.float64)), hop)
           for (i, q), ln in zip(streams, lens)]
    return esum, ref, nf, spec


def _check(esum, ref, nf):
    worst_lo = worst_hi = 0.0
    for s, (r, k) in enumerate(zip(ref, nf)):
        assert r.size == k
        if not k:
            continue
        got = esum[s, :k]
        assert np.all(np.isfinite(got)), f"stream {s}: partials not written at frames {np.flatnonzero(~np.isfinite(got))[:8]}"
        pad = np.concatenate([np.zeros(3), r, np.zeros(3)])
        near = np.lib.stride_tricks.sliding_window_view(pad, 7).sum(axis=1)  # frames within 3, same stream
        lo = r / (1.001 * got)
        hi = got / (1.001 * near)
        worst_lo, worst_hi = max(worst_lo, lo.max()), max(worst_hi, hi.max())
        print(f"stream {s}: {k} frames, max S_ref / (1.001 etot) {lo.max():.6f}, max etot / (1.001 near) {hi.max():.6f}, "
              f"median etot / S_ref {np.median(got / r):.3f}")
        assert np.all(1.001 * got >= r), f"stream {s}: not an upper bound at frames {np.flatnonzero(1.001 * got < r)[:8]}"
        assert np.all(got <= 1.001 * near), f"stream {s}: stale or foreign partial at frames {np.flatnonzero(got > 1.001 * near)[:8]}"
        assert np.all(got <= 1.001 * r), f"stream {s}: not the frame's own energy at frames {np.flatnonzero(got > 1.001 * r)[:8]}"
    return worst_lo, worst_hi


RAGGED_FRAMES = (61, 56, 0, 2, 1)


# (the given frame sums come from the int16 exact delta step: int16 only)
RAGGED_CASES = [(v, k) for v in ("hop1024", "hop1024_reserve8", "hop2048", "hop1096") for k in ("int16", "float32")]
RAGGED_CASES.append(("hop1024_given_sums", "int16"))


@pytest.mark.parametrize("variant,kind", RAGGED_CASES)
def test_energy_partials_ragged(variant, kind):
    hop = {"hop2048": 2048, "hop1096": 1096}.get(variant, 1024)
    n = (RAGGED_FRAMES[0] - 1) * hop + N
    lens = [(k - 1) * hop + N + (hop // 3 if k > 1 else 0) if k else N - 1 for k in RAGGED_FRAMES]
    lens[0] = n
    esum, ref, nf, spec = _run(kind, hop, lens, n, seed=hop + (kind == "int16"),
                               reserve=8 if variant == "hop1024_reserve8" else 0,
                               given_sums=variant == "hop1024_given_sums")
    assert tuple(nf) == RAGGED_FRAMES
    _check(esum, ref, nf)
    for s, k in enumerate(nf):  # frames past a stream's end read zero; those before it do not
        assert not spec[s, k:].any()
        assert np.all(spec[s, :k].astype(np.float64).sum(axis=1) > 0)


def test_energy_partials_large():
    """~9000 frames in 3 ragged streams, int16, hop 1024"""
    T = 3000
    n = (T - 1) * 1024 + N
    lens = [n, n - 300_001, 1_234_567]
    esum, ref, nf, past = _run("int16", 1024, lens, n, seed=77, spec_rows=8)
    assert sum(nf) > 6900 and nf[0] == T
    _check(esum, ref, nf)
    for rows in past:
        assert not rows.any()
