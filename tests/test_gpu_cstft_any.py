"""GPU: the I/Q spectrogram at any frame length (cstft_any_kernel) against scipy's float64 spectrogram.

Shapes (tests/iq_any_signals.py SHAPES): the issue's list.  The kernel switches path with log2 nfft only
-- frames per workgroup trip (256 / (nfft / 16)), the leading radix 2 / 4 / 8 pass, the LDS twiddle tables
(nfft 512 .. 8192), the output tile (nfft < 1024), 512 threads (8192) -- and the list holds every nfft
from 16 to 8192, so no value is added for the mapping; nperseg < nfft adds the zero padding (17 / 32:
threads that hold only padding; 3 / 8192: all but one).

Per case one launch holds every input class as a stream of its own (FRAMES frames each), with the
energy partials.  Bars (iq_any_signals): per frame max |S - R| / max |R| <= 1e-5; per bin, no bin
excluded, |sqrt S - sqrt R| <= chain u sqrt(1.001 sum R) + 3 u sqrt R with chain from msd_cstft_chain;
exact zeros where the reference is exactly zero; on the noise-like classes the per-frame rms of the
amplitude error within 4x the float32 numpy pipeline's; every frame's 16 partials within 1.001 of the
time-domain energy, both ways.
"""
import numpy as np
import pytest

import iq_any_signals as A
from meteorgpu import _lib, iq
from meteorgpu.dsp import context

pytestmark = pytest.mark.gpu

FS = A.FS


def _cus():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256  # MI355X


def _launch(nperseg, nfft, hop, kind, streams, lens=None, etot=True, generic=False, rows=None):
    """one launch over the streams [(i, q)] (capacity: the longest); -> (spec [ns][T][nfft] or the
    rows asked for, e [16][stride] or None, T)"""
    ns = len(streams)
    dt = np.int16 if kind == "int16" else np.float32
    n = max(len(i) for i, _ in streams)
    lens = [len(i) for i, _ in streams] if lens is None else lens
    ctx = context(0).sibling()
    try:
        if generic:
            ctx.set_option(_lib.OPT_GENERIC_CSTFT, 1)
        b = iq.IQBatch(ctx, ns, n, FS, nperseg, nperseg - hop, dtype=dt, nfft=nfft)
        assert b.N == nfft and b.plan.nfft == nfft
        for s, (i, q) in enumerate(streams):
            x = np.empty(2 * len(i), dt)
            x[0::2], x[1::2] = i, q
            b.upload(s, x)
        b.d_len.upload(np.array(lens, np.int64))
        T = b.T
        e, d_e = None, None
        if etot:
            stride = int(ctx.lib.msd_cstft_energy_stride(ns, T))
            d_e = ctx.alloc(16 * 4 * stride)
            d_e.upload(np.full(16 * stride, np.nan, np.float32))  # a frame the kernel skips stays NaN
        b.run(d_e)
        if etot:
            e = np.empty((16, stride), np.float32)
            d_e.download(e)
            d_e.free()
        if rows is None:
            spec = np.empty((ns, T, nfft), np.float32)
            b.d_out.download(spec)
        else:
            spec = [np.stack([b.frames(s, t, 1)[0] for t in ts]) if len(ts) else np.zeros((0, nfft), np.float32)
                    for s, ts in enumerate(rows)]
        b.close()
    finally:
        ctx.close()
    return spec, e, T


def _check_bars(tag, S, R, chain):
    fe = A.frame_err(S, R)
    br = A.bin_ratio(S, R, chain)
    print(f"{tag}: frame err {fe.max():.3e}, largest per-bin ratio {br.max():.3f}")
    zero = ~R.any(axis=1)
    assert not S[zero].any(), f"{tag}: nonzero output where the reference is exactly zero"
    assert fe.max() <= A.FRAME_TOL, f"{tag}: per-frame error {fe.max():.3e}"
    assert br.max() <= 1.0, f"{tag}: per-bin ratio {br.max():.3f} at {np.unravel_index(br.argmax(), br.shape)}"
    return br.max()


def _check_energy(tag, esum, z, nperseg, nfft, hop):
    ref = A.energy_ref(z, FS, nperseg, nfft, hop)
    assert np.all(np.isfinite(esum)), f"{tag}: partials not written"
    ok = A.energy_ok(esum, ref)
    assert ok.all(), f"{tag}: energy bars at frames {np.flatnonzero(~ok)[:8]}: {esum[~ok][:4]} vs {ref[~ok][:4]}"


@pytest.mark.parametrize("case", A.cases(), ids=A.case_id)
def test_signal_classes(case):
    nperseg, nfft, hop, kind = case
    names = A.classes(kind)
    data = [A.case_data(nperseg, nfft, hop, kind, nm) for nm in names]
    generic = nperseg == 4096 and nfft == 4096
    chain = _lib.cstft_chain(nperseg, nfft)
    assert chain == A.chain_recount(nperseg, nfft)
    if generic:  # the generic kernel's own count at 4096 (the bound takes the larger of the two)
        chain = max(chain, A.chain_recount(4095, 4096))
    spec, e, T = _launch(nperseg, nfft, hop, kind, [(i, q) for i, q, _ in data], generic=generic)
    assert T == A.FRAMES
    esum = e.astype(np.float64).sum(axis=0)[: len(names) * T].reshape(len(names), T)
    worst = 0.0
    for s, (nm, (i, q, R)) in enumerate(zip(names, data)):
        tag = f"{A.case_id(case)} {nm}"
        S = spec[s].astype(np.float64)
        assert R.shape == S.shape
        worst = max(worst, _check_bars(tag, S, R, chain))
        z = A.as_complex(i, q)
        _check_energy(tag, esum[s], z, nperseg, nfft, hop)
        if nm in A.NOISE_LIKE:
            Y = A.yardstick(z, FS, nperseg, nfft, hop).astype(np.float64)
            mine, theirs = A.amp_rms(S, R), A.amp_rms(Y, R)
            print(f"{tag}: rms ratio to the float32 numpy pipeline {np.max(mine / theirs):.3f}")
            assert np.all(mine <= A.RMS_FACTOR * theirs), f"{tag}: rms {np.max(mine / theirs):.2f}x the yardstick's"
    print(f"{A.case_id(case)}: largest per-bin ratio over the classes {worst:.3f} (chain {chain:g})")


RAGGED_FRAMES = (61, 56, 0, 2, 1)


@pytest.mark.parametrize("with_etot", [True, False], ids=["etot", "no_etot"])
@pytest.mark.parametrize("shape", [(1024, 1024, 256), (8192, 8192, 2048)], ids=["1024", "8192"])
def test_ragged_batch(shape, with_etot):
    nperseg, nfft, hop = shape
    n = A.n_samples(nperseg, hop, RAGGED_FRAMES[0])
    lens = [A.n_samples(nperseg, hop, k) + (hop // 3 if k > 1 else 0) if k else nperseg - 1 for k in RAGGED_FRAMES]
    lens[0] = n
    streams = [A.signal("levels", nperseg, nfft, hop + s, "int16", frames=RAGGED_FRAMES[0] + 1) for s in range(5)]
    streams = [(i[:n], q[:n]) for i, q in streams]
    spec, e, T = _launch(nperseg, nfft, hop, "int16", streams, lens=lens, etot=with_etot)
    assert T == RAGGED_FRAMES[0]
    chain = _lib.cstft_chain(nperseg, nfft)
    for s, k in enumerate(RAGGED_FRAMES):
        assert not spec[s, k:].any(), f"stream {s}: frames past its end are not zero"
        z = A.as_complex(streams[s][0][: lens[s]], streams[s][1][: lens[s]])
        if k:
            R = A.reference(z, FS, nperseg, nfft, hop)
            assert R.shape[0] == k
            _check_bars(f"ragged stream {s}", spec[s, :k].astype(np.float64), R, chain)
        if with_etot:
            col = e[:, s * T: (s + 1) * T]
            assert np.all(np.isnan(col[:, k:])), f"stream {s}: partials written past its end"
            if k:
                _check_energy(f"ragged stream {s}", col[:, :k].astype(np.float64).sum(axis=0), z, nperseg, nfft, hop)


@pytest.mark.parametrize("shape", [(16, 16, 4, 200_000, 256), (1024, 1024, 256, 20_000, 4)], ids=["16", "1024"])
def test_one_large_launch(shape):
    """every workgroup makes more than one trip: at most 8 workgroups of 256 threads stay resident per CU
    and a trip takes F frames, so more than 2 * 8 * CUs * F frames; every 97th frame, the last one and the
    first past the end (of a second, shorter stream) are checked"""
    nperseg, nfft, hop, frames, F = shape
    frames = max(frames, 2 * 8 * _cus() * F + 7)
    n = A.n_samples(nperseg, hop, frames)
    rng = np.random.default_rng([nfft, 5])
    i = np.clip(np.rint(rng.standard_normal(n, dtype=np.float32) * 6000.0), -32768, 32767).astype(np.int16)
    q = np.clip(np.rint(rng.standard_normal(n, dtype=np.float32) * 6000.0), -32768, 32767).astype(np.int16)
    short = A.n_samples(nperseg, hop, 1000) + 1
    ts = sorted(set(range(0, frames, 97)) | {999, frames - 1})
    spec, _, T = _launch(nperseg, nfft, hop, "int16", [(i, q), (i[:short], q[:short])], etot=False,
                         rows=[ts, [0, 999, 1000, 1001, frames - 1]])
    assert T == frames
    z = A.as_complex(i, q)
    R = A.reference_frames(np.stack([z[t * hop: t * hop + nperseg] for t in ts]), FS, nperseg, nfft)
    chain = _lib.cstft_chain(nperseg, nfft)
    _check_bars(f"large {nfft}", spec[0].astype(np.float64), R, chain)
    assert np.array_equal(spec[1][:2], spec[0][[ts.index(0), ts.index(999)]])  # the same samples
    assert spec[1][:2].any() and not spec[1][2:].any(), "frames past the short stream's end are not zero"


def test_dispatch_4096():
    """4096 / 4096 / 1024 without the option is cstft4096_kernel's output bit for bit (the same run through
    msd_cstft_plan_create); with the option the generic kernel's: inside the bars (test_signal_classes) and
    not the same bits"""
    nperseg = nfft = 4096
    hop = 1024
    i, q, _ = A.case_data(nperseg, nfft, hop, "int16", "white")
    x = np.empty(2 * len(i), np.int16)
    x[0::2], x[1::2] = i, q
    w = A.window(nperseg)
    scale = A.scale_of(FS, nperseg)
    ctx = context(0).sibling()
    try:
        lib = ctx.lib
        h = _lib.C.c_void_p()
        _lib.check(lib.msd_cstft_plan_create(ctx.h, nperseg, hop, _lib.ptr(w), scale, _lib.C.byref(h)))
        assert lib.msd_cstft_nfft(h) == 4096
        T = int(lib.msd_cstft_frames(h, len(i)))
        old = np.empty((T, nfft), np.float32)
        t = _lib.C.c_int64(0)
        _lib.check(lib.msd_cstft_psd(h, _lib.ptr(x), _lib.MSD_CI16, len(i), _lib.ptr(old), _lib.C.byref(t)))
        lib.msd_cstft_plan_destroy(h)
        plan = _lib.CStftPlan(ctx, nperseg, hop, w, scale, nfft=nfft)
        new = plan.run(x, _lib.MSD_CI16)
        ctx.set_option(_lib.OPT_GENERIC_CSTFT, 1)
        gen = plan.run(x, _lib.MSD_CI16)
        ctx.set_option(_lib.OPT_GENERIC_CSTFT, 0)
        back = plan.run(x, _lib.MSD_CI16)
        plan.close()
    finally:
        ctx.close()
    assert T == A.FRAMES and np.array_equal(old, new) and np.array_equal(old, back)
    assert not np.array_equal(old, gen), "the option did not change the kernel"
    assert A.frame_err(gen, old).max() <= 2 * A.FRAME_TOL


def test_public_spectrogram_iq_matches_scipy():
    """the public entry point with nfft: scipy's (f, t, Sxx) at 1000 / 1024 / 250"""
    from scipy.signal import spectrogram
    nperseg, nfft, hop = 1000, 1024, 250
    i, q, R = A.case_data(nperseg, nfft, hop, "float32", "white")
    f, t, S = iq.spectrogram_iq(i, q, FS, nperseg, nperseg - hop, nfft=nfft)
    rf, rt, _ = spectrogram(A.as_complex(i, q), FS, "hann", nperseg, nperseg - hop, nfft, return_onesided=False)
    assert np.array_equal(f, rf) and np.allclose(t, rt, rtol=0, atol=1e-12) and S.shape == (nfft, len(rt))
    assert A.frame_err(S.T, R).max() <= A.FRAME_TOL
    # a stream shorter than nperseg: 0 frames
    f0, t0, S0 = iq.spectrogram_iq(i[:999], q[:999], FS, nperseg, nperseg - hop, nfft=nfft)
    assert S0.shape == (nfft, 0)


def test_unsupported_nfft():
    ctx = context(0)
    w = A.window(1024)
    with pytest.raises(_lib.MsdError) as ei:
        _lib.CStftPlan(ctx, 1024, 256, w, 1.0, nfft=16384)
    assert ei.value.code == _lib.MSD_ERR_UNSUPPORTED and "8192" in str(ei.value)
