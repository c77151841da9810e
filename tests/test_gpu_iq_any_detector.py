"""GPU: the I/Q detector end to end at frame lengths other than C5's 4096 (cstft_any_kernel below it).

Three stations -- 48 kHz / 1024 / noverlap 768, 96 kHz / 2048 / 1536, 192 kHz / 8192 / 6144 -- on 6 s of
sigma = 1000 noise plus pings at +1 kHz (adaptive: three of 0.3 s; global: one strong one of 0.15 s), band
(950, 1050) Hz and noise (-3050, -2950) Hz (both away from 0 Hz), small detector windows; int16 and float32, adaptive and global detector; against
oracle.iq_oracle.proc_iq_ref: the detections' frames identical, dB within 1e-9, certified, and
|delta_gpu - delta_ref| <= ed on every frame with ed finite everywhere.  The seeds are such that the
oracle's smallest |delta - threshold| is above 1e-3 dB (asserted on the oracle's numbers), so no decision
hangs on the refinement; the near-tie test then builds decisions ~3e-7 dB from their thresholds at
1024 / 256 (the construction of test_gpu_certify.py), which only the float64 refinement settles.
Chunked (chunk_sec) against whole bit for bit and IQShardDetector over 3 rank-threads against one rank,
at 1024 / 256; the argument checks.
"""
import functools

import numpy as np
import pytest

from meteorgpu import _lib, iq
from meteorgpu.dsp import context
from oracle import dsp_oracle as O
from oracle import iq_oracle as Q

pytestmark = pytest.mark.gpu

BAND, NOISE = (950.0, 1050.0), (-3050.0, -2950.0)
KW = dict(threshold_estimation_window_sec=2, threshold_freeze_after_detection_sec=1,
          threshold_fixed_init_duration_sec=1)
STATIONS = {"48k-1024": (48000, 1024, 768), "96k-2048": (96000, 2048, 1536), "192k-8192": (192000, 8192, 6144)}
SECONDS = 6.0


@functools.lru_cache(maxsize=None)
def _stream(fs, kind, seed, seconds=SECONDS, pings=3, amp=1000.0, dur=0.3):
    """complex Gaussian noise of sigma 1000 plus `pings` tone bursts of `dur` s at +1 kHz after the first
    1.2 s"""
    rng = np.random.default_rng(seed)
    n = int(fs * seconds)
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (1000.0 / np.sqrt(2.0))
    t = np.arange(n) / fs
    for t0 in rng.uniform(1.2, seconds - 0.5, pings):
        a, b = int(t0 * fs), min(n, int((t0 + dur) * fs))
        z[a:b] += amp * np.exp(2j * np.pi * 1000.0 * t[a:b])
    if kind == "int16":
        return np.rint(z.real).astype(np.int16), np.rint(z.imag).astype(np.int16)
    return z.real.astype(np.float32), z.imag.astype(np.float32)


def _case_stream(fs, kind, adaptive, seed):
    """adaptive: three 0.3 s pings; global (one threshold from the whole stream's mean + 4 std): one strong
    0.15 s ping, so that the pings do not carry the std above themselves"""
    return _stream(fs, kind, seed) if adaptive else _stream(fs, kind, seed, pings=1, amp=10000.0, dur=0.15)


@functools.lru_cache(maxsize=None)
def _oracle(station, kind, adaptive, seed):
    fs, nperseg, noverlap = STATIONS[station]
    i, q = _case_stream(fs, kind, adaptive, seed)
    return Q.proc_iq_ref(i, q, fs, BAND, NOISE, nperseg, noverlap, flag_adaptive_threshold=adaptive, **KW)


SEED = 7


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "global"])
@pytest.mark.parametrize("kind", ["int16", "float32"])
@pytest.mark.parametrize("station", list(STATIONS))
def test_end_to_end_matches_oracle(station, kind, adaptive):
    fs, nperseg, noverlap = STATIONS[station]
    hop = nperseg - noverlap
    i, q = _case_stream(fs, kind, adaptive, SEED)
    rdets, rthr, _, _, rdelta = _oracle(station, kind, adaptive, SEED)
    thr = np.asarray(rthr, np.float64) if adaptive else np.full(len(rdelta), float(rthr))
    gap = np.nanmin(np.abs(rdelta - thr))
    assert len(rdets) >= 1 and gap > 1e-3, (len(rdets), gap)
    # the bound, frame by frame, before any refinement
    buf, _ = iq.interleave(i, q)
    det = iq.IQShardDetector(context(0), buf.size // 2, fs, nperseg, noverlap, BAND, NOISE, 4.0, adaptive,
                             dtype=buf.dtype, **KW)
    try:
        det.process_host(buf[2 * det.s0: 2 * det.s1])
        det.ctx.synchronize()
        d, ed = det.plan.delta(), det.plan.ed()
    finally:
        det.close()
    err = np.abs(d - rdelta)
    print(f"{station} {kind}: max err {err.max():.3e} dB, ed median {np.median(ed):.3e} max {ed.max():.3e}, "
          f"max err / ed {np.max(err / ed):.3g}, oracle gap {gap:.3e}")
    assert d.shape == rdelta.shape and np.all(np.isfinite(ed)) and np.all(err <= ed)
    # end to end
    dets, _, _, res = iq.proc_iq_samples(i, q, fs, BAND, NOISE, nperseg, noverlap, flag_adaptive_threshold=adaptive,
                                         **KW)
    assert res.certified
    bs = hop / fs
    assert [(d_.t_start, d_.t_stop) for d_ in dets] == [(x[0], x[1]) for x in rdets]
    assert [(round(d_.t_start / bs), round(d_.t_stop / bs)) for d_ in dets] == \
        [(round(x[0] / bs), round(x[1] / bs)) for x in rdets]
    assert max(abs(d_.dB - x[3]) for d_, x in zip(dets, rdets)) < 1e-9


# ------------------------------------------------------------------------------- near ties at 1024 / 256
FS, N, HOP = 48000, 1024, 256


def _frame_delta(seg):
    """the oracle's delta of one frame (scipy's arithmetic: detrend, periodic Hann, |X|^2 scale)"""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    X = np.fft.fft((seg - seg.mean()) * w)
    P = (X.conj() * X).real / (FS * (w * w).sum())
    f = np.fft.fftfreq(N, 1 / FS)
    eb = np.sum(P[(f >= BAND[0]) & (f <= BAND[1])]) + 1e-12
    en = np.sum(P[(f >= NOISE[0]) & (f <= NOISE[1])]) + 1e-12
    return 10 * np.log10(eb) - 10 * np.log10(en)


@functools.lru_cache(maxsize=None)
def _near_tie_stream(seed=41, seconds=20.0, eps=3e-7):
    """float32 I/Q whose oracle decisions at a few frames sit eps dB above or below their threshold: a tone
    at a band bin added to the newest hop block of frame fi (frames fi .. fi + 3 see it, not fi's threshold
    window), its amplitude bisected to place delta[fi]"""
    i32, q32 = _stream(FS, "float32", seed, seconds, pings=2, amp=300.0)
    z = i32.astype(np.float64) + 1j * q32.astype(np.float64)
    bs = HOP / FS
    W, F0, Fa = int(2 / bs), int(1 / bs), int(1 / bs)
    placed = []
    tone = np.exp(2j * np.pi * (21 * FS / N) * np.arange(HOP) / FS)
    # (candidates W + Fa + 20 frames apart: past the previous one's freeze, and more than the 3 s freeze
    # before a detection, which rewrites the thresholds list behind it)
    for k, fi in enumerate(range(F0 + W + 10, int(seconds * FS - N) // HOP - 8, W + Fa + 20)):
        _, _, _, _, delta = Q.proc_iq_ref(z.real, z.imag, FS, BAND, NOISE, N, N - HOP, **KW)
        thr_list = O.get_detections_adaptive_ref(delta, 4.0, bs, 2, 3, 1, 1)[1]
        win = delta[fi - W: fi]
        fresh = np.mean(win) + 4.0 * np.std(win)
        if thr_list[fi] != fresh or delta[fi] > fresh - 0.5:
            continue  # frozen there, or already near / above: not a clean target
        target = fresh + (eps if k % 2 == 0 else -eps)
        seg0 = z[fi * HOP: fi * HOP + N].copy()

        def place(alpha):
            seg = seg0.copy()
            v = seg[N - HOP:] + alpha * tone
            seg[N - HOP:] = v.real.astype(np.float32) + 1j * v.imag.astype(np.float32)
            return seg

        lo, hi = 0.0, 50.0
        while _frame_delta(place(hi)) < target:
            hi *= 2
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if _frame_delta(place(mid)) < target:
                lo = mid
            else:
                hi = mid
        best = min((lo, hi), key=lambda a: abs(_frame_delta(place(a)) - target))
        z[fi * HOP: fi * HOP + N] = place(best)
        placed.append(fi)
    i_, q_ = z.real.astype(np.float32), z.imag.astype(np.float32)
    _, thr, _, _, delta = Q.proc_iq_ref(i_, q_, FS, BAND, NOISE, N, N - HOP, **KW)
    margins = np.abs(delta[placed] - np.asarray(thr)[placed])
    return i_, q_, tuple(placed), margins


def test_near_ties_are_refined_and_decide_as_the_oracle():
    i, q, placed, margins = _near_tie_stream()
    assert len(placed) >= 3 and margins.max() < 5e-6, (placed, margins)
    rdets, _, _, _, _ = Q.proc_iq_ref(i, q, FS, BAND, NOISE, N, N - HOP, **KW)
    _, _, _, r0 = iq.proc_iq_samples(i, q, FS, BAND, NOISE, N, N - HOP, exact_decisions=False, **KW)
    assert r0.certified is False and r0.uncertain >= len(placed)
    assert set(placed) <= set(int(f) for f in r0.uncertain_frames[:, 0])
    dets, _, _, r = iq.proc_iq_samples(i, q, FS, BAND, NOISE, N, N - HOP, **KW)
    assert r.certified and not r.near_tie and r.refined_delta_frames > 0 and r.detector_passes >= 2
    assert [(d.t_start, d.t_stop) for d in dets] == [(x[0], x[1]) for x in rdets]
    for d, x in zip(dets, rdets):
        assert abs(d.dB - x[3]) < 1e-9, (d.dB, x[3])


# ------------------------------------------------------------------------------- chunked, sharded
@pytest.mark.parametrize("kind", ["int16", "float32"])
def test_chunked_equals_whole(kind):
    i, q = _stream(FS, kind, SEED)
    d1, t1, delta1, _ = iq.proc_iq_samples(i, q, FS, BAND, NOISE, N, N - HOP, **KW)
    d2, t2, delta2, _ = iq.proc_iq_samples(i, q, FS, BAND, NOISE, N, N - HOP, chunk_sec=0.7, **KW)
    assert len(d1) >= 1 and np.array_equal(delta1, delta2)
    assert [(d.t_start, d.t_stop, d.dB) for d in d1] == [(d.t_start, d.t_stop, d.dB) for d in d2]
    assert np.array_equal(np.asarray(t1), np.asarray(t2), equal_nan=True)


def test_three_rank_threads_equal_one_rank():
    from stream_np_ops import run_threads
    i, q = _stream(FS, "float32", SEED)
    buf, _ = iq.interleave(i, q)
    one, *_ = iq.proc_iq_samples(i, q, FS, BAND, NOISE, N, N - HOP, **KW)

    def body(r, comm):
        ctx = _lib.Context(0)
        try:
            det = iq.IQShardDetector(ctx, i.size, FS, N, N - HOP, BAND, NOISE, 4.0, True, rank=r, world=3,
                                     seg_len=512, dtype=buf.dtype, **KW)
            det.upload(buf[2 * det.s0: 2 * det.s1])
            det.spectrogram_and_delta()
            res = det.detect(comm)
            det.close()
            return res
        finally:
            ctx.close()

    res = run_threads(3, body)
    bs = HOP / FS
    assert len(one) >= 1
    for r in res:
        assert r.certified
        assert [(int(a) * bs, int(b) * bs) for a, b, _ in r.detections] == [(d.t_start, d.t_stop) for d in one]
        assert np.array_equal(r.detections["db"], np.array([d.dB for d in one]))


# ------------------------------------------------------------------------------- argument checks
def test_zero_padded_plan_is_refused(monkeypatch):
    """IQShardDetector has no nfft argument; a spectrogram plan with nfft != nperseg under it (here: the
    plan factory patched to pad to 2048) is refused -- the certificate covers nfft = nperseg only"""
    real = iq._plan
    monkeypatch.setattr(iq, "_plan", lambda ctx, fs, nperseg, noverlap, nfft=None: real(ctx, fs, nperseg, noverlap, 2048))
    with pytest.raises(ValueError, match="nfft == nperseg"):
        iq.IQShardDetector(context(0), FS * 2, FS, N, N - HOP, BAND, NOISE, 4.0, True, **KW)


def test_nfft_16384_is_unsupported():
    i, q = _stream(FS, "int16", SEED)
    with pytest.raises(_lib.MsdError) as ei:
        iq.spectrogram_iq(i[:40000], q[:40000], FS, 16384, 8192)
    assert ei.value.code == _lib.MSD_ERR_UNSUPPORTED
    with pytest.raises(_lib.MsdError) as ei:
        iq.spectrogram_iq(i[:40000], q[:40000], FS, 1024, 512, nfft=16384)
    assert ei.value.code == _lib.MSD_ERR_UNSUPPORTED
