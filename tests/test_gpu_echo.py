"""GPU: the echo measurement (csrc/echo.hip through meteorgpu.echo) against tests/echo_ref.py on the same
buffers -- synthetic spectrograms uploaded directly at the smallest shapes where the kernel can go wrong, one
end-to-end recording through dsp.process_samples / dsp.measure_detections, the batch pipeline, and the CSV.

Every integer field, flags, p_peak, n_peak and d_peak are byte-equal.  e_sig, e_noise, w_u and w_uu are
byte-equal on integer-valued input (every partial sum is an exact integer below 2^53 in any order); elsewhere
each of the six sums is within (n + 3) 2^-53 sum|term| of the reference, n the span length, the terms the
reference's own: the first-order bound for summing n terms in any order, each carrying at most two rounded
multiplies."""
import csv

import numpy as np
import pytest

import echo_ref as R

pytestmark = pytest.mark.gpu

EXACT = ("t0", "t1", "t_peak", "t_half_first", "t_half_last", "t_efold", "k_peak", "flags", "p_peak", "n_peak",
         "d_peak")
INT_SUMS = ("e_sig", "e_noise", "w_u", "w_uu")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from meteorgpu import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def make_spec(seed, F, K, ld, frames, c, kind, dtype):
    """[F][K][ld]: the cells the measurement may read hold values of ``kind``; the padding columns and the rows
    outside [min(k_lo, n_lo) - 1, max(k_hi, n_hi) + 1] hold 1e30 and NaN"""
    rng = np.random.default_rng(seed)
    if kind == "int3":  # three levels below 2^12: ties in frame and row are common
        v = rng.choice([0.0, 1000.0, 4095.0], size=(F, K, ld), p=[0.5, 0.3, 0.2])
    else:
        v = rng.uniform(0.0, 1.0, size=(F, K, ld))
    rows = [c["k_lo"], c["k_hi"]] + ([c["n_lo"], c["n_hi"]] if c["n_lo"] <= c["n_hi"] else [])
    poison = np.where((np.arange(K)[:, None] + np.arange(ld)[None, :]) % 2 == 0, 1e30, np.nan)
    for f in range(F):
        dead = np.zeros((K, ld), bool)
        dead[:, int(frames[f]):] = True
        dead[: max(0, min(rows) - 1)] = True
        dead[max(rows) + 2:] = True
        v[f][dead] = poison[dead]
    return v.astype(dtype)


def run_gpu(ctx, spec, frames, dets, counts, cap, c, guard=3):
    """uploads everything, measures, returns the whole record buffer [F][cap] + ``guard`` slots as bytes"""
    from meteorgpu import _lib, echo
    F, K, ld = spec.shape
    d_spec, d_frames, d_counts = ctx.alloc(spec.nbytes), ctx.alloc(8 * F), ctx.alloc(8 * F)
    d_dets = ctx.alloc(F * cap * R.DET_DTYPE.itemsize)
    d_out = ctx.alloc((F * cap + guard) * 128)
    bufs = [d_spec, d_frames, d_counts, d_dets, d_out]
    try:
        d_spec.upload(spec)
        d_frames.upload(np.asarray(frames, np.int64))
        d_counts.upload(np.asarray(counts, np.int64))
        d_dets.upload(dets)
        d_out.memset(SENTINEL)
        cfg = echo.echo_cfg(c["block_size"], c["nperseg"], c["hop"], (c["k_lo"], c["k_hi"]), (c["n_lo"], c["n_hi"]),
                            c["pre_frames"], c["post_frames"])
        echo.measure_dev(ctx, d_spec, spec.dtype, F, K, d_frames, ld, d_dets, cap, d_counts, cfg, d_out)
        raw = np.empty((F * cap + guard) * 128, np.uint8)
        d_out.download(raw)
        assert _lib.ECHO_DTYPE == R.ECHO_DTYPE
    finally:
        for b in bufs:
            b.free()
    return raw.reshape(F * cap + guard, 128)


def compare(got, ref, terms, exact_sums, what):
    """one file's records against the reference's"""
    assert got.shape == ref.shape, what
    for name in EXACT:
        assert got[name].tobytes() == ref[name].tobytes(), (what, name, got[name], ref[name])
    for i in range(ref.shape[0]):
        n = int(ref["t1"][i] - ref["t0"][i])
        for name in R.SUMS:
            if exact_sums and name in INT_SUMS:
                assert got[name][i].tobytes() == ref[name][i].tobytes(), (what, i, name, got[name][i], ref[name][i])
            else:
                bound = (n + 3) * 2.0 ** -53 * terms[i][name]
                assert abs(got[name][i] - ref[name][i]) <= bound, (what, i, name, got[name][i], ref[name][i], bound)


def check_case(ctx, seed, K, ld, frames, blocks, counts, cap, c, kind, dtype):
    """blocks[f]: the (start, stop) of the detections file f holds (at most cap are stored); counts[f] may
    exceed cap.  Returns the reference records per file and the spectrogram."""
    F = len(frames)
    spec = make_spec(seed, F, K, ld, frames, c, kind, dtype)
    dets = np.zeros((F, cap), R.DET_DTYPE)
    dets["start"], dets["stop"] = -7, -9  # slots past the count are never read as detections
    for f in range(F):
        for i, (a, b) in enumerate(blocks[f][:cap]):
            dets[f, i] = (a, b, 0.0)
    raw = run_gpu(ctx, spec, frames, dets, counts, cap, c)
    refs = []
    for f in range(F):
        m = max(0, min(int(counts[f]), cap))
        ref, terms = R.measure(spec[f], frames[f], dets[f, :m], c)
        got = raw[f * cap: f * cap + m].copy().view(R.ECHO_DTYPE).reshape(m)
        compare(got, ref, terms, kind == "int3", f"file {f}")
        assert (raw[f * cap + m: (f + 1) * cap] == SENTINEL).all(), f"file {f}: a slot past the count was written"
        refs.append(ref)
    assert (raw[F * cap:] == SENTINEL).all(), "the guard past the buffer was written"
    return refs, spec


KINDS = [("int3", np.float32), ("int3", np.float64), ("uniform", np.float32), ("uniform", np.float64)]
# blocks of 1200 samples on frames of 1024 every 128: block b starts at frame ceil((1200 b - 512) / 128)
DAY = [(0, 1), (1, 2), (3, 3), (4, 6), (6, 7), (9, 9), (10, 11), (12, 13), (14, 15), (15, 30), (31, 32)]
DAY8 = DAY[:7] + [(13, 30)]  # the last one runs past the file


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_layout_counts_and_clipping(ctx, kind, dtype):
    """K = 33, T = 150, ld = 160, three files of 150, 97 and 0 frames, cap 8; counts 0, 1, 8 and 11"""
    c = R.cfg(1200, 1024, 128, (10, 14), (20, 22), pre=3, post=12)
    frames = [150, 97, 0]
    refs, _ = check_case(ctx, 1, 33, 160, frames, [DAY[:1], DAY, []], [1, 11, 0], 8, c, kind, dtype)
    assert refs[1].shape[0] == 8  # 11 counted, 8 stored: the last stored one reaches to T
    refs += check_case(ctx, 2, 33, 160, frames, [DAY8, [], DAY[:3]], [8, 0, 3], 8, c, kind, dtype)[0]
    allr = np.concatenate(refs)
    flags = allr["flags"]
    assert (flags & 1).any() and (flags & 2).any() and (flags & 3 == 3).any() and (flags & 3 == 0).any()
    assert (allr["t0"] == 0).any() and (allr["t1"] == 150).any() and (allr["t1"] == 97).any()
    assert (refs[5]["t0"] == refs[5]["t1"]).all() and refs[5].shape[0] == 3  # T = 0: every span is empty
    d = refs[3]  # the file with 8 detections: clipped by a neighbour before, after, and post > the gap
    assert (d["t0"][1:] == d["t1"][:-1]).any() and ((d["t1"][:-1] < d["t0"][1:]) & (d["flags"][:-1] & 2 == 0)).any()
    assert (d["flags"][:-1] & 2 != 0).any() and (d["flags"][1:] & 1 != 0).any()
    assert ((d["t1"] - d["t0"] > 0) & (np.array([a == b for a, b in DAY8]))).any()  # start == stop, padding only


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_span_lengths(ctx, kind, dtype):
    """spans of 0, 1, 2, 63, 64, 65, 129 and 300 frames (blocks of one sample on frames of one sample)"""
    c = R.cfg(1, 1, 1, (2, 6), (8, 8))
    lens = [0, 1, 2, 63, 64, 65, 129]
    blocks, at = [], 5
    for n in lens:
        blocks.append((at, at + n))
        at += n + 2
    refs, _ = check_case(ctx, 3, 11, 416, [400, 400], [blocks, [(50, 350)]], [7, 1], 8, c, kind, dtype)
    assert list(refs[0]["t1"] - refs[0]["t0"]) == lens and list(refs[1]["t1"] - refs[1]["t0"]) == [300]


BANDS = [  # (K, signal band, noise band)
    (33, (7, 7), (3, 3)),          # one row
    (33, (10, 14), (0, -1)),       # five rows, no noise band
    (33, (0, 2), (31, 32)),        # at row 0
    (33, (30, 32), (0, 0)),        # at row K - 1
    (33, (0, 32), (0, 32)),        # the whole spectrogram
    (258, (1, 256), (2, 257)),     # the kernel's limit, MSD_ECHO_MAX_BAND rows
]


@pytest.mark.parametrize("K,band,noise", BANDS)
@pytest.mark.parametrize("kind,dtype", [("int3", np.float32), ("uniform", np.float64)])
def test_bands(ctx, K, band, noise, kind, dtype):
    from meteorgpu import _lib
    if K > 33:
        assert band[1] - band[0] + 1 == _lib.ECHO_MAX_BAND == noise[1] - noise[0] + 1
    c = R.cfg(1200, 1024, 128, band, noise, pre=2, post=9)
    refs, spec = check_case(ctx, 4, K, 96, [90, 70], [DAY[:5], DAY[3:6]], [5, 3], 6, c, kind, dtype)
    if noise[1] < noise[0]:
        assert all((r["e_noise"] == 0).all() and (r["n_peak"][r["t1"] > r["t0"]] == 0).all() for r in refs)
    if band[0] == 0 or band[1] == K - 1:
        # some measured frame peaks in the edge row, where there is no parabola (the seed is fixed)
        assert any(R.column(spec[0], t, c)[2] in (0, K - 1) for e in refs[0] for t in range(e["t0"], e["t1"]))


@pytest.mark.parametrize("nperseg,hop,block", [(8, 1, 7), (1024, 128, 1200), (1024, 512, 1200), (1023, 128, 1000)])
@pytest.mark.parametrize("kind,dtype", [("int3", np.float64), ("uniform", np.float32)])
def test_hops_and_block_sizes(ctx, nperseg, hop, block, kind, dtype):
    """block_size is no multiple of hop; the detections are spread over the 150 frames"""
    c = R.cfg(block, nperseg, hop, (4, 8), (12, 13), pre=2, post=5)
    per = max(1, 150 * hop // block // 12)  # blocks per twelfth of the file
    blocks = [(per * j, per * j + 1 + j % 2) for j in range(0, 12, 2)] + [(per * 11, per * 11), (per * 12, per * 14)]
    refs, _ = check_case(ctx, 5, 17, 160, [150, 149], [blocks, blocks[::2]], [8, 4], 8, c, kind, dtype)
    assert (refs[0]["t1"] > refs[0]["t0"]).sum() >= 6


def test_refusals_on_a_context(ctx):
    from meteorgpu import _lib, echo
    spec = np.ones((9, 40), np.float32)
    with pytest.raises(_lib.MsdError) as e:
        echo.measure(spec, [(0, 1)], block_size=100, nperseg=64, hop=32, band_bins=(3, 9))
    assert e.value.code == _lib.MSD_ERR_INVALID
    with pytest.raises(_lib.MsdError) as e:
        echo.measure(spec, [(0, 1)], block_size=100, nperseg=64, hop=32, band_bins=(3, 4), frames=41)
    assert e.value.code == _lib.MSD_ERR_INVALID
    assert echo.measure(spec, np.zeros(0, _lib.DET_DTYPE), block_size=100, nperseg=64, hop=32,
                        band_bins=(3, 4)).shape == (0,)


@pytest.fixture(scope="module")
def recording():
    """20 s at 6 kHz, three pings; the detections of the block detector and their echoes"""
    from meteorgpu import dsp, synth
    x = synth.synth_tones(31, 6000, 20.0, [(3.0, 0.6, 1003.0, 2500.0), (9.1, 1.0, 1001.0, 2500.0),
                                           (15.3, 0.4, 1006.0, 2500.0)])
    res = dsp.process_samples(x, 6000, 0.2, (993, 1013), (690, 710), 512, 1.5, flag_adaptive_threshold=False)
    ech = dsp.measure_detections(x, 6000, res, 0.2, (993, 1013), (690, 710), return_spectrogram=True)
    return x, res, ech


def test_end_to_end_recording(recording):
    from meteorgpu import dsp
    x, res, ech = recording
    assert len(res.detections) == ech.raw.shape[0] >= 3
    assert (ech.nperseg, ech.hop, ech.block_size, ech.pre_frames, ech.post_frames) == (1024, 128, 1200, 4, 46)
    assert ech.band_bins == dsp.band_bins(1024, 6000, (993, 1013)) == (170, 172)
    S = ech.spectrogram  # the buffer that was measured, downloaded
    assert S.dtype == np.float32 and S.shape == (513, ech.frames)
    assert np.array_equal(S, dsp.spectrogram(x, 6000, nperseg=1024, noverlap=1024 - 128)[2])
    c = R.cfg(1200, 1024, 128, ech.band_bins, ech.noise_bins, pre=4, post=46)
    ref, terms = R.measure(S, S.shape[1], ech.detections, c)
    compare(ech.raw, ref, terms, False, "recording")
    assert [(d["start"], d["stop"]) for d in ech.detections] == \
        [(round(d.t_start / 0.2), round(d.t_stop / 0.2)) for d in res.detections]
    # the three pings are found where they were put, to the sub-bin
    p = ech.params
    for t0, f in ((3.0, 1003.0), (9.1, 1001.0), (15.3, 1006.0)):
        i = int(np.argmin(np.abs(p["t_peak_s"] - (t0 + 0.2))))
        assert abs(p["t_peak_s"][i] - t0) < 1.2 and abs(p["f_peak_hz"][i] - f) < 0.5 * 6000 / 1024, (t0, p[i])


def test_echo_csv_round_trip(recording, tmp_path):
    from meteorgpu import echo
    _, res, ech = recording
    path = tmp_path / "echoes.csv"
    echo.write_echo_csv(res.detections, ech.params, path)
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == len(res.detections)
    assert list(rows[0]) == ["t_start", "t_stop", "dur_s", "dB", "utc_start", "utc_stop"] + list(echo.PARAM_FIELDS)
    for row, det, e in zip(rows, res.detections, ech.params):
        assert float(row["t_start"]) == det.t_start and float(row["dB"]) == det.dB and row["utc_start"] == ""
        for name in echo.PARAM_FIELDS:
            got, want = float(row[name]), float(e[name])
            assert got == want or (np.isnan(got) and np.isnan(want)), (name, row[name], e[name])


def test_proc_wav_file_writes_the_echo_csv(recording, tmp_path):
    from scipy.io import wavfile
    from meteorgpu import dsp, echo
    x, res, ech = recording
    wav, ref_csv, echo_csv = tmp_path / "rec.wav", tmp_path / "dets.csv", tmp_path / "echoes.csv"
    wavfile.write(wav, 6000, x)
    out = dsp.proc_wav_file(str(wav), 0.2, (993, 1013), (690, 710), 512, 1.5, out_csv_file=str(ref_csv),
                            disable_show_and_write=True, flag_adaptive_threshold=False, verbose=False,
                            out_echo_csv_file=str(echo_csv))
    assert [(d.t_start, d.t_stop) for d in out.detections] == [(d.t_start, d.t_stop) for d in res.detections]
    with open(ref_csv, newline="") as f:  # the reference's CSV is as it was
        assert list(csv.DictReader(f).fieldnames) == list(echo.DETECTION_FIELDS)
    with open(echo_csv, newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == len(res.detections)
    for row, e in zip(rows, ech.params):
        for name in echo.PARAM_FIELDS:
            got, want = float(row[name]), float(e[name])
            assert got == want or (np.isnan(got) and np.isnan(want)), (name, row[name], e[name])


@pytest.mark.parametrize("concurrent", [False, True])
def test_batch_pipeline_echoes(ctx, concurrent):
    from meteorgpu import _lib, echo, synth
    from meteorgpu.batch import BatchPipeline
    fs, n = 6000, 6000 * 10
    kw = dict(nperseg=1024, block_duration_sec=0.2, freq_band=(993, 1013), noise_band=(690, 710), n_fft=512,
              threshold_std_factor=2.0, flag_adaptive_threshold=False)
    off = BatchPipeline(ctx, 4, n, fs, **kw)
    assert off.d_echo is None and off.d_frames is None and not off.with_echoes
    off.close()
    with pytest.raises(ValueError):
        BatchPipeline(ctx, 4, n, fs, with_spectrogram=False, with_echoes=True, **kw)
    bp = BatchPipeline(ctx, 4, n, fs, with_echoes=True, concurrent=concurrent, **kw)
    try:
        for i in range(4):
            tones = [(2.0 + i, 0.6, 1003.0, 2500.0), (7.0, 0.4, 1000.0 + i, 2500.0)][: 1 + i % 2]
            bp.upload_file(i, synth.synth_tones(100 + i, fs, 10.0, tones))
        bp.run()
        bp.run()  # a second step: the detector rewrites the detections only after the first step's measurement
        ctx.synchronize()
        dets, counts, _, _ = bp.detections()
        rec = bp.echoes()
        assert bp.d_echo.nbytes == 4 * bp.cap * 128 and counts.sum() >= 4
        assert (bp.echo_cfg.pre_frames, bp.echo_cfg.post_frames) == (int(0.1 * fs / 512), int(1.0 * fs / 512))
        for i in range(4):
            one = echo.measure(bp.spectrogram(i), dets[i], block_size=bp.block_size, nperseg=1024, hop=bp.hop,
                               band_bins=bp.echo_bins[0], noise_bins=bp.echo_bins[1],
                               pre_frames=bp.echo_cfg.pre_frames, post_frames=bp.echo_cfg.post_frames)
            assert rec[i].shape == (min(counts[i], bp.cap),) and rec[i].dtype == _lib.ECHO_DTYPE
            assert rec[i].tobytes() == one.tobytes(), i  # the same kernel on the same cells: the same bits
            ref, terms = R.measure(bp.spectrogram(i), bp.T, dets[i], R.cfg(
                bp.block_size, 1024, bp.hop, *bp.echo_bins, pre=bp.echo_cfg.pre_frames,
                post=bp.echo_cfg.post_frames))
            compare(rec[i], ref, terms, False, f"batch file {i}")
    finally:
        bp.close()
