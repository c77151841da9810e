"""GPU: block plans with 4096 < L = min(B, nfft) <= 65536 -- block_long_kernel
(csrc/block_delta.hip) -- against meteorgpu/margin.py's error model and an exact long-double DFT
(tests/long_block_signals.py has the yardstick, the chain and the list of cases; the inputs, the
references and the bars are those of tests/band_signals.py and tests/test_gpu_band_bins.py).

Through _lib.BlockPlan with explicit bins, MSD_OPT_BLOCK_GOERTZEL left alone, on every block and both
bands:

 1. |dB_gpu - dB_exact| <= margin.band_db_error(dB_exact, n, chain u S_block), the device-only counted
    chain 3 SPL G + 28 (zeros and empty bands: exactly -120);
 2. |delta_gpu - delta_numpy| <= margin.delta_error_bound(...) as dsp.process_samples calls it,
    wherever that is finite, and delta == band - noise bit for bit;
 3. on fullscale_noise and dc_quiet, rms over blocks of |sqrt E_gpu - sqrt E_exact| per band within
    RMS_FACTOR times the float64 CPU yardstick's plus the dB round trip 4 u (|dB| + 1) sqrt E;

at the first length over 4096 (odd, misaligned blocks, ragged and empty lanes), a cropped window's
foot, zero padding, odd B, non-power-of-two nfft, the limit 65536, every dtype, bins 0, 1, 2, nfft / 4,
K - 2, K - 1, sweep remainders 1-7, 300 and 4096 bins, an empty noise band, and the second trip of the
persistent loop.  Then the flat 1e-9 dB of the older tests against numpy, the refusal above 65536, and
end to end: dsp.process_samples at n_fft = 8192 against the oracle with both detectors, and a
BatchPipeline against the per-file path.

Every class of a case prints
    LONG B/nfft dtype class bins: model ratio, guard ratio, rms_gpu / rms_cpu
"""
import datetime

import numpy as np
import pytest

import band_signals as G
import long_block_signals as LB
from meteorgpu import _lib, dsp
from meteorgpu import margin as M
from meteorgpu.batch import BatchPipeline
from oracle import dsp_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)]

LD10 = G.LD(10)
DB_TOL = 1e-9


def _energy(db_values):
    return np.power(LD10, np.asarray(db_values).astype(G.LD) / 10)


def _check(case, cls, got, r, fails):
    B, nfft, dt, band, noise, _ = case
    L = min(B, nfft)
    gb, gn, gd = got
    tag = f"LONG {B}/{nfft} {np.dtype(dt).name} {cls} {band[0]}-{band[1]},{noise[0]}-{noise[1]}"
    nblk = len(r["S"])
    assert gb.shape == gn.shape == gd.shape == (nblk,)
    worst, rg, rc = 0.0, [], []
    for name, g, bd in (("band", gb, r["bands"][0]), ("noise", gn, r["bands"][1])):
        if not np.all(np.isfinite(g)):
            fails.append(f"{tag}: {name} dB not finite")
            continue
        if cls == "zeros" or bd["n"] == 0:
            if not (g == -120.0).all():
                fails.append(f"{tag}: {name} of {'zeros' if cls == 'zeros' else 'an empty band'} is not exactly -120")
            continue
        bound = G.model_bound(bd["db"], bd["n"], r["chain"], r["S"])
        if not np.all(np.isfinite(bound)):
            fails.append(f"{tag}: {name} model bound infinite")
        q = G.ratio(np.abs(g - bd["db"]), bound)
        worst = max(worst, q)
        if q > 1.0:
            i = int(np.argmax(np.abs(g - bd["db"]) / bound))
            fails.append(f"{tag}: {name} {q:.3g} times the model at block {i} (gpu {g[i]!r}, exact {bd['db'][i]!r})")
        if cls in G.NOISE_LIKE:
            a, c = G.rms_amp(_energy(g), bd["E"]), G.rms_amp(bd["Ey"], bd["E"])
            rg.append(a)
            rc.append(c)
            if a > G.RMS_FACTOR * c + G.db_floor(bd["db"], bd["E"]):
                fails.append(f"{tag}: {name} rms {a:.3e} against the yardstick's {c:.3e}")
    if not np.array_equal(gd, gb - gn):
        fails.append(f"{tag}: delta is not band_dB - noise_dB")
    # the shipped guard, called as dsp.process_samples calls it
    xmax = float(np.max(np.abs(np.asarray(r["x"], dtype=np.float64))))
    guard = M.delta_error_bound(gb, gn, nfft=nfft, L=L, window=r["w"], xmax=xmax, band=band, noise=noise)
    d_np = r["bands"][0]["db_np"] - r["bands"][1]["db_np"]
    ok = np.isfinite(guard)
    gq = G.ratio(np.abs(gd - d_np)[ok], guard[ok])
    if gq > 1.0:
        fails.append(f"{tag}: |delta - numpy's| {gq:.3g} times margin.delta_error_bound")
    fmt = lambda v: "/".join(f"{t:.2e}" for t in v) if v else "-"  # noqa: E731
    print(f"{tag}: model ratio {worst:.4f}, guard ratio {gq:.4f} ({int(ok.sum())}/{nblk} finite), "
          f"rms_gpu {fmt(rg)} / rms_cpu {fmt(rc)}")


def _run_case(case, nblk=None):
    B, nfft, dt, band, noise, classes = case
    L = min(B, nfft)
    refs = {cls: LB.case_refs(case, cls, nblk) for cls in classes}
    ctx = dsp.context(0)
    got = {}
    plan = _lib.BlockPlan(ctx, B, nfft, G.block_window(B, L), band, noise)
    try:
        for cls in classes:
            got[cls] = plan.run(refs[cls]["x"])
    finally:
        plan.close()
    fails = []
    for cls in classes:
        _check(case, cls, got[cls], refs[cls], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", [pytest.param(c, id=LB.case_id(c)) for c in LB.cases()])
def test_long_block_bands_within_the_model(case):
    _run_case(case)


def test_long_block_persistent_loop_second_trip():
    """block_long_kernel's grid is min(blocks, 8 workgroups per CU), one block per workgroup and trip:
    50 blocks more than that of 4097 uint8 samples, so the first workgroups walk a second block and
    reuse their LDS after the closing barrier"""
    try:
        import torch
        cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        cus = 256  # MI355X
    _run_case((4097, 4097, G.U8, (1, 1), (2047, 2047), ("fullscale_noise",)), nblk=8 * cus + 50)


@pytest.mark.parametrize("B,nfft", LB.FLAT_SHAPES)
def test_long_block_flat_bar_against_numpy(B, nfft):
    """the older tests' |dB - numpy| <= 1e-9 on sigma = 3000 noise plus a 1 kHz tone at 48 kHz; the
    float64 yardstick alone meets it at both shapes (tests/test_long_block_signals.py: 4.3e-14 dB)"""
    band, noise = LB.flat_bins(nfft)
    ref = LB.flat_db_numpy(B, nfft)
    plan = _lib.BlockPlan(dsp.context(0), B, nfft, G.block_window(B, min(B, nfft)), band, noise)
    try:
        gb, gn, gd = plan.run(LB.flat_input(B))
    finally:
        plan.close()
    worst = max(float(np.max(np.abs(gb - ref[0]))), float(np.max(np.abs(gn - ref[1]))))
    print(f"FLAT {B}/{nfft}: gpu against numpy {worst:.3e} dB")
    assert worst <= LB.FLAT_DB and np.array_equal(gd, gb - gn)


def test_length_above_the_limit_is_refused():
    ctx = dsp.context(0)
    with pytest.raises(_lib.MsdError, match="65536") as e:
        _lib.BlockPlan(ctx, 65537, 131072, np.ones(65537), (1, 1), (2, 2))
    assert e.value.code == _lib.MSD_ERR_UNSUPPORTED
    with pytest.raises(_lib.MsdError, match="65536"):
        _lib.BlockPlan(ctx, 70000, 65538, np.ones(65538), (1, 1), (2, 2))


# ------------------------------------------------------------------------------------- end to end
FS, SECS, N_FFT = 48000, 10, 8192
BAND, NOISE = (950.0, 1050.0), (2950.0, 3050.0)
ADAPT = dict(threshold_estimation_window_sec=2, threshold_freeze_before_detection_sec=0.4,
             threshold_freeze_after_detection_sec=1, threshold_fixed_init_duration_sec=1)


def _pings(seed, secs=SECS, at=((3.0, 0.7), (6.4, 0.9))):
    """int16 noise (sigma 1000) with 1 kHz pings (amplitude 2500, 10 ms rise, exponential decay)"""
    rng = np.random.default_rng(seed)
    n = FS * secs
    x = 1000.0 * rng.standard_normal(n)
    for t0, d in at:
        if t0 + d > secs:
            continue
        i0, m = int(t0 * FS), int(d * FS)
        t = np.arange(m) / FS
        env = np.where(t < 0.01, t / 0.01, np.exp(-(t - 0.01) / (d / 3.0)))
        x[i0: i0 + m] += 2500.0 * env * np.sin(2 * np.pi * 1000.0 * (t + t0) + 0.3 * seed)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("adaptive,k", [(False, 2.0), (True, 4.0)], ids=["global", "adaptive"])
def test_process_samples_at_n_fft_8192_matches_the_oracle(tmp_path, adaptive, k):
    x = _pings(11)
    start = datetime.datetime(2025, 6, 25, 7, 51, 41)
    kw = ADAPT if adaptive else {}
    res = dsp.process_samples(x, FS, 0.2, BAND, NOISE, N_FFT, k, wav_start_date_time=start,
                              flag_adaptive_threshold=adaptive, **kw)
    rdets, rthr, rb, rn, rd = O.proc_samples_ref(x, FS, 0.2, BAND, NOISE, N_FFT, k, start, adaptive, **kw)
    assert res.num_blocks == 50 and res.block_size == 9600
    for got, ref in ((res.band_power, rb), (res.noise_power, rn), (res.delta_power, rd)):
        assert np.abs(got - ref).max() <= DB_TOL
    assert np.abs(np.asarray(res.thresholds, np.float64) - np.asarray(rthr, np.float64)).max() <= DB_TOL
    assert res.min_margin > 1e-7, "decision margin too small for a meaningful parity check"
    assert not res.near_tie and res.decision_bound < 1e-7
    dsp.write_csv(res.detections, str(tmp_path / "ours.csv"))
    O.write_csv_ref(rdets, tmp_path / "ref.csv")
    ours = (tmp_path / "ours.csv").read_text().splitlines()
    ref = (tmp_path / "ref.csv").read_text().splitlines()
    assert len(ours) == len(ref) and len(ref) >= 2, "the pings should produce detections"
    for lo, lr in zip(ours[1:], ref[1:]):
        fo, fr = lo.split(","), lr.split(",")
        assert fo[0:3] == fr[0:3] and fo[4:] == fr[4:]       # t_start, t_stop, dur_s, utc_start, utc_stop
        assert abs(float(fo[3]) - float(fr[3])) <= DB_TOL   # dB
    assert [(int(round(d.t_start / 0.2)), int(round(d.t_stop / 0.2))) for d in res.detections] == \
           [(int(round(r[0] / 0.2)), int(round(r[1] / 0.2))) for r in rdets]


def test_batch_pipeline_at_n_fft_8192_matches_the_single_file_path():
    """3 files x 5 blocks of 9600: delta, thresholds, detections, margins and the near-tie flags of
    the batch equal the per-file results bit for bit"""
    ctx = dsp.context(0)
    F, n = 3, 5 * 9600
    kw = dict(ADAPT, threshold_estimation_window_sec=0.4, threshold_freeze_after_detection_sec=0.2,
              threshold_fixed_init_duration_sec=0.4, threshold_freeze_before_detection_sec=0.2)
    xs = [_pings(20 + i, secs=1, at=((0.62, 0.3),)) for i in range(F)]
    bp = BatchPipeline(ctx, F, n, FS, freq_band=BAND, noise_band=NOISE, n_fft=N_FFT, with_spectrogram=False, **kw)
    try:
        for i, x in enumerate(xs):
            bp.upload_file(i, x)
        bp.run()
        ctx.synchronize()
        deltas, thr = bp.delta(), bp.thresholds()
        dets, counts, status, margin = bp.detections()
        assert (status == 0).all() and deltas.shape == (F, 5)
        for i, x in enumerate(xs):
            res = dsp.process_samples(x, FS, 0.2, BAND, NOISE, N_FFT, 4.0, **kw)
            np.testing.assert_array_equal(deltas[i], res.delta_power)
            np.testing.assert_array_equal(thr[i], np.asarray(res.thresholds, np.float64))
            assert [(int(a["start"]), int(a["stop"]), float(a["db"])) for a in dets[i]] == \
                   [(int(round(d.t_start / 0.2)), int(round(d.t_stop / 0.2)), d.dB) for d in res.detections]
            assert np.array_equal(margin[i: i + 1], [res.min_margin], equal_nan=True)
            assert bp.decision_bounds[i] == res.decision_bound and bool(bp.near_tie[i]) == res.near_tie
    finally:
        bp.close()
