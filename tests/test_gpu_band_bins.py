"""GPU: the float64 band-power kernels -- block_delta2_kernel, block_delta_kernel
(csrc/block_delta.hip) and welch_bands_kernel (csrc/live.hip) -- against meteorgpu/margin.py's own
error model and an exact long-double DFT (tests/band_signals.py has the references, the yardsticks,
the chains, the signal classes and the list of cases).

The older tests compare with numpy's pocketfft at a flat 1e-9 dB on noise plus a tone near 1 kHz.
Here, through _lib.BlockPlan with explicit bins, on every block and both bands:

 1. |dB_gpu - dB_exact| <= margin.band_db_error(dB_exact, n, chain u S_block), the device-only chain
    (zeros: exactly -120; the bound is finite on every block that is not all zero);
 2. |delta_gpu - delta_numpy| <= margin.delta_error_bound(...) as dsp.process_samples calls it,
    wherever that is finite;
 3. on fullscale_noise and dc_quiet, rms over blocks of |sqrt E_gpu - sqrt E_exact| per band within
    RMS_FACTOR times the float64 CPU yardstick's plus the dB round trip 4 u (|dB| + 1) sqrt E;

at one sample per lane, empty and ragged lanes, a cropped window's foot, odd B (misaligned blocks),
odd and non-power-of-two nfft, nfft >> L, every SPL and dtype, bins 0, 1, 2, nfft / 4, K - 2, K - 1,
sweep remainders 1-7, the generic kernel above 64 bins and under MSD_OPT_GENERIC_STFT, and the second
trip of the persistent loop.  Through _lib.WelchPlan, per bin of psd()

    |sqrt P_gpu - sqrt P_exact| <= sqrt(scale c_k) dx + 4 u sqrt P,  dx = chain_w u S_rms + the mean's term

the band dB of run() within margin.welch_band_db_error of the same dx, the precision bar against the
one-lane yardstick without the dB term (psd() passes through no logarithm; bands whose model bound
is finite: one without power is pure rounding on both sides), and margin.live_over_error once per
shape against scipy's rows.

Every class of a case prints
    BAND kernel B/nfft dtype class bins: model ratio, rms_gpu / rms_cpu
    WELCH nperseg/nfft/noverlap/nseg dtype class nslots: bin ratio, band ratio, rms_gpu / rms_cpu
"""
import numpy as np
import pytest

import band_signals as G
from meteorgpu import _lib, dsp
from meteorgpu import margin as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)]


class _Options:
    """set context options for a block of code, restored to their earlier values on the way out"""

    def __init__(self, ctx, *opts):
        self.ctx, self.opts = ctx, [o for o in opts if o is not None]

    def __enter__(self):
        self.before = {o: self.ctx.options.get(int(o), 0) for o in self.opts}
        for o in self.opts:
            self.ctx.set_option(o, 1)

    def __exit__(self, *exc):
        for o, v in self.before.items():
            self.ctx.set_option(o, v)


def _energy(db_values):
    return np.power(LD10, np.asarray(db_values).astype(G.LD) / 10)


LD10 = G.LD(10)


def _check_block(case, cls, got, r, fails):
    kernel, B, nfft, dt, rect, band, noise, generic, _ = case
    L = min(B, nfft)
    gb, gn, gd = got
    tag = f"BAND {kernel}{'-opt' if generic else ''} {B}/{nfft} {np.dtype(dt).name}{' rect' if rect else ''} {cls} " \
          f"{band[0]}-{band[1]},{noise[0]}-{noise[1]}"
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
    x = r["x"]
    xmax = float(np.max(np.abs(np.asarray(x, dtype=np.float64))))
    guard = M.delta_error_bound(gb, gn, nfft=nfft, L=L, window=r["w"], xmax=xmax, band=band, noise=noise)
    d_np = r["bands"][0]["db_np"] - r["bands"][1]["db_np"]
    ok = np.isfinite(guard)
    gq = G.ratio(np.abs(gd - d_np)[ok], guard[ok])
    if gq > 1.0:
        fails.append(f"{tag}: |delta - numpy's| {gq:.3g} times margin.delta_error_bound")
    fmt = lambda v: "/".join(f"{t:.2e}" for t in v) if v else "-"  # noqa: E731
    print(f"{tag}: model ratio {worst:.4f}, guard ratio {gq:.4f} ({int(ok.sum())}/{nblk} finite), "
          f"rms_gpu {fmt(rg)} / rms_cpu {fmt(rc)}")


def _run_block_case(case, nblk=G.NBLK):
    kernel, B, nfft, dt, rect, band, noise, generic, classes = case
    L = min(B, nfft)
    name = np.dtype(dt).name
    refs = {cls: G.block_refs(cls, kernel, B, nfft, name, rect, band, noise, nblk) for cls in classes}
    ctx = dsp.context(0)
    got = {}
    with _Options(ctx, _lib.OPT_BLOCK_GOERTZEL if dt == G.I16 else None, _lib.OPT_GENERIC_STFT if generic else None):
        plan = _lib.BlockPlan(ctx, B, nfft, G.block_window(B, L, rect), band, noise)
        try:
            for cls in classes:
                got[cls] = plan.run(refs[cls]["x"])
        finally:
            plan.close()
    fails = []
    for cls in classes:
        _check_block(case, cls, got[cls], refs[cls], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", [pytest.param(c, id=G.block_case_id(c)) for c in G.block_cases()])
def test_block_bands_within_the_model(case):
    _run_block_case(case)


def test_block_persistent_loop_second_trip():
    """100 000 blocks of 16 uint8 samples: more than 16 blocks x 16 workgroups x 256 CUs, so the
    workgroups walk a second group and reuse their LDS powers after the wave barrier"""
    _run_block_case(("bd2", 16, 16, G.U8, False, (1, 1), (7, 7), False, ("fullscale_noise",)), nblk=100_000)


# ------------------------------------------------------------------------------------- Welch
def _welch_cfg(case, scale):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    c = _lib.MsdWelchCfg()
    c.block_size, c.nperseg, c.noverlap, c.nfft = block, nperseg, nov, nfft
    c.sample_scale, c.scale, c.nbands = float(ss), float(scale), len(bands)
    for j, (lo, hi) in enumerate(bands):
        c.band_lo[j], c.band_hi[j] = lo, hi
    return c


def _check_welch(case, cls, psd, rows, r, fails):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    nslots = len(r["bins"])
    tag = f"WELCH {nperseg}/{nfft}/{nov}/{nseg} {np.dtype(dt).name} x{ss:g} {cls} {nslots}"
    P = r["P"]
    assert psd.shape == P.shape and rows.shape == (len(bands), P.shape[0])
    if not (np.all(np.isfinite(psd)) and np.all(psd >= 0)):
        fails.append(f"{tag}: PSD not finite or negative")
        return
    if cls in ("zeros", "constant"):
        if psd.any() or not np.all(np.isneginf(rows)):
            fails.append(f"{tag}: a constant block must give PSD exactly 0 and band dB -inf")
        print(f"{tag}: exact")
        return
    bound = G.welch_bin_bound(P, r["dx"], r["bins"], nfft, r["scale"])
    err = np.abs(np.sqrt(psd.astype(G.LD)) - np.sqrt(P)).astype(np.float64)
    q = G.ratio(err, bound)
    if q > 1.0:
        b, k = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
        fails.append(f"{tag}: {q:.3g} times the per-bin bound at block {b}, bin {r['bins'][k]}")
    ref_db = G.welch_band_db(P, bands)
    bq, rg, rc, j0 = 0.0, [], [], 0
    for j, (lo, hi) in enumerate(bands):
        n = hi - lo + 1
        e = M.welch_band_db_error(ref_db[j], n, r["dx"][:, j0: j0 + n].max(axis=1), r["scale"], nseg)
        ok = np.isfinite(e) & np.isfinite(ref_db[j])
        if not np.all(np.isfinite(rows[j][ok])):
            fails.append(f"{tag}: band {j} dB not finite")
        else:
            t = G.ratio(np.abs(rows[j] - ref_db[j])[ok], e[ok])
            bq = max(bq, t)
            if t > 1.0:
                fails.append(f"{tag}: band {j} dB {t:.3g} times margin.welch_band_db_error")
        if cls in G.NOISE_LIKE and ok.all():
            Eg, Ee, Ey = (a[:, j0: j0 + n].sum(axis=1) for a in (psd.astype(G.LD), P, r["Y"].astype(G.LD)))
            a, c = G.rms_amp(Eg, Ee), G.rms_amp(Ey, Ee)
            rg.append(a)
            rc.append(c)
            if a > G.RMS_FACTOR * c:  # psd() passes through no logarithm: no round-trip floor here
                fails.append(f"{tag}: band {j} rms {a:.3e} against the yardstick's {c:.3e}")
        j0 += n
    fmt = lambda v: "/".join(f"{t:.2e}" for t in v) if v else "-"  # noqa: E731
    print(f"{tag}: bin ratio {q:.4f}, band ratio {bq:.4f}, rms_gpu {fmt(rg)} / rms_cpu {fmt(rc)}")


def _check_live_guard(case, ctx, rows, r, fails):
    """margin.live_over_error as live.near_tie_check calls it: the device's over-noise values against
    the reference detector's on scipy's rows"""
    from scipy.signal import welch
    from oracle import live_oracle as LO
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    x = np.asarray(r["x"], np.float64) * ss
    ref = []
    for b in range(rows.shape[1]):
        _, p = welch(x[b * block: (b + 1) * block], G.FS, nperseg=nperseg, noverlap=nov, nfft=nfft)
        with np.errstate(divide="ignore"):
            ref.append([10 * np.log10(np.sum(p[lo: hi + 1])) if np.sum(p[lo: hi + 1]) > 0 else -np.inf
                        for lo, hi in bands])
    ref = np.array(ref).T
    cfg = LO.ConfigDetectionRef(proc_block_sec=block / G.FS, avg_win_sec=3 * block / G.FS)
    with np.errstate(invalid="ignore"):
        over_ref = LO.live_detect_ref(ref, G.FS, block, cfg)[2]
    lc = _lib.MsdLiveCfg()
    lc.block_size, lc.avg_win_blocks, lc.fs, lc.k_std = block, 3, G.FS, 4.0
    lc.init_wait_sec, lc.after_tracking_wait_sec, lc.min_db_mean, lc.min_dur_sec = 8.0, 12.0, -1.0, -1.0
    over = _lib.live_detect(ctx, rows, lc)[2]
    e = M.live_over_error(rows, block_size=block, nperseg=nperseg, noverlap=nov, nfft=nfft, window=r["w"],
                          span=M.block_span(r["x"], block, ss), bands=list(bands), scale=r["scale"])
    ok = np.isfinite(e) & np.isfinite(over_ref) & np.isfinite(over)
    q = G.ratio(np.abs(over - over_ref)[ok], e[ok])
    print(f"WELCH {nperseg}/{nfft}/{nov}/{nseg} live guard: ratio {q:.3e} ({int(ok.sum())}/{len(e)} finite)")
    if q > 1.0:
        fails.append(f"live guard: |over - scipy's| {q:.3g} times margin.live_over_error")


@pytest.mark.parametrize("case", [pytest.param(c, id=G.welch_case_id(c)) for c in G.welch_cases()])
def test_welch_bins_and_bands_within_the_model(case):
    nperseg, nfft, nov, nseg, block, ss, bands, dt = case
    classes = [c for c in G.WELCH_CLASSES if c != "tiny" or dt == G.F64]
    refs = {cls: G.welch_refs(cls, case) for cls in classes}
    first = refs[classes[0]]
    ctx = dsp.context(0)
    got = {}
    with _Options(ctx, _lib.OPT_WELCH_GOERTZEL if dt == G.I16 else None):
        plan = _lib.WelchPlan(ctx, _welch_cfg(case, first["scale"]), first["w"])
        try:
            for cls in classes:
                x = refs[cls]["x"]
                got[cls] = (plan.psd(x, len(first["bins"])), plan.run(x))
        finally:
            plan.close()
    fails = []
    for cls in classes:
        _check_welch(case, cls, *got[cls], refs[cls], fails)
    if dt == G.F64:  # once per shape
        _check_live_guard(case, ctx, got["fullscale_noise"][1], refs["fullscale_noise"], fails)
    assert not fails, "\n".join(fails)
