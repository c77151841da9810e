#!/usr/bin/env python3
"""A/B of the whole-band Welch row: the pruned-FFT kernel (``msd_welch_spectrum_dev``, csrc/welch_fft.hip)
against the band kernels asked for every bin (``msd_welch_bands_dev`` with one band 0 .. nfft/2 and a PSD
buffer -- what ``msd_welch_psd`` launches), on the same samples resident in HBM.

Input: 4 files x 18 000 blocks of int16 noise at the live default shape (block 800, nperseg 256,
noverlap 128, nfft 4096): 1.18 GB of float64 rows per launch.  int16 samples take the band path's
int8 matrix-core kernel by default (csrc/welch_i8.hip); ``MSD_OPT_WELCH_GOERTZEL`` puts them on the
float64 Goertzel kernel (csrc/live.hip), the path of every other sample format.  Both are timed.

Kernel times are the library's device events (``msd_timing_*``: id 4 the band kernels, id 12 the
spectrum kernel), one launch per timed span, the three variants alternating in groups after a warm-up
of each.  The roofline figure is the spectrum kernel's algorithmic bytes -- 2 B per sample in,
8 K + 8 B per block out -- over its time, as a fraction of the HBM peak (8.0 TB/s).  The rows of the
two paths are compared on the first and last file.

    python tools/welch_spectrum_ab.py [--out profiles/welch_spectrum_ab.txt]

Needs the GPU; there is no fallback."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "meteor-scatter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS, FILES, BLOCKS = 4000, 4, 18000
HBM_PEAK = 8.0e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--per-group", type=int, default=4)
    ap.add_argument("--files", type=int, default=FILES)
    ap.add_argument("--blocks", type=int, default=BLOCKS)
    a = ap.parse_args(argv)
    from meteorgpu import _lib, live
    from meteorgpu.dsp import context
    ctx = context(0)
    cfg = live.ConfigDetection()
    c, win = live.welch_cfg(FS, cfg, 1.0 / 32768.0)
    B, K = int(c.block_size), int(c.nfft) // 2 + 1
    c.nbands = 1
    c.band_lo[0], c.band_hi[0] = 0, K - 1
    F, NB = a.files, a.blocks
    n = NB * B
    rng = np.random.default_rng(12)
    x = rng.integers(-20000, 20000, F * n).astype(np.int16)
    plan = _lib.WelchPlan(ctx, c, win)
    d_x, d_off, d_len = ctx.alloc(x.nbytes), ctx.alloc(8 * F), ctx.alloc(8 * F)
    d_x.upload(x)
    d_off.upload(np.arange(F, dtype=np.int64) * n)
    d_len.upload(np.full(F, n, np.int64))
    d_rows, d_db, d_band = ctx.alloc(F * NB * K * 8), ctx.alloc(F * NB * 8), ctx.alloc(F * NB * 8)

    def bands():
        plan.run_dev(d_x, np.int16, d_off, d_len, F, NB, d_band, NB, d_rows)

    def spectrum():
        plan.spectrum_dev(d_x, np.int16, d_off, d_len, F, NB, d_rows, NB, d_db)

    def rows_of(f):
        out = np.empty((NB, K))
        d_rows.download(out, f * NB * K * 8)
        return out

    variants = (("bands, int8 matrix cores (default)", 0, bands, _lib.K_WELCH),
                ("bands, float64 Goertzel", 1, bands, _lib.K_WELCH),
                ("spectrum, pruned FFT", 0, spectrum, _lib.K_WSPEC))
    times = {name: [] for name, *_ in variants}
    kept, spans = {}, {}
    ctx.timing(True)
    for g in range(a.groups + 1):  # group 0: warm-up, and the rows for the comparison
        for name, goertzel, fn, kid in variants:
            ctx.set_option(_lib.OPT_WELCH_GOERTZEL, goertzel)
            for _ in range(a.per_group if g else 1):
                ctx.timing_reset()
                fn()
                ctx.synchronize()
                ms, launches = ctx.timing_get(kid)
                spans[name] = launches
                if g:
                    times[name].append(ms)
            if not g:
                kept[name] = (rows_of(0), rows_of(F - 1))
    ctx.set_option(_lib.OPT_WELCH_GOERTZEL, 0)
    ctx.timing(False)
    lines = [f"whole-band Welch rows, {F} files x {NB} blocks of int16 at block {B}, nperseg {int(c.nperseg)}, noverlap "
             f"{int(c.noverlap)}, nfft {int(c.nfft)} ({F * NB * K * 8 / 1e9:.2f} GB of rows), {datetime.date.today().isoformat()}",
             f"device events per launch (msd_timing), {a.groups} alternating groups of {a.per_group} launches after one "
             f"warm-up launch of each"]
    med = {}
    for name, *_ in variants:
        v = times[name]
        med[name] = statistics.median(v)
        lines.append(f"  {name:36s} median {med[name]:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)}, "
                     f"{spans[name]} timed span(s) per launch)")
    new = med[variants[2][0]]
    for name, *_ in variants[:2]:
        lines.append(f"  {name} / spectrum = {med[name] / new:.2f}")
    bytes_alg = F * NB * (2 * B + 8 * K + 8)
    lines.append(f"  spectrum kernel: {bytes_alg / 1e9:.3f} GB algorithmic (2 B per sample in, 8 K + 8 B per block out) in "
                 f"{new:.3f} ms = {bytes_alg / (new * 1e-3) / 1e12:.2f} TB/s = {bytes_alg / (new * 1e-3) / HBM_PEAK:.1%} of the "
                 f"HBM peak ({HBM_PEAK / 1e12:.1f} TB/s)")
    ref = kept[variants[1][0]]
    for name in (variants[0][0], variants[2][0]):
        d = max(float(np.max(np.abs(kept[name][i] - ref[i]) / np.max(ref[i], axis=1, keepdims=True))) for i in (0, 1))
        lines.append(f"  rows, {name} against the Goertzel rows: max |difference| / row maximum = {d:.3g}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    plan.close()
    for b in (d_x, d_off, d_len, d_rows, d_db, d_band):
        b.free()
    return 0


if __name__ == "__main__":
    sys.exit(main())
