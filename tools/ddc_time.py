"""Time the decimating down-converter's tile kernel (K_DDC) on one row resident in HBM (2 GiB by default):

* int16 I/Q (MSD_CI16), D = 48, 385 taps (the C5 configuration), tuned by p / q = 5 / 32 (one phase table)
  and by 12345 / 192000 (the product of two table entries);
* real int16 audio, D = 12, 97 taps;

as the median of 10 timed launches each (after 3 warm-up launches; HIP events around the kernel alone), with
the bytes moved per input sample (its size in, 8 / D out), the share of 8 TB/s that is, and, as the CPU
figure, scipy.signal.upfirdn on 2^22 of the same samples (mixed by numpy for the I/Q cases) on one core.

usage (GPU box): python3 tools/ddc_time.py [--gib 2.0]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12
CASES = [  # (label, ssb, D, ntaps, p, q)
    ("I/Q int16 D 48, 385 taps, q 32", True, 48, 385, 5, 32),
    ("I/Q int16 D 48, 385 taps, q 192000", True, 48, 385, 12345, 192000),
    ("real int16 D 12, 97 taps", False, 12, 97, 0, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")  # (the CPU figure is one core's)
    sys.path.insert(0, os.path.join(ROOT, "meteor-scatter_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    from scipy.signal import upfirdn
    from meteorgpu import _lib, ddc
    nbytes = int(a.gib * 2 ** 30)
    ctx = _lib.Context(0)
    pool = np.random.default_rng(1).integers(-3000, 3000, 2 ** 25).astype(np.int16)
    x = ctx.alloc(nbytes)
    for o in range(0, nbytes // 2, pool.size):
        x.upload(pool[: min(pool.size, nbytes // 2 - o)], byte_offset=2 * o)
    print(f"{nbytes / 2 ** 30:.2f} GiB of int16 resident, median of 10 launches per case", flush=True)
    for label, ssb, D, ntaps, p, q in CASES:
        es = 4 if ssb else 2
        n = nbytes // es
        taps = ddc.design_lowpass(ntaps, 0.9 / D)
        cfg = _lib.MsdDdcCfg(_lib.DDC_SSB if ssb else _lib.DDC_REAL, D, ntaps, _lib.MSD_F64, p, q, 1.0)
        plan = _lib.DdcPlan(ctx, cfg, taps, 0, 0)
        _, count = _lib.ddc_out_len(cfg, 0, n)
        meta = [ctx.alloc(8) for _ in range(4)]
        for b, v in zip(meta, (0, n, 0)):
            b.upload(np.array([v], np.int64))
        out = ctx.alloc(8 * count)
        code = _lib.MSD_CI16 if ssb else _lib.MSD_I16

        def run():
            plan.run_dev(x, code, meta[0], meta[1], meta[2], 1, out, count, meta[3])
        for _ in range(3):
            run()
        ctx.synchronize()
        ms = []
        for _ in range(10):
            ctx.timing(True)
            ctx.timing_reset()
            run()
            ctx.synchronize()
            ms.append(ctx.timing_get(_lib.K_DDC)[0])
        ctx.timing(False)
        plan.close()
        out.free()
        ms.sort()
        bps = es + 8.0 / D
        share = bps * n / (ms[5] * 1e-3) / HBM_BYTES_PER_S
        # the CPU figure: the same operation by numpy + upfirdn on 2^22 samples, one core
        m = 2 ** 22
        v = pool[: m * (2 if ssb else 1)].astype(np.float64)
        t0 = time.perf_counter()
        if ssb:
            z = (v[0::2] + 1j * v[1::2]) * np.exp(-2j * np.pi * ((np.arange(m) * p) % q) / q)
            y = upfirdn(taps, z, 1, D)
            y = (y * 1j ** (np.arange(len(y)) % 4)).real
        else:
            y = upfirdn(taps, v, 1, D)
        cpu = time.perf_counter() - t0
        print(f"{label:36s} {n:11d} samples  median {ms[5]:8.3f} ms  min {ms[0]:8.3f}  max {ms[9]:8.3f}  "
              f"{bps:5.2f} B/sample  {share:.3f} of 8 TB/s  {n / ms[5] * 1e-6:7.2f} Gsample/s  "
              f"(CPU, one core: {m / cpu * 1e-6:6.2f} Msample/s, {len(y)} outputs)", flush=True)


if __name__ == "__main__":
    main()
