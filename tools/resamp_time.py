"""Time the rational resampler's tile kernel (K_RESAMP) beside the down-converter's (K_DDC) in one run, on
int16 audio resident in HBM, float64 out:

* 44.1 kHz -> 4 kHz: 40/441, 3529 taps, 24 rows of one hour each;
* 6 kHz -> 4 kHz: 2/3, 25 taps, a day of one-minute files (1440 rows);
* msd_ddc 48 kHz -> 4 kHz: D 12, 97 taps, 24 rows with as many input samples as the first case;

as the median of 10 timed launches each (after 3 warm-up launches; HIP events around the kernel alone), with
the input samples per second, the bytes moved per input sample (2 in, 8 L / M out), the share of 8 TB/s that
is, the float64 FMAs per second, and the 40/441 case's samples per second as a share of the down-converter's.

usage (GPU box): python3 tools/resamp_time.py [--hours 1.0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0, help="audio per row of the 44.1 kHz case")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "meteor-scatter_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    from meteorgpu import _lib, ddc, resample
    row441 = int(a.hours * 3600 * 44100)
    cases = [  # (label, fs, rows, samples per row)
        ("44.1 kHz -> 4 kHz, 40/441, 3529 taps", 44100, 24, row441),
        ("6 kHz -> 4 kHz, 2/3, 25 taps, a day of minutes", 6000, 1440, 60 * 6000),
        ("ddc 48 kHz -> 4 kHz, D 12, 97 taps", 48000, 24, row441),
    ]
    ctx = _lib.Context(0)
    total = max(rows * n for _, _, rows, n in cases)
    pool = np.random.default_rng(1).integers(-3000, 3000, 2 ** 25).astype(np.int16)
    x = ctx.alloc(2 * total)
    for o in range(0, total, pool.size):
        x.upload(pool[: min(pool.size, total - o)], byte_offset=2 * o)
    print(f"{2 * total / 2 ** 30:.2f} GiB of int16 resident, float64 out, median of 10 launches per case", flush=True)
    rate = {}
    for label, fs, rows, n in cases:
        cfg, taps = resample.lowpass_resampler(fs)
        L, M, ntaps = int(cfg.up), int(cfg.down), int(cfg.ntaps)
        if L == 1:
            dcfg, taps = ddc.lowpass_decimator(fs)
            plan, kid = _lib.DdcPlan(ctx, dcfg, taps, 0, 0), _lib.K_DDC
            count = _lib.ddc_out_len(dcfg, 0, n)[1]
        else:
            plan, kid = _lib.ResampPlan(ctx, cfg, taps, 0, 0), _lib.K_RESAMP
            count = _lib.resamp_out_len(cfg, 0, n)[1]
        off, length, pos0, got = (ctx.alloc(8 * rows) for _ in range(4))
        off.upload(np.arange(rows, dtype=np.int64) * n)
        length.upload(np.full(rows, n, np.int64))
        pos0.upload(np.zeros(rows, np.int64))
        out = ctx.alloc(8 * count * rows)

        def run():
            plan.run_dev(x, _lib.MSD_I16, off, length, pos0, rows, out, count, got)
        for _ in range(3):
            run()
        ctx.synchronize()
        ms = []
        for _ in range(10):
            ctx.timing(True)
            ctx.timing_reset()
            run()
            ctx.synchronize()
            ms.append(ctx.timing_get(kid)[0])
        ctx.timing(False)
        counts = np.empty(rows, np.int64)
        got.download(counts)
        assert np.all(counts == count), (counts[:4], count)
        plan.close()
        out.free()
        ms.sort()
        samples = rows * n
        bps = 2 + 8.0 * L / M
        fma = rows * count * -(-ntaps // L)
        rate[kid] = rate.get(kid) or samples / (ms[5] * 1e-3)
        print(f"{label:48s} {rows:5d} rows of {n:10d}  median {ms[5]:8.3f} ms  min {ms[0]:8.3f}  max {ms[9]:8.3f}  "
              f"{samples / ms[5] * 1e-6:7.2f} Gsample/s in  {bps:5.2f} B/sample  "
              f"{bps * samples / (ms[5] * 1e-3) / HBM_BYTES_PER_S:.3f} of 8 TB/s  {fma / ms[5] * 1e-9:6.2f} TFMA/s",
              flush=True)
    print(f"40/441 input samples per second: {rate[_lib.K_RESAMP] / rate[_lib.K_DDC]:.3f} of the down-converter's "
          f"(expected: no less than 0.5)", flush=True)


if __name__ == "__main__":
    main()
