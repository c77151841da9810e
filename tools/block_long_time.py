"""Time the block band energies (K_BLOCK: the band kernel + block_db_kernel) of the C3 day shape,
1440 files x 300 blocks of 9600 int16 samples (48 kHz, 0.2 s) resident in HBM, with the reference's
f0 +- 10 Hz bands:

* n_fft = 8192 (nfft 16384, L = 9600): block_long_kernel;
* n_fft = 2048 (nfft 4096, L = 4096): block_delta2_kernel at its longest segment, the yardstick per
  sample and bin;
* n_fft = 512 (nfft 1024, L = 1024): the existing path (int16: the int8 matrix-core kernel) and,
  under MSD_OPT_BLOCK_GOERTZEL, block_delta2_kernel;

as the median of 10 timed calls each, in ms and in ns per sample and bin, with the share of the FP64
vector peak at the Goertzel's 2 float64 instructions per sample and bin (78.6 TFLOP/s = 39.3e12
instructions a second), and the CPU oracle's time for 150 of the files on one core.

usage (GPU box): python3 tools/block_long_time.py [--files 1440] [--oracle-files 150]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, BLOCK_SEC, BLOCKS = 48000, 0.2, 300
BAND, NOISE = (993.0, 1013.0), (690.0, 710.0)
FP64_INSTR_PER_S = 78.6e12 / 2


class _Dev:
    """a torch tensor where _lib wants a DeviceBuffer"""

    def __init__(self, t):
        self.t, self.ptr = t, t.data_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1440)
    ap.add_argument("--oracle-files", type=int, default=150)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "meteor-scatter_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from meteorgpu import _lib, dsp
    B = int(FS * BLOCK_SEC)
    F, n = a.files, BLOCKS * B
    ctx = None
    try:  # random samples made on the device; torch first, as tools/i8_time.py does
        g = torch.Generator(device="cuda").manual_seed(1)
        x = _Dev(torch.randint(-3000, 3000, (F * n,), dtype=torch.int16, device="cuda", generator=g))
        torch.cuda.synchronize()
        one = x.t[:n].cpu().numpy()
    except Exception as e:  # no device for torch in this process: a pool of 8 host files, uploaded in turn
        print(f"torch has no device here ({type(e).__name__}): samples made on the host", flush=True)
        ctx = _lib.Context(0)
        rng = np.random.default_rng(1)
        pool = [rng.integers(-3000, 3000, n).astype(np.int16) for _ in range(8)]
        x = ctx.alloc(F * n * 2)
        for i in range(F):
            x.upload(pool[i % 8], byte_offset=i * n * 2)
        one = pool[0]
    ctx = ctx or _lib.Context(0)
    off, length = ctx.alloc(F * 8), ctx.alloc(F * 8)
    off.upload(np.arange(F, dtype=np.int64) * n)
    length.upload(np.full(F, n, dtype=np.int64))
    out = [ctx.alloc(F * BLOCKS * 8) for _ in range(3)]
    rows = []
    for n_fft, goertzel in ((8192, False), (2048, True), (512, False), (512, True)):
        nfft = 2 * n_fft
        L = min(B, nfft)
        band, noise = dsp.band_bins(nfft, FS, BAND), dsp.band_bins(nfft, FS, NOISE)
        nbins = band[1] - band[0] + 1 + noise[1] - noise[0] + 1
        ctx.set_option(_lib.OPT_BLOCK_GOERTZEL, 1 if goertzel else 0)
        plan = _lib.BlockPlan(ctx, B, nfft, dsp.hanning_sym(B)[:L], band, noise)

        def run():
            plan.run_dev(x, np.int16, off, length, F, BLOCKS, out[0], out[1], out[2], BLOCKS)
        for _ in range(3):
            run()
        ctx.synchronize()
        ms = []
        for _ in range(10):
            ctx.timing(True)
            ctx.timing_reset()
            run()
            ctx.synchronize()
            ms.append(ctx.timing_get(_lib.K_BLOCK)[0])
        ctx.timing(False)
        plan.close()
        ms.sort()
        per = ms[5] * 1e6 / (F * BLOCKS * L * nbins)
        peak = 2.0 * F * BLOCKS * L * nbins / (ms[5] * 1e-3) / FP64_INSTR_PER_S
        rows.append((n_fft, L, nbins, goertzel, ms[5], ms[0], per, peak))
        print(f"n_fft {n_fft:5d} L {L:5d} bins {nbins:3d} {'goertzel' if goertzel or L > 4096 else 'default ':8s} "
              f"median {ms[5]:9.4f} ms  min {ms[0]:9.4f}  {per:.5f} ns per sample and bin  "
              f"{peak:.3f} of the FP64 vector peak at 2 instructions", flush=True)
    ctx.set_option(_lib.OPT_BLOCK_GOERTZEL, 0)
    print(f"long / L = 4096 Goertzel per sample and bin: {rows[0][6] / rows[1][6]:.3f}; "
          f"long / L = 1024 Goertzel: {rows[0][6] / rows[3][6]:.3f}", flush=True)
    if a.oracle_files > 0:
        from oracle import dsp_oracle as O
        xs = one
        t0 = time.perf_counter()
        for _ in range(a.oracle_files):
            O.block_powers_ref(xs, FS, BLOCK_SEC, BAND, NOISE, 8192)
        dt = time.perf_counter() - t0
        print(f"oracle.block_powers_ref, n_fft 8192, one core: {dt:.2f} s for {a.oracle_files} files = "
              f"{dt / a.oracle_files * 1e3:.1f} ms a file; the device's {rows[0][4] / F:.5f} ms a file", flush=True)


if __name__ == "__main__":
    main()
