"""Time the I/Q spectrogram kernels (K_CSTFT) on one stream of int16 I/Q resident in HBM (2 GiB by default):

* cstft_any_kernel at 1024 / hop 256, 2048 / hop 512 and 8192 / hop 2048;
* 4096 / hop 1024 three ways: cstft4096_kernel, cstft_any_kernel under MSD_OPT_GENERIC_CSTFT, and
  cstft_any_kernel at nperseg 4000 / nfft 4096 / hop 1000;

as the median of 10 timed launches each (after 3 warm-up launches; HIP events around the kernel alone), with
the bytes moved per sample (4 in + 4 nfft / hop out), the share of 8 TB/s that is, and the ratio to
cstft4096_kernel on the same box.

usage (GPU box): python3 tools/cstft_any_time.py [--gib 2.0]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 192000.0
HBM_BYTES_PER_S = 8e12
CASES = [  # (label, nperseg, nfft, hop, MSD_OPT_GENERIC_CSTFT)
    ("any 1024/1024/256", 1024, 1024, 256, 0),
    ("any 2048/2048/512", 2048, 2048, 512, 0),
    ("any 8192/8192/2048", 8192, 8192, 2048, 0),
    ("cstft4096 4096/4096/1024", 4096, 4096, 1024, 0),
    ("any 4096/4096/1024 (option)", 4096, 4096, 1024, 1),
    ("any 4000/4096/1000", 4000, 4096, 1000, 0),
]


class _Dev:
    """a torch tensor where _lib wants a DeviceBuffer"""

    def __init__(self, t):
        self.t, self.ptr = t, t.data_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "meteor-scatter_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from meteorgpu import _lib
    from meteorgpu.dsp import hann_periodic
    n = int(a.gib * 2 ** 30) // 4  # complex int16 samples
    ctx = None
    try:  # random samples made on the device; torch first, as tools/i8_time.py does
        g = torch.Generator(device="cuda").manual_seed(1)
        x = _Dev(torch.randint(-3000, 3000, (2 * n,), dtype=torch.int16, device="cuda", generator=g))
        torch.cuda.synchronize()
    except Exception as e:  # no device for torch in this process: a host pool, uploaded in turn
        print(f"torch has no device here ({type(e).__name__}): samples made on the host", flush=True)
        ctx = _lib.Context(0)
        pool = np.random.default_rng(1).integers(-3000, 3000, 2 ** 25).astype(np.int16)
        x = ctx.alloc(4 * n)
        for o in range(0, 2 * n, pool.size):
            x.upload(pool[: min(pool.size, 2 * n - o)], byte_offset=2 * o)
    ctx = ctx or _lib.Context(0)
    off, length = ctx.alloc(8), ctx.alloc(8)
    off.upload(np.zeros(1, np.int64))
    length.upload(np.array([n], np.int64))
    print(f"{n} complex int16 samples resident ({4 * n / 2 ** 30:.2f} GiB), "
          f"median of 10 launches per case", flush=True)
    rows = {}
    for label, nperseg, nfft, hop, opt in CASES:
        ctx.set_option(_lib.OPT_GENERIC_CSTFT, opt)
        w = hann_periodic(nperseg).astype(np.float32)
        plan = _lib.CStftPlan(ctx, nperseg, hop, w, 1.0 / (FS * float((w.astype(np.float64) ** 2).sum())), nfft=nfft)
        T = plan.frames(n)
        out = ctx.alloc(T * nfft * 4)

        def run():
            plan.run_dev(x, _lib.MSD_CI16, off, length, 1, T, out)
        for _ in range(3):
            run()
        ctx.synchronize()
        ms = []
        for _ in range(10):
            ctx.timing(True)
            ctx.timing_reset()
            run()
            ctx.synchronize()
            ms.append(ctx.timing_get(_lib.K_CSTFT)[0])
        ctx.timing(False)
        plan.close()
        out.free()
        ms.sort()
        bps = 4.0 + 4.0 * nfft / hop
        share = bps * n / (ms[5] * 1e-3) / HBM_BYTES_PER_S
        rows[label] = ms[5]
        print(f"{label:30s} {T:8d} frames  median {ms[5]:8.3f} ms  min {ms[0]:8.3f}  max {ms[9]:8.3f}  "
              f"{bps:5.2f} B/sample  {share:.3f} of 8 TB/s  {n / ms[5] * 1e-6:7.2f} Gsample/s", flush=True)
    ctx.set_option(_lib.OPT_GENERIC_CSTFT, 0)
    base = rows["cstft4096 4096/4096/1024"]
    for label in ("any 4096/4096/1024 (option)", "any 4000/4096/1000"):
        print(f"{label} / cstft4096: {rows[label] / base:.3f}", flush=True)


if __name__ == "__main__":
    main()
