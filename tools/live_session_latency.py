#!/usr/bin/env python3
"""Latency of a steady-state live-session push against the one-shot path over the same audio.

For 1 and 24 streams of 4 kHz int16 audio: one push of 30 s (150 blocks of 0.2 s) per stream through
``msd_live_session_push_samples_dev`` -- the samples already in HBM, as the one-shot batch has them --
against ``LiveBatch.run()`` (``msd_welch_bands_dev`` + ``msd_live_detect_dev``) over the same 30 s per
stream, in the same process, alternating the two in groups.  Each call is timed with a host clock around
enqueue + device synchronise (the call's latency as a station sees it); the per-kernel split comes from
the library's event timers (``msd_timing_*``: Welch and detector kernels) in a pass of its own.

    python tools/live_session_latency.py [--out profiles/live_session_latency.txt]

Needs the GPU; there is no fallback."""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "meteor-scatter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS, SEC = 4000, 30.0


def measure(nstreams: int, groups: int, per_group: int, warmup: int):
    from meteorgpu import _lib, live, synth
    from meteorgpu.dsp import context
    ctx = context(0)
    cfg = live.ConfigDetection(detection_db_over_noise_mean_min=1, detection_dur_min_sec=0.4)
    n = int(SEC * FS)
    xs = [synth.synth_real(seed=4000 + i, fs=FS, duration_s=SEC, f0=1000.0, sigma=300.0, rate_per_min=12,
                           band_hz=100.0, snr_db=(15, 30), dur_s=(0.4, 2.0))[0] for i in range(nstreams)]
    batch = live.LiveBatch(ctx, nstreams, n, FS, cfg)
    for i, x in enumerate(xs):
        batch.upload_file(i, x)
    sess = live.LiveSession(FS, cfg, nstreams=nstreams, max_push_sec=SEC)
    sess.d_x.upload(np.concatenate(xs))
    sess.d_off.upload(np.arange(nstreams, dtype=np.int64) * n)
    sess.d_len.upload(np.full(nstreams, n, np.int64))
    lib = ctx.lib

    def push():
        _lib.check(lib.msd_live_session_push_samples_dev(
            sess.h, sess.d_x.ptr, sess.d_off.ptr, sess.d_len.ptr, n, sess.d_met.ptr, sess.cap, sess.d_counts.ptr,
            sess.d_newb.ptr, sess.d_band.ptr, sess.d_thr.ptr, sess.d_over.ptr, sess.P, sess.d_status.ptr))

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(warmup):  # the session is past Init and holds a full history window afterwards
        timed(push)
        timed(batch.run)
    t_push, t_run = [], []
    for _ in range(groups):  # alternate, so that drift on a shared host hits both alike
        t_push += [timed(push) for _ in range(per_group)]
        t_run += [timed(batch.run) for _ in range(per_group)]
    split = {}
    ctx.timing(True)
    for name, fn in (("push", push), ("one-shot", batch.run)):
        ctx.timing_reset()
        for _ in range(per_group):
            fn()
        ctx.synchronize()
        split[name] = {k: ctx.timing_get(kid) for k, kid in (("welch", _lib.K_WELCH), ("detector", _lib.K_LIVE))}
    ctx.timing(False)
    status = [s.status for s in sess.raw_state]
    blocks = sess.blocks
    sess.close()
    batch.close()
    return t_push, t_run, split, per_group, blocks, status


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--per-group", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    lines = [f"live session push vs one-shot LiveBatch.run(), 30 s of 4 kHz int16 per stream (150 blocks), "
             f"{datetime.date.today().isoformat()}",
             f"host clock around enqueue + synchronise, {a.groups} alternating groups of {a.per_group} calls after "
             f"{a.warmup} warm-up calls; per-kernel: msd_timing events, ms per call"]
    for F in (1, 24):
        tp, tr, split, k, blocks, status = measure(F, a.groups, a.per_group, a.warmup)
        mp, mr = statistics.median(tp), statistics.median(tr)
        q = lambda v: (np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
        lines.append(f"streams {F:2d}: push median {mp:.4f} ms (p10 {q(tp)[0]:.4f}, p90 {q(tp)[1]:.4f}); "
                     f"one-shot median {mr:.4f} ms (p10 {q(tr)[0]:.4f}, p90 {q(tr)[1]:.4f}); "
                     f"push / one-shot = {mp / mr:.3f}")
        for name in ("push", "one-shot"):
            w, d = split[name]["welch"], split[name]["detector"]
            lines.append(f"    {name:8s} kernels: welch {w[0] / k:.4f} ms ({w[1] // k} timed span(s) per call), "
                         f"detector {d[0] / k:.4f} ms ({d[1] // k} per call)")
        lines.append(f"    session after the run: {blocks[0]} blocks per stream, status {sorted(set(status))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
