"""Time of the echo measurement in the day batch: the bench's C3 day (1440 files of 2 880 000
int16 samples, seeds 3000 + i) through BatchPipeline with and without with_echoes and, with --baseline DIR,
through another build of the package (a checkout of the commit before, DIR = its meteor-scatter_amd with
libmsdsp.so built): the echo kernel's time from HIP events (timing id 16), every kernel's time per step from
HIP events, and the step's time from a host clock around groups of back-to-back steps that end in a
synchronise (medians).  The day is synthesised once, before any GPU call; each build runs twice, alternating,
each run in a fresh forked child.  One JSON line per run, also written to --out.

    python tools/echo_time.py [--files 1440] [--baseline DIR] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILES = 1440
GROUPS, STEPS = 9, 8


def child(pkg_root, pool, tag, q):
    try:
        q.put(measure(pkg_root, pool, tag))
    except BaseException as e:  # the parent stops at the first failure
        q.put({"tag": tag, "error": repr(e)})
        raise


def measure(pkg_root, pool, tag):
    sys.path.insert(0, pkg_root)
    from meteorgpu import _lib
    from meteorgpu.batch import BatchPipeline
    import bench
    ctx = _lib.Context(0)
    n = bench.FS * bench.SECONDS
    kw = dict(nperseg=bench.NPERSEG, noverlap=bench.NOVERLAP, freq_band=bench.BAND, noise_band=bench.NOISE)
    off = BatchPipeline(ctx, FILES, n, bench.FS, **kw)
    for i in range(FILES):
        off.upload_file(i, pool[i])
    variants = {"off": off}
    if tag == "new":
        on = BatchPipeline(ctx, FILES, n, bench.FS, with_echoes=True, **kw)
        on.xmax = off.xmax
        variants["on"] = on
    res = {"tag": tag}

    def group(bp):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            bp.run(x=off.d_x)
        ctx.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3
    for bp in variants.values():
        group(bp)  # warm-up
    times = {k: [] for k in variants}
    for _ in range(GROUPS):  # alternate the variants
        for k, bp in variants.items():
            times[k].append(group(bp))
    for k, v in times.items():
        res[f"step_ms_{k}"] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "groups": len(v),
                               "steps_per_group": STEPS}
    # per-kernel HIP events, one step at a time (ids: 0 STFT, 1 block delta, 2 / 3 detector, 16 echo)
    ids = [0, 1, 2, 3] + ([16] if tag == "new" else [])
    for k, bp in variants.items():
        ctx.timing(True)
        per = {i: [] for i in ids}
        for _ in range(GROUPS):
            ctx.timing_reset()
            bp.run(x=off.d_x)
            ctx.synchronize()
            for i in ids:
                per[i].append(ctx.timing_get(i)[0])
        ctx.timing(False)
        res[f"kernel_ms_{k}"] = {str(i): float(np.median(v)) for i, v in per.items()}
        res[f"kernel_sum_ms_{k}"] = float(np.median(np.sum([per[i] for i in ids], axis=0)))
        if 16 in per and k == "on":
            res["echo_ms"] = {"median": float(np.median(per[16])), "min": min(per[16]), "max": max(per[16]),
                              "steps": len(per[16])}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dets, counts, status, _ = variants[next(reversed(variants))].detections()
    res["detections"] = int(np.minimum(counts, off.cap).sum())
    res["cap"], res["T"], res["K"] = off.cap, off.T, off.K
    if tag == "new":
        rec = on.echoes()
        res["echo_records"] = int(sum(r.shape[0] for r in rec))
        allr = np.concatenate(rec)
        res["span_frames_mean"] = float((allr["t1"] - allr["t0"]).mean()) if allr.size else 0.0
        res["echo_bins"] = [list(b) for b in on.echo_bins]
        res["echo_pad"] = [on.echo_cfg.pre_frames, on.echo_cfg.post_frames]
    return res


def main():
    global FILES
    import multiprocessing as mp
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=FILES)
    ap.add_argument("--baseline", default=None, help="meteor-scatter_amd of another build to time beside this one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.files < 2:  # one file would be synthesised in this process, which would import this build's package
        ap.error("--files must be at least 2")
    FILES = a.files
    t0 = time.time()
    pool = bench.synth_rows("real", bench.day_seeds(0, 0, FILES), bench.FS * bench.SECONDS, fs=bench.FS,
                            duration_s=bench.SECONDS, f0=1000.0)
    print(f"synthesised {FILES} files in {time.time() - t0:.1f} s", flush=True)
    new_root = os.path.join(ROOT, "meteor-scatter_amd")
    runs = [("new", new_root)] * 2
    if a.baseline:
        old_root = os.path.abspath(a.baseline)
        runs = [("parent", old_root), ("new", new_root)] * 2
    out = []
    fork = mp.get_context("fork")
    for tag, root in runs:
        q = fork.Queue()
        p = fork.Process(target=child, args=(root, pool, tag, q))
        p.start()
        try:
            res = q.get(timeout=600)
        except Exception:
            p.kill()
            print(f"{tag}: no result; stopping", flush=True)
            break
        p.join(60)
        if p.exitcode != 0 or "error" in res:
            print(json.dumps(res), flush=True)
            print(f"{tag}: exit {p.exitcode}; stopping", flush=True)
            break
        print(json.dumps(res), flush=True)
        out.append(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    return 0 if len(out) == len(runs) else 1


if __name__ == "__main__":
    sys.exit(main())
