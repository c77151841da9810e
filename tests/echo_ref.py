"""numpy float64 restatement of the echo measurement (include/msdsp.h, "echo measurement"): the span, the
per-frame values with the explicit ascending-k loop, and the record.  Independent of csrc/echo_plan.h; the GPU
tests hold the kernel to it and tests/test_echo_ref.py pins it to hand-made cases.

``measure(spec, frames, dets, cfg)`` takes one file's spectrogram [K][ld] (any float dtype; only columns below
``frames`` are read), its stored detections (structured start / stop, in blocks) and a dict with the fields of
msd_echo_cfg, and returns (records, terms): records in ECHO_DTYPE, terms[i][name] = sum of |term| of each of
the six sums of detection i (the tolerance of a free summation order is stated against them)."""
import numpy as np

ECHO_DTYPE = np.dtype([("t0", np.int64), ("t1", np.int64), ("t_peak", np.int64), ("t_half_first", np.int64),
                       ("t_half_last", np.int64), ("t_efold", np.int64), ("k_peak", np.int32), ("flags", np.int32),
                       ("p_peak", np.float64), ("n_peak", np.float64), ("d_peak", np.float64),
                       ("e_sig", np.float64), ("e_noise", np.float64), ("w_r", np.float64), ("w_u", np.float64),
                       ("w_uu", np.float64), ("w_ur", np.float64)])
DET_DTYPE = np.dtype([("start", np.int64), ("stop", np.int64), ("db", np.float64)])
SUMS = ("e_sig", "e_noise", "w_r", "w_u", "w_uu", "w_ur")
INV_E = 0.36787944117144233


def cfg(block_size, nperseg, hop, band, noise=(0, -1), pre=0, post=0):
    return dict(block_size=int(block_size), nperseg=int(nperseg), hop=int(hop), k_lo=int(band[0]), k_hi=int(band[1]),
                n_lo=int(noise[0]), n_hi=int(noise[1]), pre_frames=int(pre), post_frames=int(post))


def first_frame_at(s: int, nperseg: int, hop: int) -> int:
    """c(s): the lowest t >= 0 with t hop + nperseg // 2 >= s (python integers)"""
    t = 0
    need = s - nperseg // 2
    if need > 0:
        t = -(-need // hop)
    assert t * hop + nperseg // 2 >= s and (t == 0 or (t - 1) * hop + nperseg // 2 < s)
    return t


def core(det, c, T):
    return (min(T, first_frame_at(int(det["start"]) * c["block_size"], c["nperseg"], c["hop"])),
            min(T, first_frame_at(int(det["stop"]) * c["block_size"], c["nperseg"], c["hop"])))


def span(dets, i, c, T):
    """(a0, a1, t0, t1) of detection i among the stored detections ``dets`` of a file with T frames"""
    a0, a1 = core(dets[i], c, T)
    lo = core(dets[i - 1], c, T)[1] if i > 0 else 0
    hi = core(dets[i + 1], c, T)[0] if i + 1 < len(dets) else T
    t0 = max(a0 - c["pre_frames"], min(lo, a0), 0)
    t1 = min(a1 + c["post_frames"], max(hi, a1), T)
    return a0, a1, t0, t1


def column(spec, t, c):
    """(S, N, k*, delta) of frame t: float64, each cell converted once, ascending k from 0.0"""
    K = spec.shape[0]
    S = np.float64(0.0)
    kb, best = c["k_lo"], np.float64(spec[c["k_lo"], t])
    for k in range(c["k_lo"], c["k_hi"] + 1):
        v = np.float64(spec[k, t])
        S = S + v
        if v > best:
            kb, best = k, v
    N = np.float64(0.0)
    for k in range(c["n_lo"], c["n_hi"] + 1):
        N = N + np.float64(spec[k, t])
    delta = np.float64(0.0)
    if 0 < kb < K - 1:
        a, b, cc = np.float64(spec[kb - 1, t]), best, np.float64(spec[kb + 1, t])
        den = (a - np.float64(2.0) * b) + cc
        if den < 0:
            delta = np.float64(0.5) * (a - cc) / den
    return S, N, kb, delta


def measure(spec, frames, dets, c):
    T = int(frames)
    out = np.zeros(len(dets), ECHO_DTYPE)
    terms = []
    for i in range(len(dets)):
        a0, a1, t0, t1 = span(dets, i, c, T)
        e = out[i]
        e["t0"], e["t1"] = t0, t1
        flags = (1 if t0 > a0 - c["pre_frames"] else 0) | (2 if t1 < a1 + c["post_frames"] else 0)
        tr = dict.fromkeys(SUMS, 0.0)
        if t1 <= t0:
            for name in ("t_peak", "t_half_first", "t_half_last", "t_efold"):
                e[name] = t0
            e["k_peak"], e["flags"], e["p_peak"], e["n_peak"] = -1, flags, np.nan, np.nan
            terms.append(tr)
            continue
        cols = [column(spec, t, c) for t in range(t0, t1)]
        S = np.array([x[0] for x in cols], np.float64)
        ip = int(np.flatnonzero(S == S.max())[0])  # the lowest frame attaining the maximum
        p = S[ip]
        e["p_peak"], e["t_peak"] = p, t0 + ip
        e["n_peak"], e["k_peak"], e["d_peak"] = cols[ip][1], cols[ip][2], cols[ip][3]
        at_half = np.flatnonzero(S >= np.float64(0.5) * p)
        e["t_half_first"], e["t_half_last"] = t0 + int(at_half[0]), t0 + int(at_half[-1])
        below = np.flatnonzero(S[ip + 1:] <= p * np.float64(INV_E))
        e["t_efold"] = t0 + ip + 1 + int(below[0]) if below.size else t1
        acc = dict.fromkeys(SUMS, np.float64(0.0))
        for j, (s, n, k, d) in enumerate(cols):
            u = np.float64(j)
            r = np.float64(k - c["k_lo"]) + d
            su = s * u
            for name, v in (("e_sig", s), ("e_noise", n), ("w_r", s * r), ("w_u", su), ("w_uu", su * u),
                            ("w_ur", su * r)):
                acc[name] = acc[name] + v
                tr[name] += abs(float(v))
        for name in SUMS:
            e[name] = acc[name]
        e["flags"] = flags | (4 if e["t_efold"] == t1 else 0) | (8 if ip == 0 or ip == t1 - t0 - 1 else 0)
        terms.append(tr)
    return out, terms
