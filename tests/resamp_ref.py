"""The two references of the rational-ratio resampler (include/msdsp.h, msd_resamp_*), numpy / scipy only.

    L = up, M = down, c = (ntaps - 1) / 2.  Output m: t = m M + c, phi = t mod L, n0 = t div L,
    v[m] = sum_{i < I_phi} h[phi + i L] z[n0 - i],  z = x (REAL) or x[n] e^{-2 pi i r(n) / q} (SSB),
    r(n) = (n p) mod q in exact integers,  y[m] = gain v[m] (REAL) or gain Re(i^m v[m]) (SSB),
    a row holding samples [pos0, pos0 + N) emits every m with pos0 L <= m M < (pos0 + N) L; samples outside
    the row are zero.

``ref_ld``: long double throughout, computed branch by branch (the outputs k0, k0 + L, ... of a row share the
taps h[phi::L] and their n0 advance by M), never through a zero-stuffed window; the phase factors from
exactly reduced angles (tests/ddc_ref.py).  ``ref_f64``: float64, the phase factors rounded once from the
long-double ones, the filter by ``scipy.signal.upfirdn`` with the lead / lag alignment of
``ddc_ref.ref_f64`` (REAL at pos0 = 0 is ``scipy.signal.resample_poly(x, L, M, window=h / L)``).  ``ref_f64``
also takes the corruptions the tests use to show that the error bar bites.

Samples: a real array (REAL) or a complex array (SSB) of integer- or float32-valued numbers.
"""
import numpy as np
from scipy.signal import upfirdn

from ddc_ref import HALF_PI, LD, U, _demix, _padded, phase_index, unit_ld  # noqa: F401

_win = np.lib.stride_tricks.sliding_window_view


def out_range(pos0: int, n: int, L: int, M: int):
    """(first output index, count)"""
    lo = -((-pos0 * L) // M)
    return lo, -((-(pos0 + n) * L) // M) - lo


def _span(m_lo, count, L, M, ntaps):
    """the global sample range [g0, g1) the outputs m_lo .. m_lo + count - 1 read"""
    c, I = (ntaps - 1) // 2, -(-ntaps // L)
    return (m_lo * M + c) // L - (I - 1), ((m_lo + count - 1) * M + c) // L + 1


def _branchwise(zp, g0, taps, L, M, m_lo, count):
    """v of every output from the padded samples zp (global indices from g0), in zp's dtype"""
    c = (len(taps) - 1) // 2
    v = np.zeros(count, zp.dtype)
    for k0 in range(min(L, count)):  # the outputs k0, k0 + L, ...: one branch, n0 advancing by M
        t = (m_lo + k0) * M + c
        hb = taps[t % L:: L]
        if not len(hb):
            continue
        nb = len(range(k0, count, L))
        start = t // L - (len(hb) - 1) - g0
        v[k0::L] = _win(zp[start:], len(hb))[::M][:nb] @ hb[::-1].astype(zp.dtype)
    return v


def abs_sum(x, taps, L, M, pos0=0):
    """S_m = sum_i |h[phi + i L]| |x[n0 - i]| of every output (float64)"""
    taps = np.abs(np.asarray(taps, np.float64))
    m_lo, count = out_range(pos0, len(x), L, M)
    if count == 0:
        return np.zeros(0)
    g0, g1 = _span(m_lo, count, L, M, len(taps))
    zp = _padded(np.abs(np.asarray(x)).astype(np.float64), pos0, g0, g1, np.float64)
    return _branchwise(zp, g0, taps, L, M, m_lo, count)


def ref_ld(x, taps, L, M, ssb=False, p=0, q=1, gain=1.0, pos0=0) -> np.ndarray:
    """y in long double"""
    taps = np.asarray(taps, np.float64)
    m_lo, count = out_range(pos0, len(x), L, M)
    if count == 0:
        return np.zeros(0, LD)
    g0, g1 = _span(m_lo, count, L, M, len(taps))
    if not ssb:
        zp = _padded(np.asarray(x).astype(LD), pos0, g0, g1, LD)
        return LD(gain) * _branchwise(zp, g0, taps, L, M, m_lo, count)
    xp = _padded(np.asarray(x), pos0, g0, g1, np.complex128)  # (integer or float32 parts: exact)
    r = phase_index(g0, g1 - g0, p, q)
    if q <= 1 << 16:  # every factor once
        ct, st = unit_ld(np.arange(q), q)
        cs, sn = ct[r], st[r]
    else:
        cs, sn = unit_ld(r, q)
    xr, xi = xp.real.astype(LD), xp.imag.astype(LD)
    vr = _branchwise(xr * cs + xi * sn, g0, taps, L, M, m_lo, count)
    vi = _branchwise(xi * cs - xr * sn, g0, taps, L, M, m_lo, count)
    mm = (m_lo + np.arange(count)) & 3
    return LD(gain) * np.where(mm == 0, vr, np.where(mm == 1, -vi, np.where(mm == 2, -vr, vi)))


def ref_ld_long(x, taps, L, M, ssb=False, p=0, q=1, gain=1.0, block=32768) -> np.ndarray:
    """ref_ld of a long row at pos0 = 0, `block` outputs at a time (each from its own samples with their
    halo: a row's interior outputs do not depend on the rest)"""
    count = out_range(0, len(x), L, M)[1]
    out = np.zeros(count, LD)
    for a in range(0, count, block):
        b = min(count, a + block)
        g0, g1 = _span(a, b - a, L, M, len(taps))
        lo, hi = max(0, g0), min(len(x), g1)
        first = out_range(lo, hi - lo, L, M)[0]
        out[a:b] = ref_ld(x[lo:hi], taps, L, M, ssb, p, q, gain, lo)[a - first: b - first]
    return out


def ref_f64(x, taps, L, M, ssb=False, p=0, q=1, gain=1.0, pos0=0, drop_tap=None, c_off=0, phi_off=0, n_off=0,
            swap=False, phase_late=0, im_off=0, wrap64=False, tw32=False) -> np.ndarray:
    """y in float64 by upfirdn.  Corruptions: drop_tap = k sets h[k] to 0; c_off shifts c; phi_off takes the
    taps of branch phi + phi_off; n_off reads z[n0 - n_off - i]; swap exchanges L and M in the filter (at the
    true outputs' count); phase_late takes the phase of sample n - phase_late; im_off rotates the output
    mixer by that many steps; wrap64 forms n p in wrapped 64-bit arithmetic; tw32 rounds the phase factors
    to float32."""
    taps = np.array(taps, np.float64)
    ntaps, c = len(taps), (len(taps) - 1) // 2 + c_off
    if drop_tap is not None:
        taps[drop_tap] = 0.0
    if phi_off:
        taps = np.concatenate([taps[phi_off:], np.zeros(phi_off)])
    m_lo, count = out_range(pos0, len(x), L, M)
    if count == 0:
        return np.zeros(0)
    if swap:
        L, M = M, L
    base = (pos0 // M) * M  # the global index of local sample 0: a multiple of M, so that base L / M is whole
    lead = pos0 - base      # zeros in front of the row, 0 .. M - 1
    if ssb:
        r = phase_index(pos0 - phase_late, len(x), p, q, wrap64)
        cs, sn = unit_ld(r, q)  # (2 pi r / q formed in float64 would itself be off by up to 2 pi u near a full turn)
        w = cs.astype(np.float64) - 1j * sn.astype(np.float64)
        if tw32:
            w = w.astype(np.complex64).astype(np.complex128)
        z = np.asarray(x).astype(np.complex128) * w
    else:
        z = np.asarray(x).astype(np.float64)
    zl = np.concatenate([np.zeros(lead + n_off, z.dtype), z])
    # local output m' = m - base L / M is conv(h, up(zl))[m' M + c]: shift the filter so that the wanted lags
    # fall on multiples of M (as resample_poly does)
    pre = (M - c % M) % M
    hp = np.concatenate([np.zeros(pre), taps])
    full = upfirdn(hp, zl, L, M)
    first = (m_lo - base * L // M) + (c + pre) // M
    v = np.zeros(count, z.dtype)
    got = full[first: first + count]
    v[: len(got)] = got
    if not ssb:
        return gain * v
    return _demix(v, m_lo + im_off, gain)


def plan(L: int, M: int, ntaps: int):
    """(TM, G, K, I) as csrc/resamp_plan.h chooses them: I = ceil(ntaps / L) taps in the longest branch, TM
    outputs per tile by the LDS budget (two planes of ceil((TM - 1) M / L) + I staged samples made even, I L
    taps, 256 partial sums; 64 KB preferred, 150 KB at the most), G = 256 / TM groups of K = ceil(I / G)"""
    I = -(-ntaps // L)

    def tile_bytes(tm):
        smax = -(-(tm - 1) * M // L) + I
        return 8 * (2 * ((smax + 1) & ~1) + I * L + 256)
    sizes = (256, 128, 64, 32, 16, 8, 4, 2, 1)
    TM = next((tm for tm in sizes if tile_bytes(tm) <= 64 * 1024), None) or \
        next(tm for tm in sizes if tile_bytes(tm) <= 150 * 1024)
    G = 256 // TM
    return TM, G, -(-I // G), I


def chain_py(ssb: bool, L: int, M: int, ntaps: int, q: int = 1) -> float:
    """the header's count restated: the mix (0, 5 with one table, 9 with two), K FMAs of the longest group
    chain, G - 1 adds of the partial sums, the gain"""
    _, G, K, _ = plan(L, M, ntaps)
    return (0 if not ssb else (9 if q > 4096 else 5)) + K + (G - 1) + 1
