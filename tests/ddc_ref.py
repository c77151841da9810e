"""The two references of the decimating down-converter (include/msdsp.h, msd_ddc_*), numpy / scipy only.

    v[m] = sum_k h[k] z[m D + c - k],  c = (ntaps - 1) / 2,  z = x (REAL) or x[n] e^{-2 pi i r(n) / q} (SSB),
    r(n) = (n p) mod q in exact integers,  y[m] = gain v[m] (REAL) or gain Re(i^m v[m]) (SSB),
    a row holding samples [pos0, pos0 + N) emits every m with pos0 <= m D < pos0 + N; samples outside the
    row are zero.

``ref_ld``: long double throughout, the phase factors from exactly reduced angles; its own error is a few
2^-64 per term, 2^-11 of the float64 unit.  ``ref_f64``: float64, the filter by ``scipy.signal.upfirdn``
(REAL at pos0 = 0 is then exactly ``scipy.signal.resample_poly(x, 1, D, window=h)``).  ``ref_f64`` also
takes the corruptions the tests use to show that the error bar bites.

Samples: a real array (REAL) or a complex array (SSB) of integer- or float32-valued numbers.
"""
import numpy as np
from scipy.signal import upfirdn

U = 2.0 ** -53
LD = np.longdouble
HALF_PI = LD("1.57079632679489661923132169163975144")


def out_range(pos0: int, n: int, D: int):
    """(first output index, count)"""
    lo = -((-pos0) // D)
    return lo, -((-(pos0 + n)) // D) - lo


def phase_index(n0: int, count: int, p: int, q: int, wrap64: bool = False) -> np.ndarray:
    """r(n) for n = n0 .. n0 + count - 1 (n0 any Python int); wrap64: the corruption that forms n p in
    wrapped 64-bit arithmetic without reducing n first"""
    if wrap64:  # (int64: the product wraps from 2^63 on)
        return np.array([((((n0 + j) * p + (1 << 63)) % (1 << 64)) - (1 << 63)) % q for j in range(count)], np.int64)
    base = ((n0 % q) * p) % q
    return (base + (np.arange(count, dtype=np.int64) % q) * p) % q


def unit_ld(r: np.ndarray, q: int):
    """(cos, sin) of 2 pi r / q in long double: r / q reduced exactly to j quarter turns + (pi / 2) num / q"""
    r = np.asarray(r, np.int64)
    j = (8 * r + q) // (2 * q)
    num = 4 * r - j * q
    a = num.astype(LD) / LD(q) * HALF_PI
    ca, sa = np.cos(a), np.sin(a)
    j = j & 3
    c = np.where(j == 0, ca, np.where(j == 1, -sa, np.where(j == 2, -ca, sa)))
    s = np.where(j == 0, sa, np.where(j == 1, ca, np.where(j == 2, -sa, -ca)))
    return c, s


def _padded(x, pos0, g0, g1, dtype):
    """the samples of global indices [g0, g1), zero outside the row [pos0, pos0 + len(x))"""
    out = np.zeros(g1 - g0, dtype)
    lo, hi = max(g0, pos0), min(g1, pos0 + len(x))
    if hi > lo:
        out[lo - g0: hi - g0] = x[lo - pos0: hi - pos0]
    return out


def _windows(zp, ntaps, D, count):
    return np.lib.stride_tricks.sliding_window_view(zp, ntaps)[::D][:count]


def abs_sum(x, taps, D, pos0=0):
    """S_m = sum_k |h_k| |x_{m D + c - k}| of every output (float64)"""
    taps = np.asarray(taps, np.float64)
    ntaps, c = len(taps), (len(taps) - 1) // 2
    m_lo, count = out_range(pos0, len(x), D)
    if count == 0:
        return np.zeros(0)
    g0 = m_lo * D + c - (ntaps - 1)
    zp = _padded(np.abs(np.asarray(x)).astype(np.float64), pos0, g0, g0 + (count - 1) * D + ntaps, np.float64)
    return _windows(zp, ntaps, D, count) @ np.abs(taps)[::-1]


def _demix(v, m_lo, gain):
    """gain Re(i^m v[m])"""
    mm = (m_lo + np.arange(len(v))) & 3
    return gain * np.where(mm == 0, v.real, np.where(mm == 1, -v.imag, np.where(mm == 2, -v.real, v.imag)))


def ref_ld(x, taps, D, ssb=False, p=0, q=1, gain=1.0, pos0=0) -> np.ndarray:
    """y in long double"""
    taps = np.asarray(taps, np.float64)
    ntaps, c = len(taps), (len(taps) - 1) // 2
    m_lo, count = out_range(pos0, len(x), D)
    if count == 0:
        return np.zeros(0, LD)
    g0 = m_lo * D + c - (ntaps - 1)
    g1 = g0 + (count - 1) * D + ntaps
    hr = taps[::-1].astype(LD)
    if not ssb:
        zp = _padded(np.asarray(x).astype(LD), pos0, g0, g1, LD)
        return LD(gain) * (_windows(zp, ntaps, D, count) @ hr)
    xp = _padded(np.asarray(x), pos0, g0, g1, np.complex128)  # (integer or float32 parts: exact)
    r = phase_index(g0, g1 - g0, p, q)
    if q <= 1 << 16:  # every factor once
        ct, st = unit_ld(np.arange(q), q)
        cs, sn = ct[r], st[r]
    else:
        cs, sn = unit_ld(r, q)
    xr, xi = xp.real.astype(LD), xp.imag.astype(LD)
    zr, zi = xr * cs + xi * sn, xi * cs - xr * sn
    # Re(i^m v) needs Re v at even m and Im v at odd m only
    v = np.zeros(count, LD)
    e0 = m_lo & 1  # the first even output's local index
    ne, no = len(range(e0, count, 2)), len(range(1 - e0, count, 2))
    if ne:
        v[e0::2] = _windows(zr[e0 * D:], ntaps, 2 * D, ne) @ hr
    if no:
        v[1 - e0::2] = _windows(zi[(1 - e0) * D:], ntaps, 2 * D, no) @ hr
    mm = (m_lo + np.arange(count)) & 3
    return LD(gain) * np.where((mm == 1) | (mm == 2), -v, v)


def ref_ld_long(x, taps, D, ssb=False, p=0, q=1, gain=1.0, block=16384) -> np.ndarray:
    """ref_ld of a long row at pos0 = 0, `block` outputs at a time (each from its own samples with their
    halo: a row's interior outputs do not depend on the rest)"""
    ntaps, c = len(taps), (len(taps) - 1) // 2
    count = out_range(0, len(x), D)[1]
    out = np.zeros(count, LD)
    for a in range(0, count, block):
        b = min(count, a + block)
        lo, hi = max(0, a * D + c - (ntaps - 1)), min(len(x), (b - 1) * D + c + 1)
        first = -(-lo // D)
        out[a:b] = ref_ld(x[lo:hi], taps, D, ssb, p, q, gain, lo)[a - first: b - first]
    return out


def ref_f64(x, taps, D, ssb=False, p=0, q=1, gain=1.0, pos0=0, drop_tap=None, c_off=0, phase_late=0, im_off=0,
            wrap64=False, tw32=False) -> np.ndarray:
    """y in float64 by upfirdn.  Corruptions: drop_tap = k sets h[k] to 0; c_off shifts c; phase_late takes
    the phase of sample n - phase_late; im_off rotates the output mixer by that many steps; wrap64 forms
    n p in wrapped 64-bit arithmetic; tw32 rounds the phase factors to float32."""
    taps = np.array(taps, np.float64)
    ntaps, c = len(taps), (len(taps) - 1) // 2 + c_off
    if drop_tap is not None:
        taps[drop_tap] = 0.0
    m_lo, count = out_range(pos0, len(x), D)
    if count == 0:
        return np.zeros(0)
    base = (pos0 // D) * D  # the global index of local sample 0: the multiple of D at or below pos0
    lead = pos0 - base      # zeros in front of the row, 0 .. D - 1
    if ssb:
        r = phase_index(pos0 - phase_late, len(x), p, q, wrap64)
        ang = 2.0 * np.pi * r.astype(np.float64) / q
        w = np.cos(ang) - 1j * np.sin(ang)
        if tw32:
            w = w.astype(np.complex64).astype(np.complex128)
        z = np.asarray(x).astype(np.complex128) * w
    else:
        z = np.asarray(x).astype(np.float64)
    zl = np.concatenate([np.zeros(lead, z.dtype), z])
    # local output m' = m - base / D is conv(h, zl)[m' D + c]: shift the filter so that the wanted lags fall
    # on multiples of D (as resample_poly does)
    pre = (D - c % D) % D
    hp = np.concatenate([np.zeros(pre), taps])
    full = upfirdn(hp, zl, 1, D)
    first = (m_lo - base // D) + (c + pre) // D
    v = np.zeros(count, z.dtype)
    got = full[first: first + count]
    v[: len(got)] = got
    if not ssb:
        return gain * v
    return _demix(v, m_lo + im_off, gain)
