"""Shapes, chain, yardstick and cases for the long-block band-power kernel, block_long_kernel
(csrc/block_delta.hip), which takes block plans with 4096 < L = min(B, nfft) <= 65536 (helper, not a
test module).  The inputs, the exact long-double DFT, numpy's numbers and the bars are those of
tests/band_signals.py.

The kernel spreads a block over one 256-thread workgroup.  Lane l owns the SPL samples from l SPL on,
SPL = ceil(L / 256) rounded up to a multiple of 8, runs a Goertzel recurrence per bin over them
(lanes at or past L do nothing), rotates its partial sum to the block origin by the exactly reduced
twiddle e^{-2 pi i ((k (n0 + SPL - 1)) mod nfft) / nfft}, and the 256 partial sums are added: 6 adds
in the wave, 2 across the 4 waves.

Chain (the longest chain of roundings from a sample to a bin, in units of u S): the 16-lane kernel's
3 SPL G + 24 (band_signals' docstring: the recurrence over the SPL steps a lane runs at gain
G = min(1 / |sin theta|, SPL); 24 for the window product, the rotation, the 4 adds of 16 lanes and
|X|^2) and the 4 further adds of 256 lanes:

    chain = 3 SPL G + 28
"""
from __future__ import annotations

import functools

import numpy as np

import band_signals as G
from meteorgpu import margin as M

LONG = 4096       # plans above this length run the long kernel
MAX_L = 65536
LANES = 256
NBLK_RMS, NBLK = 33, 5
CLASSES = ("fullscale_noise", "dc_quiet", "carrier_weak", "edge_impulses", "zeros", "staircase")
COUNT_CLASSES = ("staircase", "fullscale_noise", "carrier_weak")


def long_spl(L):
    """block_long_kernel's samples per lane (csrc/msd_internal.h block_long_spl)"""
    return ((L + LANES - 1) // LANES + 7) // 8 * 8


def chain_long(L, bins, nfft):
    """3 SPL G + 28 (module docstring)"""
    return M._goertzel_chain(long_spl(L), bins, nfft) + 4.0


def nblk_of(cls):
    return NBLK_RMS if cls in G.NOISE_LIKE else NBLK


# ------------------------------------------------------------------------------ yardstick
def goertzel256_powers(x, B, nfft, w, bins, twiddle=np.float64, drop_segment=None, shift=0, leak=False):
    """textbook float64 Goertzel with block_long_kernel's segmentation: 256 segments of spl samples,
    y = s_{N-1} - e^{-i th} s_{N-2}, rotated by e^{-i th (n0 + N - 1)} to the block origin, the 256
    summed.  |X_k|^2 [blocks][bins] float64.
    The keyword arguments corrupt it on purpose (tests/test_long_block_signals.py, the teeth):
    `twiddle` rounds 2 cos th to that type, `drop_segment` zeroes one lane's segment, `shift` reads
    the samples one later, `leak` lets the stream's sample at index L of the block in (with the last
    window value; for B == L that is the next block's first sample)."""
    L = min(B, nfft)
    spl = long_spl(L)
    xs = np.asarray(x)
    nb = len(xs) // B
    xs = np.concatenate([xs[shift:], np.zeros(shift + 1, xs.dtype)])  # room for the shift and the leak
    v = np.zeros((nb, LANES * spl))
    v[:, :L] = xs[: nb * B].reshape(nb, B)[:, :L].astype(np.float64) * w
    if leak:
        v[:, L - 1] += xs[np.arange(nb) * B + L].astype(np.float64) * w[-1]
    if drop_segment is not None:
        v[:, spl * drop_segment: spl * (drop_segment + 1)] = 0.0
    k = np.asarray(bins, np.int64)
    th = 2.0 * np.pi * (k % nfft).astype(np.float64) / float(nfft)
    c2 = G.round_twiddle(2.0 * np.cos(th), twiddle)
    s1, s2 = G._goertzel(v.reshape(nb, LANES, spl, 1), c2, spl)
    y = (s1 - np.cos(th) * s2) + 1j * (np.sin(th) * s2)
    seg = np.arange(LANES, dtype=np.int64)[:, None]
    a = -2.0 * np.pi * ((k[None, :] * (seg * spl + spl - 1)) % nfft).astype(np.float64) / float(nfft)
    X = (y * (np.cos(a) + 1j * np.sin(a))).sum(axis=1)
    return X.real ** 2 + X.imag ** 2


def block_powers_ld(x, B, nfft, w, bins, step=512):
    """band_signals.block_powers_ld in slices of `step` bins (dft_ld's table is L x bins long doubles)"""
    bins = list(bins)
    if len(bins) <= step:
        return G.block_powers_ld(x, B, nfft, w, bins)
    return np.concatenate([G.block_powers_ld(x, B, nfft, w, bins[j: j + step]) for j in range(0, len(bins), step)],
                          axis=1)


# ------------------------------------------------------------------------------ cases
# (B, nfft, all five dtypes)
SHAPES = [
    (4097, 4097, False),     # the first length over the old wall: odd, every later block misaligned,
                             # SPL 24: lane 170 ragged, 85 lanes empty
    (4112, 8192, False),
    (9600, 8192, False),     # the cropped foot of hanning(9600)
    (9600, 16384, True),     # the station's own block; zero-padded; ceil(L / 256) = 38 rounds up to 40
    (9601, 19202, False),    # odd B
    (38400, 32768, False),   # 192 kHz
    (65536, 65536, False),   # the limit
    (65536, 131072, False),  # the limit, zero-padded
    (40000, 6000, False),    # nfft not a power of two and far below B
]
COUNT_SHAPE = (9600, 16384)
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 63, 64, 65, 300)
MAXBINS_SHAPE = (4112, 8192, 4096)


def cases():
    """(B, nfft, dtype, band, noise, classes)"""
    out = []
    for B, nfft, first in SHAPES:
        e = G.edge_bins(nfft)
        pairs = [((e[0],) * 2, (e[1],) * 2), ((e[2],) * 2, (e[3],) * 2), ((e[4],) * 2, (e[5],) * 2),
                 ((e[3],) * 2, (0, -1))]  # the last: an empty noise band
        for dt in (G.ALL_DTYPES if first else (G.I16, G.F32)):
            out += [(B, nfft, dt, bd, nz, CLASSES) for bd, nz in pairs]
    B, nfft = COUNT_SHAPE
    for dt in (G.I16, G.F32):
        for n in COUNTS:
            out.append((B, nfft, dt, *G.split_count(n, nfft), COUNT_CLASSES))
    B, nfft, n = MAXBINS_SHAPE
    out.append((B, nfft, G.I16, *G.split_count(n, nfft), ("fullscale_noise",)))  # one class: 17 M table entries
    return out


def case_id(c):
    B, nfft, dt, band, noise, _ = c
    return f"long-{B}-{nfft}-{np.dtype(dt).name}-{band[0]}_{band[1]}-{noise[0]}_{noise[1]}"


def case_nblk(c, cls):
    """33 blocks for the rms classes, 5 otherwise; 5 throughout at the largest bin count"""
    return NBLK if (c[0], c[1]) == MAXBINS_SHAPE[:2] else nblk_of(cls)


@functools.lru_cache(maxsize=None)
def refs(cls, B, nfft, dtname, band, noise, nblk):
    """of one case and class, computed once and read-only (band_signals.block_refs with the long
    kernel's yardstick and chain): the samples, S per block, the window, the device chain and per
    band the exact dB and energy, the yardstick's energy and numpy's dB"""
    bins = tuple(G.plan_bins(band, noise))
    x = G.block_input(cls, B, nfft, dtname, bins, nblk)
    L = min(B, nfft)
    w = G.block_window(B, L)
    S = G.block_S(x, B, nfft, w)
    P = block_powers_ld(x, B, nfft, w, bins)
    Y = goertzel256_powers(x, B, nfft, w, bins) if bins else np.zeros((len(S), 0))
    N = G.block_powers_numpy(x, B, nfft, w, bins) if bins else np.zeros((len(S), 0))
    chain = chain_long(L, bins, nfft) if bins else 0.0
    nband = max(0, band[1] - band[0] + 1)
    per = []
    for sl in (slice(0, nband), slice(nband, None)):
        E = G.band_energy(P[:, sl])
        per.append(dict(n=P[:, sl].shape[1], E=E, db=G.db(E), Ey=G.band_energy(Y[:, sl]),
                        db_np=G.db(G.band_energy(N[:, sl]))))
    for a in (S, w):
        a.setflags(write=False)
    return dict(x=x, S=S, w=w, chain=chain, bands=per)


def case_refs(c, cls, nblk=None):
    B, nfft, dt, band, noise, _ = c
    return refs(cls, B, nfft, np.dtype(dt).name, band, noise, case_nblk(c, cls) if nblk is None else nblk)


# ------------------------------------------------------------------------------ the flat bar
FLAT_FS = 48000
FLAT_SHAPES = [(9600, 16384), (65536, 65536)]
FLAT_BAND, FLAT_NOISE = (993.0, 1013.0), (690.0, 710.0)
FLAT_DB = 1e-9


@functools.lru_cache(maxsize=None)
def flat_input(B, nblk=NBLK):
    """sigma = 3000 noise plus a 1 kHz tone at 48 kHz, int16"""
    rng = np.random.default_rng([48, B, nblk])
    n = nblk * B
    x = 3000.0 * rng.standard_normal(n) + 2000.0 * np.cos(2 * np.pi * 1000.0 * np.arange(n) / FLAT_FS)
    x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    return x


def flat_bins(nfft):
    from meteorgpu import dsp
    return dsp.band_bins(nfft, FLAT_FS, FLAT_BAND), dsp.band_bins(nfft, FLAT_FS, FLAT_NOISE)


def flat_db_numpy(B, nfft):
    """numpy's band and noise dB of flat_input [2][blocks]"""
    x = flat_input(B)
    w = G.block_window(B, min(B, nfft))
    return [G.db(G.band_energy(G.block_powers_numpy(x, B, nfft, w, range(lo, hi + 1)))) for lo, hi in flat_bins(nfft)]


def flat_db_yardstick(B, nfft):
    x = flat_input(B)
    w = G.block_window(B, min(B, nfft))
    return [G.db(G.band_energy(goertzel256_powers(x, B, nfft, w, range(lo, hi + 1)))) for lo, hi in flat_bins(nfft)]
