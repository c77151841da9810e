"""GPU: every bin of the real-input spectrogram kernels against a per-bin float32 (float64) error
bound -- stft1024_kernel, stft_psd_kernel<128 | 256 | 512 | 1024> and stft_any_kernel, through
dsp.spectrogram, at the smallest shapes that reach each code path (tests/spec_signals.py has the
bound, the chain constants counted from the kernels' code, the signal classes and the references).

The older tests hold max_k |S - R| / max_k |R| <= 1e-5 per frame on noise plus a tone, which sees
nothing below -50 dB of a frame's strongest bin.  Here, on every bin of every frame,

    |sqrt S - sqrt R| <= sqrt(c_k) chain u sqrt(1.001 sum_k R) + 3 u sqrt R,

R scipy's float64 spectrogram of the same samples (float32 plans) or the long-double pipeline
(float64 plans), on a -80 dB tone beside a full-scale carrier, full-scale noise, a tone at every bin
in turn, impulses, DC + Nyquist alone, a square wave, a large DC offset over 3 LSB of noise, a
constant (exactly zero out) and float samples with an offset whose sums are not exact (f32_dc, and
f64_dc on the float64 plans: also the older normwise bars, 1e-5 and 1e-10).
On the two noise-like classes a frame's rms amplitude error must also stay within 4 times that of a
float32 CPU pipeline with another FFT (float64 plans: scipy's float64 pipeline) on the same frame.

Every case prints  BINS kernel shape dtype class: bound ratio, rms_gpu / rms_cpu.
"""
import functools

import numpy as np
import pytest

import spec_signals as G
from meteorgpu import _lib, dsp

pytestmark = pytest.mark.gpu

I16, F32, U8, I32, F64 = np.int16, np.float32, np.uint8, np.int32, np.float64
BASE = ("carrier_weak", "fullscale_noise", "nyquist_dc", "dc_quiet", "const")
EXTRA = ("staircase", "impulses", "square")

# kernel, nperseg, noverlap, nfft, dtypes, frames, MSD_OPT_GENERIC_STFT, first row of its family
ROWS = [
    ("stft1024-shared", 1024, 512, 1024, (I16, F32, U8), 33, False, True),   # crosses the 32-frame tile
    ("stft1024", 1024, 256, 1024, (I16,), 33, False, False),
    ("stft1024", 1024, 768, 1024, (I16,), 33, False, False),
    ("stft_psd512", 1024, 512, 1024, (I16, F32), 33, True, True),
    ("stft_psd512", 1024, 513, 1024, (I16, F32), 33, False, False),          # odd hop: not stft1024's
    ("stft_psd128", 256, 128, 256, (I16,), 33, False, True),
    ("stft_psd256", 512, 256, 512, (I16,), 33, False, False),
    ("stft_psd1024", 2048, 1024, 2048, (I16, F32), 17, False, False),        # 16-frame tile
    ("stft_any", 16, 8, 16, (I16, F32), 33, False, True),                    # M = 8: radix 2, radix 4
    ("stft_any", 32, 16, 32, (I16, F32), 33, False, True),                   # M = 16: radix 4 twice
    ("stft_any", 64, 32, 64, (I16, F32), 33, False, True),
    ("stft_any", 128, 64, 128, (I16, F32), 33, False, True),
    ("stft_any", 4096, 2048, 4096, (I16,), 5, False, True),                  # log2 M odd
    ("stft_any", 8192, 4096, 8192, (I16,), 5, False, False),                 # even
    ("stft_any", 16384, 8192, 16384, (I16,), 5, False, False),
    ("stft_any-pad", 1000, 500, 1024, (I16, F32), 5, False, True),
    ("stft_any-pad", 3000, 1000, 4096, (I16, F32), 5, False, False),
    ("stft_any-pad", 17, 4, 1024, (I16, F32), 5, False, False),
    ("stft_any-f64", 16, 8, 16, (I32, F64), 5, False, True),
    ("stft_any-f64", 1024, 512, 1024, (I32, F64), 5, False, False),
    ("stft_any-f64", 16384, 8192, 16384, (I32, F64), 5, False, False),       # one LDS buffer, in place
    ("stft_any-f64", 8192, 2048, 16384, (I32, F64), 5, False, False),
]
# f32_dc beyond the rows' own float32 entries: stft_any at a large float32 shape
F32_DC_ONLY = [("stft_any", 4096, 2048, 4096, (F32,), 5, False, False)]


def _cases():
    out = []
    for row in ROWS:
        kernel, N, nov, nfft, dtypes, frames, generic, first = row
        for dt in dtypes:
            classes = BASE + (EXTRA if first else ())
            if dt == F32 and (kernel.startswith("stft_any") or N in (1024, 2048)):
                classes += ("f32_dc",)
            if dt == F64:
                classes += ("f64_dc",)
            out += [(kernel, N, nov, nfft, dt, frames, generic, cls) for cls in classes]
    for kernel, N, nov, nfft, dtypes, frames, generic, _ in F32_DC_ONLY:
        out.append((kernel, N, nov, nfft, F32, frames, generic, "f32_dc"))
    return out


def _param(c):
    kernel, N, nov, nfft, dt, frames, generic, cls = c
    marks = [pytest.mark.skipif(not G.LD_OK, reason=G.LD_REASON)] if kernel.endswith("f64") else []
    return pytest.param(c, id=f"{kernel}-{N}-{nov}-{nfft}-{np.dtype(dt).name}-{cls}", marks=marks)


def _chain(kernel, nfft):
    if kernel.startswith("stft1024"):
        return G.CHAIN_STFT1024, G.U32
    if kernel.startswith("stft_psd"):
        return G.CHAIN_TILED[nfft], G.U32
    return G.CHAIN_ANY[nfft], (G.U64 if kernel.endswith("f64") else G.U32)


@functools.lru_cache(maxsize=None)
def _refs(cls, N, nov, nfft, frames, dtname, double):
    """(samples, the truth, the CPU yardstick of the rms check) of a case, computed once, read-only"""
    x = G.signal(cls, N, N - nov, frames, np.dtype(dtname))
    shape = (G.FS, N, nov, nfft)
    if double:
        R, C = G.ref_ld(x, *shape), G.ref64(x, *shape)
    else:
        R, C = G.ref64(x, *shape), G.ref32_cpu(x, *shape)
    for a in (x, R, C):
        a.setflags(write=False)
    return x, R, C


@pytest.mark.parametrize("case", [_param(c) for c in _cases()])
def test_every_bin_within_the_bound(case):
    kernel, N, nov, nfft, dt, frames, generic, cls = case
    chain, u = _chain(kernel, nfft)
    double = u == G.U64
    x, R, C = _refs(cls, N, nov, nfft, frames, np.dtype(dt).name, double)
    ctx = dsp.context(0)
    try:
        if generic:
            ctx.set_option(_lib.OPT_GENERIC_STFT, 1)
        _, _, S = dsp.spectrogram(x, fs=G.FS, nperseg=N, noverlap=nov, nfft=nfft)
    finally:
        if generic:
            ctx.set_option(_lib.OPT_GENERIC_STFT, 0)
    assert S.shape == R.shape == (nfft // 2 + 1, (len(x) - N) // (N - nov) + 1)
    assert S.dtype == (np.float64 if double else np.float32)
    ratio, at = G.bound_ratio(S, R, chain, u)
    rg, rc = G.rms_err(S, R), G.rms_err(C, R)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = float(np.max(np.where(rc > 0, rg / rc, np.where(rg > 0, np.inf, 0.0))))
    old = G.normwise(S, R)
    print(f"BINS {kernel} {N}/{nov}/{nfft} {np.dtype(dt).name} {cls}: chain {chain} ratio {ratio:.4f} at {at}, "
          f"rms_gpu {rg.max():.3e} / rms_cpu {rc.max():.3e} factor {fac:.3f}, normwise {old:.3e}")
    if cls == "const":
        assert not R.any() and not S.any()
    assert ratio <= 1.0, f"per-bin bound exceeded {ratio:.3g} times at (bin, frame) {at}"
    if cls in G.NOISE_LIKE:
        assert fac <= G.RMS_FACTOR, f"rms error {fac:.3g} times the CPU pipeline's"
    if cls in ("f32_dc", "f64_dc"):
        assert old <= (1e-10 if double else 1e-5)
