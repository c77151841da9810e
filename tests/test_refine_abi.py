"""CPU: the C-ABI of the two host-only functions behind the exact delta step's restatement (include/msdsp.h:
msd_iq_delta64_chain, and msd_i8_coeffs kind 2) -- the prototypes against meteorgpu/_lib.py's ctypes
declarations, the exported symbols, the argument checks, the path / chain table for the geometries
tests/test_gpu_refine_exact.py runs, and own + combine + reference against a hand count for C5."""
import ctypes as C
import math
import os
import re

import pytest

from conftest import ROOT
from meteorgpu import _lib

FS = 192000.0
CI16, CF32 = _lib.MSD_CI16, _lib.MSD_CF32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msdsp.h")).read(), flags=re.S)


def _prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        out.append("ptr:" + arg.split("*")[0].replace("const", "").strip() if "*" in arg else arg.rsplit(" ", 1)[0])
    return out


def test_prototypes_match_the_binding():
    res, args = next((r, a) for n, r, a in _lib._SIGS if n == "msd_iq_delta64_chain")
    assert res is C.c_int
    head = _prototype("msd_iq_delta64_chain")
    assert head == ["int32_t", "int64_t", "double", "int32_t", "int32_t", "int32_t", "int32_t", "int32_t", "int32_t",
                    "ptr:double", "ptr:double", "ptr:double"]
    kinds = {C.c_int: "int32_t", C.c_int64: "int64_t", C.c_double: "double"}
    assert [kinds.get(a, "ptr:double" if a == C.POINTER(C.c_double) else None) for a in args] == head
    assert _prototype("msd_i8_coeffs") == ["int", "ptr:double", "int", "int", "int", "int", "ptr:int64_t"]
    lib = _lib.load()
    assert hasattr(lib, "msd_iq_delta64_chain") and "msd_iq_delta64_chain" in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    for name, v in (("QUANT", _lib.REFINE_I8_CHAIN_QUANT), ("HORNER", _lib.REFINE_I8_CHAIN_HORNER),
                    ("SUBBLOCK", _lib.REFINE_I8_CHAIN_SUBBLOCK)):
        assert re.search(rf"#define MSD_REFINE_I8_CHAIN_{name} {v:.1f}\b", src), name
    assert _lib.I8_REFINE == 2


def _chain(N, hop, band, noise, dtype, goertzel=0, fs=FS, ptrs=(True, True, True)):
    v = [C.c_double(-1.0) for _ in range(3)]
    rc = _lib.load().msd_iq_delta64_chain(N, hop, fs, band[0], band[1], noise[0], noise[1], dtype, goertzel,
                                          *[C.byref(x) if p else None for x, p in zip(v, ptrs)])
    return rc, [x.value for x in v]


def test_null_and_invalid_arguments():
    lib = _lib.load()
    c5 = (4096, 1024, (21, 22), (-65, -63))
    rc, _ = _chain(*c5, CI16, ptrs=(False, False, False))
    assert rc == _lib.MSD_ERR_INVALID and b"msd_iq_delta64_chain" in lib.msd_last_error()
    for ptrs in ((True, False, False), (False, True, False), (False, False, True)):  # any one alone is fine
        rc, v = _chain(*c5, CI16, ptrs=ptrs)
        assert rc == _lib.MSD_OK and [x != -1.0 for x in v] == list(ptrs)
    bad = [
        ((2, 1024, (0, 0), (0, -1)), CI16, FS, _lib.MSD_ERR_INVALID),           # nperseg below 4
        ((4096, 0, (21, 22), (0, -1)), CI16, FS, _lib.MSD_ERR_INVALID),         # hop
        ((4096, 1024, (21, 22), (0, -1)), CI16, 0.0, _lib.MSD_ERR_INVALID),     # fs
        ((4096, 1024, (21, 2048), (0, -1)), CI16, FS, _lib.MSD_ERR_INVALID),    # band outside -N/2 .. N/2 - 1
        ((4096, 1024, (21, 22), (-2049, -2040)), CI16, FS, _lib.MSD_ERR_INVALID),
        ((131072, 1024, (21, 22), (0, -1)), CI16, FS, _lib.MSD_ERR_UNSUPPORTED),  # nperseg above 65536
        ((4096, 1024, (100, 120), (0, -1)), CI16, FS, _lib.MSD_ERR_UNSUPPORTED),  # band wider than 16 bins
        ((4096, 1024, (21, 22), (0, -1)), _lib.MSD_I16, FS, _lib.MSD_ERR_UNSUPPORTED),  # a real dtype
    ]
    for geom, dtype, fs, code in bad:
        rc, v = _chain(*geom, dtype, fs=fs)
        assert rc == code, (geom, dtype, fs)
        assert v == [-1.0, -1.0, -1.0]
        msg = lib.msd_last_error()
        assert msg.startswith(b"msd_iq_delta64_chain: ") and len(msg) > len(b"msd_iq_delta64_chain: ")
    with pytest.raises(_lib.MsdError):
        _lib.iq_delta64_chain(4096, 0, FS, (21, 22), (0, -1), CI16)


def _goertzel_own(N, hop, band, noise):
    """csrc/refine_plan.h's count for the 16-lane rows: 3 L Gmax + 12"""
    D = math.gcd(N, hop)
    L = D // 16
    ks = set()
    for lo, hi in (band, noise):
        for b in range(lo, hi + 1):
            ks.update(((b - 1) % N, b % N, (b + 1) % N))
    gmax = 1.0
    for km in ks:
        if km:
            sn = abs(math.sin(2.0 * math.pi * km / N))
            gmax = max(gmax, min(1.0 / sn if sn > 0 else 1e300, float(L)))
    return 3.0 * L * gmax + 12.0


# (N, hop, band, noise, dtype) -> path; the geometries of tests/test_gpu_refine_exact.py
TABLE = [
    ((4096, 1024, (21, 22), (-65, -63)), CI16, _lib.REFINE_INT8_MFMA),      # C5: 9 bins
    ((1024, 1024, (100, 100), (0, -1)), CI16, _lib.REFINE_INT8_MFMA),       # R 1, 3 bins
    ((2048, 1024, (511, 512), (-700, -699)), CI16, _lib.REFINE_INT8_MFMA),  # R 2
    ((3072, 1024, (300, 302), (-5, -4)), CI16, _lib.REFINE_INT8_MFMA),      # R 3
    ((5120, 1024, (700, 701), (0, -1)), CI16, _lib.REFINE_INT8_MFMA),       # R 5
    ((8192, 1024, (4094, 4095), (-4096, -4095)), CI16, _lib.REFINE_INT8_MFMA),  # R 8, the wrap at N / 2
    ((4096, 2048, (21, 22), (-65, -63)), CI16, _lib.REFINE_GOERTZEL_ROWS),  # D 2048: not the int8 step
    ((4096, 3072, (21, 22), (-65, -63)), CI16, _lib.REFINE_INT8_MFMA),
    ((4096, 5120, (21, 22), (-65, -63)), CI16, _lib.REFINE_INT8_MFMA),      # hop above nperseg
    ((4096, 1024, (21, 24), (-65, -63)), CI16, _lib.REFINE_GOERTZEL_ROWS),  # 11 bins
    ((4096, 1024, (1, 1), (-65, -63)), CI16, _lib.REFINE_GOERTZEL_ROWS),    # needs bin 0
    ((4096, 1024, (21, 22), (-65, -63)), CF32, _lib.REFINE_GOERTZEL_ROWS),
    ((4096, 512, (21, 22), (-65, -63)), CF32, _lib.REFINE_GOERTZEL_ROWS),
    ((4096, 64, (21, 22), (-65, -63)), CF32, _lib.REFINE_GOERTZEL_ROWS),
    ((1000, 500, (10, 12), (-9, -8)), CI16, _lib.REFINE_DIRECT),
    ((1000, 500, (10, 12), (-9, -8)), CF32, _lib.REFINE_DIRECT),
]


@pytest.mark.parametrize("geom,dtype,path", TABLE)
def test_path_and_chain_table(geom, dtype, path):
    N, hop, band, noise = geom
    assert _lib.iq_delta64_path(N, hop, FS, band, noise, dtype) == path
    D = math.gcd(N, hop)
    R = N // D
    want_own = {_lib.REFINE_INT8_MFMA: 91.0 + 6.0 + 22.0, _lib.REFINE_DIRECT: D + 4.0}.get(path)
    if want_own is None:
        want_own = _goertzel_own(N, hop, band, noise)
    own, combine, reference = _lib.iq_delta64_chain(N, hop, FS, band, noise, dtype)
    assert own == pytest.approx(want_own, rel=1e-15)
    assert combine == (R + 4) + 8
    assert reference == 4.0 * math.log2(N) + 11.0
    # MSD_OPT_REFINE_GOERTZEL moves int16 off the int8 step only
    g = _lib.iq_delta64_chain(N, hop, FS, band, noise, dtype, goertzel=True)
    if path == _lib.REFINE_INT8_MFMA:
        assert g == (pytest.approx(_goertzel_own(N, hop, band, noise), rel=1e-15), combine, reference)
        assert g[0] > own
    else:
        assert g == (own, combine, reference)
    # fs does not enter
    assert _lib.iq_delta64_chain(N, hop, 48000.0, band, noise, dtype) == (own, combine, reference)


def test_c5_hand_count():
    """C5 (N 4096, hop 1024, int16): 91 + 6 + 22 for the block step, 4 + 4 + 8 for the frame step,
    4 * 12 + 11 for the reference: 119 + 16 + 59 = 194 (DESIGN §4.5c's ~120 u block bound + tail)"""
    own, combine, reference = _lib.iq_delta64_chain(4096, 1024, FS, (21, 22), (-65, -63), CI16)
    assert (own, combine, reference) == (119.0, 16.0, 59.0)
    assert own + combine + reference == 194.0
    assert (_lib.REFINE_I8_CHAIN_QUANT, _lib.REFINE_I8_CHAIN_HORNER, _lib.REFINE_I8_CHAIN_SUBBLOCK) == (91.0, 6.0, 22.0)
    assert own == _lib.REFINE_I8_CHAIN_QUANT + _lib.REFINE_I8_CHAIN_HORNER + _lib.REFINE_I8_CHAIN_SUBBLOCK
