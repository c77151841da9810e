"""CPU: the C-ABI of the rational-ratio resampler (include/msdsp.h, msd_resamp_*) -- the prototypes against
meteorgpu/_lib.py's ctypes declarations, the exported symbols, the timing id, the argument checks that need
no GPU, the refusals with code and message, and the two host-only functions against Python."""
import ctypes as C
import os
import re

import pytest

import resamp_ref as R
from conftest import ROOT
from meteorgpu import _lib

NEW = ("msd_resamp_plan_create", "msd_resamp_out_len", "msd_resamp_chain", "msd_resamp_run_dev", "msd_resamp_run",
       "msd_resamp_push_dev", "msd_resamp_push", "msd_resamp_flush", "msd_resamp_reset")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msdsp.h")).read(), flags=re.S)


def _prototype(name):
    """[argument kinds] of `int name(...)` as the header declares it"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "*" in arg:
            out.append("ptr:" + arg.split("*")[0].replace("const", "").strip())
        else:
            out.append(arg.rsplit(" ", 1)[0])
    return out


def _bound(name):
    res, args = next((r, a) for n, r, a in _lib._SIGS if n == name)
    assert res is C.c_int
    out = []
    for a in args:
        if a is C.c_void_p:
            out.append("ptr")
        elif a is C.c_int:  # (ctypes' c_int32 is c_int)
            out.append("int")
        elif a is C.c_int64:
            out.append("int64_t")
        elif a == C.POINTER(C.c_int64):
            out.append("ptr:int64_t")
        elif a == C.POINTER(C.c_double):
            out.append("ptr:double")
        elif a == C.POINTER(_lib.MsdResampCfg):
            out.append("ptr:msd_resamp_cfg")
        elif a == C.POINTER(C.c_void_p):
            out.append("ptr:handle")
        else:
            raise AssertionError((name, a))
    return out


def test_prototypes_match_the_binding():
    for name in NEW:
        head, bind = _prototype(name), _bound(name)
        assert len(head) == len(bind), (name, head, bind)
        for h, b in zip(head, bind):
            if h.startswith("ptr:"):
                assert b == "ptr" or b == h or (b == "ptr:handle" and h == "ptr:msd_resamp_plan"), (name, h, b)
            else:
                assert ("int" if h == "int32_t" else h) == b, (name, h, b)
    # mirroring the down-converter one for one
    for name in NEW:
        ddc = [a.replace("msd_ddc", "msd_resamp") for a in _prototype_of_ddc(name)]
        assert _prototype(name) == ddc, name
    # the struct: {int32 mode, up, down, ntaps, out_dtype, reserved; int64 shift_num, shift_den; double gain}
    m = re.search(r"typedef struct \{([^}]*)\} msd_resamp_cfg;", _header())
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip()
              for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MsdResampCfg._fields_]
    assert fields == ["mode", "up", "down", "ntaps", "out_dtype", "reserved", "shift_num", "shift_den", "gain"]
    assert C.sizeof(_lib.MsdResampCfg) == 48


def _prototype_of_ddc(name):
    return _prototype(name.replace("msd_resamp", "msd_ddc"))


def test_symbols_exported_and_timing_id():
    lib = _lib.load()
    for name in NEW + ("msd_resamp_plan_destroy",):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.K_RESAMP == 14 and _lib.K_DDC == 13
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    assert "14 = resampler" in src and "13 = DDC" in src


def test_null_and_invalid_arguments_fail_without_gpu():
    lib = _lib.load()
    cfg = _lib.MsdResampCfg(_lib.DDC_REAL, 2, 3, 25, _lib.MSD_F64, 0, 0, 1, 1.0)
    h = C.c_void_p()
    n = C.c_int64(0)
    calls = {
        "msd_resamp_plan_create": lambda: lib.msd_resamp_plan_create(None, C.byref(cfg), None, 1, 1, C.byref(h)),
        "msd_resamp_run_dev": lambda: lib.msd_resamp_run_dev(None, None, 2, None, None, None, 1, None, 1, None),
        "msd_resamp_run": lambda: lib.msd_resamp_run(None, None, 2, 0, 0, None, 0, C.byref(n)),
        "msd_resamp_push_dev": lambda: lib.msd_resamp_push_dev(None, None, 2, None, None, None, 1, None),
        "msd_resamp_push": lambda: lib.msd_resamp_push(None, 0, None, 2, 0, None, 0, C.byref(n)),
        "msd_resamp_flush": lambda: lib.msd_resamp_flush(None, 0, None, 0, C.byref(n)),
        "msd_resamp_reset": lambda: lib.msd_resamp_reset(None, 0, 0),
        "msd_resamp_chain": lambda: lib.msd_resamp_chain(C.byref(cfg), None),
        "msd_resamp_out_len": lambda: lib.msd_resamp_out_len(None, 0, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.MSD_ERR_INVALID, name
        assert name.encode() in lib.msd_last_error(), (name, lib.msd_last_error())
    lib.msd_resamp_plan_destroy(None)  # a null plan is ignored


INV, UNS = _lib.MSD_ERR_INVALID, _lib.MSD_ERR_UNSUPPORTED
BAD = [  # (mode, L, M, ntaps, out, p, q, code, a word of the message)
    (_lib.DDC_REAL, 4, 6, 25, _lib.MSD_F64, 0, 1, INV, b"coprime"),
    (_lib.DDC_REAL, 3, 3, 25, _lib.MSD_F64, 0, 1, INV, b"coprime"),
    (_lib.DDC_REAL, 2, 3, 24, _lib.MSD_F64, 0, 1, INV, b"odd"),
    (_lib.DDC_REAL, 2, 3, 25, _lib.MSD_F32, 0, 1, INV, b"out_dtype"),
    (_lib.DDC_SSB, 2, 3, 25, _lib.MSD_CI16, 1, 4, INV, b"out_dtype"),
    (7, 2, 3, 25, _lib.MSD_F64, 0, 1, INV, b"mode"),
    (_lib.DDC_SSB, 2, 3, 25, _lib.MSD_F64, 4, 4, INV, b"shift"),
    (_lib.DDC_SSB, 2, 3, 25, _lib.MSD_F64, -1, 4, INV, b"shift"),
    (_lib.DDC_SSB, 2, 3, 25, _lib.MSD_F64, 0, 0, INV, b"shift"),
    (_lib.DDC_REAL, 0, 3, 25, _lib.MSD_F64, 0, 1, UNS, b"up"),
    (_lib.DDC_REAL, 257, 3, 25, _lib.MSD_F64, 0, 1, UNS, b"up"),
    (_lib.DDC_REAL, 2, 0, 25, _lib.MSD_F64, 0, 1, UNS, b"down"),
    (_lib.DDC_REAL, 2, 1025, 25, _lib.MSD_F64, 0, 1, UNS, b"down"),
    (_lib.DDC_REAL, 2, 3, -1, _lib.MSD_F64, 0, 1, UNS, b"ntaps"),
    (_lib.DDC_SSB, 2, 3, 4097, _lib.MSD_F64, 0, 1, UNS, b"ntaps"),
    (_lib.DDC_SSB, 2, 3, 25, _lib.MSD_F64, 1, (1 << 24) + 1, UNS, b"2^24"),
    (_lib.DDC_REAL, 2, 3, 25, _lib.MSD_F64, 1, 4, UNS, b"REAL"),
]


@pytest.mark.parametrize("mode,L,M,ntaps,out,p,q,code,word", BAD)
def test_refusals_carry_code_and_message(mode, L, M, ntaps, out, p, q, code, word):
    lib = _lib.load()
    cfg = _lib.MsdResampCfg(mode, L, M, ntaps, out, 0, p, q, 1.0)
    v = C.c_double(0)
    assert lib.msd_resamp_chain(C.byref(cfg), C.byref(v)) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_resamp_chain: ") and word in msg, msg
    m0, cnt = C.c_int64(0), C.c_int64(0)
    assert lib.msd_resamp_out_len(C.byref(cfg), 0, 10, C.byref(m0), C.byref(cnt)) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_resamp_out_len: ") and word in msg, msg
    with pytest.raises(_lib.MsdError) as e:
        _lib.resamp_out_len(cfg, 0, 10)
    assert e.value.code == code


def test_valid_limits_are_accepted():
    for L, M, ntaps in ((1, 1, 1), (256, 1, 4095), (255, 1024, 4095), (1, 1024, 4095), (256, 1023, 1)):
        for mode, p, q in ((_lib.DDC_REAL, 0, 1), (_lib.DDC_SSB, (1 << 24) - 1, 1 << 24)):
            assert _lib.resamp_chain(_lib.MsdResampCfg(mode, L, M, ntaps, _lib.MSD_I16, 0, p, q, -2.0)) > 0


def test_out_len_against_python():
    for L, M in ((1, 1), (2, 3), (3, 2), (7, 5), (40, 441), (160, 441), (2, 125), (256, 1), (255, 1024), (1, 12)):
        cfg = _lib.MsdResampCfg(_lib.DDC_REAL, L, M, 5, _lib.MSD_F64, 0, 0, 1, 1.0)
        lim = (1 << 62) // L
        for n in (0, 1, 2, 3, M - 1, M, M + 1, 200001):
            for pos0 in (0, 1, M - 1, M, (1 << 40) + 3, lim - n):
                assert _lib.resamp_out_len(cfg, pos0, n) == R.out_range(pos0, n, L, M), (L, M, pos0, n)
        assert _lib.resamp_out_len(cfg, 0, lim)[1] == -(-lim * L // M)
        for pos0, n in ((lim, 1), (lim + 1, 0), (0, lim + 1), (-1, 4), (4, -1), ((1 << 63) - 6, 100)):
            with pytest.raises(_lib.MsdError) as e:
                _lib.resamp_out_len(cfg, pos0, n)
            assert e.value.code == _lib.MSD_ERR_INVALID and "msd_resamp_out_len" in e.value.msg


SHAPES = [(1, 1, 1), (2, 3, 1), (2, 3, 25), (3, 2, 25), (7, 5, 3), (2, 125, 1001), (40, 441, 3529), (20, 147, 1177),
          (160, 441, 4095), (256, 1, 4095), (255, 1024, 4095), (1, 12, 97), (1, 1024, 4095), (3, 1000, 4095)]


def test_chain_against_python_and_the_cap():
    for L, M, ntaps in SHAPES:
        TM, G, K, I = R.plan(L, M, ntaps)
        assert TM * G == 256 and K * G >= I >= K
        for ssb, q in ((False, 1), (True, 32), (True, 192000), (True, (1 << 24) - 3)):
            cfg = _lib.MsdResampCfg(_lib.DDC_SSB if ssb else _lib.DDC_REAL, L, M, ntaps, _lib.MSD_F64, 0, 1 if ssb else 0, q, 1.0)
            chain = _lib.resamp_chain(cfg)
            assert chain == R.chain_py(ssb, L, M, ntaps, q), (L, M, ntaps, ssb, q)
            assert chain <= 10 + -(-ntaps // L) + (G - 1)
    # the sound-card configuration: 128 outputs per tile, 2 groups of 45 of the 89 taps of a branch
    assert R.plan(40, 441, 3529) == (128, 2, 45, 89)
    assert _lib.resamp_chain(_lib.MsdResampCfg(_lib.DDC_REAL, 40, 441, 3529, _lib.MSD_F64, 0, 0, 1, 1.0)) == 45 + 1 + 1
    # the archive's: one group of 13
    assert _lib.resamp_chain(_lib.MsdResampCfg(_lib.DDC_SSB, 2, 3, 25, _lib.MSD_F64, 0, 5, 32, 1.0)) == 5 + 13 + 0 + 1
