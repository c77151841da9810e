"""CPU: the C-ABI of the decimating down-converter (include/msdsp.h, msd_ddc_*) -- the prototypes against
meteorgpu/_lib.py's ctypes declarations, the exported symbols, the timing id, the argument checks that need
no GPU, and the two host-only functions against Python."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from meteorgpu import _lib

NEW = ("msd_ddc_plan_create", "msd_ddc_out_len", "msd_ddc_chain", "msd_ddc_run_dev", "msd_ddc_run",
       "msd_ddc_push_dev", "msd_ddc_push", "msd_ddc_flush", "msd_ddc_reset")


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
        elif a == C.POINTER(_lib.MsdDdcCfg):
            out.append("ptr:msd_ddc_cfg")
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
                assert b == "ptr" or b == h or (b == "ptr:handle" and h == "ptr:msd_ddc_plan"), (name, h, b)
            else:
                assert ("int" if h == "int32_t" else h) == b, (name, h, b)
    assert _prototype("msd_ddc_run_dev") == ["ptr:msd_ddc_plan", "ptr:void", "int", "ptr:int64_t", "ptr:int64_t",
                                             "ptr:int64_t", "int64_t", "ptr:void", "int64_t", "ptr:int64_t"]
    assert _prototype("msd_ddc_push") == ["ptr:msd_ddc_plan", "int64_t", "ptr:void", "int", "int64_t", "ptr:void",
                                          "int64_t", "ptr:int64_t"]
    # the struct: {int32 mode, decim, ntaps, out_dtype; int64 shift_num, shift_den; double gain}
    m = re.search(r"typedef struct \{([^}]*)\} msd_ddc_cfg;", _header())
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip()
              for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [f for f, _ in _lib.MsdDdcCfg._fields_]
    assert C.sizeof(_lib.MsdDdcCfg) == 40


def test_symbols_exported_and_timing_id():
    lib = _lib.load()
    for name in NEW + ("msd_ddc_plan_destroy",):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.K_DDC == 13
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    assert "13 = DDC" in src
    assert re.search(r"#define MSD_DDC_REAL 0\b", src) and re.search(r"#define MSD_DDC_SSB 1\b", src)
    assert (_lib.DDC_REAL, _lib.DDC_SSB) == (0, 1)


def test_null_and_invalid_arguments_fail_without_gpu():
    lib = _lib.load()
    cfg = _lib.MsdDdcCfg(_lib.DDC_REAL, 12, 97, _lib.MSD_F64, 0, 1, 1.0)
    h = C.c_void_p()
    n = C.c_int64(0)
    calls = {
        "msd_ddc_plan_create": lambda: lib.msd_ddc_plan_create(None, C.byref(cfg), None, 1, 1, C.byref(h)),
        "msd_ddc_run_dev": lambda: lib.msd_ddc_run_dev(None, None, 2, None, None, None, 1, None, 1, None),
        "msd_ddc_run": lambda: lib.msd_ddc_run(None, None, 2, 0, 0, None, 0, C.byref(n)),
        "msd_ddc_push_dev": lambda: lib.msd_ddc_push_dev(None, None, 2, None, None, None, 1, None),
        "msd_ddc_push": lambda: lib.msd_ddc_push(None, 0, None, 2, 0, None, 0, C.byref(n)),
        "msd_ddc_flush": lambda: lib.msd_ddc_flush(None, 0, None, 0, C.byref(n)),
        "msd_ddc_reset": lambda: lib.msd_ddc_reset(None, 0, 0),
        "msd_ddc_chain": lambda: lib.msd_ddc_chain(C.byref(cfg), None),
        "msd_ddc_out_len": lambda: lib.msd_ddc_out_len(None, 0, 0, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.MSD_ERR_INVALID, name
        assert name.encode() in lib.msd_last_error(), (name, lib.msd_last_error())


BAD = [  # (mode, D, ntaps, out, p, q, code)
    (_lib.DDC_REAL, 12, 96, _lib.MSD_F64, 0, 1, _lib.MSD_ERR_INVALID),        # even ntaps
    (_lib.DDC_REAL, 12, 97, _lib.MSD_F64, 1, 4, _lib.MSD_ERR_UNSUPPORTED),    # REAL with a shift
    (_lib.DDC_REAL, 1025, 97, _lib.MSD_F64, 0, 1, _lib.MSD_ERR_UNSUPPORTED),
    (_lib.DDC_REAL, 0, 97, _lib.MSD_F64, 0, 1, _lib.MSD_ERR_UNSUPPORTED),
    (_lib.DDC_SSB, 12, 4097, _lib.MSD_F64, 0, 1, _lib.MSD_ERR_UNSUPPORTED),
    (_lib.DDC_SSB, 12, 97, _lib.MSD_F64, 1, (1 << 24) + 1, _lib.MSD_ERR_UNSUPPORTED),
    (_lib.DDC_SSB, 12, 97, _lib.MSD_F64, 4, 4, _lib.MSD_ERR_INVALID),
    (_lib.DDC_SSB, 12, 97, _lib.MSD_F32, 1, 4, _lib.MSD_ERR_INVALID),         # output dtype
    (7, 12, 97, _lib.MSD_F64, 0, 1, _lib.MSD_ERR_INVALID),
]


@pytest.mark.parametrize("mode,D,ntaps,out,p,q,code", BAD)
def test_refusals_carry_a_message(mode, D, ntaps, out, p, q, code):
    cfg = _lib.MsdDdcCfg(mode, D, ntaps, out, p, q, 1.0)
    v = C.c_double(0)
    assert _lib.load().msd_ddc_chain(C.byref(cfg), C.byref(v)) == code
    msg = _lib.load().msd_last_error()
    assert msg.startswith(b"msd_ddc_chain: ") and len(msg) > len(b"msd_ddc_chain: ")
    with pytest.raises(_lib.MsdError):
        _lib.ddc_out_len(cfg, 0, 10)


def test_out_len_against_python():
    for D in (1, 2, 12, 48, 1024):
        cfg = _lib.MsdDdcCfg(_lib.DDC_REAL, D, 5, _lib.MSD_F64, 0, 1, 1.0)
        for pos0 in (0, 1, D - 1, D, (1 << 40) + 3, 1 << 62):
            for n in (0, 1, 2, 3, D - 1, D, D + 1, 200001):
                if pos0 < 0 or n < 0:
                    continue
                m0 = -(-pos0 // D)
                assert _lib.ddc_out_len(cfg, pos0, n) == (m0, -(-(pos0 + n) // D) - m0), (D, pos0, n)
    with pytest.raises(_lib.MsdError):
        _lib.ddc_out_len(cfg, -1, 4)


def _chain_py(ssb, D, ntaps, q):
    """the count of csrc/ddc_plan.h restated: the tile's outputs by the LDS budget, G groups of K4 FMAs,
    G - 1 adds, the gain, the mix (5 with one table, 9 with two)"""
    def tile_bytes(tm):
        U = (-(-(tm * D + ntaps - 1) // D)) | 1
        return 8 * (2 * ((D * U + 1) & ~1) + 256)
    TM = next((tm for tm in (256, 128, 64, 32, 16, 8, 4, 2, 1) if tile_bytes(tm) <= 64 * 1024), None) \
        or next(tm for tm in (256, 128, 64, 32, 16, 8, 4, 2, 1) if tile_bytes(tm) <= 150 * 1024)
    G = 256 // TM
    return (0 if not ssb else (9 if q > 4096 else 5)) + -(-ntaps // G) + (G - 1) + 1


def test_chain_against_python():
    for D, ntaps in ((1, 1), (2, 3), (12, 5), (12, 97), (48, 385), (1024, 4095), (3, 4095)):
        for ssb, q in ((False, 1), (True, 32), (True, 192000), (True, (1 << 24) - 3)):
            cfg = _lib.MsdDdcCfg(_lib.DDC_SSB if ssb else _lib.DDC_REAL, D, ntaps, _lib.MSD_F64, 1 if ssb else 0, q, 1.0)
            assert _lib.ddc_chain(cfg) == _chain_py(ssb, D, ntaps, q), (D, ntaps, ssb, q)
    # the C5 configuration: 64 outputs per tile, 4 groups of 97 taps
    assert _lib.ddc_chain(_lib.MsdDdcCfg(_lib.DDC_SSB, 48, 385, _lib.MSD_F64, 5, 32, 1.0)) == 5 + 97 + 3 + 1
