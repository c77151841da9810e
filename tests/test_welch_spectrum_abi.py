"""CPU: the C-ABI of the whole-band Welch row (include/msdsp.h) -- the two prototypes against
meteorgpu/_lib.py's ctypes declarations, the exported symbols, the timing id, and the argument checks
that need no GPU."""
import ctypes as C
import os
import re

from conftest import ROOT
from meteorgpu import _lib

NEW = ("msd_welch_spectrum_dev", "msd_welch_spectrum")


def _prototype(name):
    """[argument ctypes] of `int name(...)` as the header declares it: a pointer to int64_t stays typed where
    the binding types it, every other pointer is a void pointer"""
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
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
        elif a is C.c_int:  # (ctypes' c_int32 is c_int: the two are one 4-byte type here)
            out.append("int")
        elif a is C.c_int64:
            out.append("int64_t")
        elif a == C.POINTER(C.c_int64):
            out.append("ptr:int64_t")
        else:
            raise AssertionError((name, a))
    return out


def test_prototypes_match_the_binding():
    for name in NEW:
        head, bind = _prototype(name), _bound(name)
        assert len(head) == len(bind), (name, head, bind)
        for h, b in zip(head, bind):
            if h.startswith("ptr:"):
                assert b == "ptr" or b == h, (name, h, b)
            else:
                assert ("int" if h == "int32_t" else h) == b, (name, h, b)
    assert _prototype("msd_welch_spectrum_dev") == [
        "ptr:msd_welch_plan", "ptr:void", "int", "ptr:int64_t", "ptr:int64_t", "int64_t", "int64_t", "ptr:double",
        "int64_t", "ptr:double"]
    assert _prototype("msd_welch_spectrum") == [
        "ptr:msd_welch_plan", "ptr:void", "int", "int64_t", "ptr:double", "ptr:double", "ptr:int64_t"]


def test_symbols_exported_and_timing_id():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert _lib.K_WSPEC == 12
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    assert "12 = Welch spectrum" in src


def test_null_arguments_fail_without_gpu():
    lib = _lib.load()
    assert lib.msd_welch_spectrum_dev(None, None, 1, None, None, 1, 1, None, 1, None) == _lib.MSD_ERR_INVALID
    assert b"msd_welch_spectrum_dev" in lib.msd_last_error()
    assert lib.msd_welch_spectrum(None, None, 1, 0, None, None, None) == _lib.MSD_ERR_INVALID
    assert b"msd_welch_spectrum" in lib.msd_last_error()
