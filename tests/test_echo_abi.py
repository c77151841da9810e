"""CPU: the C-ABI of the echo measurement (include/msdsp.h, msd_echo_measure*) -- the exported symbols, the
struct layouts against meteorgpu/_lib.py's ctypes and numpy declarations (sizeof(msd_echo) == 128), the
timing id and the band limit, and every refusal with its code and a message (the configuration checks run
before anything touches a context, so they need no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from meteorgpu import _lib

NEW = ("msd_echo_measure_dev", "msd_echo_measure_f64_dev", "msd_echo_measure", "msd_echo_measure_f64")
INV, UNS = _lib.MSD_ERR_INVALID, _lib.MSD_ERR_UNSUPPORTED


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msdsp.h")).read(), flags=re.S)


def _fields(struct):
    m = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", _header())
    return [f.strip() for decl in m.group(1).split(";") if decl.strip()
            for f in decl.strip().split(" ", 1)[1].split(",")]


def test_symbols_constants_and_timing_id():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    assert _lib.K_ECHO == 16 and "16 = echo measurement" in src
    assert re.search(r"#define MSD_ABI_VERSION 1\b", src) and lib.msd_abi_version() == 1
    limit = int(re.search(r"#define MSD_ECHO_MAX_BAND (\d+)", src).group(1))
    assert limit == _lib.ECHO_MAX_BAND >= 64
    from meteorgpu import echo
    assert echo.ECHO_DTYPE is _lib.ECHO_DTYPE and echo.MAX_BAND == limit


def test_struct_layouts():
    assert _fields("msd_echo_cfg") == [f for f, _ in _lib.MsdEchoCfg._fields_]
    assert C.sizeof(_lib.MsdEchoCfg) == 40 and _lib.MsdEchoCfg.nperseg.offset == 8
    assert _fields("msd_echo") == list(_lib.ECHO_DTYPE.names)
    assert _lib.ECHO_DTYPE.itemsize == 128
    offsets = [_lib.ECHO_DTYPE.fields[n][1] for n in _lib.ECHO_DTYPE.names]
    assert offsets == [0, 8, 16, 24, 32, 40, 48, 52] + list(range(56, 128, 8))  # the C layout: no padding
    kinds = {"int64_t": np.int64, "int32_t": np.int32, "double": np.float64}
    m = re.search(r"typedef struct \{([^}]*)\} msd_echo;", _header())
    for decl in (d.strip() for d in m.group(1).split(";") if d.strip()):
        ctype, names = decl.split(" ", 1)
        for n in names.split(","):
            assert _lib.ECHO_DTYPE.fields[n.strip()][0] == kinds[ctype], n
    import echo_ref
    assert echo_ref.ECHO_DTYPE == _lib.ECHO_DTYPE and echo_ref.DET_DTYPE == _lib.DET_DTYPE


def _cfg(block_size=1200, nperseg=1024, hop=128, k_lo=2, k_hi=3, n_lo=0, n_hi=-1, pre=0, post=0):
    return _lib.MsdEchoCfg(block_size, nperseg, hop, k_lo, k_hi, n_lo, n_hi, pre, post)


BAD = [  # (K, cfg, code, a word of the message)
    (0, _cfg(), INV, b"K"),
    (-3, _cfg(), INV, b"K"),
    (8, _cfg(k_lo=3, k_hi=2), INV, b"k_lo"),
    (8, _cfg(k_lo=-1), INV, b"k_lo"),
    (8, _cfg(k_hi=8), INV, b"k_hi"),
    (8, _cfg(n_lo=-1, n_hi=1), INV, b"noise"),
    (8, _cfg(n_lo=5, n_hi=8), INV, b"noise"),
    (8, _cfg(hop=0), INV, b"hop"),
    (8, _cfg(nperseg=0), INV, b"nperseg"),
    (8, _cfg(block_size=0), INV, b"block_size"),
    (8, _cfg(pre=-1), INV, b"padding"),
    (8, _cfg(post=-1), INV, b"padding"),
    (1000, _cfg(k_lo=0, k_hi=_lib.ECHO_MAX_BAND), UNS, b"MSD_ECHO_MAX_BAND"),
    (1000, _cfg(n_lo=10, n_hi=10 + _lib.ECHO_MAX_BAND), UNS, b"MSD_ECHO_MAX_BAND"),
]


@pytest.mark.parametrize("K,cfg,code,word", BAD)
def test_refusals_carry_code_and_message(K, cfg, code, word):
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        if name.endswith("_dev"):
            rc = fn(None, None, 1, K, None, 160, None, 8, None, C.byref(cfg), None)
        else:
            rc = fn(None, None, K, 150, 160, None, 1, C.byref(cfg), None)
        assert rc == code, name
        msg = lib.msd_last_error()
        assert msg.startswith(name.encode() + b": ") and word in msg, msg


def test_null_arguments_fail_without_gpu():
    lib = _lib.load()
    cfg = _cfg()
    for name in NEW:
        fn = getattr(lib, name)
        dev = name.endswith("_dev")
        rc = fn(None, None, 1, 8, None, 160, None, 8, None, C.byref(cfg), None) if dev else \
            fn(None, None, 8, 150, 160, None, 1, C.byref(cfg), None)
        assert rc == INV and lib.msd_last_error().startswith(name.encode() + b": null"), lib.msd_last_error()
        rc = fn(None, None, 1, 8, None, 160, None, 8, None, None, None) if dev else \
            fn(None, None, 8, 150, 160, None, 1, None, None)
        assert rc == INV and b"null configuration" in lib.msd_last_error()
