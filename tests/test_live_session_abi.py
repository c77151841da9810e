"""CPU: the live session's C-ABI (include/msdsp.h) -- exported symbols, struct layouts, argument
checks that need no GPU, and the session kernels' resources in the shipped code objects."""
import ctypes
import os
import shutil

import pytest

from conftest import ROOT
from meteorgpu import _lib

SO = os.path.join(ROOT, "meteor-scatter_amd", "meteorgpu", "libmsdsp.so")

SESSION_SYMBOLS = ("msd_live_session_create", "msd_live_session_destroy", "msd_live_session_push_rows_dev",
                   "msd_live_session_push_samples_dev", "msd_live_session_push_rows", "msd_live_session_push_samples",
                   "msd_live_session_state", "msd_live_session_history", "msd_live_session_reset")

SESSION_KERNELS = ("live_session_over_kernel", "live_session_history_kernel", "live_session_scan_kernel",
                   "live_session_gather_kernel", "live_session_carry_kernel", "live_session_reset_kernel")


def _cfg(W=40):
    c = _lib.MsdLiveCfg()
    c.block_size, c.avg_win_blocks, c.fs, c.k_std = 800, W, 4000.0, 4.0
    c.init_wait_sec, c.after_tracking_wait_sec, c.min_db_mean, c.min_dur_sec = 8.0, 12.0, -1.0, -1.0
    return c


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in SESSION_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name


def test_struct_layouts():
    # msd_live_stream_state {i32 state, i32 status, i64 blocks, i64 trig, f64 lock, f64 until, f64 t_start,
    #                        i64 meteors, i64 retained, i64 remainder}
    assert ctypes.sizeof(_lib.MsdLiveStreamState) == 72
    assert _lib.MsdLiveStreamState.blocks.offset == 8 and _lib.MsdLiveStreamState.remainder.offset == 64
    # msd_live_cfg {i32, i32, 6 * f64}; msd_welch_cfg {4 * i32, 2 * f64, 2 * i32, 2 * 8 * i32}
    assert ctypes.sizeof(_lib.MsdLiveCfg) == 56
    assert ctypes.sizeof(_lib.MsdWelchCfg) == 104
    assert _lib.METEOR_DTYPE.itemsize == 72


def _header_struct(name):
    import re
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        w = {"int32_t": 4, "int64_t": 8, "double": 8}[typ]
        for n in names.split(","):
            m = re.search(r"\[(\w+)\]", n)
            k = 1 if not m else (8 if m.group(1) == "MSD_WELCH_MAX_BANDS" else int(m.group(1)))
            size = (size + w - 1) // w * w + w * k
    return (size + 7) // 8 * 8


def test_struct_sizes_equal_the_headers():
    assert ctypes.sizeof(_lib.MsdLiveStreamState) == _header_struct("msd_live_stream_state")
    assert ctypes.sizeof(_lib.MsdLiveCfg) == _header_struct("msd_live_cfg")
    assert ctypes.sizeof(_lib.MsdWelchCfg) == _header_struct("msd_welch_cfg")
    assert _lib.METEOR_DTYPE.itemsize == _header_struct("msd_meteor")


def test_null_arguments_fail_without_gpu():
    lib = _lib.load()
    h = ctypes.c_void_p()
    c = _cfg()
    assert lib.msd_live_session_create(None, None, None, None, 1, 10, 40, 0, ctypes.byref(h)) == _lib.MSD_ERR_INVALID
    assert b"msd_live_session_create" in lib.msd_last_error() and b"null" in lib.msd_last_error()
    assert lib.msd_live_session_create(None, ctypes.byref(c), None, None, 1, 10, 40, 0, None) == _lib.MSD_ERR_INVALID
    assert lib.msd_live_session_create(None, ctypes.byref(c), None, None, 1, 10, 40, 0, ctypes.byref(h)) == \
        _lib.MSD_ERR_INVALID
    assert b"null ctx" in lib.msd_last_error()
    for call, name in ((lambda: lib.msd_live_session_push_rows_dev(None, None, None, 0, 0, None, 0, None, None, None,
                                                                   None), b"msd_live_session_push_rows_dev"),
                       (lambda: lib.msd_live_session_push_samples_dev(None, None, None, None, 0, None, 0, None, None,
                                                                      None, None, None, 0, None),
                        b"msd_live_session_push_samples_dev"),
                       (lambda: lib.msd_live_session_push_rows(None, 0, None, 0, None, 0, None, None, None, None),
                        b"msd_live_session_push_rows"),
                       (lambda: lib.msd_live_session_push_samples(None, 0, None, 0, None, 0, None, None, None, None,
                                                                  None, 0, None), b"msd_live_session_push_samples"),
                       (lambda: lib.msd_live_session_state(None, 0, 1, None), b"msd_live_session_state"),
                       (lambda: lib.msd_live_session_history(None, 0, None, 0, None), b"msd_live_session_history"),
                       (lambda: lib.msd_live_session_reset(None, -1), b"msd_live_session_reset")):
        assert call() == _lib.MSD_ERR_INVALID
        assert name in lib.msd_last_error()
    lib.msd_live_session_destroy(None)  # a no-op


def test_sizes_rejected_without_gpu():
    lib = _lib.load()
    h = ctypes.c_void_p()
    c = _cfg(W=40)
    assert lib.msd_live_session_create(None, ctypes.byref(c), None, None, 1, 10, 39, 0, ctypes.byref(h)) == \
        _lib.MSD_ERR_INVALID
    assert b"hist_blocks" in lib.msd_last_error()
    assert lib.msd_live_session_create(None, ctypes.byref(c), None, None, 1, 0, 40, 0, ctypes.byref(h)) == \
        _lib.MSD_ERR_INVALID
    assert b"max_push_blocks" in lib.msd_last_error()
    assert lib.msd_live_session_create(None, ctypes.byref(c), None, None, 0, 10, 40, 0, ctypes.byref(h)) == \
        _lib.MSD_ERR_INVALID
    assert b"nstreams" in lib.msd_last_error()
    bad = _cfg()
    bad.block_size = 0
    assert lib.msd_live_session_create(None, ctypes.byref(bad), None, None, 1, 10, 40, 0, ctypes.byref(h)) == \
        _lib.MSD_ERR_INVALID
    # a Welch configuration that does not fit the detector's
    w = _lib.MsdWelchCfg()
    w.block_size, w.nbands = 400, 3
    win = (ctypes.c_double * 256)()
    assert lib.msd_live_session_create(None, ctypes.byref(c), ctypes.byref(w), win, 1, 10, 40, _lib.MSD_I16,
                                       ctypes.byref(h)) == _lib.MSD_ERR_INVALID
    assert b"block_size" in lib.msd_last_error()
    w.block_size = 800
    assert lib.msd_live_session_create(None, ctypes.byref(c), ctypes.byref(w), win, 1, 10, 40, 99,
                                       ctypes.byref(h)) == _lib.MSD_ERR_INVALID
    assert b"dtype" in lib.msd_last_error()
    assert not h.value


@pytest.mark.skipif(not (os.path.exists(SO) and shutil.which("/opt/rocm/lib/llvm/bin/llvm-objdump")),
                    reason="libmsdsp.so or the ROCm LLVM tools are missing")
def test_session_kernels_use_no_scratch_and_call_nothing():
    from tools import kernel_resources as kr
    audit = kr.audit(SO)
    for name in SESSION_KERNELS:
        hits = {k: r for k, r in audit.items() if f"{len(name)}{name}" in k}
        assert hits, name
        for k, r in hits.items():
            assert r["private_segment_fixed_size"] == 0, (k, r["private_segment_fixed_size"])
            assert not r["calls"] and not r.get("uses_dynamic_stack"), k
    # the sample movers exist for every sample width
    assert sum("live_session_gather_kernel" in k for k in audit) == 4
