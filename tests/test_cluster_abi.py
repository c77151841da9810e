"""CPU: the C-ABI of the burst clustering (include/msdsp.h, msd_spec_peaks_f64* / msd_cluster*) -- the
prototypes against meteorgpu/_lib.py's ctypes declarations, the struct layouts, the exported symbols, the
timing id, and the refusals with code and message for every out-of-range argument (configuration checks run
before anything touches a context, so they need no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from meteorgpu import _lib

NEW = ("msd_spec_peaks_f64_dev", "msd_cluster_dev", "msd_spec_peaks_f64", "msd_cluster")
INV, UNS = _lib.MSD_ERR_INVALID, _lib.MSD_ERR_UNSUPPORTED


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


def _bound(name):
    res, args = next((r, a) for n, r, a in _lib._SIGS if n == name)
    assert res is C.c_int
    kinds = {C.c_void_p: "ptr", C.c_int: "int32_t", C.c_int64: "int64_t", C.c_double: "double",
             C.POINTER(C.c_int32): "ptr:int32_t", C.POINTER(_lib.MsdClusterCfg): "ptr:msd_cluster_cfg",
             C.POINTER(_lib.MsdClusterSummary): "ptr:msd_cluster_summary"}
    return [kinds[a] for a in args]


def test_prototypes_match_the_binding():
    for name in NEW:
        head, bind = _prototype(name), _bound(name)
        assert len(head) == len(bind), (name, head, bind)
        for h, b in zip(head, bind):
            assert b == h or (b == "ptr" and h.startswith("ptr:")), (name, h, b)
    assert _prototype("msd_cluster_dev") == ["ptr:msd_ctx", "ptr:msd_cluster_cfg", "ptr:double", "ptr:int32_t", "int64_t",
                                             "ptr:int32_t", "ptr:double", "ptr:msd_cluster_summary"]
    assert _prototype("msd_spec_peaks_f64_dev") == [
        "ptr:msd_ctx", "ptr:double", "int64_t", "int32_t", "int64_t", "int64_t", "int32_t", "int32_t", "ptr:double",
        "double", "double", "int32_t", "ptr:double", "ptr:int32_t", "ptr:int32_t", "ptr:int32_t"]


def _fields(struct):
    m = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", _header())
    return [re.sub(r"\[.*\]", "", f).strip() for decl in m.group(1).split(";") if decl.strip()
            for f in decl.strip().split(" ", 1)[1].split(",")]


def test_struct_layouts():
    assert _fields("msd_cluster_cfg") == [f for f, _ in _lib.MsdClusterCfg._fields_]
    assert _fields("msd_cluster_cfg") == ["eps", "critical_min_extent", "min_samples", "max_points"]
    assert C.sizeof(_lib.MsdClusterCfg) == 24 and _lib.MsdClusterCfg.min_samples.offset == 16
    assert _fields("msd_cluster_summary") == [f for f, _ in _lib.MsdClusterSummary._fields_]
    assert C.sizeof(_lib.MsdClusterSummary) == 32 == _lib.CLUSTER_SUMMARY_DTYPE.itemsize
    for f, _ in _lib.MsdClusterSummary._fields_:
        assert getattr(_lib.MsdClusterSummary, f).offset == _lib.CLUSTER_SUMMARY_DTYPE.fields[f][1]


def test_symbols_constants_and_timing_id():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    src = open(os.path.join(ROOT, "include", "msdsp.h")).read()
    assert _lib.K_CLUSTER == 15 and "15 = burst clustering" in src
    assert re.search(r"#define MSD_ABI_VERSION 1\b", src) and lib.msd_abi_version() == 1
    assert int(re.search(r"#define MSD_CLUSTER_MAX_POINTS (\d+)", src).group(1)) == _lib.CLUSTER_MAX_POINTS == 512
    assert int(re.search(r"#define MSD_CLUSTER_STATUS_NPTS (\d+)", src).group(1)) == _lib.CLUSTER_STATUS_NPTS
    import meteorgpu
    from meteorgpu import cluster
    assert meteorgpu.dbscan is cluster.dbscan and meteorgpu.cluster_points is cluster.cluster_points
    assert meteorgpu.spec_peaks is cluster.spec_peaks


BAD_CFG = [  # (eps, extent, min_samples, max_points, code, a word of the message)
    (-1.0, 5.0, 5, 500, INV, b"eps"),
    (float("inf"), 5.0, 5, 500, INV, b"eps"),
    (float("nan"), 5.0, 5, 500, INV, b"eps"),
    (30.0, 5.0, 0, 500, INV, b"min_samples"),
    (30.0, 5.0, -2, 500, INV, b"min_samples"),
    (30.0, 5.0, 5, 0, UNS, b"max_points"),
    (30.0, 5.0, 5, 513, UNS, b"max_points"),
    (30.0, 5.0, 5, -1, UNS, b"max_points"),
]


@pytest.mark.parametrize("eps,ext,ms,mp,code,word", BAD_CFG)
def test_cluster_refusals_carry_code_and_message(eps, ext, ms, mp, code, word):
    lib = _lib.load()
    cfg = _lib.MsdClusterCfg(eps, ext, ms, mp)
    s = _lib.MsdClusterSummary()
    assert lib.msd_cluster_dev(None, C.byref(cfg), None, None, 1, None, None, None) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_cluster_dev: ") and word in msg, msg
    assert lib.msd_cluster(None, C.byref(cfg), None, 0, None, None, C.byref(s)) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_cluster: ") and word in msg, msg


BAD_WINDOW = [  # (K, frames, ld, k_lo, k_hi, max_points, code, word)
    (1025, 145, 160, 491, 328, 500, INV, b"k_lo"),
    (1025, 145, 160, 328, 1025, 500, INV, b"k_hi"),
    (1025, 145, 160, 328, 4000, 500, INV, b"k_hi"),
    (1025, 145, 160, -1, 10, 500, INV, b"k_lo"),
    (1025, 145, 160, 328, 491, 0, UNS, b"max_points"),
    (1025, 145, 160, 328, 491, 513, UNS, b"max_points"),
]


@pytest.mark.parametrize("K,frames,ld,k_lo,k_hi,mp,code,word", BAD_WINDOW)
def test_peaks_refusals_carry_code_and_message(K, frames, ld, k_lo, k_hi, mp, code, word):
    lib = _lib.load()
    assert lib.msd_spec_peaks_f64_dev(None, None, 1, K, frames, ld, k_lo, k_hi, None, 1.0, 1.0, mp, None, None, None,
                                      None) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_spec_peaks_f64_dev: ") and word in msg, msg
    n = C.c_int32(0)
    assert lib.msd_spec_peaks_f64(None, None, K, frames, k_lo, k_hi, 1.0, 1.0, 1.0, mp, None, None, C.byref(n),
                                  C.byref(n)) == code
    msg = lib.msd_last_error()
    assert msg.startswith(b"msd_spec_peaks_f64: ") and word in msg, msg


def test_null_arguments_fail_without_gpu():
    lib = _lib.load()
    cfg = _lib.MsdClusterCfg(30.0, 5.0, 5, 500)
    s = _lib.MsdClusterSummary()
    n = C.c_int32(0)
    xy = np.zeros((600, 2))
    lab = np.zeros(600, np.int32)
    calls = {
        "msd_cluster_dev": lambda: lib.msd_cluster_dev(None, C.byref(cfg), None, None, 1, None, None, None),
        "msd_cluster": lambda: lib.msd_cluster(None, C.byref(cfg), None, 0, None, None, C.byref(s)),
        "msd_spec_peaks_f64_dev": lambda: lib.msd_spec_peaks_f64_dev(None, None, 1, 8, 4, 4, 0, 7, None, 1.0, 1.0, 4,
                                                                     None, None, None, None),
        "msd_spec_peaks_f64": lambda: lib.msd_spec_peaks_f64(None, None, 8, 4, 0, 7, 1.0, 1.0, 1.0, 4, None, None,
                                                             C.byref(n), C.byref(n)),
    }
    for name, call in calls.items():
        assert call() == INV, name
        assert lib.msd_last_error().startswith(name.encode() + b": null"), (name, lib.msd_last_error())
    assert lib.msd_cluster_dev(None, None, None, None, 0, None, None, None) == INV
    # the host form refuses more points than max_points before it needs a context: nothing is clamped
    assert lib.msd_cluster(None, C.byref(cfg), _lib.ptr(xy), 501, _lib.ptr(lab), None, C.byref(s)) == UNS
    assert b"max_points" in lib.msd_last_error()
