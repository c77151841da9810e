"""Build check of stft1024_kernel's int16 forms in the shipped libmsdsp.so (CPU only: reads the gfx950 code
objects, runs nothing).

The forms with 32-bit output offsets keep the transposes' 16 LDS read bases in registers across the tile loop
(DESIGN.md §4.1).  That is worth its registers only while the kernel stays at 4 waves per SIMD without scratch,
and only while the reads it serves stay single ds_read_b64: paired into ds_read2_b64 they cost 8 LDS cycles on
lane groups the frame layout is not built for (measured +12 %).

* every int16 form: at most 128 VGPRs and no scratch (what the forms had before the bases were hoisted);
* the benchmarked form (hop 512, 32-bit offsets, static schedule): no paired 64-bit LDS read and no flat
  instruction.
"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT
from tools import kernel_resources as kr

SO = os.path.join(ROOT, "meteor-scatter_amd", "meteorgpu", "libmsdsp.so")

pytestmark = pytest.mark.skipif(not (os.path.exists(SO) and shutil.which(f"{kr.LLVM}/llvm-objdump")),
                                reason="libmsdsp.so or the ROCm LLVM tools are missing")

# stft1024_kernel<int16_t, WIDE, SH, DYN> in the Itanium mangling
INT16_FORMS = [f"stft1024_kernelIsLi{w}ELb{sh}ELb{dyn}EE" for w in (0, 1) for sh in (0, 1) for dyn in (0, 1)]
BENCHMARKED = "stft1024_kernelIsLi0ELb1ELb0EE"


@pytest.fixture(scope="module")
def audit():
    return kr.audit(SO)


@pytest.mark.parametrize("form", INT16_FORMS)
def test_int16_forms_keep_four_waves_without_scratch(audit, form):
    hits = [r for k, r in audit.items() if form in k]
    assert len(hits) == 1, f"{form}: {len(hits)} kernels"
    r = hits[0]
    assert r["vgpr_count"] <= 128, r
    assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0, r
    assert r["flat"] == 0 and r["scratch"] == 0 and r["calls"] == 0, r


def test_benchmarked_form_reads_lds_unpaired():
    ops = None
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(kr.code_objects(SO)):
            path = os.path.join(td, f"co{k}.o")
            open(path, "wb").write(co)
            txt = subprocess.run([f"{kr.LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True,
                                 text=True, check=True).stdout
            m = re.search(r"^[0-9a-f]+ <[^>]*" + BENCHMARKED + r"[^>]*>:\n(.*?)(?=^[0-9a-f]+ <[^>]+>:|\Z)", txt, re.S | re.M)
            if m:
                ops = [ln.split()[0] for ln in m.group(1).splitlines() if ln.strip() and not ln.strip().startswith(";")]
                break
    assert ops, "the benchmarked form was not found"
    assert ops.count("ds_read_b64") >= 48, "the transposes' reads are missing"
    paired = [o for o in ops if o.startswith("ds_read2") and o.endswith("_b64")]
    assert not paired, f"{len(paired)} paired 64-bit LDS reads"
    assert not [o for o in ops if o.startswith("flat_")]
