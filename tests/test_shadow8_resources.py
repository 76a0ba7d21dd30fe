"""CPU: register budget of the shadow-8 scan kernels in the built libhiprag.so (gfx950 code-object metadata, read by
tools/kernel_resources.py -- no GPU needed).

The shadow-8 SAMPLE / FILTER (k_scan_sample / k_scan_filter with the f16 MFMA type and the int8 fragment: template
arguments <2, 3, QB, P, ...>) run two waves per SIMD like the 16-bit ones, so they have 256 registers per wave; their
int8 -> f16 conversion adds temporaries to a body that already sits near that limit.  A VGPR spill in their tile loop
would turn the HBM-bound stream into a scratch-bound one, so it must fail here, on the CPU."""
import os
import re
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not shutil.which("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="libhiprag.so or the ROCm LLVM tools are missing")

# Itanium mangling of k_scan_{sample,filter}<MT = F16 (2), DT = I8S (3), QB, P, NT, TPB>
SHADOW8 = re.compile(r"k_scan_(filter|sample)ILi2ELi3ELi([12])ELi(16|8|4|2)E")


def test_shadow8_scan_kernels_fit_their_registers():
    from kernel_resources import kernel_resources

    res = {k: v for k, v in kernel_resources(LIB).items() if SHADOW8.search(k)}
    forms = {SHADOW8.search(k).groups() for k in res}
    # SAMPLE and FILTER, one and two 32-query blocks, ring depths 16 / 8 / 4 / 2
    assert forms == {(m, qb, p) for m in ("filter", "sample") for qb in "12" for p in ("16", "8", "4", "2")}, sorted(res)
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["vgpr_count"] <= 256, (name, r)  # two waves per SIMD
