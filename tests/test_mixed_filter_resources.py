"""CPU: register budget of the per-query-mask scan kernels in the built libhiprag.so (gfx950 code-object metadata, read
by tools/kernel_resources.py -- no GPU needed).

The QM instantiations of k_scan_sample / k_scan_filter (template arguments <MT, DT, QB, P, NT, 512, QM = true>) hold
the lane's allow word across the k-loop and test one of its bits per accumulator register in a body that already
sits near the 256-register limit of two waves per SIMD.  A VGPR spill in their tile loop would turn the HBM-bound
stream into a scratch-bound one, so it must fail here, on the CPU."""
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

# Itanium mangling of k_scan_{sample,filter}<MT, DT, QB, P, NT, TPB = 512, QM = true>; DT: 0 fp32, 1 bf16, 2 f16
QM = re.compile(r"k_scan_(filter|sample)ILi([12])ELi([012])ELi([12])ELi(16|8|4)ELb[01]ELi512ELb1EE")


def test_per_query_mask_scan_kernels_fit_their_registers():
    from kernel_resources import kernel_resources

    res = {k: v for k, v in kernel_resources(LIB).items() if QM.search(k)}
    forms = {QM.search(k).groups() for k in res}
    # SAMPLE and FILTER; 16-bit rows (bf16 on the bf16 MFMA, f16 on the f16 one): one and two 32-query blocks at ring
    # depths 16 / 8 / 4; fp32 rows (either MFMA type): the ring depths their plans use (make_plan: 8 / 4, 4 with two
    # blocks)
    want = {(m, mt, dt, qb, p) for m in ("filter", "sample") for mt, dt in (("1", "1"), ("2", "2"))
            for qb in "12" for p in ("16", "8", "4")}
    want |= {(m, mt, "0", qb, p) for m in ("filter", "sample") for mt in "12"
             for qb, p in (("1", "8"), ("1", "4"), ("2", "4"))}
    assert forms == want, sorted(forms ^ want)
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["vgpr_count"] <= 256, (name, r)  # two waves per SIMD


def test_plain_scan_kernels_keep_their_names():
    """The instantiations without per-query masks are still there, one per form (QM = false)."""
    from kernel_resources import kernel_resources

    plain = [k for k in kernel_resources(LIB) if re.search(r"k_scan_(filter|sample)I.*Li512ELb0EE", k)]
    assert len(plain) >= 36
