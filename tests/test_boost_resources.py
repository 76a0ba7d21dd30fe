"""CPU: resources of the boosted-search kernels in the built libhiprag.so (gfx950 code-object metadata, read by
tools/kernel_resources.py -- no GPU needed).

k_boost_rescore runs one wave per window record and k_boost_order one 1024-thread workgroup per query, sorting up to
8192 16-byte records in (dynamic) LDS: scratch traffic in either would sit on the tail of every boosted call, and
k_boost_order's 16 waves leave a lane 128 registers.  So a spill, any private segment, or static LDS beyond a gfx950
CU's 160 KB must fail here, on the CPU."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

RESCORE = re.compile(r"k_boost_rescoreILi([012])EE")  # <DT>; DT: 0 fp32, 1 bf16, 2 f16
PLAIN = ["k_boost_extrema", "k_boost_floor", "k_boost_order", "k_boost_rekey", "k_boost_gather", "k_boost_take"]


def test_boost_kernels_exist_and_need_no_scratch():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "libhiprag.so not built (run __graft_entry__.build())"
    res = {k: v for k, v in kernel_resources(LIB).items() if "k_boost" in k}
    assert {RESCORE.search(k).group(1) for k in res if RESCORE.search(k)} == set("012"), sorted(res)  # every dtype
    for name in PLAIN:
        assert any(name in k for k in res), (name, sorted(res))
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert 0 <= r["group_segment_fixed_size"] <= 160 * 1024, (name, r)
        if "k_boost_order" in name and r.get("max_flat_workgroup_size", 1024) >= 1024:
            assert r["vgpr_count"] <= 128, (name, r)  # 16 waves per workgroup: four per SIMD
