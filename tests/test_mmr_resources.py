"""CPU: resources of the MMR kernels in the built libhiprag.so (gfx950 code-object metadata, read by
tools/kernel_resources.py -- no GPU needed).

k_mmr_select runs one workgroup of up to 16 waves per query, and its time is one workgroup's latency: scratch traffic
in the per-candidate dot loop would sit on that latency, and at 16 waves per workgroup a lane has 128 registers.  So
a spill, any private segment, or static LDS beyond a gfx950 CU's 160 KB must fail here, on the CPU."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

SELECT = re.compile(r"k_mmr_selectILi([012])ELi([24])EE")  # <DT, ILP>; DT: 0 fp32, 1 bf16, 2 f16


def test_mmr_kernels_exist_and_need_no_scratch():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "libhiprag.so not built (run __graft_entry__.build())"
    res = {k: v for k, v in kernel_resources(LIB).items() if "k_mmr" in k}
    forms = {SELECT.search(k).groups() for k in res if SELECT.search(k)}
    assert forms == {(dt, ilp) for dt in "012" for ilp in "24"}, sorted(res)  # every dtype, two and four dots abreast
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert 0 <= r["group_segment_fixed_size"] <= 160 * 1024, (name, r)
        if SELECT.search(name):
            assert r["vgpr_count"] <= 128, (name, r)  # 16 waves per workgroup: four per SIMD
            # the static part: rel, maxsim, rowid, taken, the waves' bests (the selected row is dynamic, <= 16 KB)
            assert 3 * 128 * 8 + 128 * 4 <= r["group_segment_fixed_size"] <= 8 * 1024, (name, r)
