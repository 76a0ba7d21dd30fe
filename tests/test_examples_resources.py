"""CPU: resources of the search-by-example kernels in the built libhiprag.so (gfx950 code-object metadata, read by
tools/kernel_resources.py -- no GPU needed).

k_build_queries keeps up to eight examples' row chunks and eight fp64 accumulators per thread in registers, with every
loop over them unrolled: an index that stopped being a constant would move those arrays to scratch and put private
memory traffic on what is one workgroup's latency per query.  k_drop_examples is a wave-level compaction with nothing
to spill.  So a spill, any private segment or any LDS must fail here, on the CPU."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

BUILD = re.compile(r"k_build_queriesILi([012])EE")  # <DT>; DT: 0 fp32, 1 bf16, 2 f16


def test_example_kernels_exist_and_need_no_scratch():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "libhiprag.so not built (run __graft_entry__.build())"
    res = {k: v for k, v in kernel_resources(LIB).items() if "k_build_queries" in k or "k_drop_examples" in k}
    assert {BUILD.search(k).group(1) for k in res if BUILD.search(k)} == set("012"), sorted(res)  # every dtype
    assert any("k_drop_examples" in k for k in res), sorted(res)
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)  # registers only
        # a workgroup is one wave per SIMD; a SIMD has 512 registers per lane: two workgroups fit a CU up to 256
        assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, (name, r)
