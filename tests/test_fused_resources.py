"""CPU: resources of the fusion kernel in the built libhiprag.so (gfx950 code-object metadata, read by
tools/kernel_resources.py -- no GPU needed).

k_fuse_lists keeps one group's 2048 entries, the segment heads' keys, fused scores and member bits in STATIC LDS and
runs as one workgroup of up to 1024 threads: a spill or a private segment would put scratch traffic into the two
bitonic sorts' inner loops, and LDS beyond 64 KiB is not a static allocation any more.  So a spill, any private
segment or more than 65536 bytes of LDS must fail here, on the CPU."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_fusion_kernel_exists_and_needs_no_scratch():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "libhiprag.so not built (run __graft_entry__.build())"
    res = {k: v for k, v in kernel_resources(LIB).items() if "k_fuse_lists" in k or "k_fuse_pad" in k}
    assert any("k_fuse_lists" in k for k in res), sorted(res)
    assert any("k_fuse_pad" in k for k in res), sorted(res)
    for name, r in res.items():
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 65536, (name, r)
        if "k_fuse_lists" in name:
            assert r["group_segment_fixed_size"] > 0, (name, r)  # the sorts run in LDS
            # 1024 threads are four waves per SIMD; a SIMD has 512 registers per lane: 128 each
            assert r["vgpr_count"] + r.get("agpr_count", 0) <= 128, (name, r)
