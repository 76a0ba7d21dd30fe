"""CPU: resources of the shadow-8 scan kernels with the bias fold in the built libhiprag.so (gfx950 code-object
metadata, read by tools/kernel_resources.py -- no GPU needed).

Every I8S kernel: no VGPR spill, no private segment, static LDS within a CU's 160 KiB, and no more VGPRs than the
parent commit's kernel of the same instantiation (PARENT below, read from the parent's library the same way).  The
fold's kernels stand for the parent's of the same block count and ring depth: lds_refresh::k_scan_filter for itself,
bias_fold::k_scan_filter for the per-wave-refresh k_scan_filter.  The subtracting kernels -- the SAMPLE, and the
FILTER's fallback where the row of -C_q does not fit in LDS -- are still built and must not move."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "youtu-rag_amd", "hiprag", "libhiprag.so")
sys.path.insert(0, os.path.join(REPO, "tools"))

# Itanium mangling of [ns::]k_scan_{sample,filter}<MT = F16 (2), DT = I8S (3), QB, P, ...>
I8S = re.compile(r"(?:(\d+)(lds_refresh|bias_fold))?13k_scan_(filter|sample)ILi2ELi3ELi([12])ELi(16|8|4|2)E")
DEBUG = re.compile(r"k_debug_approxILi2ELi3ELi([12])E")

# VGPRs of the parent commit's kernels: (kernel, QB, P)
PARENT = {
    "lds_refresh": {(1, 16): 190, (1, 2): 130, (1, 4): 153, (1, 8): 158, (2, 16): 238, (2, 2): 186, (2, 4): 190, (2, 8): 206},
    "filter": {(1, 16): 189, (1, 2): 129, (1, 4): 155, (1, 8): 159, (2, 16): 238, (2, 2): 186, (2, 4): 190, (2, 8): 206},
    "sample": {(1, 16): 148, (1, 2): 96, (1, 4): 121, (1, 8): 112, (2, 16): 192, (2, 2): 124, (2, 4): 130, (2, 8): 146},
}


def _i8s_kernels():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "libhiprag.so not built (run __graft_entry__.build())"
    out = {}
    for name, r in kernel_resources(LIB).items():
        m = I8S.search(name)
        if m:
            ns, mode, qb, p = m.group(2) or "", m.group(3), int(m.group(4)), int(m.group(5))
            out[(ns, mode, qb, p)] = (name, r)
    return out


def test_every_form_is_built():
    forms = set(_i8s_kernels())
    shapes = [(qb, p) for qb in (1, 2) for p in (16, 8, 4, 2)]
    want = {(ns, mode, qb, p) for qb, p in shapes
            for ns, mode in (("", "filter"), ("", "sample"), ("lds_refresh", "filter"), ("bias_fold", "filter"))}
    assert forms == want, sorted(forms ^ want)


def test_no_spill_no_scratch_lds_within_a_cu():
    from kernel_resources import kernel_resources

    res = [v for v in _i8s_kernels().values()] + [(k, r) for k, r in kernel_resources(LIB).items() if DEBUG.search(k)]
    assert len(res) == 34
    for name, r in res:
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert 0 <= r.get("group_segment_fixed_size", 0) <= 160 * 1024, (name, r)
        assert r["vgpr_count"] <= 256, (name, r)  # two waves per SIMD


def test_query_prep_needs_no_scratch():
    """k_prep_q<F16> holds the query's dequantised elements for the fold's sums: one wave per SIMD, so up to 512
    registers, but no VGPR spill and no private segment."""
    from kernel_resources import kernel_resources

    res = {k: r for k, r in kernel_resources(LIB).items() if "k_prep_qILi" in k}
    assert len(res) == 2, sorted(res)  # <BF16> and <F16>
    for name, r in res.items():
        print(f"PREP {name}: {r}")
        assert r.get("vgpr_spill_count", 0) == 0, (name, r)
        assert r.get("private_segment_fixed_size", 0) == 0, (name, r)
        assert r["vgpr_count"] <= 512, (name, r)


def test_vgprs_at_most_the_parents():
    over = []
    for (ns, mode, qb, p), (name, r) in sorted(_i8s_kernels().items()):
        parent = PARENT["lds_refresh" if ns == "lds_refresh" else mode][(qb, p)]
        print(f"VGPR {ns or '-'} {mode} <{qb}, {p}>: {r['vgpr_count']} (parent {parent})")
        if r["vgpr_count"] > parent:
            over.append((ns, mode, qb, p, r["vgpr_count"], parent))
    assert not over, over
