"""GPU: k_merge (hr_merge_candidates[_strided]), k_merge_sorted (hr_merge_sorted) and k_topk_cand (hr_topk_records)
on crafted records against the numpy restatements of tests/merge_ref.py, bit for bit: rows, scores, the k-th score and
the exactness guard.  tests/test_merge_ref_cpu.py proves on the CPU that the cases are what they are named for (the
k_topk_cand path each takes, the hand-written guard flags).  Many cases share one launch, as queries or segments.

Scores are compared as values (assert_array_equal): the sign of a zero is not pinned, -0.0 and +0.0 are one score."""
import numpy as np
import pytest

import merge_ref as M

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rank_major(per_rank, gap_bytes, records=True):
    """per_rank [G, words] float64 -> a buffer whose rank stride is gap_bytes longer than dense.  The gap holds what
    would win: records (+inf, row 0) on the rank's record grid (an odd last word is +inf), or +inf bounds."""
    G, words = per_rank.shape
    assert gap_bytes % 8 == 0
    buf = np.empty((G, words + gap_bytes // 8), np.float64)
    buf[:, :words] = per_rank
    buf[:, words:] = np.where(np.arange(gap_bytes // 8) % 2 == 0, np.inf, 0.0) if records else np.inf
    return buf


def _merge(scores, rows, bounds, k, cand_gap=0, bound_gap=0, cand_stride=None, bound_stride=None):
    import torch

    from hiprag import _native

    G, B, kc = scores.shape
    rec = M.pack(scores, rows).reshape(G, -1)
    cand = _dev(_rank_major(rec, cand_gap))
    bnd = _dev(_rank_major(np.asarray(bounds, np.float64), bound_gap, records=False))
    s = torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda")
    r = torch.full((B, k), -99, dtype=torch.int64, device="cuda")
    kth = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    fail = torch.full((B,), -99, dtype=torch.int32, device="cuda")
    _native.merge_candidates(0, cand.data_ptr(), bnd.data_ptr(), G, B, kc, k, s.data_ptr(), r.data_ptr(),
                             kth.data_ptr(), fail.data_ptr(),
                             cand_rank_stride=cand_stride if cand_stride is not None else
                             (B * kc * 16 + cand_gap if cand_gap or bound_gap else 0),
                             bound_rank_stride=bound_stride if bound_stride is not None else
                             (B * 8 + bound_gap if cand_gap or bound_gap else 0))
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy(), kth.cpu().numpy(), fail.cpu().numpy()


def _assert_merge(got, ref, tag):
    for g, e, what in zip(got, ref, ("scores", "rows", "kth", "fail")):
        np.testing.assert_array_equal(g, e, err_msg=f"{what} {tag}")


# ---------------------------------------------------------------- k_merge
# (3, 48): n = 144, no power of two, the counting rank; (5, 256): n = 1280, the bitonic sort
@pytest.mark.parametrize("G,kc", [(3, 48), (5, 256)])
def test_merge_guard_table(G, kc):
    for k in (1, 10, kc):
        cases = M.merge_cases(G, kc, k)
        names = [c["name"] for c in cases]
        scores, rows, bounds = M.stack_merge_cases(cases)
        got = _merge(scores, rows, bounds, k)
        # the table's hand-written expectations first: the guard and the k-th score, case by case
        np.testing.assert_array_equal(got[3], [c["fail"] for c in cases], err_msg=f"fail k={k} {names}")
        np.testing.assert_array_equal(got[2], [c["kth"] for c in cases], err_msg=f"kth k={k} {names}")
        _assert_merge(got, M.ref_merge(M.pack(scores, rows), bounds, k), f"k={k} {names}")


@pytest.mark.parametrize("G,kc", [(3, 48), (5, 256)])
def test_merge_strided_equals_dense(G, kc):
    """Rank strides larger than dense, the gaps full of winning records and +inf bounds: nothing of a gap is read.
    The second stride is 8 mod 16 bytes, as the packed [B*kc records][B bounds] exchange record of an odd batch is."""
    for k in (1, 10, kc):
        cases = M.merge_cases(G, kc, k)
        scores, rows, bounds = M.stack_merge_cases(cases)
        dense = _merge(scores, rows, bounds, k)
        _assert_merge(dense, M.ref_merge(M.pack(scores, rows), bounds, k), f"dense k={k}")
        for cand_gap, bound_gap in ((5 * 16, 3 * 8), (3 * 16 + 8, 0), (0, 2 * 8)):
            _assert_merge(_merge(scores, rows, bounds, k, cand_gap, bound_gap), dense,
                          f"k={k} gaps=({cand_gap}, {bound_gap})")


@pytest.mark.parametrize("G,kc,ks", [
    (1, 16, (1, 9, 16)),
    (2, 512, (1, 257, 512)),  # n = 1024: the last counting size
    (3, 342, (1, 172, 342)),  # n = 1026: the first bitonic size
    (8, 1024, (1, 128, 1024)),  # n = 8192: the LDS maximum
])
def test_merge_fuzz(G, kc, ks):
    B = 12 if G * kc > 2048 else 24
    for i, k in enumerate(ks):
        scores, rows, bounds = M.merge_fuzz(G, kc, B, seed=i)
        ref = M.ref_merge(M.pack(scores, rows), bounds, k)
        assert 0 < ref[3].sum() < B  # both outcomes of the guard
        _assert_merge(_merge(scores, rows, bounds, k), ref, f"G={G} kc={kc} k={k}")


def test_merge_rejects_bad_geometry():
    scores, rows, bounds = M.merge_fuzz(9, 1024, 1, seed=0)
    with pytest.raises(ValueError):  # 9216 candidates: above the 8192 the kernel's LDS holds
        _merge(scores, rows, bounds, 10)
    scores, rows, bounds = M.merge_fuzz(3, 48, 4, seed=0)
    dense_c, dense_b = 4 * 48 * 16, 4 * 8
    for cs, bs in ((dense_c - 16, dense_b), (dense_c, dense_b - 8), (dense_c + 4, dense_b), (dense_c, dense_b + 4)):
        with pytest.raises(ValueError):  # a rank stride smaller than one rank's data, or no multiple of 8
            _merge(scores, rows, bounds, 10, cand_gap=16, bound_gap=8, cand_stride=cs, bound_stride=bs)
    with pytest.raises(ValueError):
        _merge(scores, rows, bounds, 49)  # k > kc


# ---------------------------------------------------------------- k_merge_sorted
def _merge_sorted(scores, rows, k, gap=0):
    import torch

    from hiprag import _native

    G, B, m = scores.shape
    cand = _dev(_rank_major(M.pack(scores, rows).reshape(G, -1), gap))
    s = torch.full((B, k), float("nan"), dtype=torch.float32, device="cuda")
    r = torch.full((B, k), -99, dtype=torch.int64, device="cuda")
    _native.merge_sorted(0, cand.data_ptr(), G, B, m, k, s.data_ptr(), r.data_ptr(),
                         cand_rank_stride=B * m * 16 + gap if gap else 0)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_merge_sorted(G):
    """B = 5 queries (blockIdx.y) per launch: see merge_ref.merge_sorted_case for what each holds."""
    for m, k in ((64, 10), (64, 64), (64, 100), (64, 3 * 64 + 5), (3000, 5000)):
        scores, rows = M.merge_sorted_case(G, m, k)
        ref_s, ref_r = M.ref_merge_sorted(M.pack(scores, rows), k)
        if k > G * m:  # more asked for than the lists hold: the tail is padding
            assert (ref_r[:, G * m:] == -1).all() and (ref_s[:, G * m:] == -np.inf).all()
        assert (ref_r[4] == -1).all() and (ref_r[1, :min(k, G * m)] >= 0).all()
        for gap in (0, 7 * 16 + 8):  # dense; a larger rank stride with winning records in the gap
            s, r = _merge_sorted(scores, rows, k, gap)
            np.testing.assert_array_equal(r, ref_r, err_msg=f"rows G={G} m={m} k={k} gap={gap}")
            np.testing.assert_array_equal(s, ref_s, err_msg=f"scores G={G} m={m} k={k} gap={gap}")


# ---------------------------------------------------------------- k_topk_cand
def _topk(rec, B, m, seg_off=None, seg_stride=0):
    import torch

    from hiprag import _native

    rd = _dev(rec)
    out = torch.full((B, m, 2), float("nan"), dtype=torch.float64, device="cuda")
    off = _dev(np.asarray(seg_off, np.int64)) if seg_off is not None else None
    _native.topk_records(rd.data_ptr(), B, m, out.data_ptr(), seg_stride=seg_stride,
                         seg_off_ptr=off.data_ptr() if off is not None else 0)
    torch.cuda.synchronize()
    return M.unpack(out.cpu().numpy())


@pytest.fixture(scope="module")
def topk_cases():
    cases = M.topk_cases()
    for c in cases:
        c["ref"] = M.ref_topk(c["scores"], c["ids"], c["m"])
    return cases


@pytest.mark.parametrize("mode", ["seg_off", "seg_stride"])
@pytest.mark.parametrize("m", [1, 10, 100, 1024])
def test_topk_cases(topk_cases, m, mode):
    """Every crafted segment with this m in one launch, one segment per block."""
    cases = [c for c in topk_cases if c["m"] == m]
    assert cases
    empty = dict(name="empty", scores=np.empty(0), ids=np.empty(0, np.int64),
                 ref=(np.full(m, -np.inf), np.full(m, -1, np.int64)))
    if mode == "seg_off":  # empty segments first, in the middle and last
        segs = [empty] + cases[:len(cases) // 2] + [empty, empty] + cases[len(cases) // 2:] + [empty]
        off = np.concatenate([[0], np.cumsum([len(c["ids"]) for c in segs])])
        rec = M.pack(np.concatenate([c["scores"] for c in segs]), np.concatenate([c["ids"] for c in segs]))
        got_s, got_r = _topk(rec, len(segs), m, seg_off=off)
    else:  # equal strides: shorter segments end in absent records that would win, (+inf, -1)
        segs = cases
        stride = max(len(c["ids"]) for c in segs)
        scores = np.full((len(segs), stride), np.inf)
        ids = np.full((len(segs), stride), -1, np.int64)
        for b, c in enumerate(segs):
            scores[b, :len(c["ids"])], ids[b, :len(c["ids"])] = c["scores"], c["ids"]
        got_s, got_r = _topk(M.pack(scores, ids), len(segs), m, seg_stride=stride)
    for b, c in enumerate(segs):
        np.testing.assert_array_equal(got_r[b], c["ref"][1], err_msg=f"ids {c['name']} m={m} {mode}")
        np.testing.assert_array_equal(got_s[b], c["ref"][0], err_msg=f"scores {c['name']} m={m} {mode}")


def test_topk_rejects_bad_m():
    import torch

    from hiprag import _native

    rd = _dev(M.pack(np.zeros(8), np.arange(8)))
    out = torch.empty((1, 1025, 2), dtype=torch.float64, device="cuda")
    for m in (0, 1025):  # the LDS holds 1024 winners
        with pytest.raises(ValueError):
            _native.topk_records(rd.data_ptr(), 1, m, out.data_ptr(), seg_stride=8)
