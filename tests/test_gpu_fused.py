"""GPU: the fused multi-query search (hr_fuse.hip) against tests/fused_ref.py, bit for bit: fused scores
equal as fp64 bit patterns, rows and member masks equal.  hr_fuse_lists alone on crafted device lists -- overlapping,
disjoint at the LDS's capacity, padded, short, NaN / -inf scores, the exact fp64 tie, zero and negative weights,
rrf_k = 0, k beyond the distinct rows, groups of every size in one call, 1 and 70 groups --, then search_fused with
pools taken from the oracle's exact top-fetch_k (never from the library's own search): every dtype and metric, 70
queries with a group across the scan's 64-query chunk, fetch_k beyond the rows, planted duplicates, a repeated query,
deletes, shared and per-member masks, the device forms, the errors, and the store and retriever on a real index."""
import asyncio

import numpy as np
import pytest

import oracle
from fused_ref import assert_same, fuse_ref, search_fused_ref
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["cosine", "ip", "l2"]


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _fuse(native, rows, scores, groups, k, mode="rrf", rrf_k=60.0, weights=None, members=True):
    """hr_fuse_lists on device copies of the lists; returns host (fused, rows, members or None)."""
    import torch

    dev = torch.device("cuda", 0)
    rows = np.ascontiguousarray(rows, np.int64)
    scores = np.ascontiguousarray(scores, np.float32)
    G = len(groups)
    rd, sd = torch.from_numpy(rows).to(dev), torch.from_numpy(scores).to(dev)
    f = torch.full((G, k), 7.0, dtype=torch.float64, device=dev)
    r = torch.full((G, k), 7, dtype=torch.int64, device=dev)
    m = torch.full((G, k), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    native.fuse_lists(0, rd.data_ptr(), sd.data_ptr(), rows.shape[1], groups, k, f.data_ptr(), r.data_ptr(),
                      m.data_ptr() if members else 0, mode, rrf_k, weights)
    if not members:
        assert (m.cpu().numpy() == 7).all()  # never written
    return f.cpu().numpy(), r.cpu().numpy(), m.cpu().numpy().view(np.uint32) if members else None


def _lists(rng, Q, P, n, short=None):
    """Q ranked lists of P distinct rows of an n-row corpus; list i keeps P - short[i] entries; scores descending."""
    rows = np.stack([rng.choice(n, P, replace=False) for _ in range(Q)]).astype(np.int64)
    scores = -np.sort(-rng.standard_normal((Q, P)).astype(np.float32), axis=1)
    for i, cut in enumerate(short or []):
        if cut:
            rows[i, P - cut:] = -1
            scores[i, P - cut:] = -np.inf
    return rows, scores


# ---------------------------------------------------------------- hr_fuse_lists alone
@pytest.mark.parametrize("mode", ["rrf", "max"])
def test_groups_of_every_size_in_one_call(native, mode):
    """Groups of 1, 2, 3 and 16 members in one call, rows drawn from a small corpus so that members overlap; lists
    shorter than P; k at P; with and without member bits; weights of every sign."""
    rng = np.random.default_rng(1 + (mode == "max"))
    groups = [1, 2, 3, 16, 5, 1]
    Q = sum(groups)
    for P, n, k in ((50, 90, 10), (128, 200, 128), (7, 8, 7), (1, 5, 1)):
        rows, scores = _lists(rng, Q, P, n, short=[int(c) for c in rng.integers(0, P, Q)])
        scores[rng.random((Q, P)) < 0.05] = np.nan
        for w in ((None,) if mode == "max" else (None, rng.uniform(-1.0, 2.0, Q).astype(np.float32))):
            if w is not None:
                w[::5] = 0.0
            ref = fuse_ref(rows, scores, groups, k, mode, 60.0, w)
            assert_same(_fuse(native, rows, scores, groups, k, mode, 60.0, w), ref)
            assert_same(_fuse(native, rows, scores, groups, k, mode, 60.0, w, members=False), ref)


def test_fully_overlapping_and_fully_disjoint_members(native):
    rng = np.random.default_rng(3)
    P = 128
    same = np.tile(rng.choice(5000, P, replace=False).astype(np.int64), (16, 1))
    for i in range(16):  # the same rows in every member, each in an order of its own
        same[i] = rng.permutation(same[i])
    disjoint = rng.permutation(16 * P).astype(np.int64).reshape(16, P) * 3 + 1  # 2048 distinct rows: the largest set
    scores = -np.sort(-rng.standard_normal((16, P)).astype(np.float32), axis=1)
    w = rng.uniform(0.5, 1.5, 16).astype(np.float32)
    for rows in (same, disjoint):
        for mode, ww in (("rrf", None), ("rrf", w), ("max", None)):
            for k in (1, 128):
                got = _fuse(native, rows, scores, [16], k, mode, 60.0, ww)
                assert_same(got, fuse_ref(rows, scores, [16], k, mode, 60.0, ww))
                bits = got[2][0].astype(np.int64)
                if rows is same:
                    assert (bits == 0xFFFF).all()  # every member holds every row
                else:
                    assert ((bits & (bits - 1)) == 0).all() and (bits > 0).all()  # exactly one member each
    # disjoint members under RRF without weights: position p of every member ties; row ascending within the tie
    got = _fuse(native, disjoint, scores, [16], 32)
    assert got[1][0, :16].tolist() == sorted(disjoint[:, 0].tolist())
    assert got[1][0, 16:].tolist() == sorted(disjoint[:, 1].tolist())


def test_padding_short_lists_and_k_beyond_the_distinct_rows(native):
    P = 16
    rows = np.full((5, P), -1, np.int64)
    scores = np.full((5, P), -np.inf, np.float32)
    f, r, m = _fuse(native, rows, scores, [2, 3], 16)  # all padding
    assert (r == -1).all() and np.isneginf(f).all() and (m == 0).all()
    rows[0, :3], rows[1, :2], rows[3, :1] = [5, 9, 2], [9, 7], [11]
    scores[0, :3], scores[1, :2], scores[3, :1] = [0.9, 0.8, 0.7], [0.95, 0.1], [0.2]
    for mode in ("rrf", "max"):
        got = _fuse(native, rows, scores, [2, 3], 16, mode)
        assert_same(got, fuse_ref(rows, scores, [2, 3], 16, mode))
        assert (got[1][0, :4] >= 0).all() and (got[1][0, 4:] == -1).all() and np.isneginf(got[0][0, 4:]).all()
        assert got[1][1].tolist() == [11] + [-1] * 15 and got[2][1].tolist() == [2] + [0] * 15
    assert _fuse(native, rows, scores, [2, 3], 16, "max")[1][0, :4].tolist() == [9, 5, 2, 7]


def test_nan_and_infinite_scores_in_max(native):
    rows = np.asarray([[3, 1, 2, -1], [2, 3, 9, 1], [7, -1, -1, -1]], np.int64)
    scores = np.asarray([[0.9, np.nan, -0.0, -np.inf], [0.0, 0.95, -np.inf, 0.5], [np.nan, 0, 0, 0]], np.float32)
    got = _fuse(native, rows, scores, [3], 4, "max")
    assert_same(got, fuse_ref(rows, scores, [3], 4, "max"))
    assert got[1][0].tolist() == [3, 1, 2, 7] and np.signbit(got[0][0, 2]) and np.isneginf(got[0][0, 3])
    scores[:] = np.inf
    scores[1, 1] = -np.inf
    assert_same(_fuse(native, rows, scores, [3], 4, "max"), fuse_ref(rows, scores, [3], 4, "max"))


def test_the_exact_tie_zero_and_negative_weights_and_rrf_k_zero(native):
    P = 64
    for first_row, both_row in ((900, 5), (5, 900)):  # 1 / (60 + 1) == 1 / (60 + 62) + 1 / (60 + 62) in fp64
        rows = np.stack([1000 + np.arange(P), 2000 + np.arange(P)]).astype(np.int64)
        rows[0, 0] = first_row
        rows[0, 61] = rows[1, 61] = both_row
        got = _fuse(native, rows, np.zeros((2, P), np.float32), [2], 3)
        assert_same(got, fuse_ref(rows, np.zeros((2, P), np.float32), [2], 3))
        assert got[0][0, 0] == got[0][0, 1] == 1.0 / 61.0 and got[1][0, :2].tolist() == sorted([first_row, both_row])
    rng = np.random.default_rng(4)
    rows, scores = _lists(rng, 6, 40, 70, short=[0, 3, 39, 0, 12, 0])
    for w in ([0.0] * 6, [-1.0, 2.0, 0.0, -0.5, 1e-30, 3e38], [0.0, 0.0, 1.0, -1.0, 1.0, -1.0]):
        for rrf_k in (0.0, 60.0, 0.5, 1e6):
            w32 = np.asarray(w, np.float32)
            assert_same(_fuse(native, rows, scores, [3, 3], 40, "rrf", rrf_k, w32),
                        fuse_ref(rows, scores, [3, 3], 40, "rrf", rrf_k, w32))
    got = _fuse(native, rows, scores, [3, 3], 5, "rrf", 0.0)
    assert got[0].max() <= 3.0 and (got[0][:, 0] >= 1.0).all()  # rrf_k = 0: the first rank counts 1


@pytest.mark.parametrize("G", [1, 70])
def test_group_counts(native, G):
    rng = np.random.default_rng(G)
    groups = [int(c) for c in rng.integers(1, 5, G)]
    rows, scores = _lists(rng, sum(groups), 50, 120)
    for mode in ("rrf", "max"):
        assert_same(_fuse(native, rows, scores, groups, 10, mode), fuse_ref(rows, scores, groups, 10, mode))


def test_fuse_lists_refusals(native):
    rows, scores = _lists(np.random.default_rng(5), 3, 8, 20)
    bad = [dict(groups=[0, 3]), dict(groups=[17]), dict(groups=[]), dict(k=0), dict(k=9), dict(mode="sum"),
           dict(rrf_k=-1.0), dict(rrf_k=float("nan")), dict(rrf_k=float("inf")), dict(weights=[1.0, float("nan"), 1.0]),
           dict(weights=[1.0, 1.0]), dict(mode="max", weights=[1.0, 1.0, 1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            _fuse(native, rows, scores, **{**dict(groups=[2, 1], k=4), **kw})
    assert_same(_fuse(native, rows, scores, [2, 1], 4), fuse_ref(rows, scores, [2, 1], 4))


# ---------------------------------------------------------------- the whole search
def _build(native, x, dtype="bf16", metric="cosine"):
    idx = native.NativeIndex(x.shape[1], dtype, metric)
    idx.add(x)
    return idx, R.process_rows(x, metric, dtype)


def _corpus(rng, n, dim=64, metric="cosine"):
    """Clustered rows, so that the members of a group (noisy copies of one centre) share most of their pools."""
    centres = _unit(rng.standard_normal((max(1, n // 40), dim)).astype(np.float32))
    x = _unit(centres[rng.integers(0, len(centres), n)] + 0.5 * _unit(rng.standard_normal((n, dim)).astype(np.float32)))
    return x if metric == "cosine" else x * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)


def _queries(rng, x, groups, noise=0.3):
    """Per group one anchor row, per member a noisy copy of it."""
    out = []
    for m in groups:
        a = x[rng.integers(0, len(x))]
        out.append(a[None, :] + noise * _unit(rng.standard_normal((m, x.shape[1])).astype(np.float32)))
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_dtypes_and_metrics(native, dtype, metric):
    rng = np.random.default_rng(10 * DTYPES.index(dtype) + METRICS.index(metric))
    x = _corpus(rng, 1000, metric=metric)
    idx, stored = _build(native, x, dtype, metric)
    groups = [4, 1, 2, 16]
    q = _queries(rng, x, groups)
    w = rng.uniform(0.1, 2.0, len(q)).astype(np.float32)
    for kw in (dict(), dict(weights=w, rrf_k=10.0), dict(mode="max"), dict(mode="max", fetch_k=40), dict(fetch_k=128)):
        assert_same(idx.search_fused(q, groups, 10, **kw),
                    search_fused_ref(stored, dtype, q, groups, 10, metric=metric, **kw))
    idx.close()


@pytest.mark.parametrize("n", [1, 33, 4099])
def test_row_counts_and_fetch_k_beyond_the_rows(native, n):
    rng = np.random.default_rng(n)
    x = _corpus(rng, n)
    idx, stored = _build(native, x)
    groups = [3, 2]
    q = _queries(rng, x, groups)
    for mode in ("rrf", "max"):
        for k, fetch_k in ((1, 0), (10, 0), (10, 128), (128, 128)):
            got = idx.search_fused(q, groups, k, fetch_k, mode)
            assert_same(got, search_fused_ref(stored, "bf16", q, groups, k, fetch_k, mode))
            assert ((got[1] >= 0).sum(axis=1) == min(k, n)).all() or n > 128
    idx.close()


def test_seventy_queries_with_a_group_across_the_scan_chunk(native):
    rng = np.random.default_rng(6)
    x = _corpus(rng, 4099)
    idx, stored = _build(native, x)
    groups = [4] * 15 + [8, 2]  # queries 60..67 are one group: it straddles the 64-query chunk
    q = _queries(rng, x, groups)
    assert len(q) == 70
    for mode in ("rrf", "max"):
        assert_same(idx.search_fused(q, groups, 10, 50, mode), search_fused_ref(stored, "bf16", q, groups, 10, 50, mode))
    half = np.arange(4099) % 2 == 0
    masks = np.stack([oracle.mask_from_bool(half), oracle.mask_from_bool(~half)])
    mask_of = (np.arange(70) % 3 - 1).astype(np.int32)  # -1, 0, 1 in turn: per-member masks across the chunk too
    allowed = [None if d < 0 else (half if d == 0 else ~half) for d in mask_of]
    assert_same(idx.search_fused(q, groups, 10, 50, masks=masks, mask_of=mask_of),
                search_fused_ref(stored, "bf16", q, groups, 10, 50, allowed=allowed))
    idx.close()


def test_dim_1024(native):
    rng = np.random.default_rng(7)
    x = _corpus(rng, 1000, dim=1024)
    idx, stored = _build(native, x)
    groups = [4, 3]
    q = _queries(rng, x, groups)
    for mode in ("rrf", "max"):
        assert_same(idx.search_fused(q, groups, 10, 0, mode), search_fused_ref(stored, "bf16", q, groups, 10, 0, mode))
    idx.close()


def test_planted_duplicates_and_a_repeated_query(native):
    """corpus[dst] = corpus[src] as tests/golden/ties.npz plants them: equal scores in every pool, so equal fused
    scores, ordered by row; a query given twice in a group doubles every RRF term and leaves MAX alone."""
    rng = np.random.default_rng(8)
    x = _corpus(rng, 1000)
    src = rng.choice(1000, 12, replace=False)
    for s in src:
        x[rng.choice(1000, 3, replace=False)] = x[s]
    for dtype, metric in (("bf16", "cosine"), ("f32", "ip")):
        idx, stored = _build(native, x, dtype, metric)
        q = np.concatenate([x[src[:4]], x[src[:4]] + 0.01 * _unit(rng.standard_normal((4, 64)).astype(np.float32)),
                            x[src[4:6]], x[src[4:6]]]).astype(np.float32)  # the last group: the same two queries twice
        groups = [8, 4]
        ties = 0
        for mode in ("rrf", "max"):
            got = idx.search_fused(q, groups, 20, 50, mode)
            assert_same(got, search_fused_ref(stored, dtype, q, groups, 20, 50, mode, metric=metric))
            ties += int((np.diff(got[0], axis=1) == 0).sum())
            bits = got[2][1].astype(np.int64)
            assert ((bits & 0b0011) == ((bits >> 2) & 0b0011)).all()  # members 0 / 2 and 1 / 3 hold the same rows
        assert ties >= 4
        one = idx.search_fused(q[8:10], [2], 20, 50, "max")
        np.testing.assert_array_equal(one[0], idx.search_fused(q[8:], [4], 20, 50, "max")[0][:1])
        idx.close()


def test_one_member_is_the_plain_search(native):
    rng = np.random.default_rng(9)
    x = _corpus(rng, 1000)
    idx, stored = _build(native, x)
    q = _queries(rng, x, [1, 1, 1])
    s, r = idx.search(q, 10)
    f, fr, m = idx.search_fused(q, [1, 1, 1], 10)
    np.testing.assert_array_equal(fr, r)
    assert (m == 1).all()
    f, fr, m = idx.search_fused(q, [1, 1, 1], 10, mode="max")
    np.testing.assert_array_equal(fr, r)
    np.testing.assert_array_equal(f, s.astype(np.float64))
    idx.close()


def test_deletes_and_masks(native):
    rng = np.random.default_rng(11)
    n = 1000
    x = _corpus(rng, n)
    idx, stored = _build(native, x)
    groups = [3, 4, 1]
    q = _queries(rng, x, groups)
    live = np.ones(n, bool)
    third = [np.arange(n) % 3 == c for c in range(3)]  # masks that partition the corpus
    masks = np.stack([oracle.mask_from_bool(t) for t in third])
    for round_ in range(2):
        for mode in ("rrf", "max"):
            assert_same(idx.search_fused(q, groups, 10, 50, mode),
                        search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, allowed=live))
            shared = np.zeros(8, np.int32) + 1  # one shared mask: the single-mask path
            got = idx.search_fused(q, groups, 10, 50, mode, masks=masks, mask_of=shared)
            assert_same(got, search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, allowed=live & third[1]))
            assert (got[1] % 3 == 1).all()
            part = np.asarray([0, 1, 2, 0, 1, 2, -1, 0], np.int32)  # every member its own third
            got = idx.search_fused(q, groups, 10, 50, mode, masks=masks, mask_of=part)
            allowed = [live if d < 0 else live & third[d] for d in part]
            assert_same(got, search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, allowed=allowed))
            on = got[1][0] >= 0  # a partition: every row of the first group was found by exactly one member
            assert (got[2][0][on] == 1 << (got[1][0][on] % 3)).all()
            none = np.full(8, -1, np.int32)
            assert_same(idx.search_fused(q, groups, 10, 50, mode, masks=masks, mask_of=none),
                        search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, allowed=live))
        gone = np.unique(idx.search_fused(q, groups, 10)[1][:, :3])  # every group's three best go
        idx.remove(gone)
        live[gone] = False
    idx.close()


def test_device_forms(native):
    import torch

    rng = np.random.default_rng(12)
    n = 1000
    x = _corpus(rng, n)
    idx, stored = _build(native, x)
    groups = [4, 2, 1]
    q = _queries(rng, x, groups)
    w = rng.uniform(0.2, 1.5, 7).astype(np.float32)
    half = np.arange(n) % 2 == 0
    masks = np.stack([oracle.mask_from_bool(half), oracle.mask_from_bool(~half)])
    mask_of = np.asarray([0, 1, 0, -1, 1, 1, 0], np.int32)
    allowed = [None if d < 0 else (half if d == 0 else ~half) for d in mask_of]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)  # a non-default stream
    with torch.cuda.stream(stream):
        qd = torch.from_numpy(q).to(dev)
        md = torch.from_numpy(masks.view(np.int64)).to(dev)
        od = torch.from_numpy(mask_of).to(dev)
        f = torch.empty((3, 10), dtype=torch.float64, device=dev)
        r = torch.empty((3, 10), dtype=torch.int64, device=dev)
        m = torch.empty((3, 10), dtype=torch.int32, device=dev)
        out = lambda: (f.cpu().numpy(), r.cpu().numpy(), m.cpu().numpy().view(np.uint32))  # noqa: E731
        for mode, ww in (("rrf", None), ("rrf", w), ("max", None)):
            idx.search_fused_device(qd.data_ptr(), groups, 10, f.data_ptr(), r.data_ptr(), m.data_ptr(), 50, mode,
                                    weights=ww, stream=stream.cuda_stream)
            assert_same(out(), search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, weights=ww))
            assert_same(out(), idx.search_fused(q, groups, 10, 50, mode, weights=ww))
            idx.search_fused_device(qd.data_ptr(), groups, 10, f.data_ptr(), r.data_ptr(), m.data_ptr(), 50, mode,
                                    weights=ww, masks_ptr=md.data_ptr(), D=2, mask_stride=masks.shape[1],
                                    mask_of_ptr=od.data_ptr(), stream=stream.cuda_stream)
            assert_same(out(), search_fused_ref(stored, "bf16", q, groups, 10, 50, mode, weights=ww, allowed=allowed))
        m.fill_(7)
        stream.synchronize()
        idx.search_fused_device(qd.data_ptr(), groups, 10, f.data_ptr(), r.data_ptr(), 0, stream=stream.cuda_stream)
        assert (m.cpu().numpy() == 7).all()  # members_out NULL: never written
        assert_same(out()[:2], search_fused_ref(stored, "bf16", q, groups, 10))
        # the pools of a plain device search, fused where they lie: hr_fuse_lists is hr_index_search_fused's last step
        ps = torch.empty((7, 50), dtype=torch.float32, device=dev)
        pr = torch.empty((7, 50), dtype=torch.int64, device=dev)
        idx.search_device(qd.data_ptr(), 7, 50, ps.data_ptr(), pr.data_ptr(), stream=stream.cuda_stream)
        idx.fuse_lists(pr.data_ptr(), ps.data_ptr(), 50, groups, 10, f.data_ptr(), r.data_ptr(), m.data_ptr(),
                       stream=stream.cuda_stream)
        assert_same(out(), search_fused_ref(stored, "bf16", q, groups, 10))
    idx.close()


def test_errors_leave_the_handle_working(native):
    rng = np.random.default_rng(13)
    n = 100
    x = _corpus(rng, n)
    idx, stored = _build(native, x)
    q = _queries(rng, x, [2, 1])
    ok = dict(q=q, groups=[2, 1], k=5)
    short = np.zeros((1, 1), np.uint64)
    bad = [dict(groups=[2]), dict(groups=[2, 0, 1]), dict(groups=[]), dict(k=0), dict(k=129), dict(fetch_k=4),
           dict(fetch_k=129), dict(mode="sum"), dict(rrf_k=-1.0), dict(rrf_k=float("nan")), dict(rrf_k=float("inf")),
           dict(weights=[1.0, 1.0]), dict(weights=[1.0, float("nan"), 1.0]), dict(weights=[1.0, float("inf"), 1.0]),
           dict(mode="max", weights=[1.0, 1.0, 1.0]), dict(q=q[:, :32]),
           dict(masks=short, mask_of=[0, 0, 0]),  # a bitmap shorter than the index
           dict(masks=oracle.mask_from_bool(np.ones(n, bool)), mask_of=[0, 1, 0]),  # mask_of outside [-1, D)
           dict(masks=oracle.mask_from_bool(np.ones(n, bool)), mask_of=[0, -2, 0]),
           dict(masks=oracle.mask_from_bool(np.ones(n, bool)), mask_of=[0, 0]), dict(mask_of=[0, 0, 0])]
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_fused(**{**ok, **kw})
    with pytest.raises(ValueError):
        idx.search_fused(np.repeat(q[:1], 17, axis=0), [17], 5)
    assert_same(idx.search_fused(np.repeat(q[:1], 16, axis=0), [16], 5),
                search_fused_ref(stored, "bf16", np.repeat(q[:1], 16, axis=0), [16], 5))
    assert_same(idx.search_fused(**ok, weights=[0.0, -1.0, 1.0], rrf_k=0.0),
                search_fused_ref(stored, "bf16", q, [2, 1], 5, weights=[0.0, -1.0, 1.0], rrf_k=0.0))
    s0, r0 = idx.search(q, 5)  # the handle still answers a plain search
    ws, wr = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 5, None, nthreads=2)
    np.testing.assert_array_equal(r0, wr)
    idx.remove(np.arange(n))  # an empty index pads
    f, r, m = idx.search_fused(**ok)
    assert (r == -1).all() and np.isneginf(f).all() and (m == 0).all()
    idx.close()
    two = native.NativeIndex(64, "bf16", "cosine", devices=[0, 0])  # a multi-device handle is out of scope
    two.add(x)
    with pytest.raises(NotImplementedError):
        two.search_fused(**ok)
    assert (two.search(q, 5)[1] >= 0).all()
    two.close()


# ---------------------------------------------------------------- the store and the retriever
def _chunks(n=240):
    from hash_embed import vec
    from hiprag.rag import Chunk

    texts = [f"document {i // 8} passage {i % 8}" for i in range(n)]
    x = np.stack([vec(t) for t in texts])
    for i in range(0, n, 8):  # a document's passages resemble its first one
        x[i + 1:i + 8] = x[i] + 0.6 * x[i + 1:i + 8]
    return [Chunk(id=f"c{i}", document_id=f"d{i // 8}", content=texts[i], chunk_index=i, metadata={"part": i % 3},
                  embedding=x[i].tolist()) for i in range(n)], x


def _store(tmp_path, name, **kw):
    from hiprag.rag import HipVectorStore, VectorStoreConfig

    index_type = kw.pop("index_type", None)
    return HipVectorStore(VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                                            index_type=index_type,
                                            index_params={"dtype": "bf16", "fsync": False, **kw}))


def _want(x, groups, k, allowed=None, **kw):
    q = np.concatenate([np.asarray(g, np.float32).reshape(-1, x.shape[1]) for g in groups])
    f, r, m = search_fused_ref(R.process_rows(x, "cosine", "bf16"), "bf16", q, [len(g) for g in groups], k,
                               allowed=allowed, **kw)
    return [([(f"c{row}", float(sc)) for sc, row in zip(f[g], r[g]) if row >= 0],
             [int(b) for b, row in zip(m[g], r[g]) if row >= 0]) for g in range(len(groups))]


def _got(res):
    return [([(c.id, s) for c, s in h.hits], list(h.members)) for h in res]


def test_store_search_fused_batch_is_the_host_composition(native, tmp_path):
    from hiprag.rag.storage import fuse_lists_host

    chunks, x = _chunks()
    rng = np.random.default_rng(14)
    noisy = lambda rows: (x[rows] + 0.5 * rng.standard_normal((len(rows), x.shape[1]))).astype(np.float32)  # noqa: E731
    groups = [noisy([8, 9, 10, 40]), noisy([80]), noisy([16, 17])]
    store = _store(tmp_path, "kb", mixed_filters=True)
    asyncio.run(store.add_chunks(chunks))
    assert hasattr(store._index, "search_fused")
    part = np.arange(len(chunks)) % 3
    flt = [{"part": i % 3} if i % 4 else None for i in range(7)]
    per_member = [None if f is None else part == f["part"] for f in flt]
    for kw, ref_kw, allowed in ((dict(), dict(), None), (dict(fusion="max"), dict(mode="max"), None),
                                (dict(weights=[[1, 0.5, 0.25, 2], [1], [0, -1]], rrf_k=20),
                                 dict(weights=[1, 0.5, 0.25, 2, 1, 0, -1], rrf_k=20.0), None),
                                (dict(filters={"part": 1}), dict(), part == 1), (dict(filters=flt), dict(), per_member),
                                (dict(fusion="max", filters=flt, fetch_k=30), dict(mode="max", fetch_k=30), per_member)):
        got = _got(store.search_fused_batch(groups, 6, **kw))
        assert got == _want(x, groups, 6, allowed, **ref_kw), kw
        # ... and the host composition over the index's own plain search
        q = np.concatenate(groups)
        P = ref_kw.get("fetch_k") or (6 if ref_kw.get("mode") == "max" else 50)
        s = np.empty((7, P), np.float32)
        r = np.empty((7, P), np.int64)
        for i in range(7):
            ok = allowed[i] if isinstance(allowed, list) else allowed
            s[i], r[i] = store._index.search(q[i:i + 1], P, None if ok is None else oracle.mask_from_bool(ok))
        f, fr, m = fuse_lists_host(s, r, [4, 1, 2], 6, ref_kw.get("mode", "rrf"), ref_kw.get("rrf_k", 60.0),
                                   ref_kw.get("weights"))
        assert got == [([(f"c{row}", float(sc)) for sc, row in zip(f[g], fr[g]) if row >= 0],
                        [int(b) for b, row in zip(m[g], fr[g]) if row >= 0]) for g in range(3)], kw
    one = asyncio.run(store.search_fused(groups[0], 5, fusion="max"))
    assert _got([one]) == _want(x, groups[:1], 5, mode="max")
    store.close()


def test_ivf_store_composes_on_the_host(native, tmp_path):
    chunks, x = _chunks()
    rng = np.random.default_rng(15)
    groups = [(x[[8, 9, 40]] + 0.5 * rng.standard_normal((3, x.shape[1]))).astype(np.float32)]
    store = _store(tmp_path, "kb_ivf", index_type="IVF_FLAT", nlist=4, nprobe=4, ivf_train_rows=64, ivf_seed=1)
    asyncio.run(store.add_chunks(chunks))
    assert store._index.trained and not hasattr(store._index, "search_fused")
    for kw, ref_kw in ((dict(), dict()), (dict(fusion="max"), dict(mode="max"))):
        assert _got(store.search_fused_batch(groups, 6, **kw)) == _want(x, groups, 6, **ref_kw)  # every list probed
    store.close()


def test_retrieve_fused_with_the_hash_embedder(native, tmp_path):
    from hash_embed import HashEmbedder, vec
    from hiprag.rag import RetrieverConfig
    from hiprag.rag.retriever import VectorRetriever

    chunks, x = _chunks()
    store = _store(tmp_path, "kb_r")
    asyncio.run(store.add_chunks(chunks))
    queries = ["what is in document 3", "document 3 passage", "contents of the third document"]
    qv = np.stack([vec("query: " + q) for q in queries])
    ret = VectorRetriever(store, HashEmbedder(), RetrieverConfig(top_k=5, similarity_threshold=0.9))
    res = asyncio.run(ret.retrieve_fused(queries))
    w = _want(x, [qv], 5)[0][0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    assert len(res) == 5  # an RRF score is no similarity: the threshold does not cut it
    full = _want(x, [qv], 8, mode="max")[0][0]
    th = (full[2][1] + full[3][1]) / 2
    assert full[2][1] > th > full[3][1]
    res = asyncio.run(ret.retrieve_fused(queries, 8, fusion="max", similarity_threshold=th))
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(full[:3])]
    store.close()
