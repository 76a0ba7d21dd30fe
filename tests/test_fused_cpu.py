"""CPU: the fused multi-query search without a GPU -- the reference restatement (tests/fused_ref.py) against
retriever.rrf_fuse and a brute force, the C boundary's argument checks (they run on the host before any device call),
the Python wrappers' checks, and the store / retriever on fake indexes: the native route (FusedOracleIndex) and the
host composition (an index without search_fused) must agree."""
import asyncio
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle
from conftest import REPO
from fake_index import OracleIndex
from fake_index_fused import FusedOracleIndex
from fused_ref import assert_same, check_args, default_fetch, fuse_ref, pools_ref, search_fused_ref
from hash_embed import HashEmbedder, vec
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.retriever import VectorRetriever, rrf_fuse
from hiprag.rag.storage import FusedHits, fuse_lists_host
from oracle import ref_numpy as R


def run(coro):
    return asyncio.run(coro)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _lists(rng, Q, P, n, short=0):
    """Q ranked lists of P distinct rows of an n-row corpus, the last `short` slots padding; scores descending."""
    rows = np.stack([rng.choice(n, P, replace=False) for _ in range(Q)]).astype(np.int64)
    scores = -np.sort(-rng.standard_normal((Q, P)).astype(np.float32), axis=1)
    if short:
        rows[:, P - short:] = -1
        scores[:, P - short:] = -np.inf
    return rows, scores


# ---------------------------------------------------------------- the restatement
def test_two_members_are_rrf_fuse_bit_for_bit():
    rng = np.random.default_rng(0)
    for P, n, rrf_k in ((50, 80, 60.0), (7, 9, 60.0), (128, 150, 0.0), (20, 1000, 10.5)):
        rows, scores = _lists(rng, 2, P, n, short=P // 5)
        want = rrf_fuse(*[[(int(r), p + 1, None) for p, r in enumerate(rows[i]) if r >= 0] for i in range(2)], rrf_k)
        k = min(P, len(want))
        f, r, m = fuse_ref(rows, scores, [2], k, "rrf", rrf_k)
        assert r[0].tolist() == [key for key, _, _ in want[:k]]
        assert [x.hex() for x in f[0].tolist()] == [float(v).hex() for _, v, _ in want[:k]]
        held = [set(rows[i][rows[i] >= 0].tolist()) for i in range(2)]
        assert m[0].tolist() == [(row in held[0]) | (row in held[1]) << 1 for row in r[0].tolist()]
        assert_same(fuse_lists_host(scores, rows, [2], k, "rrf", rrf_k), (f, r, m))


def test_the_exact_tie_is_ordered_by_row():
    assert 1.0 / (60.0 + 1.0) == 1.0 / (60.0 + 62.0) + 1.0 / (60.0 + 62.0)  # an exact fp64 tie
    P = 64
    for first_row, both_row in ((900, 5), (5, 900)):
        rows = np.full((2, P), -1, np.int64)
        rows[0, :] = 1000 + np.arange(P)
        rows[1, :] = 2000 + np.arange(P)
        rows[0, 0] = first_row  # rank 1 in member 0 only
        rows[0, 61] = rows[1, 61] = both_row  # rank 62 in both
        f, r, m = fuse_ref(rows, np.zeros((2, P), np.float32), [2], 3)
        assert f[0, 0] == f[0, 1] == 1.0 / 61.0
        assert r[0, :2].tolist() == sorted([first_row, both_row])
        assert sorted(m[0, :2].tolist()) == [1, 3]
        assert_same(fuse_lists_host(np.zeros((2, P), np.float32), rows, [2], 3), (f, r, m))


def test_one_member_rrf_keeps_the_pools_order():
    rng = np.random.default_rng(1)
    rows, scores = _lists(rng, 3, 40, 100, short=4)
    for w in (None, [0.25, 3.0, 1e-3]):
        f, r, m = fuse_ref(rows, scores, [1, 1, 1], 40, "rrf", 60.0, w)
        np.testing.assert_array_equal(r, rows)
        assert (m[rows >= 0] == 1).all() and (m[rows < 0] == 0).all() and np.isneginf(f[rows < 0]).all()
        assert (np.diff(f[:, :36], axis=1) < 0).all()


def test_max_fusion_details():
    rows = np.asarray([[3, 1, 2, -1], [2, 3, 9, 1], [7, -1, -1, -1]], np.int64)
    scores = np.asarray([[0.9, np.nan, -0.0, -np.inf], [0.0, 0.95, -np.inf, 0.5], [np.nan, 0, 0, 0]], np.float32)
    f, r, m = fuse_ref(rows, scores, [3], 4, "max")
    assert r[0].tolist() == [3, 1, 2, 7] and m[0].tolist() == [3, 3, 3, 4]  # 9 and 7 tie at -inf: row ascending
    assert f[0].tolist()[:2] == [float(np.float32(0.95)), 0.5] and np.isneginf(f[0, 3])
    assert math.copysign(1.0, f[0, 2]) == -1.0  # -0.0 came first and 0.0 is not larger: member order decides
    f, r, m = fuse_ref(rows, scores, [3], 4, "rrf", 60.0, [0.0, -1.0, 2.0])  # zero and negative weights
    assert r[0].tolist() == [7, 1, 9, 3] and f[0].tolist() == [0.0 + 2.0 / 61.0, 0.0 + 0.0 / 62.0 + -1.0 / 64.0,
                                                              -1.0 / 63.0, 0.0 + 0.0 / 61.0 + -1.0 / 62.0]
    assert_same(fuse_lists_host(scores, rows, [3], 4, "max"), fuse_ref(rows, scores, [3], 4, "max"))
    assert_same(fuse_lists_host(scores, rows, [2, 1], 3, "rrf", 0.0, [0.0, -1.0, 2.0]),
                fuse_ref(rows, scores, [2, 1], 3, "rrf", 0.0, [0.0, -1.0, 2.0]))


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "ip"), ("f16", "l2")])
def test_max_is_the_corpus_wide_top_k_of_the_max(dtype, metric):
    rng = np.random.default_rng(2)
    n, dim, k = 300, 16, 10
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    stored = R.process_rows(x, metric, dtype)
    q = rng.standard_normal((7, dim)).astype(np.float32)
    groups = [4, 1, 2]
    full = np.full((7, n), -np.inf, np.float32)
    for i in range(7):
        s, r = oracle.c_search(stored, dtype, R.process_queries(q[i:i + 1], metric), n, None, nthreads=2, metric=metric)
        full[i, r[0]] = s[0].astype(np.float32)
    for fetch_k in (0, k, 25):
        f, r, m = search_fused_ref(stored, dtype, q, groups, k, fetch_k, "max", metric=metric)
        pool_r = pools_ref(stored, dtype, q, fetch_k or k, None, metric)[1]
        q0 = 0
        for g, cnt in enumerate(groups):
            best = full[q0:q0 + cnt].max(axis=0).astype(np.float64)
            order = sorted(range(n), key=lambda row: (-best[row], row))[:k]
            np.testing.assert_array_equal(f[g], best[order])
            above = f[g] > f[g, -1]  # (the choice among equal scores at the cut is pool-defined)
            np.testing.assert_array_equal(r[g][above], np.asarray(order)[above])
            for t in range(k):  # (a member that scores the row below its own pool's last entry does not hold it)
                holds = [j for j in range(cnt) if r[g, t] in pool_r[q0 + j]]
                assert m[g, t] == sum(1 << j for j in holds) and holds
            q0 += cnt


def test_default_fetch_and_every_refusal_of_the_reference():
    assert default_fetch(10, "rrf") == 50 and default_fetch(20, "rrf") == 80 and default_fetch(100, "rrf") == 128
    assert default_fetch(10, "max") == 10
    ok = dict(groups=[2, 1], k=3, P=5, mode="rrf", rrf_k=60.0, weights=None)
    check_args(**ok)
    for bad in (dict(groups=[]), dict(groups=[0, 3]), dict(groups=[17]), dict(k=0), dict(k=6), dict(P=129, k=3),
                dict(mode="sum"), dict(rrf_k=-1.0), dict(rrf_k=math.inf), dict(rrf_k=math.nan),
                dict(weights=[1.0, 2.0]), dict(weights=[1.0, math.inf, 1.0]), dict(weights=[1.0, math.nan, 1.0]),
                dict(mode="max", weights=[1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            check_args(**{**ok, **bad})
    check_args(**{**ok, "weights": [0.0, -2.0, 1.0], "rrf_k": 0.0})


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_fuse_lists", "hr_index_search_fused", "hr_index_search_fused_device"]


def _lib():
    from hiprag import _native

    assert os.path.exists(_native.LIB_PATH), "libhiprag.so not built (run __graft_entry__.build())"
    return _native, _native.load_library()


def test_new_symbols_are_declared_and_exported():
    _native, L = _lib()
    text = open(os.path.join(REPO, "include", "hiprag.h")).read()
    assert set(NEW) <= set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))
    assert "#define HR_FUSE_MAX_MEMBERS 16" in text
    assert re.search(r"HR_FUSE_RRF\s*=\s*0\s*,\s*HR_FUSE_MAX\s*=\s*1", text)
    assert _native.HR_FUSE_MAX_MEMBERS == 16 and _native.FUSE_MODES == {"rrf": 0, "max": 1}
    assert set(NEW) <= set(_native.EXPORTS)
    for m in ("fuse_lists", "search_fused", "search_fused_device"):
        assert callable(getattr(_native.NativeIndex, m))
    assert callable(_native.fuse_lists)
    assert "hr_fuse.hip" in open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert L.hr_abi_version() == 2
    for name in NEW:
        assert hasattr(L, name)


def test_the_library_refuses_on_the_host_before_any_device_call():
    """hr_fuse_lists checks every argument before it touches a device, so each refusal is visible without a GPU."""
    _native, L = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(P=8, off=(0, 2, 3), w=None, G=None, k=4, mode=0, rrf_k=60.0, rows=p, out=p):
        off_a = np.asarray(off, np.int64)
        w_a = None if w is None else np.asarray(w, np.float32)
        return L.hr_fuse_lists(0, rows, p, P, off_a.ctypes.data_as(ctypes.c_void_p),
                               None if w_a is None else w_a.ctypes.data_as(ctypes.c_void_p),
                               len(off_a) - 1 if G is None else G, k, mode, rrf_k, out, out, None, None)

    for kw in (dict(rows=None), dict(out=None), dict(G=0), dict(G=-1), dict(mode=2), dict(mode=-1), dict(P=0),
               dict(P=129, k=4), dict(k=0), dict(k=9), dict(rrf_k=-0.5), dict(rrf_k=math.inf), dict(rrf_k=math.nan),
               dict(off=(0, 0, 3)), dict(off=(0, 17)), dict(off=(1, 2)), dict(off=(0, 2, 1)),
               dict(w=[1.0, math.nan, 1.0]), dict(w=[1.0, math.inf, 1.0]), dict(w=[1.0, 1.0, 1.0], mode=1)):
        assert call(**kw) == -1, kw
        assert L.hr_last_error()
    assert L.hr_fuse_lists(0, p, p, 8, None, None, 1, 4, 0, 60.0, p, p, None, None) == -1
    assert b"null" in L.hr_last_error()
    off = np.asarray([0, 1], np.int64).ctypes.data_as(ctypes.c_void_p)
    assert L.hr_index_search_fused(None, p, off, None, 1, 1, 0, 0, 60.0, None, 0, 0, None, p, p, None) == -1
    assert L.hr_index_search_fused_device(None, p, off, None, 1, 1, 0, 0, 60.0, None, 0, 0, None, p, p, None, None) == -1


def test_the_wrappers_refuse_before_the_library():
    _native, _ = _lib()
    off, w = _native._fuse_groups([2, 1, 16], [1, 0.0, -2, *([1.0] * 16)])
    assert off.tolist() == [0, 2, 3, 19] and off.dtype == np.int64 and w.dtype == np.float32 and len(w) == 19
    assert _native._fuse_groups([3], None)[1] is None
    for groups, weights in (([], None), ([0], None), ([17], None), ([2], [1.0])):
        with pytest.raises(ValueError):
            _native._fuse_groups(groups, weights)
    with pytest.raises(ValueError):
        _native._fuse_mode("sum")
    assert _native._fuse_mode("rrf") == 0 and _native._fuse_mode("max") == 1


# ---------------------------------------------------------------- the store and the retriever
def make_store(tmp_path, index=FusedOracleIndex, name="kb", **params):
    cfg = VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                            index_params={"dtype": "f32", "persist": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"))


def corpus(n=160, dim=48):
    texts = [f"document {i // 8} passage {i % 8}" for i in range(n)]
    x = np.stack([vec(t, dim) for t in texts])
    for i in range(0, n, 8):  # a document's passages resemble its first one
        x[i + 1:i + 8] = x[i] + 0.6 * x[i + 1:i + 8]
    return [Chunk(id=f"c{i}", document_id=f"d{i // 8}", content=texts[i], chunk_index=i, metadata={"part": i % 3},
                  embedding=x[i].tolist()) for i in range(n)], x


def want(store, groups, k, allowed=None, **kw):
    idx = store._index
    q = np.concatenate([np.asarray(g, np.float32).reshape(-1, idx.dim) for g in groups])
    if isinstance(allowed, list):
        allowed = [idx.live if a is None else idx.live & a for a in allowed]
    else:
        allowed = idx.live if allowed is None else idx.live & allowed
    f, r, m = search_fused_ref(idx.rows, "f32", q, [len(np.atleast_2d(g)) for g in groups], k, allowed=allowed, **kw)
    return [([(f"c{row}", float(sc)) for sc, row in zip(f[g], r[g]) if row >= 0],
             [int(b) for b, row in zip(m[g], r[g]) if row >= 0]) for g in range(len(groups))]


def got(res):
    assert all(isinstance(h, FusedHits) for h in res)
    return [([(c.id, s) for c, s in h.hits], list(h.members)) for h in res]


def _groups(x, rng):
    noisy = lambda rows: (x[rows] + 0.4 * rng.standard_normal((len(rows), x.shape[1]))).astype(np.float32)  # noqa: E731
    return [noisy([8, 9, 10, 40]), noisy([80]), noisy([16, 17]), noisy([3] * 16)]


def test_store_native_and_host_composed_agree(tmp_path):
    chunks, x = corpus()
    rng = np.random.default_rng(3)
    groups = _groups(x, rng)
    native = make_store(tmp_path, FusedOracleIndex, "a", mixed_filters=True)
    host = make_store(tmp_path, OracleIndex, "b", mixed_filters=True)
    for s in (native, host):
        run(s.add_chunks(chunks))
    assert not hasattr(host._index, "search_fused")
    part = np.arange(len(chunks)) % 3
    w = [[1.0, 0.5, 0.25, 2.0], [1.0], [0.0, -1.0], [1.0] * 16]
    cases = [dict(), dict(fusion="max"), dict(fusion="max", fetch_k=40), dict(rrf_k=0, fetch_k=20), dict(weights=w),
             dict(filters={"part": 1}), dict(fusion="max", filters={"part": 2})]
    for kw in cases:
        ref_kw = {"mode": kw.get("fusion", "rrf")}
        if "rrf_k" in kw:
            ref_kw["rrf_k"] = float(kw["rrf_k"])
        if "fetch_k" in kw:
            ref_kw["fetch_k"] = kw["fetch_k"]
        if "weights" in kw:
            ref_kw["weights"] = [v for ws in w for v in ws]
        allowed = None if "filters" not in kw else part == kw["filters"]["part"]
        a, b = got(native.search_fused_batch(groups, 6, **kw)), got(host.search_fused_batch(groups, 6, **kw))
        assert a == b == want(native, groups, 6, allowed, **ref_kw), kw
    # one filter per member, in flattened order
    flt = [{"part": i % 3} if i % 4 else None for i in range(23)]
    allowed = [None if f is None else part == f["part"] for f in flt]
    a, b = got(native.search_fused_batch(groups, 6, filters=flt)), got(host.search_fused_batch(groups, 6, filters=flt))
    assert a == b == want(native, groups, 6, allowed)
    assert native._index.fused_calls[-1][-1] is not None and host.grouped_launches >= 4
    # after deletes; top_k beyond the live rows of a filter
    for s in (native, host):
        run(s.delete([f"c{i}" for i in range(8, 12)]))
    a, b = got(native.search_fused_batch(groups, 6)), got(host.search_fused_batch(groups, 6))
    assert a == b == want(native, groups, 6) and not {"c8", "c9", "c10", "c11"} & {cid for h, _ in a for cid, _ in h}
    one = run(native.search_fused(groups[0], 5, fusion="max"))
    assert got([one]) == want(native, groups[:1], 5, mode="max") == got([run(host.search_fused(groups[0], 5, fusion="max"))])
    for s in (native, host):
        s.close()


def test_store_refusals_and_empty_cases(tmp_path):
    chunks, x = corpus(40)
    store = make_store(tmp_path)
    assert store.search_fused_batch([x[:2]], 3) == [FusedHits([], [])]  # an empty store
    run(store.add_chunks(chunks))
    assert store.search_fused_batch([], 3) == []
    for kw in (dict(fusion="sum"), dict(rrf_k=-1), dict(rrf_k=float("nan")), dict(fetch_k=2), dict(fetch_k=129),
               dict(weights=[[1.0]]), dict(weights=[[1.0, float("inf")]]), dict(fusion="max", weights=[[1.0, 1.0]]),
               dict(filters=[None]), dict(filters=[{"part": 1}, None])):  # (per-member filters need mixed_filters)
        with pytest.raises(ValueError):
            store.search_fused_batch([x[:2]], 3, **kw)
    with pytest.raises(ValueError):
        store.search_fused_batch([x[:17]], 3)
    with pytest.raises(ValueError):
        store.search_fused_batch([x[:2]], 129)
    with pytest.raises(ValueError):
        store.search_fused_batch([x[:2, :5]], 3)
    assert got(store.search_fused_batch([x[:2]], 3, filters=[{"part": 1}, {"part": 1}])) == \
        want(store, [x[:2]], 3, np.arange(40) % 3 == 1)  # one distinct clause: no mixed_filters needed
    big = got(store.search_fused_batch([x[:2]], 100, fusion="max"))  # top_k beyond the rows: every row, once
    assert len(big[0][0]) == 40 and big == want(store, [x[:2]], 100, mode="max")
    store.close()


def test_retrieve_fused(tmp_path):
    chunks, x = corpus()
    store = make_store(tmp_path)
    run(store.add_chunks(chunks))
    emb = HashEmbedder()
    queries = ["what is in document 3", "document 3 passage", "contents of the third document"]
    qv = np.stack([vec("query: " + q) for q in queries])
    ret = VectorRetriever(store, emb, RetrieverConfig(top_k=5, similarity_threshold=0.9))
    res = run(ret.retrieve_fused(queries))
    w = want(store, [qv], 5)[0][0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    assert len(res) == 5 and all(r.score < 0.9 for r in res)  # an RRF score is no similarity: the threshold is ignored
    assert store._index.fused_calls[-1][:5] == ([3], 5, 50, "rrf", 60.0)
    full = want(store, [qv], 8, mode="max")[0][0]
    th = (full[2][1] + full[3][1]) / 2
    assert full[2][1] > th > full[3][1]
    res = run(ret.retrieve_fused(queries, 8, fusion="max", similarity_threshold=th, filters=None))
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(full[:3])]
    res = run(ret.retrieve_fused(queries, 4, weights=[1.0, 0.5, 0.25], rrf_k=10, fetch_k=30, filters={"part": 0}))
    w = want(store, [qv], 4, np.arange(len(chunks)) % 3 == 0, weights=[1.0, 0.5, 0.25], rrf_k=10.0, fetch_k=30)[0][0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    assert run(ret.retrieve_fused([])) == []
    store.close()
