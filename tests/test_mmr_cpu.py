"""CPU: MMR search above the kernel -- the restatement itself (tests/mmr_ref.py) on a hand-worked case and its stated
consequences (lambda = 1, prefix stability, the role assignment under l2 / fp32), the new symbols and their null-handle
validation, and the store, batcher, retriever and kb_tools wiring over a numpy-backed stand-in index
(tests/fake_index_mmr.py)."""
import asyncio
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import REPO
from fake_index import OracleIndex
from fake_index_mmr import AsyncMmrOracleIndex, MmrOracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag import kb_tools as K
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.retriever import BatchedVectorRetriever, HybridRetriever, VectorRetriever
from mmr_ref import assert_same, default_fetch_k, greedy, mmr_ref, pool_sim
from oracle import ref_numpy as R


def run(coro):
    return asyncio.run(coro)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _dup_rows(rng, n, dim=64, spread=0.5):
    """Near-duplicate runs of 2..7 rows: unit(centre of the run + spread * unit noise)."""
    run_of = []
    while len(run_of) < n:
        run_of += [len(set(run_of))] * int(rng.integers(2, 8))
    run_of = np.asarray(run_of[:n])
    centres = _unit(rng.standard_normal((run_of[-1] + 1, dim)).astype(np.float32))
    return _unit(centres[run_of] + spread * _unit(rng.standard_normal((n, dim)).astype(np.float32)))


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("use_c", [True, False])
def test_hand_worked_case(use_c):
    """q = (1, 0), inner product, lambda = 0.5, every number a dyadic fraction (exact in fp32 and fp64).
    rel = [1, .9375, .75, .5].  Step 0 takes row 0.  sim(0, .) = [., 1.1875, .5, .5]:
    v = [., .46875 - .59375, .375 - .25, .25 - .25] = [., -.125, .125, 0] -> row 2.  sim(2, .) = [., .453125, ., .375]
    leaves maxsim = [., 1.1875, ., .5]: v = [., -.125, ., 0] -> row 3, then row 1."""
    x = np.zeros((4, 2), np.float32)
    x[:] = [[1, 0.5], [0.9375, 0.5], [0.75, -0.5], [0.5, 0]]
    q = np.asarray([[1.0, 0.0]], np.float32)
    st = R.process_rows(x, "ip", "f32")
    s, r = mmr_ref(st, "f32", q, 4, 0.5, 4, metric="ip", use_c=use_c)
    assert r.tolist() == [[0, 2, 3, 1]]
    assert s.tolist() == [[1.0, 0.75, 0.5, 0.9375]]  # each row's relevance: not monotone
    assert mmr_ref(st, "f32", q, 4, 1.0, 4, metric="ip", use_c=use_c)[1].tolist() == [[0, 1, 2, 3]]
    # lambda = 0: relevance only breaks ties; after row 0 the least similar of rows 2, 3 (both .5): the lower position
    assert mmr_ref(st, "f32", q, 3, 0.0, 4, metric="ip", use_c=use_c)[1].tolist() == [[0, 2, 3]]
    # a pool of 2 never sees rows 2, 3; k beyond the rows pads
    assert mmr_ref(st, "f32", q, 2, 0.5, 2, metric="ip", use_c=use_c)[1].tolist() == [[0, 1]]
    s, r = mmr_ref(st, "f32", q, 6, 0.5, 8, metric="ip", use_c=use_c)
    assert r.tolist() == [[0, 2, 3, 1, -1, -1]] and np.isneginf(s[0, 4:]).all()
    allowed = np.asarray([True, True, False, True])
    assert mmr_ref(st, "f32", q, 4, 0.5, 4, allowed, "ip", use_c)[1].tolist() == [[0, 3, 1, -1]]


def test_greedy_ties_and_nan():
    rel = np.asarray([1.0, 0.5, 0.5, 0.5])
    sim = np.zeros((4, 4))
    assert greedy(rel, sim, 4, 0.5) == [0, 1, 2, 3]  # equal values: the lowest position
    sim[0, 1] = np.inf  # lambda = 1: 0 * inf = NaN counts as -inf, so position 1 goes last
    assert greedy(rel, sim, 4, 1.0) == [0, 2, 3, 1]
    assert greedy(rel, sim, 9, 0.5) == [0, 2, 3, 1] and greedy(rel, sim, 1, 0.5) == [0]


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("metric", ["cosine", "ip", "l2"])
def test_lambda_one_prefix_stability_and_a_real_penalty(dtype, metric):
    rng = np.random.default_rng(["f32", "bf16", "f16"].index(dtype) * 3 + ["cosine", "ip", "l2"].index(metric))
    x = _dup_rows(rng, 300)
    st = R.process_rows(x, metric, dtype)
    q = R.process_queries(x[rng.choice(300, 3)] + 0.05 * _unit(rng.standard_normal((3, 64)).astype(np.float32)), metric)
    plain_s, plain_r = R.search(st, dtype, q, 10, metric=metric)
    assert_same(mmr_ref(st, dtype, q, 10, 1.0, 32, metric=metric), (plain_s.astype(np.float32), plain_r))
    full = mmr_ref(st, dtype, q, 20, 0.5, 32, metric=metric)
    for k in (1, 5, 10):
        got = mmr_ref(st, dtype, q, k, 0.5, 32, metric=metric)
        assert_same(got, (full[0][:, :k], full[1][:, :k]))
    # near-duplicate runs: the penalty changes every query's list, so a selection that ignores it cannot pass
    assert all((full[1][b, :10] != plain_r[b]).any() for b in range(3))
    assert default_fetch_k(1) == 32 and default_fetch_k(10) == 40 and default_fetch_k(64) == 128


def test_l2_fp32_similarity_depends_on_the_roles():
    """(|s|^2 - 2 s.j) + |j|^2 rounds differently when s and j swap: the selected row takes the query role."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((32, 64)).astype(np.float32)
    rows = np.arange(32)
    l2 = pool_sim(R.process_rows(x, "l2", "f32"), "f32", rows, "l2")
    assert (l2 != l2.T).any() and np.abs(l2 - l2.T).max() < 1e-12
    for metric in ("cosine", "ip"):
        sym = pool_sim(R.process_rows(x, metric, "f32"), "f32", rows, metric)
        assert (sym == sym.T).all()
    # the restatement reads sim[s, j] with s the selected row: with the transposed matrix some value v differs
    s, j = np.argwhere(l2 != l2.T)[0]
    rel = np.zeros(32)
    rel[0], first = 1.0, [int(s)] + [i for i in range(32) if i != s]
    a = l2[np.ix_(first, first)]
    v_fwd = 0.5 * rel[1:] - 0.5 * a[0, 1:]
    v_rev = 0.5 * rel[1:] - 0.5 * a.T[0, 1:]
    assert (v_fwd != v_rev).any()


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_index_search_mmr", "hr_index_search_mmr_device"]
NEW_DIAG = ["hr_index_set_mmr_timing", "hr_index_mmr_last_ms"]


def test_new_symbols_are_declared_exported_and_validate():
    from hiprag import _native

    def decls(name):
        text = open(os.path.join(REPO, "include", name)).read()
        return set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))

    assert set(NEW) <= decls("hiprag.h") and set(NEW_DIAG) <= decls("hiprag_diag.h")
    assert set(NEW + NEW_DIAG) <= set(_native.EXPORTS)
    for m in ("search_mmr", "search_mmr_device", "set_mmr_timing", "mmr_last_ms"):
        assert callable(getattr(_native.NativeIndex, m))
    assert "hr_mmr.hip" in open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert os.path.exists(_native.LIB_PATH), "libhiprag.so not built (run __graft_entry__.build())"
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in NEW + NEW_DIAG:
        assert hasattr(L, name)
    # no handle, no device needed: every entry point refuses a null handle or null arrays with HR_E_INVALID
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hr_index_search_mmr(None, p, 1, 1, 0, 0.5, None, p, p) == -1
    assert b"null" in L.hr_last_error()
    assert L.hr_index_search_mmr_device(None, p, 1, 1, 0, 0.5, None, p, p, None) == -1
    assert L.hr_index_set_mmr_timing(None, 1) == -1 and L.hr_index_mmr_last_ms(None, p) == -1


# ---------------------------------------------------------------- the store
def make_store(tmp_path, index=MmrOracleIndex, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"))


def dup_chunks(n=120, seed=1, dim=16):
    rng = np.random.default_rng(seed)
    x = _dup_rows(rng, n, dim)
    return [Chunk(id=f"c{i}", document_id=f"d{i % 3}", content=f"t{i}", chunk_index=i, metadata={"part": i % 3},
                  embedding=x[i].tolist()) for i in range(n)], x


def want_ids(store, q, k, lam, fetch_k=0, allowed=None):
    idx = store._index
    live = idx.live if allowed is None else idx.live & allowed
    s, r = mmr_ref(idx.rows, "f32", R.process_queries(np.atleast_2d(np.asarray(q, np.float32)), "cosine"), k, lam,
                   fetch_k, live)
    return [[(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0] for b in range(len(s))]


def ids(hits):
    return [(c.id, s) for c, s in hits]


def test_store_keywords_reach_the_index(tmp_path):
    s = make_store(tmp_path)
    chunks, x = dup_chunks()
    run(s.add_chunks(chunks))
    q = (x[[3, 50]] + 0.02).tolist()
    got = s.search_batch(q, 10, mmr_lambda=0.5)
    assert s._index.mmr_calls == [(2, 10, 0.5, 40, False)]  # fetch_k resolved to its default by the store
    assert [ids(h) for h in got] == want_ids(s, q, 10, 0.5, 40)
    assert [ids(h) for h in got] != [ids(h) for h in s.search_batch(q, 10)]  # diversified
    scores = [sc for _, sc in got[0]]
    assert scores != sorted(scores, reverse=True)  # selection order: not monotone
    got = s.search_batch(q, 5, {"part": 1}, mmr_lambda=0.25, fetch_k=32)
    assert s._index.mmr_calls[-1] == (2, 5, 0.25, 32, True)
    part1 = np.arange(len(chunks)) % 3 == 1
    assert [ids(h) for h in got] == want_ids(s, q, 5, 0.25, 32, part1)
    one = run(s.search(q[0], 5, mmr_lambda=0.5, fetch_k=64))
    assert s._index.mmr_calls[-1] == (1, 5, 0.5, 64, False) and ids(one) == want_ids(s, q[:1], 5, 0.5, 64)[0]
    assert [ids(h) for h in s.search_batch(q, 7, mmr_lambda=1.0)] == [ids(h) for h in s.search_batch(q, 7)]
    # k = min(top_k, n_live); off: the plain path, and the index is not asked
    before = len(s._index.mmr_calls)
    assert len(s.search_batch(q[:1], 128, mmr_lambda=0.5)[0]) == 120 and s._index.mmr_calls[-1][1] == 120
    s.search_batch(q, 5, mmr_lambda=None, fetch_k=64)
    assert len(s._index.mmr_calls) == before + 1
    assert run(s.search(q[0], 0, mmr_lambda=0.5)) == []


def test_store_error_cases(tmp_path):
    s = make_store(tmp_path)
    chunks, x = dup_chunks(40)
    run(s.add_chunks(chunks))
    q = x[0].tolist()
    bad = [dict(top_k=129, mmr_lambda=0.5), dict(top_k=5, mmr_lambda=1.5), dict(top_k=5, mmr_lambda=-0.1),
           dict(top_k=5, mmr_lambda=float("nan")), dict(top_k=10, mmr_lambda=0.5, fetch_k=9),
           dict(top_k=10, mmr_lambda=0.5, fetch_k=129), dict(top_k=5, mmr_lambda=0.5, collapse=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            s.search_batch([q], **kw)
        with pytest.raises(ValueError):
            run(s.search(q, **kw))
    assert s._index.mmr_calls == [] and s._batcher.launches == 0  # refused before queueing

    async def one_bad_among_good():
        return await asyncio.gather(s.search(q, 3, mmr_lambda=0.5), s.search(q, 3, mmr_lambda=2.0),
                                    s.search(q, 3, mmr_lambda=0.5), return_exceptions=True)

    r = run(one_bad_among_good())
    assert isinstance(r[1], ValueError) and ids(r[0]) == ids(r[2]) == want_ids(s, q, 3, 0.5, 32)[0]
    assert len(s.search_batch([q], 10, mmr_lambda=0.5, fetch_k=10)[0]) == 10  # fetch_k = top_k is allowed
    with pytest.raises(TypeError):
        s.search_batch([q], 3, None, False, 0.5)  # keyword-only
    s._index.devices = [0, 1]
    with pytest.raises(ValueError, match="single-device"):
        s.search_batch([q], 3, mmr_lambda=0.5)
    plain = make_store(tmp_path / "plain", index=OracleIndex)
    run(plain.add_chunks(chunks))
    with pytest.raises(NotImplementedError):
        plain.search_batch([q], 3, mmr_lambda=0.5)
    with pytest.raises(NotImplementedError):
        run(plain.search(q, 3, mmr_lambda=0.5))  # the waiter sees the worker's error
    assert len(plain.search_batch([q], 3)[0]) == 3


def test_batcher_keeps_modes_apart_and_shares_prefixes(tmp_path):
    s = make_store(tmp_path, index=AsyncMmrOracleIndex)
    chunks, x = dup_chunks()
    run(s.add_chunks(chunks))
    q = (x[7] + 0.02).tolist()

    async def mixed_modes():
        return await asyncio.gather(*[s.search(q, 5, mmr_lambda=0.5 if i % 2 else None) for i in range(8)])

    launches, native = s._batcher.launches, s._batcher.native_launches
    res = run(mixed_modes())
    assert s._index.mmr_calls == [(4, 5, 0.5, 32, False)] and s._batcher.launches - launches == 2
    assert s._batcher.native_launches - native == 1  # the plain batch took the asynchronous entry point, as ever
    plain, mmr = ids(s.search_batch([q], 5)[0]), want_ids(s, q, 5, 0.5, 32)[0]
    assert plain != mmr and all(ids(r) == (mmr if i % 2 else plain) for i, r in enumerate(res))

    # different top_k, one (lambda, fetch_k): one launch at the largest top_k, every caller gets its prefix
    async def mixed_k():
        return await asyncio.gather(*[s.search(q, k, mmr_lambda=0.5, fetch_k=64) for k in (3, 12, 1, 7)])

    del s._index.mmr_calls[:]
    res = run(mixed_k())
    assert s._index.mmr_calls == [(4, 12, 0.5, 64, False)]
    full = want_ids(s, q, 12, 0.5, 64)[0]
    assert [ids(r) for r in res] == [full[:3], full, full[:1], full[:7]]

    # another lambda, another pool size, a filter: launches of their own
    async def apart():
        return await asyncio.gather(s.search(q, 4, mmr_lambda=0.5, fetch_k=64), s.search(q, 4, mmr_lambda=0.25, fetch_k=64),
                                    s.search(q, 4, mmr_lambda=0.5, fetch_k=32), s.search(q, 4, mmr_lambda=0.5),
                                    s.search(q, 4, {"part": 1}, mmr_lambda=0.5, fetch_k=64))

    del s._index.mmr_calls[:]
    res = run(apart())
    assert sorted(s._index.mmr_calls) == sorted([(1, 4, 0.5, 64, False), (1, 4, 0.25, 64, False),
                                                 (2, 4, 0.5, 32, False), (1, 4, 0.5, 64, True)])
    assert ids(res[2]) == ids(res[3]) == want_ids(s, q, 4, 0.5, 32)[0]
    assert ids(res[4]) == want_ids(s, q, 4, 0.5, 64, np.arange(len(chunks)) % 3 == 1)[0]


@pytest.mark.parametrize("mixed_filters", [False, True])
def test_filter_list_is_answered_per_distinct_filter(tmp_path, mixed_filters):
    s = make_store(tmp_path, mixed_filters=mixed_filters)
    chunks, x = dup_chunks()
    run(s.add_chunks(chunks))
    q = (x[[7, 20, 33, 90]] + 0.02).tolist()
    flt = [{"part": 1}, None, {"part": 1}, {"part": 2}]
    before = s.grouped_launches
    got = s.search_batch(q, 6, flt, mmr_lambda=0.5)
    assert sorted(c[:4] + (c[4],) for c in s._index.mmr_calls) == sorted(
        [(2, 6, 0.5, 32, True), (1, 6, 0.5, 32, False), (1, 6, 0.5, 32, True)])
    assert s.grouped_launches - before == 3
    part = np.arange(len(chunks)) % 3
    for i, f in enumerate(flt):
        allowed = None if f is None else part == f["part"]
        assert ids(got[i]) == want_ids(s, q[i], 6, 0.5, 32, allowed)[0]

    async def concurrent():
        return await asyncio.gather(*[s.search(q[i], 6, flt[i], mmr_lambda=0.5) for i in range(4)])

    del s._index.mmr_calls[:]
    res = run(concurrent())
    assert len(s._index.mmr_calls) == 3 and [ids(r) for r in res] == [ids(g) for g in got]


# ---------------------------------------------------------------- retrievers
class StubStore:
    """Records what the retriever asks for; returns `n` hits per query, scores not monotone (an MMR list)."""

    def __init__(self, n=10):
        self.calls, self.n = [], n

    def _hits(self, top_k):
        return [(Chunk(id=f"c{i}", document_id=f"d{i}", content=f"t{i}", chunk_index=0, metadata={}),
                 [0.9, 0.5, 0.8, 0.4, 0.7, 0.3, 0.6, 0.2, 0.1, 0.0][i]) for i in range(min(self.n, top_k))]

    async def search(self, query_embedding, top_k=5, filters=None, **kw):
        self.calls.append(("search", top_k, filters, kw))
        return self._hits(top_k)

    def search_batch(self, qvs, top_k=5, filters=None, **kw):
        self.calls.append(("search_batch", top_k, filters, kw))
        return [self._hits(top_k) for _ in qvs]


class Emb:
    async def embed_query(self, q):
        return [0.0, 1.0]


class Reverse:
    async def rerank(self, query, results, top_k=None):
        return list(reversed(results))


def test_retrievers_pass_the_keywords():
    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=4))
    res = run(ret.retrieve("q", mmr_lambda=0.5, fetch_k=64, similarity_threshold=0.45, filters={"a": 1}))
    assert st.calls == [("search", 4, {"a": 1}, {"mmr_lambda": 0.5, "fetch_k": 64})]
    # threshold and ranks apply to the MMR list: ranks are positions in selection order, before the threshold
    assert [(r.chunk.id, r.rank) for r in res] == [("c0", 1), ("c1", 2), ("c2", 3)]
    run(ret.retrieve("q", mmr_lambda=0.0))
    run(ret.retrieve("q"))
    run(ret.retrieve("q", mmr_lambda=None, fetch_k=64))
    assert st.calls[1:] == [("search", 4, None, {"mmr_lambda": 0.0}), ("search", 4, None, {}), ("search", 4, None, {})]
    rr = VectorRetriever(StubStore(), Emb(), RetrieverConfig(top_k=3, similarity_threshold=0.0), reranker=Reverse())
    res = run(rr.retrieve("q", mmr_lambda=0.5))
    assert rr.vector_store.calls == [("search", 6, None, {"mmr_lambda": 0.5})]  # 2 * top_k under a reranker
    assert [r.chunk.id for r in res] == ["c5", "c4", "c3"]
    bst = StubStore()
    bat = BatchedVectorRetriever(bst, Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.0))
    res = run(bat.batch_retrieve(["a", "b"], mmr_lambda=0.5, fetch_k=32))
    assert bst.calls == [("search_batch", 2, None, {"mmr_lambda": 0.5, "fetch_k": 32})] and [len(r) for r in res] == [2, 2]
    run(bat.batch_retrieve(["a"]))
    assert bst.calls[1] == ("search_batch", 2, None, {})


def test_mmr_skips_the_fused_path():
    class FusedStub:
        submitted = 0

        def submit(self, query, top_k, threshold):
            self.submitted += 1
            f = asyncio.get_running_loop().create_future()
            f.set_result([])
            return f

    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.0))
    ret._fused = FusedStub()
    assert run(ret.retrieve("q")) == [] and ret._fused.submitted == 1 and st.calls == []
    assert len(run(ret.retrieve("q", mmr_lambda=0.5))) == 2 and ret._fused.submitted == 1
    assert st.calls == [("search", 2, None, {"mmr_lambda": 0.5})]


def test_hybrid_retriever_refuses_mmr_with_keyword_search():
    class LexStore(StubStore):
        lexical = True

        def keyword_search_batch(self, queries, top_k=5, filters=None):
            return [[] for _ in queries]

    hy = HybridRetriever(LexStore(), Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.0))
    with pytest.raises(ValueError, match="MMR"):
        run(hy.retrieve("q", mmr_lambda=0.5))
    with pytest.raises(ValueError, match="MMR"):
        run(hy.batch_retrieve(["q"], mmr_lambda=0.5))
    assert len(run(hy.retrieve("q"))) == 2
    plain = HybridRetriever(StubStore(), Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.0))  # no keyword search: the delegation
    assert len(run(plain.retrieve("q", mmr_lambda=0.5))) == 2
    assert plain.vector_store.calls[-1][3] == {"mmr_lambda": 0.5}


# ---------------------------------------------------------------- kb_embedding_search
def test_kb_embedding_search_option(tmp_path, monkeypatch):
    def no_reranker(backend):
        raise RuntimeError("no reranker")

    monkeypatch.setattr(K, "_reranker_from", no_reranker)
    chunks, x = dup_chunks()
    qv = (x[7] + 0.02).tolist()

    class E:
        async def embed_query(self, q):
            return qv

    out = {}
    for name, conf in (("off", {}), ("on", {"mmr_lambda": 0.5}), ("pool", {"mmr_lambda": 0.5, "mmr_fetch_k": 64})):
        def factory(cfg, name=name):
            cfg = cfg.model_copy(update={"persist_directory": str(tmp_path / name),
                                         "index_params": {**cfg.index_params, "dtype": "f32", "persist": False}})
            return HipVectorStore(cfg, index_factory=lambda d: MmrOracleIndex(d, "f32"))

        tk = K.KBSearchToolkit(config=conf, kb_resolver=lambda kb: ("coll", "KB"), store_factory=factory)
        tk._embedder_cache = E()
        store = tk._get_or_create_vector_store("coll", "./rag_data/vector_store")
        run(store.add_chunks(chunks))
        out[name] = json.loads(run(tk.kb_embedding_search(1, "q", top_k=6, auto_rerank=False)))
        calls = store._index.mmr_calls
        assert calls == {"off": [], "on": [(1, 6, 0.5, 32, False)], "pool": [(1, 6, 0.5, 64, False)]}[name]
        assert (tk.mmr_lambda, tk.mmr_fetch_k) == (conf.get("mmr_lambda"), conf.get("mmr_fetch_k"))
        want = want_ids(store, qv, 6, 0.5, calls[0][3])[0] if calls else ids(store.search_batch([qv], 6)[0])
        assert [r["chunk_id"] for r in out[name]["results"]] == [c for c, _ in want]
    assert out["on"]["results"] != out["off"]["results"] and set(out["on"]) == set(out["off"])  # the same JSON shape
