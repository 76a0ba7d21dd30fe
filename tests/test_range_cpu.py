"""CPU: range search above the kernel -- the restatement itself (tests/range_ref.py) against the cut of the reference's
full ranking, the new symbols and their null-handle validation, and the store, retriever and IVF-store wiring over a
numpy-backed stand-in index (tests/fake_index_range.py)."""
import asyncio
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from fake_index import OracleIndex
from fake_index_range import RangeOracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.ivf_store import IvfStoreIndex
from hiprag.rag.retriever import VectorRetriever
from hiprag.rag.storage import RangeHits
from oracle import ref_numpy as R
from range_ref import assert_same, range_ref

DTYPES = ["f32", "bf16", "f16"]
METRICS = ["cosine", "ip", "l2"]


def run(coro):
    return asyncio.run(coro)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_range_ref_is_the_cut_of_the_full_ranking(dtype, metric):
    """range_ref == R.search(k = n) cut where its fp32 score drops below the threshold, bit for bit, with the
    boundary row in (t = its score) and out (one ulp above)."""
    rng = np.random.default_rng(3 * DTYPES.index(dtype) + METRICS.index(metric))
    n, dim, B = 4099, 64, 3
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    if metric != "cosine":
        x = x * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    st = R.process_rows(x, metric, dtype)
    q = R.process_queries(_unit(x[rng.choice(n, B)]) + 0.05 * _unit(rng.standard_normal((B, dim)).astype(np.float32)),
                          metric)
    allowed = rng.random(n) < 0.8
    scores = R.exact_scores(st, dtype, q, metric)
    full_s, full_r = R.search(st, dtype, q, n, allowed, metric=metric)
    full32 = full_s.astype(np.float32)
    for j in (0, 9, 99, 1500):
        t_in = full32[:, j].copy()
        for t in (t_in, np.nextafter(t_in, np.float32(np.inf)), np.float32(-np.inf), np.float32(np.inf)):
            for max_hits in (1, 128, n):
                s, r, c = range_ref(st, dtype, q, t, max_hits, allowed, metric, scores=scores)
                for b in range(B):
                    tb = np.broadcast_to(np.asarray(t, np.float32), (B,))[b]
                    cut = int(((full_r[b] >= 0) & (full32[b] >= tb)).sum())
                    assert c[b] == cut
                    m = min(cut, max_hits)
                    np.testing.assert_array_equal(r[b, :m], full_r[b, :m])
                    np.testing.assert_array_equal(s[b, :m].view(np.uint32), full32[b, :m].view(np.uint32))
                    assert (r[b, m:] == -1).all() and np.isneginf(s[b, m:]).all()
        # the boundary row is a hit at its own score and not one ulp above it
        assert (range_ref(st, dtype, q, t_in, 0, allowed, metric, scores=scores)[2] >= j + 1).all()
        up = range_ref(st, dtype, q, np.nextafter(t_in, np.float32(np.inf)), 0, allowed, metric, scores=scores)[2]
        assert (up <= j).all()


def test_range_ref_nan_scores_ties_and_empty():
    x = np.zeros((6, 2), np.float32)
    x[:] = [[1, 0], [0.5, 0], [0.5, 0], [np.nan, 0], [0.25, 0], [0.5, 0]]
    st = R.process_rows(x, "ip", "f32")
    q = np.asarray([[1.0, 0.0]], np.float32)
    s, r, c = range_ref(st, "f32", q, 0.5, 3, metric="ip")
    assert c.tolist() == [4] and r.tolist() == [[0, 1, 2]] and s.tolist() == [[1.0, 0.5, 0.5]]  # ties: rows ascending
    s, r, c = range_ref(st, "f32", q, -np.inf, 8, metric="ip")
    assert c.tolist() == [5] and r.tolist() == [[0, 1, 2, 5, 4, -1, -1, -1]]  # the NaN row is never a hit
    assert range_ref(st, "f32", q, np.inf, 2, metric="ip")[2].tolist() == [0]
    allowed = np.asarray([False, True, True, True, True, False])
    assert range_ref(st, "f32", q, 0.5, 0, allowed, "ip")[2].tolist() == [2]
    s, r, c = range_ref(st[:0], "f32", q, 0.0, 2, metric="ip")
    assert c.tolist() == [0] and r.tolist() == [[-1, -1]]
    with pytest.raises(AssertionError):
        assert_same((s, r, c), (s, r, c + 1))
    assert_same((None, None, c), (s, r, c))


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_index_search_range", "hr_index_search_range_device"]
NEW_DIAG = ["hr_index_range_stats", "hr_index_range_wave_tiles"]


def test_new_symbols_are_declared_exported_and_validate():
    from hiprag import _native

    def decls(name):
        text = open(os.path.join(REPO, "include", name)).read()
        return set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))

    assert set(NEW) <= decls("hiprag.h") and set(NEW_DIAG) <= decls("hiprag_diag.h")
    assert "#define HR_RANGE_MAX_HITS 65536" in open(os.path.join(REPO, "include", "hiprag.h")).read()
    assert _native.HR_RANGE_MAX_HITS == 65536
    assert set(NEW + NEW_DIAG) <= set(_native.EXPORTS)
    for m in ("search_range", "search_range_device", "range_stats", "range_wave_tiles"):
        assert callable(getattr(_native.NativeIndex, m))
    assert "hr_range.hip" in open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert os.path.exists(_native.LIB_PATH), "libhiprag.so not built (run __graft_entry__.build())"
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in NEW + NEW_DIAG:
        assert hasattr(L, name)
    # no handle, no device needed: every entry point refuses a null handle or null arrays with HR_E_INVALID
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hr_index_search_range(None, p, 1, p, 1, None, p, p, p) == -1
    assert b"null" in L.hr_last_error()
    assert L.hr_index_search_range_device(None, p, 1, p, 1, None, p, p, p, None) == -1
    assert L.hr_index_range_stats(None, p) == -1
    assert L.hr_index_range_wave_tiles(None, p, 1, p) == -1


# ---------------------------------------------------------------- the store
def make_store(tmp_path, index=RangeOracleIndex, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"))


def cluster_chunks(n=120, seed=1, dim=16):
    """Three clusters of 40 rows around three centres: a query near a centre has ~40 rows far above the rest."""
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((3, dim)).astype(np.float32))
    x = _unit(centres[np.arange(n) % 3] + 0.3 * _unit(rng.standard_normal((n, dim)).astype(np.float32)))
    return [Chunk(id=f"c{i}", document_id=f"d{i % 3}", content=f"t{i}", chunk_index=i, metadata={"part": i % 5},
                  embedding=x[i].tolist()) for i in range(n)], x, centres


def want(store, q, t, max_hits, allowed=None):
    idx = store._index
    live = idx.live if allowed is None else idx.live & allowed
    s, r, c = range_ref(idx.rows, "f32", R.process_queries(np.atleast_2d(np.asarray(q, np.float32)), "cosine"), t,
                        max_hits, live)
    return [([(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0], int(c[b])) for b in range(len(c))]


def got_of(res):
    return [([(c.id, s) for c, s in h.hits], h.total) for h in res]


def test_store_scalar_and_per_query_thresholds(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    q = centres[:2].tolist()
    res = s.search_range_batch(q, 0.955)
    assert s._index.range_calls == [(2, [np.float32(0.955)] * 2, 1024, False)]
    assert all(isinstance(h, RangeHits) for h in res)
    assert got_of(res) == want(s, q, 0.955, 1024)
    assert all(5 <= h.total < 40 and not h.truncated and len(h.hits) == h.total for h in res)
    res = s.search_range_batch(q, [0.955, 0.965], max_hits=7)
    assert s._index.range_calls[-1] == (2, [np.float32(0.955), np.float32(0.965)], 7, False)
    assert got_of(res) == want(s, q, [0.955, 0.965], 7)
    assert res[0].truncated and len(res[0].hits) == 7 and res[0].total > 7  # the list was cut, the count was not
    assert res[1].total < res[0].total
    one = run(s.search_range(q[0], 0.955, max_hits=7))
    assert s._index.range_calls[-1] == (1, [np.float32(0.955)], 7, False) and got_of([one]) == want(s, q[:1], 0.955, 7)
    # 0.0 is a threshold like any other, -inf returns every row
    assert s.search_range_batch(q[:1], -np.inf, max_hits=200)[0].total == 120
    assert got_of(s.search_range_batch(q[:1], 0.0)) == want(s, q[:1], 0.0, 1024)


def test_store_count_only_filters_and_deletes(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    q = centres.tolist()
    part = np.arange(len(chunks)) % 5
    counts = s.count_above_batch(q, 0.955)
    assert s._index.range_calls[-1] == (3, [np.float32(0.955)] * 3, 0, False)  # max_hits = 0: no lists asked for
    assert counts == [w[1] for w in want(s, q, 0.955, 0)] and all(isinstance(c, int) for c in counts)
    # one where-clause for the batch
    res = s.search_range_batch(q, 0.955, 50, {"part": 1})
    assert s._index.range_calls[-1][3] is True and got_of(res) == want(s, q, 0.955, 50, part == 1)
    assert s.count_above_batch(q, 0.955, {"part": 1}) == [h.total for h in res]
    # one clause (or None) per query: one launch per distinct clause, scattered back in query order
    flt = [{"part": 1}, None, {"part": 1}]
    del s._index.range_calls[:]
    before = s.grouped_launches
    res = s.search_range_batch(q, [0.955, 0.95, 0.965], 50, flt)
    assert sorted((c[0], c[3]) for c in s._index.range_calls) == [(1, False), (2, True)]
    assert s.grouped_launches - before == 2
    ts = [0.955, 0.95, 0.965]
    for i, f in enumerate(flt):
        assert got_of([res[i]]) == want(s, q[i], ts[i], 50, None if f is None else part == 1)
    assert s.count_above_batch(q, ts, flt) == [h.total for h in res]
    # a list holding one distinct clause is the single-mask call
    del s._index.range_calls[:]
    s.search_range_batch(q, 0.955, 50, [{"part": 1}] * 3)
    assert [(c[0], c[3]) for c in s._index.range_calls] == [(3, True)]
    # deletes: the removed chunks leave the hits and the count
    top = [cid for cid, _ in want(s, q[:1], 0.955, 1024)[0][0]][:5]
    total = s.count_above_batch(q[:1], 0.955)[0]
    run(s.delete(top))
    res = s.search_range_batch(q[:1], 0.955)
    assert res[0].total == total - 5 and not set(top) & {c.id for c, _ in res[0].hits}
    assert got_of(res) == want(s, q[:1], 0.955, 1024)


def test_store_error_cases(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks(40)
    empty = s.search_range_batch([centres[0].tolist()], 0.5)  # nothing stored: no index yet
    assert empty == [RangeHits([], 0)] and s.count_above_batch([centres[0].tolist()], 0.5) == [0]
    run(s.add_chunks(chunks))
    q = centres[0].tolist()
    bad = [dict(min_score=float("nan")), dict(min_score=0.5, max_hits=-1), dict(min_score=0.5, max_hits=65537),
           dict(min_score=[0.5, 0.6])]
    for kw in bad:
        with pytest.raises(ValueError):
            s.search_range_batch([q], **kw)
        with pytest.raises(ValueError):
            run(s.search_range(q, **kw))
    with pytest.raises(ValueError):
        s.count_above_batch([q], float("nan"))
    with pytest.raises(ValueError, match="dim"):
        s.search_range_batch([q + [0.0]], 0.5)
    with pytest.raises(ValueError, match="filters"):
        s.search_range_batch([q], 0.5, 10, [None, None])
    assert s._index.range_calls == []  # every limit is checked before any native call
    assert s.search_range_batch([q], 0.5, max_hits=65536)[0].total == s.count_above_batch([q], 0.5)[0]
    s._index.devices = [0, 1]
    with pytest.raises(ValueError, match="single-device"):
        s.search_range_batch([q], 0.5)
    with pytest.raises(ValueError, match="single-device"):
        s.count_above_batch([q], 0.5)
    plain = make_store(tmp_path / "plain", index=OracleIndex)
    run(plain.add_chunks(chunks))
    with pytest.raises(NotImplementedError):
        plain.search_range_batch([q], 0.5)
    with pytest.raises(NotImplementedError):
        run(plain.search_range(q, 0.5))
    assert len(plain.search_batch([q], 3)[0]) == 3


def test_ivf_store_delegates_to_its_exact_index():
    exact = RangeOracleIndex(16, "f32")
    chunks, x, centres = cluster_chunks()
    exact.add(x)
    ivf = IvfStoreIndex(16, "f32", "cosine", nlist=4, nprobe=1, _exact=exact)
    got = ivf.search_range(centres[:2], [0.955, 0.965], 9)
    assert exact.range_calls == [(2, [np.float32(0.955), np.float32(0.965)], 9, False)]
    assert_same(got, range_ref(exact.rows, "f32", R.process_queries(centres[:2], "cosine"), [0.955, 0.965], 9))


# ---------------------------------------------------------------- the retriever
class StubStore:
    def __init__(self, n=6, total=9):
        self.calls, self.n, self.total = [], n, total

    async def search_range(self, query_embedding, min_score, max_hits=1024, filters=None):
        self.calls.append((min_score, max_hits, filters))
        hits = [(Chunk(id=f"c{i}", document_id=f"d{i}", content=f"t{i}", chunk_index=0, metadata={}), 0.9 - 0.1 * i)
                for i in range(min(self.n, max_hits))]
        return RangeHits(hits, self.total)


class Emb:
    async def embed_query(self, q):
        return [0.0, 1.0]


class Reverse:
    async def rerank(self, query, results, top_k=None):
        return list(reversed(results))


def test_retrieve_above_ranks_default_and_reranker():
    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=4, similarity_threshold=0.35))
    res = run(ret.retrieve_above("q"))
    assert st.calls == [(0.35, 1024, None)]  # None: the config's threshold, the default limit
    assert [(r.chunk.id, r.rank) for r in res] == [(f"c{i}", i + 1) for i in range(6)]  # 1-based, not cut by top_k
    run(ret.retrieve_above("q", threshold=0.0, limit=3, filters={"a": 1}))
    assert st.calls[-1] == (0.0, 3, {"a": 1})  # 0.0 is used as given, unlike retrieve()
    run(ret.retrieve_above("q", threshold=-1.5))
    assert st.calls[-1] == (-1.5, 1024, None)
    zero = VectorRetriever(st, Emb(), RetrieverConfig(top_k=4, similarity_threshold=0.0))
    run(zero.retrieve_above("q"))
    assert st.calls[-1] == (0.0, 1024, None)
    rr = VectorRetriever(StubStore(), Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.1), reranker=Reverse())
    res = run(rr.retrieve_above("q", limit=4))
    assert [r.chunk.id for r in res] == ["c3", "c2", "c1", "c0"] and [r.rank for r in res] == [4, 3, 2, 1]

    class NoRange:
        async def search(self, *a, **kw):
            return []

    with pytest.raises(NotImplementedError):
        run(VectorRetriever(NoRange(), Emb(), RetrieverConfig()).retrieve_above("q", 0.5))


def test_retrieve_above_over_the_store(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    qv = centres[0].tolist()

    class E:
        async def embed_query(self, q):
            return qv

    ret = VectorRetriever(s, E(), RetrieverConfig(top_k=3, similarity_threshold=0.955))
    res = run(ret.retrieve_above("q"))
    w = want(s, qv, 0.955, 1024)[0][0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    assert len(res) > 3  # everything relevant, not config.top_k of it
    assert len(run(ret.retrieve_above("q", limit=5))) == 5
