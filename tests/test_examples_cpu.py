"""CPU: search by example above the kernels -- the restatement itself (tests/examples_ref.py) against the reference's
plain ranking, the new symbols and their null-handle validation, the store and retriever wiring over a numpy-backed
stand-in index (tests/fake_index_examples.py), and the host composition route of an index without search_examples."""
import asyncio
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO
from examples_ref import assert_same, assert_same_bits, build_ref, examples_ref
from fake_index import OracleIndex
from fake_index_examples import ExamplesOracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.retriever import VectorRetriever
from hiprag.rag.storage import build_queries_host, search_examples_host
from oracle import ref_numpy as R


def run(coro):
    return asyncio.run(coro)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------- the restatement
def test_build_ref_is_the_ordered_float64_sum():
    x = np.asarray([[1.0, 2.0 ** -30, -0.0], [2.0 ** 25, 1.0, 0.0], [-(2.0 ** 25), 3.0, 0.0]], np.float32)
    st = R.process_rows(x, "ip", "f32")
    # float64 keeps 2^25 + 1 exactly where an fp32 accumulator would drop the 1; the order of the list is the order
    got = build_ref(st, "f32", [[1, 0, 2], [0, 0], []], [[1.0, 1.0, 1.0], [0.5, 0.25], []],
                    np.asarray([[0, 0, 0], [1, 1, 1], [-0.0, 5, -0.0]], np.float32))
    assert got[0].tolist() == [1.0, 4.0, 0.0]  # (4 + 2^-30 rounds to 4 in the one cast)
    assert got[1].tolist() == [1.75, np.float32(1.0 + 0.75 * 2.0 ** -30), 1.0]  # a row listed twice adds its weights
    assert_same_bits(got[2], np.asarray([-0.0, 5, -0.0], np.float32))  # no example: the base vector's bits, -0.0 kept
    assert build_ref(st, "f32", [[0]])[0].tolist() == x[0].tolist()  # default weight 1 / m


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "ip"), ("f16", "l2")])
def test_examples_ref_is_the_plain_search_minus_the_examples(dtype, metric):
    rng = np.random.default_rng(3)
    n, dim = 300, 64
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    st = R.process_rows(x, metric, dtype)
    ex = [[5], [7, 200, 7], [17, 18, 19, 250]]
    w = [[1.0], [0.5, -0.25, 0.5], [0.25, 0.25, 0.25, -1.0]]
    allowed = rng.random(n) < 0.8
    built = R.process_queries(build_ref(st, dtype, ex, w), metric)
    for k in (1, 10):
        s, r = examples_ref(st, dtype, ex, k, w, None, allowed, metric)
        ks, kr = examples_ref(st, dtype, ex, k, w, None, allowed, metric, keep=True)
        for b in range(3):
            ok = allowed.copy()
            fs, fr = R.search(st, dtype, built[b:b + 1], k, ok, metric=metric)
            assert_same((ks[b:b + 1], kr[b:b + 1]), (fs.astype(np.float32), fr))
            ok[ex[b]] = False
            fs, fr = R.search(st, dtype, built[b:b + 1], k, ok, metric=metric)
            assert_same((s[b:b + 1], r[b:b + 1]), (fs.astype(np.float32), fr))
            assert not np.isin(r[b], ex[b]).any()
    s, r = examples_ref(st[:3], dtype, [[0, 1]], 4, metric=metric)  # fewer rows than k: padding
    assert r.tolist() == [[2, -1, -1, -1]] and np.isneginf(s[0, 1:]).all()
    with pytest.raises(AssertionError):
        assert_same((s, r), (s, r + 1))


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_index_build_queries", "hr_index_build_queries_device", "hr_index_search_examples",
       "hr_index_search_examples_device"]


def test_new_symbols_are_declared_exported_and_validate():
    from hiprag import _native

    text = open(os.path.join(REPO, "include", "hiprag.h")).read()
    assert set(NEW) <= set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))
    assert "#define HR_EX_MAX 32" in text and re.search(r"HR_EX_KEEP\s*=\s*1", text)
    assert _native.HR_EX_MAX == 32 and _native.HR_EX_KEEP == 1
    assert set(NEW) <= set(_native.EXPORTS)
    for m in ("build_queries", "build_queries_device", "search_examples", "search_examples_device"):
        assert callable(getattr(_native.NativeIndex, m))
    assert "hr_examples.hip" in open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert os.path.exists(_native.LIB_PATH), "libhiprag.so not built (run __graft_entry__.build())"
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in NEW:
        assert hasattr(L, name)
    # no handle, no device needed: every entry point refuses a null handle with HR_E_INVALID
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.hr_index_build_queries(None, p, p, p, 1, None, p) == -1
    assert b"null" in L.hr_last_error()
    assert L.hr_index_build_queries_device(None, p, p, p, 1, None, p, None) == -1
    assert L.hr_index_search_examples(None, None, p, p, p, 1, 1, 0, None, p, p) == -1
    assert L.hr_index_search_examples_device(None, None, p, p, p, 1, 1, 0, None, p, p, None) == -1


def test_default_weights_are_float64_reciprocals_cast_once():
    from hiprag import _native

    rows, w, off = _native.NativeIndex._example_lists([[4, 5, 6], [], [9]], None)
    assert rows.tolist() == [4, 5, 6, 9] and off.tolist() == [0, 3, 3, 4]
    assert_same_bits(w, np.asarray([1 / 3] * 3 + [1.0], np.float64).astype(np.float32))
    rows, w, off = _native.NativeIndex._example_lists([[1, 2]], [[0.5, -2.0]])
    assert w.tolist() == [0.5, -2.0] and w.dtype == np.float32 and rows.dtype == np.int64 and off.dtype == np.int64
    with pytest.raises(ValueError):
        _native.NativeIndex._example_lists([[1, 2]], [[0.5]])


# ---------------------------------------------------------------- the store
def make_store(tmp_path, index=ExamplesOracleIndex, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"))


def cluster_chunks(n=120, seed=1, dim=16):
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((3, dim)).astype(np.float32))
    x = _unit(centres[np.arange(n) % 3] + 0.3 * _unit(rng.standard_normal((n, dim)).astype(np.float32)))
    return [Chunk(id=f"c{i}", document_id=f"d{i % 3}", content=f"t{i}", chunk_index=i, metadata={"part": i % 5},
                  embedding=x[i].tolist()) for i in range(n)], x, centres


def want(store, ex, w, k, q=None, allowed=None):
    idx = store._index
    live = idx.live if allowed is None else idx.live & allowed
    s, r = examples_ref(idx.rows, "f32", ex, k, w, q, live)
    return [[(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0] for b in range(len(ex))]


def ids(res):
    return [[(c.id, s) for c, s in hits] for hits in res]


def f32(v):
    return np.float32(v)


def test_store_weights_and_negatives(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    res = s.search_similar_batch([["c0", "c3", "c6"], "c1"], top_k=5)
    third = f32(np.float64(1.0) / 3)
    assert s._index.example_calls == [([[0, 3, 6], [1]], [[third] * 3, [f32(1.0)]], 5, False, False, False)]
    assert ids(res) == want(s, [[0, 3, 6], [1]], [[third] * 3, [1.0]], 5)
    assert not {"c0", "c3", "c6"} & {c.id for c, _ in res[0]} and "c1" not in {c.id for c, _ in res[1]}
    assert all(c.metadata["document_id"] == "d0" for c, _ in res[0])  # its own cluster
    # negatives: -neg_weight / |N| each, float64 then fp32, after the positives; a base vector on top
    res = s.search_similar_batch([["c0", "c3"]], [["c1", "c4", "c7"]], 4, query_embeddings=centres[:1], pos_weight=2.0,
                                 neg_weight=0.5)
    ex, w, k, has_q, masked, keep = s._index.example_calls[-1]
    assert ex == [[0, 3, 1, 4, 7]] and (k, has_q, masked, keep) == (4, True, False, False)
    nw = f32(-np.float64(0.5) / 3)
    assert_same_bits(w[0], [f32(1.0), f32(1.0), nw, nw, nw])
    assert ids(res) == want(s, ex, w, 4, centres[:1])
    assert not {"c0", "c3", "c1", "c4", "c7"} & {c.id for c, _ in res[0]}
    # a base vector alone is the plain search
    res = s.search_similar_batch([[]], top_k=3, query_embeddings=centres[1:2])
    assert ids(res) == ids(s.search_batch(centres[1:2], 3))
    # top_k beyond the live rows, and 0
    assert len(s.search_similar_batch(["c0"], top_k=500)[0]) == 119
    assert s.search_similar_batch(["c0"], top_k=0) == [[]]


def test_store_errors_fail_alone(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks(40)
    assert s.search_similar_batch([[]], query_embeddings=centres[:1]) == [[]]  # nothing stored: no index yet
    run(s.add_chunks(chunks))
    with pytest.raises(ValueError, match="'nope'"):
        s.search_similar_batch([["c0"], ["c1", "nope"]])
    with pytest.raises(ValueError, match="'nope'"):
        run(s.search_similar("c0", negative_ids=["nope"]))
    with pytest.raises(ValueError, match="at most 32"):
        s.search_similar_batch([[f"c{i}" for i in range(20)]], [[f"c{i}" for i in range(20, 33)]])
    with pytest.raises(ValueError, match="needs a query embedding"):
        s.search_similar_batch([[]])
    with pytest.raises(ValueError, match="dim"):
        s.search_similar_batch(["c0"], query_embeddings=[[0.0] * 17])
    with pytest.raises(ValueError, match="filters"):
        s.search_similar_batch(["c0"], filters=[None, None])
    with pytest.raises(ValueError, match="negative lists"):
        s.search_similar_batch(["c0"], [["c1"], ["c2"]])
    with pytest.raises(ValueError, match="finite"):
        s.search_similar_batch(["c0"], pos_weight=float("nan"))
    assert s._index.example_calls == []  # every limit is checked before any native call
    run(s.delete(["c5"]))
    with pytest.raises(ValueError, match="'c5'"):  # a deleted chunk is unknown
        s.search_similar_batch(["c5"])
    assert len(s.search_similar_batch(["c0"], top_k=3)[0]) == 3


def test_store_filters_and_the_async_form(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    part = np.arange(len(chunks)) % 5
    res = s.search_similar_batch(["c0", "c2"], top_k=6, filters={"part": 1})
    assert s._index.example_calls[-1][4] is True
    assert ids(res) == want(s, [[0], [2]], [[1.0], [1.0]], 6, allowed=part == 1)
    # a filter that forbids the example itself: it still steers the query
    assert part[0] != 1 and all(c.metadata["part"] == 1 for c, _ in res[0])
    # one clause (or None) per query: one call per distinct clause, scattered back in query order
    flt = [{"part": 1}, None, {"part": 1}]
    del s._index.example_calls[:]
    before = s.grouped_launches
    res = s.search_similar_batch(["c0", "c1", "c2"], top_k=4, filters=flt)
    assert sorted((len(c[0]), c[4]) for c in s._index.example_calls) == [(1, False), (2, True)]
    assert s.grouped_launches - before == 2
    for i, f in enumerate(flt):
        assert ids([res[i]]) == want(s, [[i]], [[1.0]], 4, allowed=None if f is None else part == 1)
    one = run(s.search_similar(["c0", "c3"], 5, {"part": 2}, negative_ids="c1", query_embedding=centres[0].tolist()))
    ex, w, k, has_q, masked, keep = s._index.example_calls[-1]
    assert (ex, k, has_q, masked) == ([[0, 3, 1]], 5, True, True)
    assert_same_bits(w[0], [f32(0.5), f32(0.5), f32(-1.0)])
    assert ids([one]) == want(s, ex, w, 5, centres[:1], part == 2)
    assert ids([run(s.search_similar("c7", 3))]) == want(s, [[7]], [[1.0]], 3)


def test_host_composition_gives_the_native_bits(tmp_path):
    """An index without search_examples (several devices, IVF_FLAT, a plain fake): get_rows, the same float64
    accumulation, search at k + M, drop -- the same rows and score bits as the native-shaped route."""
    a = make_store(tmp_path / "a")
    b = make_store(tmp_path / "b", index=OracleIndex)
    chunks, x, centres = cluster_chunks()
    run(a.add_chunks(chunks))
    run(b.add_chunks(chunks))
    assert not hasattr(b._index, "search_examples")
    calls = [dict(positive_ids=[["c0", "c3", "c6"], "c1", ["c2", "c2"]], top_k=7),
             dict(positive_ids=[["c0"], []], negative_ids=[["c1", "c4"], ["c9"]], top_k=5, query_embeddings=centres[:2],
                  pos_weight=0.7, neg_weight=1.3),
             dict(positive_ids=["c0", "c1", "c2"], top_k=4, filters=[{"part": 1}, None, {"part": 1}]),
             dict(positive_ids=[["c0"]], negative_ids=[["c0"]], top_k=6),  # w x - w x: the zero query
             dict(positive_ids=["c0"], top_k=119), dict(positive_ids=["c0"], top_k=500)]
    for kw in calls:
        got, ref = b.search_similar_batch(**kw), a.search_similar_batch(**kw)
        assert ids(got) == ids(ref) and all(len(h) for h in got)
    zero = a.search_similar_batch([["c0"]], [["c0"]], top_k=6)[0]  # scores 0 everywhere: rows ascending, c0 excluded
    assert [c.id for c, _ in zero] == ["c1", "c2", "c3", "c4", "c5", "c6"] and all(sc == 0.0 for _, sc in zero)
    assert ids([run(b.search_similar("c7", 3))]) == ids([run(a.search_similar("c7", 3))])
    # a multi-device native index takes the host route too
    a._index.devices = [0, 1]
    n_calls = len(a._index.example_calls)
    assert ids(a.search_similar_batch(**calls[1])) == ids(b.search_similar_batch(**calls[1]))
    assert len(a._index.example_calls) == n_calls
    # the pieces, directly
    idx = a._index
    ex, w = [[0, 3], [5]], [[f32(0.5), f32(-0.25)], [f32(1.0)]]
    assert_same_bits(build_queries_host(idx, ex, w, centres[:2]), idx.build_queries(ex, w, centres[:2]))
    assert_same(search_examples_host(idx, ex, 5, w, keep=True), idx.search_examples(ex, 5, w, keep=True))


# ---------------------------------------------------------------- the retriever
class Emb:
    def __init__(self, v):
        self.v, self.asked = v, []

    async def embed_query(self, q):
        self.asked.append(q)
        return self.v


class Reverse:
    async def rerank(self, query, results, top_k=None):
        return list(reversed(results))


def test_retrieve_similar(tmp_path):
    s = make_store(tmp_path)
    chunks, x, centres = cluster_chunks()
    run(s.add_chunks(chunks))
    emb = Emb(centres[0].tolist())
    ret = VectorRetriever(s, emb, RetrieverConfig(top_k=4, similarity_threshold=0.0))
    res = run(ret.retrieve_similar("c0"))
    w = want(s, [[0]], [[1.0]], 4)[0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    assert emb.asked == []  # no query, nothing embedded
    res = run(ret.retrieve_similar(["c0", "c3"], top_k=6, filters={"part": 1}, negative_ids=["c1"], query="what"))
    assert emb.asked == ["what"]
    ex, wts, k, has_q, masked, keep = s._index.example_calls[-1]
    assert (ex, k, has_q, masked) == ([[0, 3, 1]], 6, True, True)
    w = want(s, ex, wts, 6, centres[:1], np.arange(120) % 5 == 1)[0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    # the threshold cuts after the ranks are taken, as in retrieve()
    full = want(s, [[0]], [[1.0]], 10)[0]
    th = (full[3][1] + full[4][1]) / 2
    assert full[3][1] > th > full[4][1]
    cut = VectorRetriever(s, emb, RetrieverConfig(top_k=10, similarity_threshold=th))
    res = run(cut.retrieve_similar("c0"))
    assert [(r.chunk.id, r.rank) for r in res] == [(cid, i + 1) for i, (cid, _) in enumerate(full[:4])]
    # a reranker ranks against a text: it applies with a query (2 top_k fetched), not without one
    rr = VectorRetriever(s, emb, RetrieverConfig(top_k=3, similarity_threshold=0.0), reranker=Reverse())
    assert [r.rank for r in run(rr.retrieve_similar("c0"))] == [1, 2, 3]
    assert [r.rank for r in run(rr.retrieve_similar("c0", query="what"))] == [6, 5, 4]
    assert s._index.example_calls[-1][2] == 6

    class NoSimilar:
        async def search(self, *a, **kw):
            return []

    with pytest.raises(NotImplementedError):
        run(VectorRetriever(NoSimilar(), emb, RetrieverConfig()).retrieve_similar("c0"))
