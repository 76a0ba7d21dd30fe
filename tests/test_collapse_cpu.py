"""CPU: collapsed search above the kernels -- the reference itself (tests/collapse_ref.py) on hand-written cases, the
store's wiring (lazy group column, collapse_field with its document_id fallback, (type, value) keys, growth, deletes,
clear, reload, the micro-batcher, every error case) over a numpy-backed stand-in index, the retrievers' kwargs over
stub stores, kb_file_search with and without collapse_files, and the new symbols in the header and EXPORTS."""
import asyncio
import json
import os
import re

import numpy as np
import pytest

from collapse_ref import assert_same, collapse_ref, dedup
from conftest import REPO
from fake_index import AsyncOracleIndex, OracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag import kb_tools as K
from hiprag.rag.base import RetrievalResult
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.retriever import BatchedVectorRetriever, HybridRetriever, VectorRetriever
from oracle import ref_numpy as R


def run(coro):
    return asyncio.run(coro)


# ---------------------------------------------------------------- the reference
def test_dedup_by_first_occurrence():
    groups = [0, 1, 0, -1, 2, 1]
    s, r = dedup([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], [2, 3, 0, 5, 1, 4], groups, 4)
    assert r.tolist() == [2, 5, 4, -1]  # row 3 has no group; rows 0, 1 repeat groups 0, 1
    assert s[:3].tolist() == [np.float32(0.9), np.float32(0.6), np.float32(0.4)] and np.isneginf(s[3])
    s, r = dedup([0.9, 0.8, -np.inf], [7, 0, -1], groups, 2)  # row 7 lies beyond the ids: no group
    assert r.tolist() == [0, -1]
    assert dedup([0.5, 0.5], [0, 2], groups, 1)[1].tolist() == [0]


@pytest.mark.parametrize("use_c", [True, False])
def test_collapse_ref_hand_cases(use_c):
    x = np.zeros((6, 8), np.float32)
    x[:, 0] = [0.9, 0.8, 0.8, 0.7, 0.6, 0.5]
    q = np.zeros((1, 8), np.float32)
    q[0, 0] = 1.0
    st = R.process_rows(x, "ip", "f32")
    groups = np.asarray([0, 1, 2, 0, 1, 3])
    s, r = collapse_ref(st, "f32", q, groups, 5, metric="ip", use_c=use_c)
    assert r.tolist() == [[0, 1, 2, 5, -1]]  # equal scores in different groups: the lower row first
    assert s[0, :4].tolist() == [np.float32(v) for v in (0.9, 0.8, 0.8, 0.5)]
    allowed = np.asarray([False, True, True, True, True, True])  # the best row of group 0 hidden: row 3 stands in
    assert collapse_ref(st, "f32", q, groups, 2, allowed, "ip", use_c)[1].tolist() == [[1, 2]]
    assert collapse_ref(st, "f32", q, groups, 4, allowed, "ip", use_c)[1].tolist() == [[1, 2, 3, 5]]
    assert collapse_ref(st, "f32", q, np.zeros(6, int), 3, metric="ip", use_c=use_c)[1].tolist() == [[0, -1, -1]]
    every = collapse_ref(st, "f32", q, np.arange(6), 6, metric="ip", use_c=use_c)
    assert every[1].tolist() == [[0, 1, 2, 3, 4, 5]]  # singleton groups: the plain ranking
    assert collapse_ref(st, "f32", q, groups[:2], 3, metric="ip", use_c=use_c)[1].tolist() == [[0, 1, -1]]


# ---------------------------------------------------------------- a stand-in index with a group column
class CollapseIndex(OracleIndex):
    """OracleIndex + the group column and the collapsed search of NativeIndex, computed by the reference."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.groups = np.zeros(0, np.int32)
        self.set_calls, self.collapsed = [], 0

    def set_groups(self, row0, groups):
        g = np.asarray(groups, np.int32).reshape(-1)
        if (g < -1).any() or row0 < 0 or row0 + len(g) > len(self.rows):
            raise ValueError("bad group ids or rows")
        if len(self.groups) < row0 + len(g):
            self.groups = np.concatenate([self.groups, np.full(row0 + len(g) - len(self.groups), -1, np.int32)])
        self.groups[row0:row0 + len(g)] = g
        self.set_calls.append((int(row0), len(g)))

    def search_collapsed(self, q, k, mask=None, probe=0):
        self.collapsed += 1
        allowed = self.live.copy()
        if mask is not None:
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        return collapse_ref(self.rows, self.dtype, R.process_queries(np.atleast_2d(q), self.metric), self.groups, k,
                            allowed, self.metric)


def make_store(tmp_path, index=CollapseIndex, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": True, "fsync": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"),
                          index_loader=lambda path, dim, dt, metric: _load(index, path))


def _load(cls, path):
    base = OracleIndex.load(path)
    idx = cls(base.dim, base.dtype, base.metric)
    idx.rows, idx.live = base.rows, base.live
    return idx


def doc_chunks(doc, n, seed, dim=16, source="default", start=0):
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(dim)
    out = []
    for i in range(start, start + n):
        meta = {"index_type": "index_summary"}
        if source == "default":
            meta["source"] = f"{doc}.pdf"
        elif source is not None:
            meta["source"] = source
        v = centre + 0.3 * rng.standard_normal(dim)
        out.append(Chunk(id=f"{doc}_{i}", document_id=doc, content=f"{doc} {i}", chunk_index=i, metadata=meta,
                         embedding=v.astype(np.float32).tolist()))
    return out


def host_dedup(store, q, k, key, filters=None):
    hits = store.search_batch([q], store.count_sync(), filters)[0]
    seen, out = set(), []
    for c, s in hits:
        if key(c) in seen:
            continue
        seen.add(key(c))
        out.append((c.id, s))
    return out[:k]


def ids(hits):
    return [(c.id, s) for c, s in hits]


def by_doc(c):
    return c.document_id


def by_source(c):
    v = c.metadata.get("source", c.document_id)
    return type(v), v  # (a bare set would merge 1, 1.0 and True)


def test_store_builds_the_column_lazily_and_extends_it(tmp_path):
    s = make_store(tmp_path)
    run(s.add_chunks(doc_chunks("a", 30, 1) + doc_chunks("b", 3, 2) + doc_chunks("c", 4, 3)))
    q = doc_chunks("a", 1, 1)[0].embedding
    plain = run(s.search(q, 3))
    assert {c.document_id for c, _ in plain} == {"a"} and s._group_ids is None and s._index.set_calls == []
    got = s.search_batch([q], 3, collapse=True)[0]
    assert ids(got) == host_dedup(s, q, 3, by_doc) and [c.document_id for c, _ in got][0] == "a"
    assert len({c.document_id for c, _ in got}) == 3
    assert s._index.set_calls == [(0, 37)] and len(s._group_ids) == 3
    s.search_batch([q], 2, collapse=True)
    assert s._index.set_calls == [(0, 37)]  # nothing new to upload
    run(s.add_chunks(doc_chunks("d", 5, 4) + doc_chunks("a", 2, 5, start=30)))  # _append_tables extends the column
    assert s._group_rows == 44 and s._group_sent == 37 and s._group_col[37:44].tolist() == [3] * 5 + [0] * 2
    got = s.search_batch([q], 10, collapse=True)[0]
    assert s._index.set_calls == [(0, 37), (37, 7)] and ids(got) == host_dedup(s, q, 10, by_doc) and len(got) == 4
    # deletes: the best row's group is represented by its next row; a deleted document leaves the result
    best = got[0][0].id
    run(s.delete([best]))
    got = s.search_batch([q], 10, collapse=True)[0]
    assert got[0][0].document_id == "a" and got[0][0].id != best and ids(got) == host_dedup(s, q, 10, by_doc)
    assert run(s.delete_by_document_id("a")) == 31
    got = s.search_batch([q], 10, collapse=True)[0]
    assert sorted(c.document_id for c, _ in got) == ["b", "c", "d"]
    # k = min(top_k, n_live): the index is asked for no more than the live rows
    assert len(s.search_batch([q], 100, collapse=True)[0]) == 3
    # clear drops the tables; a new collection starts from nothing
    run(s.clear())
    assert s._group_ids is None and s._group_rows == s._group_sent == 0
    assert s.search_batch([q], 3, collapse=True) == [[]]
    run(s.add_chunks(doc_chunks("z", 2, 9)))
    assert [c.document_id for c, _ in s.search_batch([q], 3, collapse=True)[0]] == ["z"]
    assert s._index.set_calls == [(0, 2)]


def test_collapse_field_with_document_id_fallback_and_typed_keys(tmp_path):
    s = make_store(tmp_path, collapse_field="source")
    assert s.collapse_field == "source" and make_store(tmp_path / "x").collapse_field == "document_id"
    cs = (doc_chunks("a", 6, 1, source="shared.pdf") + doc_chunks("b", 3, 1, source="shared.pdf")  # one file, two docs
          + doc_chunks("c", 4, 3, source=None)            # no source: grouped by document_id
          + doc_chunks("d", 2, 4, source=1) + doc_chunks("e", 2, 4, source=1.0) + doc_chunks("f", 2, 4, source=True)
          + doc_chunks("g", 2, 6, source="c"))            # a source equal to another row's document_id: one group
    run(s.add_chunks(cs))
    q = cs[0].embedding
    got = s.search_batch([q], 20, collapse=True)[0]
    assert ids(got) == host_dedup(s, q, 20, by_source)
    col = s._group_col[: s._group_rows].tolist()
    assert col[:9] == [0] * 9 and col[9:13] == [1] * 4
    assert col[13:19] == [2, 2, 3, 3, 4, 4]  # 1, 1.0 and True stay apart
    assert col[19:21] == [1, 1]
    assert set(s._group_ids) == {(str, "shared.pdf"), (str, "c"), (int, 1), (float, 1.0), (bool, True)}
    # python's own dict would merge 1, 1.0 and True: the host loop of kb_file_search does; the typed keys do not
    assert len(got) == 5
    # a filter applies inside the collapsed search
    flt = {"source": {"$ne": "shared.pdf"}}
    assert ids(s.search_batch([q], 20, flt, collapse=True)[0]) == host_dedup(s, q, 20, by_source, flt)


def test_reload_rebuilds_the_ids_from_the_tables(tmp_path):
    s = make_store(tmp_path)
    run(s.add_chunks(doc_chunks("a", 5, 1) + doc_chunks("b", 3, 2)))
    q = doc_chunks("b", 1, 2)[0].embedding
    want = ids(s.search_batch([q], 2, collapse=True)[0])
    run(s.add_chunks(doc_chunks("c", 2, 3)))  # journalled after the first snapshot
    run(s.delete(["a_0"]))
    s.close()
    assert not any("group" in f for f in os.listdir(tmp_path))  # nothing of the column is persisted
    s2 = make_store(tmp_path)
    assert s2.count_sync() == 9 and s2._group_ids is None and s2._index.set_calls == []
    got = s2.search_batch([q], 3, collapse=True)[0]
    assert ids(got)[:2] == want and ids(got) == host_dedup(s2, q, 3, by_doc)
    assert s2._index.set_calls == [(0, 10)] and s2._group_col[0] == -1  # the deleted row has no group


def test_batcher_keeps_collapsed_and_plain_queries_apart(tmp_path):
    class Idx(CollapseIndex, AsyncOracleIndex):
        pass

    s = make_store(tmp_path, index=Idx)
    run(s.add_chunks(doc_chunks("a", 20, 1) + doc_chunks("b", 5, 2) + doc_chunks("c", 5, 3)))
    q = doc_chunks("a", 1, 1)[0].embedding

    async def both():
        return await asyncio.gather(*[s.search(q, 3, collapse=bool(i % 2)) for i in range(8)])

    before, launches, native = s._index.collapsed, s._batcher.launches, s._batcher.native_launches
    res = run(both())
    assert s._index.collapsed - before == 1 and s._batcher.launches - launches == 2
    assert s._batcher.native_launches - native == 1  # the plain batch went through the asynchronous entry point
    for i, r in enumerate(res):
        docs = [c.document_id for c, _ in r]
        assert docs == (["a", "b", "c"] if i % 2 else ["a", "a", "a"]) or (i % 2 and sorted(docs) == ["a", "b", "c"])
    # a filter splits collapsed queries too
    async def filtered():
        return await asyncio.gather(s.search(q, 2, collapse=True),
                                    s.search(q, 2, {"document_id": {"$ne": "a"}}, collapse=True))

    before = s._index.collapsed
    r0, r1 = run(filtered())
    assert s._index.collapsed - before == 2 and "a" not in [c.document_id for c, _ in r1]


def test_store_error_cases(tmp_path):
    s = make_store(tmp_path)
    run(s.add_chunks(doc_chunks("a", 5, 1)))
    q = doc_chunks("a", 1, 1)[0].embedding
    with pytest.raises(ValueError, match="128"):
        s.search_batch([q], 129, collapse=True)
    with pytest.raises(ValueError, match="128"):
        run(s.search(q, 129, collapse=True))
    assert len(s.search_batch([q], 128, collapse=True)[0]) == 1
    assert run(s.search(q, 0, collapse=True)) == []
    with pytest.raises(TypeError):
        s.search_batch([q], 3, None, True)  # keyword-only
    s._index.devices = [0, 1]
    with pytest.raises(ValueError, match="single-device"):
        s.search_batch([q], 3, collapse=True)
    plain = make_store(tmp_path / "plain", index=OracleIndex)
    run(plain.add_chunks(doc_chunks("a", 5, 1)))
    with pytest.raises(NotImplementedError):
        plain.search_batch([q], 3, collapse=True)
    assert len(plain.search_batch([q], 3)[0]) == 3  # off: today's path, for any index object
    with pytest.raises(NotImplementedError):
        run(plain.search(q, 3, collapse=True))  # the waiter sees the worker's error


# ---------------------------------------------------------------- retrievers
class StubStore:
    """Records what the retriever asks for; returns `n` hits per query with falling scores."""

    def __init__(self, n=10, accepts_collapse=True):
        self.calls, self.n, self.accepts = [], n, accepts_collapse

    def _hits(self, top_k):
        return [(Chunk(id=f"c{i}", document_id=f"d{i}", content=f"t{i}", chunk_index=0, metadata={}),
                 1.0 - 0.1 * i) for i in range(min(self.n, top_k))]

    async def search(self, query_embedding, top_k=5, filters=None, **kw):
        if kw and not self.accepts:
            raise TypeError(f"unexpected {kw}")
        self.calls.append(("search", top_k, filters, kw))
        return self._hits(top_k)

    def search_batch(self, qvs, top_k=5, filters=None, **kw):
        self.calls.append(("search_batch", top_k, filters, kw))
        return [self._hits(top_k) for _ in qvs]


class Emb:
    async def embed_query(self, q):
        return [0.0, 1.0]


class HalfReranker:
    async def rerank(self, query, results, top_k=None):
        return [RetrievalResult(chunk=r.chunk, score=-r.score, rank=i + 1) for i, r in enumerate(reversed(results))]


def test_vector_retriever_passes_collapse():
    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=4))
    res = run(ret.retrieve("q", collapse=True, similarity_threshold=0.85, filters={"a": 1}))
    assert st.calls == [("search", 4, {"a": 1}, {"collapse": True})]
    assert [(r.chunk.id, r.rank) for r in res] == [("c0", 1), ("c1", 2)]  # threshold and ranks on the collapsed list
    run(ret.retrieve("q"))
    run(ret.retrieve("q", collapse=False))
    assert st.calls[1:] == [("search", 4, None, {}), ("search", 4, None, {})]  # off: the reference's call
    old = StubStore(accepts_collapse=False)  # a store that never heard of the flag keeps working while it is off
    assert len(run(VectorRetriever(old, Emb(), RetrieverConfig(top_k=3)).retrieve("q"))) == 3
    rr = VectorRetriever(StubStore(), Emb(), RetrieverConfig(top_k=3, similarity_threshold=0.0),
                         reranker=HalfReranker())
    res = run(rr.retrieve("q", collapse=True))
    assert rr.vector_store.calls == [("search", 6, None, {"collapse": True})]  # 2 * top_k under a reranker
    assert [r.chunk.id for r in res] == ["c5", "c4", "c3"]


def test_batched_retriever_passes_collapse():
    st = StubStore()
    ret = BatchedVectorRetriever(st, Emb(), RetrieverConfig(top_k=2))
    res = run(ret.batch_retrieve(["a", "b"], collapse=True))
    assert st.calls == [("search_batch", 2, None, {"collapse": True})] and [len(r) for r in res] == [2, 2]
    run(ret.batch_retrieve(["a"]))
    assert st.calls[1] == ("search_batch", 2, None, {})


def test_collapse_skips_the_fused_path():
    class FusedStub:
        def __init__(self):
            self.submitted = 0

        def submit(self, query, top_k, threshold):
            self.submitted += 1
            f = asyncio.get_running_loop().create_future()
            f.set_result([])
            return f

    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=2))
    ret._fused = FusedStub()
    assert run(ret.retrieve("q")) == [] and ret._fused.submitted == 1 and st.calls == []
    assert len(run(ret.retrieve("q", collapse=True))) == 2 and ret._fused.submitted == 1
    assert st.calls == [("search", 2, None, {"collapse": True})]


def test_hybrid_retriever_refuses_collapse_with_keyword_search():
    class LexStore(StubStore):
        lexical = True

        def keyword_search_batch(self, queries, top_k=5, filters=None):
            return [[] for _ in queries]

    hy = HybridRetriever(LexStore(), Emb(), RetrieverConfig(top_k=2))
    with pytest.raises(ValueError, match="collapse"):
        run(hy.retrieve("q", collapse=True))
    with pytest.raises(ValueError, match="collapse"):
        run(hy.batch_retrieve(["q"], collapse=True))
    assert len(run(hy.retrieve("q"))) == 2
    plain = HybridRetriever(StubStore(), Emb(), RetrieverConfig(top_k=2))  # no keyword search: the delegation
    assert len(run(plain.retrieve("q", collapse=True))) == 2
    assert plain.vector_store.calls[-1][3] == {"collapse": True}


# ---------------------------------------------------------------- kb_file_search
def _toolkit(tmp_path, monkeypatch, collapse, chunks, qv):
    def no_reranker(backend):
        raise RuntimeError("no reranker")

    monkeypatch.setattr(K, "_reranker_from", no_reranker)
    made = []

    def factory(cfg):
        made.append(cfg)
        cfg = cfg.model_copy(update={"persist_directory": str(tmp_path / f"c{int(collapse)}"),
                                     "index_params": {**cfg.index_params, "dtype": "f32", "persist": False}})
        return HipVectorStore(cfg, index_factory=lambda d: CollapseIndex(d, "f32"))

    conf = {"collapse_files": True} if collapse else {}
    tk = K.KBSearchToolkit(config=conf, kb_resolver=lambda kb: ("coll", "KB"), store_factory=factory)

    class E:
        async def embed_query(self, q):
            return qv

    tk._embedder_cache = E()
    store = tk._get_or_create_vector_store("coll", "./rag_data/vector_store")
    run(store.add_chunks(chunks))
    return tk, store, made


def test_kb_file_search_with_and_without_collapse_files(tmp_path, monkeypatch):
    chunks = (doc_chunks("big", 40, 1, source=None) + doc_chunks("b", 3, 2) + doc_chunks("c", 2, 3)
              + doc_chunks("d", 2, 4) + doc_chunks("e", 1, 5))
    qv = chunks[0].embedding
    out = {}
    for collapse in (False, True):
        tk, store, made = _toolkit(tmp_path, monkeypatch, collapse, chunks, qv)
        assert tk.collapse_files is collapse
        assert made[0].index_params.get("collapse_field") == ("source" if collapse else None)
        assert store.collapse_field == ("source" if collapse else "document_id")
        out[collapse] = json.loads(run(tk.kb_file_search(1, "q", top_k=4, auto_rerank=False)))
        assert store._index.collapsed == (1 if collapse else 0)
        # kb_embedding_search shares the store and stays a plain chunk search
        emb = json.loads(run(tk.kb_embedding_search(1, "q", top_k=4, auto_rerank=False)))
        assert {r["document_id"] for r in emb["results"]} == {"big"}
        assert store._index.collapsed == (1 if collapse else 0)
    assert out[False]["total_files"] == 1 and [f["file_name"] for f in out[False]["files"]] == ["big"]
    assert out[True]["total_files"] == 4 and out[True]["files"][0] == out[False]["files"][0]
    names = [f["file_name"] for f in out[True]["files"]]
    assert names[0] == "big" and len(set(names)) == 4 and set(names) <= {"big", "b.pdf", "c.pdf", "d.pdf", "e.pdf"}
    scores = [f["embedding_score"] for f in out[True]["files"]]
    assert scores == sorted(scores, reverse=True) and [f["rank"] for f in out[True]["files"]] == [1, 2, 3, 4]
    assert {k for k in out[True]} == {k for k in out[False]}  # the same JSON shape


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_index_set_groups", "hr_index_search_collapsed", "hr_index_search_collapsed_device"]
NEW_DIAG = ["hr_index_collapse_stats"]


def test_new_symbols_are_declared_and_exported():
    from hiprag import _native

    def decls(name):
        text = open(os.path.join(REPO, "include", name)).read()
        return set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))

    assert set(NEW) <= decls("hiprag.h") and set(NEW_DIAG) <= decls("hiprag_diag.h")
    assert set(NEW + NEW_DIAG) <= set(_native.EXPORTS)
    for m in ("set_groups", "search_collapsed", "search_collapsed_device", "collapse_stats"):
        assert callable(getattr(_native.NativeIndex, m))
    src = open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert "hr_collapse.hip" in src
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libhiprag.so not built (run __graft_entry__.build())")
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in NEW + NEW_DIAG:
        assert hasattr(L, name)
