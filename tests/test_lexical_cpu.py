"""CPU: the host half of the keyword (BM25) search -- the analyzer's two paths, hr_lex_pack against the reference
packing (tests/lex_ref.py), the reciprocal-rank fusion of HybridRetriever over stub stores, the store's wiring of
the lexical index (a reference-backed stand-in for the device index), and the ABI.  Every comparison is exact."""
import asyncio
import zlib

import numpy as np
import pytest

import lex_ref
from hash_embed import HashEmbedder
from hiprag import _native
from hiprag.rag import (BatchedVectorRetriever, Chunk, HipVectorStore, HybridRetriever, RetrieverConfig,
                        VectorStoreConfig)
from hiprag.rag import lexical as LX


def run(coro):
    return asyncio.run(coro)


# ---------------------------------------------------------------- analyzer
MIXED = ["Error E1234: connection_reset (code=0x1F)!", "", "   \t\n ", "The quick brown fox; the QUICK fox.",
         "a_b c-d e.f 42", "tabs\tand\x1cseparators\x1fhere", "part no. XK-77/B rev.2", "x"]


def test_native_and_python_paths_agree_on_mixed_texts():
    ids_n, off_n = LX.analyze_batch(MIXED, native=True)
    ids_p, off_p = LX.analyze_batch(MIXED, native=False)
    assert ids_n.dtype == ids_p.dtype == np.uint32
    assert np.array_equal(off_n, off_p) and np.array_equal(ids_n, ids_p)
    for i, t in enumerate(MIXED):  # and both are the reference analyzer
        assert ids_n[off_n[i]:off_n[i + 1]].tolist() == lex_ref.analyze(t)
    assert int(ids_n.max()) < 1 << 22


def test_cjk_one_token_per_ideograph_and_empty_texts():
    ids, off = LX.analyze_batch(["知识库检索", "GPU 检索 v2", "", " \n"])
    assert np.diff(off).tolist() == [5, 4, 0, 0]
    assert ids[:5].tolist() == [zlib.crc32(c.encode("utf-8")) % (1 << 22) for c in "知识库检索"]
    assert ids[5:9].tolist() == [zlib.crc32(t.encode("utf-8")) % (1 << 22) for t in ("gpu", "检", "索", "v2")]
    assert lex_ref.analyze("知识库检索") == ids[:5].tolist()
    ids, off = LX.analyze_batch(["", "  "])  # (an ASCII batch: the native path)
    assert len(ids) == 0 and off.tolist() == [0, 0, 0]


# ---------------------------------------------------------------- packing
def _colliding_pair():
    seen = {}
    for i in range(1 << 20):
        w = f"w{i}"
        t = zlib.crc32(w.encode()) % (1 << 22)
        if t in seen:
            return seen[t], w
        seen[t] = w
    raise AssertionError("no 22-bit collision found")


def test_pack_equals_reference():
    a, b = _colliding_pair()
    assert a != b and lex_ref.analyze(a) == lex_ref.analyze(b)
    rng = np.random.default_rng(0)
    rows = [
        [],                                                   # an empty row
        [7],                                                  # a single token
        [123456] * 2000,                                      # tf caps at 1023
        lex_ref.analyze(f"{a} {b} {a} other"),                # two words in one 22-bit bucket: one entry, tf 3
        rng.integers(0, 1 << 22, 70000).tolist(),             # dl caps at 65535
        [(1 << 22) - 1, 0, (1 << 22) - 1],                    # the id range's ends
        [],
    ]
    ent, off, dl = _native.lex_pack(rows)
    r_ent, r_off, r_dl = lex_ref.pack(rows)
    assert ent.tolist() == r_ent and off.tolist() == r_off and dl.tolist() == r_dl
    assert dl[2] == 2000 and ent[off[2]] == (123456 << 10) | 1023
    assert dl[4] == 65535
    e3 = ent[off[3]:off[4]]
    assert len(e3) == 2 and sorted(int(x) & 1023 for x in e3) == [1, 3]
    with pytest.raises(ValueError):
        _native.lex_pack([[1 << 22]])


# ---------------------------------------------------------------- fusion
class StubStore:
    """search_batch / keyword_search_batch from fixed rankings of ids; rows = position in `ids`."""

    def __init__(self, ids, dense, lexical):
        self.rows = {c: i for i, c in enumerate(ids)}
        self.dense, self.lex = dense, lexical  # lists of (id, score)
        self.asked = []

    def _hits(self, ranking, k):
        return [(Chunk(id=c, document_id="d", content=c, chunk_index=self.rows[c], metadata={}), s)
                for c, s in ranking[:k]]

    def row_of(self, chunk_id):
        return self.rows.get(chunk_id)

    def search_batch(self, qvs, k, filters=None):
        self.asked.append(("dense", k, filters))
        return [self._hits(self.dense, k) for _ in qvs]

    def keyword_search_batch(self, queries, k, filters=None):
        self.asked.append(("lex", k, filters))
        return [self._hits(self.lex, k) for _ in queries]


def _fused(store, top_k=10, rrf_k=60, fetch_k=None, **kw):
    cfg = RetrieverConfig(top_k=top_k, similarity_threshold=0.0)
    r = HybridRetriever(store, HashEmbedder(), cfg, rrf_k=rrf_k, fetch_k=fetch_k)
    return [(x.chunk.id, x.score, x.rank) for x in run(r.retrieve("q", **kw))]


def test_rrf_disjoint_lists():
    s = StubStore(["a", "b", "c", "d"], [("c", 0.9), ("a", 0.8)], [("d", 3.0), ("b", 1.0)])
    # ranks 1: c (row 2) and d (row 3) tie at 1/61 -> row order; ranks 2: a (row 0), b (row 1)
    assert _fused(s) == [("c", 1.0 / 61.0, 1), ("d", 1.0 / 61.0, 2), ("a", 1.0 / 62.0, 3), ("b", 1.0 / 62.0, 4)]
    assert s.asked == [("dense", 50, None), ("lex", 50, None)]  # fetch_k = min(128, max(4 * 10, 50))


def test_rrf_identical_lists():
    rk = [("b", 0.9), ("a", 0.5), ("c", 0.1)]
    s = StubStore(["a", "b", "c"], rk, rk)
    assert _fused(s) == [("b", 1.0 / 61.0 + 1.0 / 61.0, 1), ("a", 1.0 / 62.0 + 1.0 / 62.0, 2),
                         ("c", 1.0 / 63.0 + 1.0 / 63.0, 3)]
    assert _fused(s, top_k=2, rrf_k=1, fetch_k=7)[:2] == [("b", 0.5 + 0.5, 1), ("a", 1.0 / 3.0 + 1.0 / 3.0, 2)]
    assert s.asked[-2:] == [("dense", 7, None), ("lex", 7, None)]


def test_rrf_tie_resolves_by_row():
    s = StubStore(["a", "b", "c"], [("c", 0.9), ("b", 0.8)], [("b", 2.0), ("c", 1.0)])
    # both hold ranks {1, 2}: equal fused scores, the lower row first
    both = 1.0 / 61.0 + 1.0 / 62.0
    assert _fused(s) == [("b", 1.0 / 62.0 + 1.0 / 61.0, 1), ("c", both, 2)]
    assert 1.0 / 62.0 + 1.0 / 61.0 == both


def test_rrf_threshold_drops_dense_hits_only():
    s = StubStore(["a", "b", "c"], [("a", 0.9), ("b", 0.2), ("c", 0.7)], [("b", 0.01), ("a", 0.001)])
    got = _fused(s, similarity_threshold=0.5, filters={"k": "v"})
    # dense keeps a (rank 1) and c (rank 3: ranks are taken before the threshold); b's dense hit is dropped,
    # its keyword hit (score far below the threshold) stays
    assert got == [("a", 1.0 / 61.0 + 1.0 / 62.0, 1), ("b", 1.0 / 61.0, 2), ("c", 1.0 / 63.0, 3)]
    assert s.asked == [("dense", 50, {"k": "v"}), ("lex", 50, {"k": "v"})]
    r = HybridRetriever(s, HashEmbedder(), RetrieverConfig(top_k=2))
    assert [[x.chunk.id for x in q] for q in run(r.batch_retrieve(["q1", "q2"]))] == [["a", "b"], ["a", "b"]]
    with pytest.raises(ValueError):
        HybridRetriever(s, HashEmbedder(), fusion="weighted")


# ---------------------------------------------------------------- store wiring (no GPU: reference-backed indexes)
class RefLexIndex:
    """LexicalIndex's interface over lex_ref.RefIndex."""

    def __init__(self):
        self.ref = lex_ref.RefIndex()

    def add_texts(self, texts):
        return self.ref.add([lex_ref.analyze(t) for t in texts])

    def remove_rows(self, rows):
        self.ref.remove(rows)

    def search(self, queries, k, mask=None):
        allowed = None
        if mask is not None:
            allowed = [bool((int(mask[r >> 6]) >> (r & 63)) & 1) for r in range(len(self.ref.rows))]
        s, r = self.ref.search([lex_ref.analyze(q) for q in queries], k, allowed)
        return np.array(s, np.float64).reshape(len(queries), k), np.array(r, np.int64).reshape(len(queries), k)

    def close(self):
        pass


def _store(tmp_path, lexical, fake=True):
    from fake_index import OracleIndex

    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": True, "fsync": False, "lexical": lexical})
    return HipVectorStore(cfg, index_factory=lambda dim: OracleIndex(dim, "f32"),
                          index_loader=lambda path, dim, dt, metric: OracleIndex.load(path),
                          lexical_factory=RefLexIndex if fake else None)


DOCS = {"manual": ["reset the pump with code E1234", "the pump manual, chapter two", "valve torque table"],
        "faq": ["why does the pump stop", "error E1234 means overheating", "contact support"]}


def _doc_chunks(doc):
    rng = np.random.default_rng(zlib.crc32(doc.encode()))
    return [Chunk(id=f"{doc}_{i}", document_id=doc, content=t, chunk_index=i, metadata={"source": doc},
                  embedding=rng.standard_normal(16).astype(np.float32).tolist()) for i, t in enumerate(DOCS[doc])]


def _ref_hits(contents, query, k):
    ref = lex_ref.RefIndex()
    ref.add([lex_ref.analyze(t) for t in contents])
    s, r = ref.search([lex_ref.analyze(query)], k)
    return [(contents[i], sc) for sc, i in zip(s[0], r[0]) if i >= 0]


def test_store_feeds_and_mirrors_the_lexical_index(tmp_path):
    s = _store(tmp_path, True)
    for d in DOCS:
        run(s.add_chunks(_doc_chunks(d)))
    everything = DOCS["manual"] + DOCS["faq"]
    got = s.keyword_search("pump E1234", 10)
    assert [(c.content, sc) for c, sc in got] == _ref_hits(everything, "pump E1234", 6)
    only = s.keyword_search("pump E1234", 10, filters={"source": "faq"})
    assert {c.document_id for c, _ in only} == {"faq"} and len(only) == 2
    assert [c.content for c, _ in s.keyword_search_batch(["torque", "nothing matches this"], 3)[0]] == \
        ["valve torque table"]
    run(s.delete_by_document_id("manual"))
    after = [(c.content, sc) for c, sc in s.keyword_search("pump E1234", 10)]
    assert after == _ref_hits(DOCS["faq"], "pump E1234", 3) and len(after) == 2  # statistics follow the delete
    ids = [c.id for c, _ in s.keyword_search("pump E1234", 10)]
    s.close()
    s2 = _store(tmp_path, True)  # reload: rebuilt from the stored contents, dead rows keep their numbers
    again = s2.keyword_search("pump E1234", 10)
    assert [(c.content, sc) for c, sc in again] == after and [c.id for c, _ in again] == ids
    assert s2._lex.ref.live == [False] * 3 + [True] * 3
    run(s2.clear())
    assert s2.keyword_search("pump", 5) == []
    run(s2.add_chunks(_doc_chunks("faq")))
    assert [c.id for c, _ in s2.keyword_search("overheating", 5)] == ["faq_1"]


def test_lexical_off_by_default_and_multi_device_refused(tmp_path):
    s = _store(tmp_path, False)
    run(s.add_chunks(_doc_chunks("faq")))
    assert s._lex is None
    with pytest.raises(ValueError):
        s.keyword_search("pump", 3)
    cfg = VectorStoreConfig(backend="hip", collection_name="kb2", persist_directory=str(tmp_path),
                            index_params={"lexical": True, "devices": [0, 1]})
    with pytest.raises(ValueError, match="single-device"):
        HipVectorStore(cfg)


def test_hybrid_without_lexical_index_is_the_vector_retriever(tmp_path):
    s = _store(tmp_path, False)
    for d in DOCS:
        run(s.add_chunks(_doc_chunks(d)))
    emb = HashEmbedder(dim=16)
    cfg = RetrieverConfig(top_k=4, similarity_threshold=0.0)
    queries = ["pump E1234", "torque", "support"]
    want = run(BatchedVectorRetriever(s, emb, cfg).batch_retrieve(queries))
    h = HybridRetriever(s, emb, cfg)
    got = run(h.batch_retrieve(queries))
    key = lambda res: [[(x.chunk.id, x.score, x.rank) for x in q] for q in res]  # noqa: E731
    assert key(got) == key(want) and all(len(q) == 4 for q in got)
    assert key([run(h.retrieve(q)) for q in queries]) == key(want)

    class Plain:  # a store with no keyword search at all
        search_batch = staticmethod(s.search_batch)
        search = s.search

    assert key(run(HybridRetriever(Plain(), emb, cfg).batch_retrieve(queries))) == key(want)


# ---------------------------------------------------------------- ABI
def test_new_symbols_and_abi_version():
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in ("hr_lex_pack", "hr_lex_create", "hr_lex_destroy", "hr_lex_add", "hr_lex_remove", "hr_lex_size",
                 "hr_lex_stats", "hr_lex_df", "hr_lex_search", "hr_lex_last_ms"):
        assert hasattr(L, name) and name in _native.EXPORTS
    assert (_native.HR_LEX_TERM_BITS, _native.HR_LEX_MAX_QTERMS, _native.HR_LEX_MAX_K) == (22, 64, 1024)
    assert callable(_native.NativeLexIndex) and callable(LX.LexicalIndex)
