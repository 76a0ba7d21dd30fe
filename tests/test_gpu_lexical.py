"""GPU: the keyword (BM25) search against the pure-Python reference (tests/lex_ref.py).  Every comparison is exact:
rows equal, scores equal as float64 bit patterns.  The shapes are the smallest at which the scan can go wrong: the
row-block edges (64 rows per block), empty rows and blocks, rows starting at every offset of a 16-byte load, a row
spanning many loads, the query-term cap, several sub-batches, ties, every k regime, growth of the device arrays,
tombstones and masks."""
import asyncio

import numpy as np
import pytest

import lex_ref
from hash_embed import HashEmbedder, vec
from hiprag import _native
from hiprag.rag import Chunk, HipVectorStore, HybridRetriever, RetrieverConfig, VectorStoreConfig

pytestmark = pytest.mark.gpu


def run(coro):
    return asyncio.run(coro)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def mask_words(allowed):
    n = len(allowed)
    w = np.zeros((n + 63) // 64, np.uint64)
    for r, ok in enumerate(allowed):
        if ok:
            w[r >> 6] |= np.uint64(1) << np.uint64(r & 63)
    return w


def check(idx, ref, queries, k, allowed=None, k1=1.2, b=0.75):
    """One native search against the reference; returns the native (scores, rows)."""
    s, r = idx.search(queries, k, None if allowed is None else mask_words(allowed), k1, b)
    s_ref, r_ref = ref.search(queries, k, allowed, k1, b)
    assert s.shape == r.shape == (len(queries), k)
    assert np.array_equal(r, np.array(r_ref, np.int64).reshape(len(queries), k))
    assert np.array_equal(bits(s), bits(np.array(s_ref, np.float64).reshape(len(queries), k)))
    return s, r


def check_stats(idx, ref):
    n, sum_dl, df = ref.stats()
    assert idx.stats() == (n, sum_dl)
    assert idx.size() == (len(ref.rows), n)
    terms = sorted(df) + [4194303, 4000000]
    assert idx.df(terms).tolist() == [df.get(t, 0) for t in terms]


def both(rows):
    idx, ref = _native.NativeLexIndex(0), lex_ref.RefIndex()
    assert idx.add(rows) == ref.add(rows) == 0
    return idx, ref


# ---------------------------------------------------------------- row counts and empty rows
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_row_block_edges_and_empty_rows(n):
    rng = np.random.default_rng(n)
    rows = [[100] + rng.integers(0, 20, int(rng.integers(1, 12))).tolist() for _ in range(n)]
    if n >= 63:
        for r in (0, 31, 62 if n == 63 else 63):  # empty rows at the start, middle and end of a block
            rows[r] = []
    if n == 129:
        for r in range(64, 128):  # a block whose rows are all empty
            rows[r] = []
    idx, ref = both(rows)
    queries = [[100], [3], [3, 7, 100], [19, 0], [5, 5, 5], [21]]
    check(idx, ref, queries, 8)
    _, r = check(idx, ref, queries, n + 5)  # k beyond the hits
    assert (r[0] >= 0).sum() == sum(1 for row in rows if row)
    check_stats(idx, ref)
    idx.close()


# ---------------------------------------------------------------- entry layout
def test_rows_at_every_load_offset_and_a_long_row():
    rows, t = [], 1000
    for i in range(70):  # 1, 3, 4, 5 entries: the rows start at every offset within a 16-byte load
        c = (1, 3, 4, 5)[i % 4]
        rows.append([50] + list(range(t, t + c - 1)))
        t += 3
    long_row = list(range(200000, 205000))  # 5000 distinct terms: many loads, several lanes' iterations
    rows.insert(37, long_row + [50, 1003])
    rows.append([50, 204999])
    idx, ref = both(rows)
    queries = [[50], [1003], [1003, 1006, 1009, 50], [200000], [204999], [202500, 1030], list(range(1000, 1064)),
               [200000 + 79 * i for i in range(60)]]
    check(idx, ref, queries, 10)
    check(idx, ref, queries, 80)
    check_stats(idx, ref)
    idx.close()


# ---------------------------------------------------------------- queries
@pytest.fixture(scope="module")
def small():
    """150 rows over terms 0..99 (term 7 in every row), one row holding only the largest id of the 65-term query."""
    rng = np.random.default_rng(5)
    rows = [[7] + rng.integers(0, 100, int(rng.integers(0, 30))).tolist() for _ in range(150)]
    rows[40] = [7, 3000]
    rows[41] = [3000, 3000]
    idx, ref = both(rows)
    yield idx, ref
    idx.close()


def test_empty_unknown_and_duplicated_queries(small):
    idx, ref = small
    s, r = check(idx, ref, [[], [999999], [999999, 888888]], 5)
    assert np.all(r == -1) and np.all(np.isneginf(s))
    s, r = check(idx, ref, [[3, 3, 3, 9, 9], [3, 9], [], [9, 3, 999999]], 6)
    assert np.array_equal(r[0], r[1]) and np.array_equal(bits(s[0]), bits(s[1])) and np.array_equal(r[0], r[3])
    assert idx.last_ms()[2] >= 1


def test_query_term_cap(small):
    idx, ref = small
    q64 = list(range(36, 100))             # 64 known terms
    q65 = list(range(36, 100)) + [3000]    # 65: the largest id is dropped
    s, r = check(idx, ref, [q64, q65, [3000]], 150)
    assert np.array_equal(r[0], r[1]) and np.array_equal(bits(s[0]), bits(s[1]))
    assert 41 not in r[1].tolist() and r[2].tolist()[:2] == [41, 40]
    # the cap counts distinct terms, after de-duplication; unknown terms still take a place
    check(idx, ref, [q64 + q64, [0] + list(range(200, 263)) + [50], list(range(0, 100))], 20)


def test_term_in_every_row(small):
    idx, ref = small
    s, r = check(idx, ref, [[7]], 150)
    assert (r[0] >= 0).sum() == 149  # cap_b = n: every row but the one without the term
    check(idx, ref, [[7], [7, 3000], [7, 1, 2]], 150)


@pytest.mark.parametrize("B", [1, 64, 65, 200])
def test_batch_sizes(small, B):
    idx, ref = small
    rng = np.random.default_rng(B)
    queries = [rng.integers(0, 110, int(rng.integers(0, 9))).tolist() for _ in range(B)]
    check(idx, ref, queries, 10)
    df = ref.stats()[2]
    active = sum(1 for q in queries if any(t in df for t in q))  # (queries without a known term launch nothing)
    assert active > (B * 3) // 4 and idx.last_ms()[2] >= -(-active // 64)  # B > 64: several sub-batches


def test_long_queries_split_by_the_lds_budget(small):
    idx, ref = small
    queries = [list(range(i % 37, i % 37 + 64)) for i in range(64)]  # 64 queries x 64 terms: 4096 pairs
    check(idx, ref, queries, 10)
    assert idx.last_ms()[2] >= 2


# ---------------------------------------------------------------- ties and k
def test_ties_return_the_lowest_rows():
    idx, ref = both([[11, 12, 12, 13]] * 300)
    s, r = check(idx, ref, [[12], [11, 13]], 10)
    assert r.tolist() == [list(range(10))] * 2 and len(set(bits(s[0]).tolist())) == 1
    idx.close()


@pytest.fixture(scope="module")
def mid():
    rng = np.random.default_rng(17)
    rows = [[1] + rng.integers(2, 60, int(rng.integers(0, 25))).tolist() for _ in range(1500)]
    idx, ref = both(rows)
    yield idx, ref
    idx.close()


@pytest.mark.parametrize("k", [1, 128, 1024])
def test_k_regimes(mid, k):
    idx, ref = mid
    s, r = check(idx, ref, [[1], [5, 9], [59], [2, 3, 4, 1]], k)
    assert (r[0] >= 0).sum() == min(k, 1500)
    with pytest.raises(ValueError):
        idx.search([[1]], 1025)
    with pytest.raises(ValueError):
        idx.search([[1]], 0)


# ---------------------------------------------------------------- mutations and masks
def test_appends_grow_the_arrays_and_removes_update_statistics():
    rng = np.random.default_rng(23)
    idx, ref = _native.NativeLexIndex(0), lex_ref.RefIndex()
    rows_all = []
    for n_add in (600, 700, 900):  # past 1024 rows / 16384 entries, then past their doubles
        rows = [rng.integers(0, 300, int(rng.integers(0, 30))).tolist() for _ in range(n_add)]
        assert idx.add(rows) == ref.add(rows) == len(rows_all)
        rows_all += rows
        check(idx, ref, [[1, 2, 3], [299], [150, 7]], 10)
    assert idx.size() == (2200, 2200)
    check_stats(idx, ref)
    queries = [rng.integers(0, 300, int(rng.integers(1, 6))).tolist() for _ in range(20)]
    gone = sorted(set(rng.integers(0, 2200, 400).tolist()) | {0, 63, 64, 2199})
    idx.remove(gone)
    ref.remove(gone)
    check_stats(idx, ref)
    s, r = check(idx, ref, queries, 10)
    # a reference rebuilt from the survivors alone: same statistics, same scores, rows renumbered
    keep = [i for i in range(2200) if i not in set(gone)]
    fresh = lex_ref.RefIndex()
    fresh.add([rows_all[i] for i in keep])
    assert fresh.stats() == ref.stats()
    s2, r2 = fresh.search(queries, 10)
    assert [[keep[x] if x >= 0 else -1 for x in q] for q in r2] == r.tolist()
    assert np.array_equal(bits(s2), bits(s))
    idx.remove(gone[:5] + [gone[0]])  # removing removed rows changes nothing
    check_stats(idx, ref)
    check(idx, ref, queries, 10)
    with pytest.raises(ValueError):
        idx.remove([2200])
    first = idx.add([[5, 6], []])  # appends after removes keep numbering
    assert first == ref.add([[5, 6], []]) == 2200
    check(idx, ref, queries + [[5, 6]], 10)
    idx.close()


def test_mask_and_tombstones():
    rng = np.random.default_rng(31)
    rows = [[7] + rng.integers(0, 40, int(rng.integers(0, 12))).tolist() for _ in range(200)]
    idx, ref = both(rows)
    queries = [[7], [1, 2, 3], [39, 7], [12]]
    allowed = (rng.random(200) < 0.5).tolist()
    before = ref.stats()
    check(idx, ref, queries, 200, allowed)                 # mask only
    check_stats(idx, ref)
    assert ref.stats() == before                           # the mask does not change the statistics
    check(idx, ref, queries, 10, [False] * 200)            # nothing allowed
    dead = rng.choice(200, 60, replace=False).tolist()
    idx.remove(dead)
    ref.remove(dead)
    check(idx, ref, queries, 200)                          # tombstones only
    check(idx, ref, queries, 200, allowed)                 # both
    check(idx, ref, queries, 7, allowed, 0.9, 0.4)
    check_stats(idx, ref)
    with pytest.raises(ValueError):
        idx.search(queries, 5, np.zeros(3, np.uint64))     # a mask shorter than the rows
    idx.close()


# ---------------------------------------------------------------- random corpus
def _zipf_corpus(seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 501)
    p /= p.sum()
    vocab = rng.choice(1 << 22, 500, replace=False)
    rows = [vocab[rng.choice(500, int(rng.integers(0, 201)), p=p)].tolist() for _ in range(3000)]
    queries = [vocab[rng.choice(500, int(rng.integers(1, 9)), p=p)].tolist() for _ in range(64)]
    return rows, queries


@pytest.fixture(scope="module")
def zipf():
    rows, queries = _zipf_corpus(77)
    idx, ref = both(rows)
    yield idx, ref, queries
    idx.close()


@pytest.mark.parametrize("k1,b", [(1.2, 0.75), (0.9, 0.4)])
def test_random_corpus(zipf, k1, b):
    idx, ref, queries = zipf
    s, r = check(idx, ref, queries, 10, None, k1, b)
    rows2, queries2 = _zipf_corpus(77)  # the same seed again, a fresh index: identical output
    idx2 = _native.NativeLexIndex(0)
    idx2.add(rows2)
    s2, r2 = idx2.search(queries2, 10, None, k1, b)
    s3, r3 = idx.search(queries, 10, None, k1, b)
    idx2.close()
    assert np.array_equal(r, r2) and np.array_equal(bits(s), bits(s2))
    assert np.array_equal(r, r3) and np.array_equal(bits(s), bits(s3))


# ---------------------------------------------------------------- store level
WORDS = ["pump", "valve", "torque", "manual", "error", "reset", "overheating", "support", "chapter", "table"]


def _doc_chunks(doc, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        text = " ".join(rng.choice(WORDS, int(rng.integers(2, 9))).tolist()) + (f" E{1000 + i}" if i % 3 == 0 else "")
        out.append(Chunk(id=f"{doc}_{i}", document_id=doc, content=text, chunk_index=i, metadata={"source": doc},
                         embedding=vec(text, 16).tolist()))
    return out


def _lex_store(tmp_path, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "fsync": False, "lexical": True, **params})
    return HipVectorStore(cfg)


def _ref_hits(chunks, query, k):
    ref = lex_ref.RefIndex()
    ref.add([lex_ref.analyze(c.content) for c in chunks])
    s, r = ref.search([lex_ref.analyze(query)], k)
    return [(chunks[i].id, sc) for sc, i in zip(s[0], r[0]) if i >= 0]


def _ids(hits):
    return [(c.id, sc) for c, sc in hits]


def test_store_keyword_search_follows_every_mutation(tmp_path):
    s = _lex_store(tmp_path)
    docs = {d: _doc_chunks(d, n, i) for i, (d, n) in enumerate((("manual", 70), ("faq", 40), ("notes", 30)))}
    for d in docs:
        run(s.add_chunks(docs[d]))
    everything = docs["manual"] + docs["faq"] + docs["notes"]
    for q in ("pump torque", "E1003", "Reset, the PUMP!", "unknownword"):
        assert _ids(s.keyword_search(q, 12)) == _ref_hits(everything, q, 12)
    # a where filter: the statistics stay those of the whole collection, only the candidates shrink
    got = _ids(s.keyword_search("pump torque", 200, filters={"source": "faq"}))
    assert got == [h for h in _ref_hits(everything, "pump torque", 140) if h[0].startswith("faq_")] and got
    assert run(s.delete_by_document_id("manual")) == 70
    run(s.delete(["faq_0", "nope"]))
    left = [c for c in docs["faq"] + docs["notes"] if c.id != "faq_0"]
    batch = s.keyword_search_batch(["pump torque", "E1003 error"], 9)
    assert [_ids(h) for h in batch] == [_ref_hits(left, "pump torque", 9), _ref_hits(left, "E1003 error", 9)]
    s.close()
    s2 = _lex_store(tmp_path)  # reload: the lexical index is rebuilt from the stored contents
    assert [_ids(h) for h in s2.keyword_search_batch(["pump torque", "E1003 error"], 9)] == [_ids(h) for h in batch]
    run(s2.add_chunks(_doc_chunks("late", 5, 9)))  # (journalled: replayed into both indexes on the next load)
    left += _doc_chunks("late", 5, 9)
    assert _ids(s2.keyword_search("valve", 20)) == _ref_hits(left, "valve", 20)
    s2.close()
    s3 = _lex_store(tmp_path)
    assert _ids(s3.keyword_search("valve", 20)) == _ref_hits(left, "valve", 20)
    run(s3.clear())
    assert s3.keyword_search("pump", 5) == []
    run(s3.add_chunks(docs["notes"]))
    assert _ids(s3.keyword_search("pump", 40)) == _ref_hits(docs["notes"], "pump", 30)
    s3.close()


def test_store_lexical_refuses_several_devices(tmp_path):
    with pytest.raises(ValueError, match="single-device"):
        _lex_store(tmp_path, devices=[0, 0])


# ---------------------------------------------------------------- hybrid
def test_hybrid_equals_host_rrf_and_finds_the_identifier(tmp_path):
    s = _lex_store(tmp_path, persist=False)
    chunks = _doc_chunks("manual", 60, 3) + _doc_chunks("faq", 30, 4)
    ident = "ZX-48151623-Q"
    chunks[47] = Chunk(id="manual_47", document_id="manual", content=f"spare part {ident} for the pump", chunk_index=47,
                       metadata={"source": "manual"}, embedding=vec("spare part", 16).tolist())
    run(s.add_chunks(chunks))
    emb = HashEmbedder(dim=16)
    h = HybridRetriever(s, emb, RetrieverConfig(top_k=5, similarity_threshold=0.0))
    queries = [ident, "pump torque", "where is the reset valve"]
    got = run(h.batch_retrieve(queries))
    fetch = 50  # min(128, max(4 * 5, 50))
    dense = s.search_batch(run(emb.embed_queries(queries)), fetch)
    lexical = s.keyword_search_batch(queries, fetch)
    for q, res, d, lx in zip(queries, got, dense, lexical):
        fused = {}
        for hits in (d, lx):
            for rank, (c, _) in enumerate(hits, 1):
                fused[c.id] = fused.get(c.id, 0.0) + 1.0 / (60.0 + rank)
        want = sorted(fused.items(), key=lambda kv: (-kv[1], s.row_of(kv[0])))[:5]
        assert [(x.chunk.id, x.score) for x in res] == want and [x.rank for x in res] == [1, 2, 3, 4, 5]
    assert "manual_47" in [x.chunk.id for x in got[0]]
    assert [(x.chunk.id, x.score) for x in run(h.retrieve(ident))] == [(x.chunk.id, x.score) for x in got[0]]
    s.close()
