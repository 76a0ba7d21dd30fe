"""CPU: boosted search above the kernels -- the restatement (tests/boost_ref.py) against a brute force in plain Python
floats, the mechanism's window as a superset of the blended top-k over the issue's grid, the new symbols with their
host-side validation (no handle, no device), and the store, retriever and IVF-store wiring over a numpy-backed
stand-in index (tests/fake_index_boost.py)."""
import asyncio
import ctypes
import math
import os
import re

import numpy as np
import pytest

import boost_ref as BR
from conftest import REPO
from fake_index import OracleIndex
from fake_index_boost import BoostOracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from hiprag.rag.config import RetrieverConfig
from hiprag.rag.ivf_store import IvfStoreIndex
from hiprag.rag.retriever import VectorRetriever
from hiprag.rag.storage import BoostedHits
from oracle import ref_numpy as R

METRICS = ["cosine", "ip", "l2"]
WEIGHTS = [(1.0, 0.0), (1.0, 0.05), (1.0, 0.25), (0.5, 0.5), (1.0, -0.25), (1.0, 2.0)]


def run(coro):
    return asyncio.run(coro)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------- the restatement and the mechanism
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("metric", METRICS)
def test_boost_ref_brute_force_and_the_window_is_a_superset(dtype, metric):
    """n = 4099, dim 64, planted queries with noise 0.05, one U[0, 1) column, the issue's weight grid: boost_ref equals
    a brute force over Python floats (one rounding per operation by construction), and the mechanism's window -- the
    allowed rows with (float)s >= t -- holds every row of the blended top-10."""
    rng = np.random.default_rng(7 * METRICS.index(metric) + (dtype == "f32"))
    n, dim, B, k = 4099, 64, 3, 10
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    if metric != "cosine":
        x = x * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    st = R.process_rows(x, metric, dtype)
    q = R.process_queries(_unit(x[rng.choice(n, B)]) + 0.05 * _unit(rng.standard_normal((B, dim)).astype(np.float32)),
                          metric)
    col = rng.random(n).astype(np.float32)
    allowed = rng.random(n) < 0.9
    s = R.exact_scores(st, dtype, q, metric)
    s32 = s.astype(np.float32)
    for alpha, beta in WEIGHTS:
        v, sc, r = BR.boost_ref(st, dtype, q, k, alpha, [beta], [col], allowed, metric, scores=s)
        mech = BR.mechanism(st, dtype, q, k, alpha, [beta], [col], allowed, metric, scores=s)
        for b in range(B):
            brute = sorted((-(alpha * float(s[b, i]) + beta * float(col[i])), i) for i in range(n) if allowed[i])[:k]
            assert r[b].tolist() == [i for _, i in brute]
            assert v[b].tolist() == [-nv + 0.0 for nv, _ in brute]
            assert sc[b].tolist() == [float(s32[b, i]) for _, i in brute]
            window = allowed & (s32[b] >= mech["t"][b])
            assert window[r[b]].all() and mech["count"][b] == window.sum() >= k
            assert (v[b] >= mech["tau"][b]).all()  # tau is a lower bound of the true k-th blended value
        assert (mech["stage"] == 1).all()  # the default window holds these corpora
        if beta == 0.0:  # no boost: the floor sits one fp32 step below the k-th score
            assert (mech["count"] <= k + 2).all()


def test_boost_ref_nan_ties_padding_and_columns():
    x = np.zeros((6, 2), np.float32)
    x[:, 0] = [1, 0.5, 0.5, np.nan, 0.25, 0.5]
    st = R.process_rows(x, "ip", "f32")
    q = np.asarray([[1.0, 0.0]], np.float32)
    col = np.asarray([0, 0.5, 0.5, 9, 1.0], np.float32)  # shorter than the index: row 5 reads 0.0
    v, s, r = BR.boost_ref(st, "f32", q, 8, 1.0, [1.0], [col], metric="ip")
    assert r.tolist() == [[4, 0, 1, 2, 5, -1, -1, -1]]  # the NaN row is never returned; ties by row
    assert v[0, :5].tolist() == [1.25, 1.0, 1.0, 1.0, 0.5] and np.isneginf(v[0, 5:]).all()
    assert s[0, :5].tolist() == [0.25, 1.0, 0.5, 0.5, 0.5] and np.isneginf(s[0, 5:]).all()
    v, s, r = BR.boost_ref(st, "f32", q, 2, 1.0, [-1.0], [col], np.asarray([1, 1, 1, 1, 1, 0], bool), "ip")
    assert r.tolist() == [[0, 1]] and v.tolist() == [[1.0, 0.0]]
    v, s, r = BR.boost_ref(st[:0], "f32", q, 2, 1.0, [], [], metric="ip")
    assert r.tolist() == [[-1, -1]]
    m = BR.mechanism(st[:3], "f32", q, 2, 1.0, [1.0], [col[:3]], metric="ip", probe=2, window=2)
    # pool rows 0, 1: v = 1.0, 1.0 -> tau = 1.0; bext = 0.5: Vmax(x) = x + 0.5 >= 1 from x = 0.5; t one step below
    assert m["tau"].tolist() == [1.0] and m["t"][0] == np.nextafter(np.float32(0.5), np.float32(0)) and m["count"][0] == 3
    assert m["stage"].tolist() == [2]
    with pytest.raises(AssertionError):
        BR.assert_same((v, s, r), (v, s, r + 1))


# ---------------------------------------------------------------- the C boundary
NEW = ["hr_index_set_boost", "hr_index_search_boosted", "hr_index_search_boosted_device"]
NEW_DIAG = ["hr_index_boost_stats"]


def test_new_symbols_are_declared_exported_and_validate():
    from hiprag import _native

    def decls(name):
        text = open(os.path.join(REPO, "include", name)).read()
        return set(re.findall(r"^\s*int\s+(hr_\w+)\s*\(", text, re.M))

    header = open(os.path.join(REPO, "include", "hiprag.h")).read()
    assert set(NEW) <= decls("hiprag.h") and set(NEW_DIAG) <= decls("hiprag_diag.h")
    assert "#define HR_BOOST_MAX_COLS 4" in header and "#define HR_BOOST_MAX_WINDOW 8192" in header
    assert _native.HR_BOOST_MAX_COLS == 4 and _native.HR_BOOST_MAX_WINDOW == 8192
    assert set(NEW + NEW_DIAG) <= set(_native.EXPORTS)
    for m in ("set_boost", "search_boosted", "search_boosted_device", "boost_stats"):
        assert callable(getattr(_native.NativeIndex, m))
    assert "hr_boost.hip" in open(os.path.join(REPO, "youtu-rag_amd", "csrc", "Makefile")).read()
    assert os.path.exists(_native.LIB_PATH), "libhiprag.so not built (run __graft_entry__.build())"
    L = _native.load_library()
    assert L.hr_abi_version() == 2
    for name in NEW + NEW_DIAG:
        assert hasattr(L, name)
    # no handle, no device needed: the limits are checked on the host before the handle is looked at, so each bad
    # argument is named even without one; with good arguments the null handle is what is refused
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def boosted(alpha=1.0, k=10, n_cols=1, probe=0, window=0, device=False):
        if device:
            return L.hr_index_search_boosted_device(None, p, 1, k, alpha, p, n_cols, probe, window, None, p, p, p, None)
        return L.hr_index_search_boosted(None, p, 1, k, alpha, p, n_cols, probe, window, None, p, p, p)

    for device in (False, True):
        for kw, word in ((dict(alpha=0.0), b"alpha"), (dict(alpha=math.nan), b"alpha"), (dict(alpha=math.inf), b"alpha"),
                         (dict(window=9), b"window"), (dict(window=8193), b"window"), (dict(n_cols=5), b"n_cols"),
                         (dict(n_cols=-1), b"n_cols"), (dict(probe=9), b"probe"), (dict(probe=129), b"probe"),
                         (dict(k=0), b"k must"), (dict(k=129), b"k must"), (dict(), b"null")):
            assert boosted(device=device, **kw) == -1 and word in L.hr_last_error(), (kw, L.hr_last_error())
    buf[0] = 2.0 ** 65
    assert boosted() == -1 and b"beta" in L.hr_last_error()
    buf[0] = math.nan
    assert boosted() == -1 and b"beta" in L.hr_last_error()
    buf[0] = -2.0 ** 64  # a legal penalty
    assert boosted() == -1 and b"null" in L.hr_last_error()
    vals = (ctypes.c_float * 2)(1.0, math.nan)
    pv = ctypes.cast(vals, ctypes.c_void_p)
    assert L.hr_index_set_boost(None, 0, 0, 2, pv) == -1 and b"finite" in L.hr_last_error()
    vals[1] = math.inf
    assert L.hr_index_set_boost(None, 0, 0, 2, pv) == -1 and b"finite" in L.hr_last_error()
    assert L.hr_index_set_boost(None, 4, 0, 1, pv) == -1 and b"col" in L.hr_last_error()
    assert L.hr_index_set_boost(None, -1, 0, 1, pv) == -1 and b"col" in L.hr_last_error()
    assert L.hr_index_set_boost(None, 0, 0, 1, pv) == -1 and b"null" in L.hr_last_error()
    assert L.hr_index_boost_stats(None, p) == -1


# ---------------------------------------------------------------- the store
FIELDS = ["importance_score", "recency_base"]


def make_store(tmp_path, index=BoostOracleIndex, persist=False, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": persist, "fsync": False, "boost_fields": FIELDS,
                                          **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index(dim, "f32"),
                          index_loader=lambda path, dim, dt, metric: _load(index, path))


def _load(cls, path):
    base = OracleIndex.load(path)
    idx = cls(base.dim, base.dtype, base.metric)
    idx.rows, idx.live = base.rows, base.live
    return idx


ODD = {3: "high", 4: None, 5: float("nan"), 6: float("inf"), 7: [1.0], 8: True, 9: 7, 10: 10 ** 60, 11: "0.9"}


def memory_chunks(n=60, seed=1, dim=16, start=0):
    """Chunks with an importance in [0, 1) and a recency base; rows 3..11 carry values that are no finite float32
    number (or a bool / an int, which are), row 12 has no importance at all."""
    rng = np.random.default_rng(seed)
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    imp = rng.random(n).astype(np.float32)
    rec = np.exp2(-rng.uniform(0, 6, n)).astype(np.float32)
    chunks, want_imp = [], imp.copy()
    for i in range(n):
        meta = {"part": i % 3, "importance_score": float(imp[i]), "recency_base": float(rec[i])}
        if start == 0 and i in ODD:
            meta["importance_score"] = ODD[i]
            want_imp[i] = {8: 1.0, 9: 7.0}.get(i, 0.0)
        if start == 0 and i == 12:
            del meta["importance_score"]
            want_imp[i] = 0.0
        chunks.append(Chunk(id=f"c{start + i}", document_id=f"d{i % 4}", content=f"t{i}", chunk_index=i, metadata=meta,
                            embedding=x[i].tolist()))
    return chunks, x, want_imp, rec


def want(store, q, k, alpha, betas, cols, allowed=None):
    idx = store._index
    live = idx.live if allowed is None else idx.live & allowed
    v, s, r = BR.boost_ref(idx.rows, "f32", R.process_queries(np.atleast_2d(np.asarray(q, np.float32)), "cosine"), k,
                           alpha, betas, cols, live)
    return [([(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0], [float(x) for x, row in zip(v[b], r[b])
                                                                                if row >= 0]) for b in range(len(r))]


def got_of(res):
    return [([(c.id, s) for c, s in h.hits], list(h.blended)) for h in res]


W = {"importance_score": 0.3, "recency_base": 0.2}


def test_store_columns_from_metadata_growth_and_deletes(tmp_path):
    s = make_store(tmp_path)
    chunks, x, imp, rec = memory_chunks()
    run(s.add_chunks(chunks))
    q = x[:3].tolist()
    assert s._boost_cols is None and s._index.set_calls == []  # lazy: nothing until the first boosted search
    res = s.search_boosted_batch(q, 5, boost_weights=W, sim_weight=0.5)
    assert s._index.set_calls == [(0, 0, 60), (1, 0, 60)]
    np.testing.assert_array_equal(s._index.cols[0], imp)  # missing / non-numeric / non-finite -> 0.0; bool, int kept
    np.testing.assert_array_equal(s._index.cols[1], rec)
    assert s._index.boost_calls == [(3, 5, 0.5, [0.3, 0.2], False, 0, 0)]
    assert all(isinstance(h, BoostedHits) for h in res)
    assert got_of(res) == want(s, q, 5, 0.5, [0.3, 0.2], [imp, rec])
    # one field named: the other column's weight is 0.0; a negative weight is a penalty
    res = s.search_boosted_batch(q, 5, boost_weights={"recency_base": -2.0}, probe=40, window=50)
    assert s._index.boost_calls[-1] == (3, 5, 1.0, [0.0, -2.0], False, 40, 50)
    assert got_of(res) == want(s, q, 5, 1.0, [0.0, -2.0], [imp, rec])
    assert len(s._index.set_calls) == 2  # nothing new to send
    # rows added after the first boosted search go up under the next one's lock hold
    more, x2, imp2, rec2 = memory_chunks(25, seed=2, start=60)
    run(s.add_chunks(more))
    assert len(s._index.set_calls) == 2
    res = s.search_boosted_batch(q, 8, boost_weights=W, sim_weight=0.5)
    assert s._index.set_calls[2:] == [(0, 60, 25), (1, 60, 25)]
    imp_all, rec_all = np.concatenate([imp, imp2]), np.concatenate([rec, rec2])
    assert got_of(res) == want(s, q, 8, 0.5, [0.3, 0.2], [imp_all, rec_all])
    # deletes leave the hits
    top = [cid for cid, _ in got_of(res)[0][0]][:3]
    run(s.delete(top))
    res = s.search_boosted_batch(q, 8, boost_weights=W, sim_weight=0.5)
    assert not set(top) & {c.id for c, _ in res[0].hits}
    assert got_of(res) == want(s, q, 8, 0.5, [0.3, 0.2], [imp_all, rec_all])
    one = run(s.search_boosted(q[0], 4, boost_weights=W, sim_weight=0.5))
    assert got_of([one]) == want(s, q[:1], 4, 0.5, [0.3, 0.2], [imp_all, rec_all])
    # top_k beyond the stored chunks: every chunk, no padding
    assert len(s.search_boosted_batch(q[:1], 128, boost_weights=W)[0].hits) == s.count_sync()


def test_store_filters_per_query_lists(tmp_path):
    s = make_store(tmp_path)
    chunks, x, imp, rec = memory_chunks()
    run(s.add_chunks(chunks))
    q = x[:3].tolist()
    part = np.arange(60) % 3
    res = s.search_boosted_batch(q, 5, boost_weights=W, filters={"part": 1})
    assert s._index.boost_calls[-1][4] is True
    assert got_of(res) == want(s, q, 5, 1.0, [0.3, 0.2], [imp, rec], part == 1)
    flt = [{"part": 1}, None, {"part": 1}]
    del s._index.boost_calls[:]
    before = s.grouped_launches
    res = s.search_boosted_batch(q, 5, boost_weights=W, filters=flt)
    assert sorted((c[0], c[4]) for c in s._index.boost_calls) == [(1, False), (2, True)]
    assert s.grouped_launches - before == 2
    for i, f in enumerate(flt):
        assert got_of([res[i]]) == want(s, q[i], 5, 1.0, [0.3, 0.2], [imp, rec], None if f is None else part == 1)


def test_store_reload_rebuilds_the_columns(tmp_path):
    s = make_store(tmp_path, persist=True)
    chunks, x, imp, rec = memory_chunks()
    run(s.add_chunks(chunks))
    q = x[:2].tolist()
    first = got_of(s.search_boosted_batch(q, 5, boost_weights=W, sim_weight=0.5))
    s.close()
    assert not any("boost" in f for f in os.listdir(tmp_path))  # nothing of the columns is persisted
    s2 = make_store(tmp_path, persist=True)
    assert s2.count_sync() == 60 and s2._boost_cols is None and s2._index.set_calls == []
    assert got_of(s2.search_boosted_batch(q, 5, boost_weights=W, sim_weight=0.5)) == first
    assert s2._index.set_calls == [(0, 0, 60), (1, 0, 60)]
    s2.close()


def test_store_error_cases(tmp_path):
    s = make_store(tmp_path)
    chunks, x, imp, rec = memory_chunks(40)
    q = x[0].tolist()
    assert s.search_boosted_batch([q], 3, boost_weights=W) == [BoostedHits([], [])]  # nothing stored: no index yet
    run(s.add_chunks(chunks))
    bad = [dict(boost_weights={"popularity": 1.0}), dict(boost_weights={"importance_score": float("nan")}),
           dict(boost_weights={"importance_score": 2.0 ** 65}), dict(boost_weights=[0.3]),
           dict(boost_weights=W, sim_weight=0.0), dict(boost_weights=W, sim_weight=float("inf")),
           dict(boost_weights=W, top_k=0), dict(boost_weights=W, top_k=129), dict(boost_weights=W, top_k=10, probe=9),
           dict(boost_weights=W, top_k=10, window=9), dict(boost_weights=W, window=8193)]
    for kw in bad:
        with pytest.raises(ValueError):
            s.search_boosted_batch([q], **kw)
        with pytest.raises(ValueError):
            run(s.search_boosted(q, **kw))
    with pytest.raises(ValueError, match="not a configured boost field"):
        s.search_boosted_batch([q], boost_weights={"popularity": 1.0})
    with pytest.raises(ValueError, match="dim"):
        s.search_boosted_batch([q + [0.0]], boost_weights=W)
    with pytest.raises(ValueError, match="filters"):
        s.search_boosted_batch([q], boost_weights=W, filters=[None, None])
    assert s._index.boost_calls == [] and s._index.set_calls == []  # every limit is checked before any native call
    s._index.devices = [0, 1]
    with pytest.raises(ValueError, match="single-device"):
        s.search_boosted_batch([q], boost_weights=W)
    plain = make_store(tmp_path / "plain", index=OracleIndex)
    run(plain.add_chunks(chunks))
    with pytest.raises(NotImplementedError):
        plain.search_boosted_batch([q], boost_weights=W)
    with pytest.raises(NotImplementedError):
        run(plain.search_boosted(q, boost_weights=W))
    assert len(plain.search_batch([q], 3)[0]) == 3
    with pytest.raises(ValueError, match="boost_fields"):
        make_store(tmp_path / "five", boost_fields=["a", "b", "c", "d", "e"])


def test_ivf_store_delegates_to_its_exact_index():
    exact = BoostOracleIndex(16, "f32")
    chunks, x, imp, rec = memory_chunks()
    exact.add(x)
    ivf = IvfStoreIndex(16, "f32", "cosine", nlist=4, nprobe=1, _exact=exact)
    ivf.set_boost(1, 0, rec)
    assert exact.set_calls == [(1, 0, 60)]
    got = ivf.search_boosted(x[:2], 7, 0.5, [0.0, 0.2], None, 32, 64)
    assert exact.boost_calls == [(2, 7, 0.5, [0.0, 0.2], False, 32, 64)]
    BR.assert_same(got, BR.boost_ref(exact.rows, "f32", R.process_queries(x[:2], "cosine"), 7, 0.5, [0.0, 0.2],
                                     [np.zeros(0, np.float32), rec]))
    assert ivf.boost_stats() == exact.boost_stats()


# ---------------------------------------------------------------- the retriever
class StubStore:
    def __init__(self, n=6):
        self.calls, self.n = [], n

    async def search_boosted(self, query_embedding, top_k=5, *, boost_weights, sim_weight=1.0, filters=None):
        self.calls.append((top_k, boost_weights, sim_weight, filters))
        m = min(self.n, top_k)
        hits = [(Chunk(id=f"c{i}", document_id=f"d{i}", content=f"t{i}", chunk_index=0, metadata={}),
                 [0.5, 0.9, 0.2, 0.8, 0.1, 0.7][i]) for i in range(m)]
        return BoostedHits(hits, [3.0 - 0.25 * i for i in range(m)])


class Emb:
    async def embed_query(self, q):
        return [0.0, 1.0]


class Reverse:
    async def rerank(self, query, results, top_k=None):
        return list(reversed(results))


def test_retrieve_boosted_scores_ranks_threshold_and_reranker():
    st = StubStore()
    ret = VectorRetriever(st, Emb(), RetrieverConfig(top_k=4, similarity_threshold=0.45))
    res = run(ret.retrieve_boosted("q", boost_weights=W, sim_weight=0.5, filters={"a": 1}))
    assert st.calls == [(4, W, 0.5, {"a": 1})]
    # score: the blended value; the threshold cuts by the similarity (c2: 0.2 is out); ranks 1-based, before the cut
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [("c0", 3.0, 1), ("c1", 2.75, 2), ("c3", 2.25, 4)]
    res = run(ret.retrieve_boosted("q", 6, boost_weights=W, similarity_threshold=0.0))
    assert [r.rank for r in res] == [1, 2, 3, 4, 5, 6] and st.calls[-1][0] == 6
    rr = VectorRetriever(StubStore(), Emb(), RetrieverConfig(top_k=2, similarity_threshold=0.0), reranker=Reverse())
    res = run(rr.retrieve_boosted("q", boost_weights=W))
    assert rr.vector_store.calls == [(4, W, 1.0, None)]  # the reranker sees twice top_k
    assert [r.chunk.id for r in res] == ["c3", "c2"] and [r.rank for r in res] == [4, 3]

    class NoBoost:
        async def search(self, *a, **kw):
            return []

    with pytest.raises(NotImplementedError):
        run(VectorRetriever(NoBoost(), Emb(), RetrieverConfig()).retrieve_boosted("q", boost_weights=W))


def test_retrieve_boosted_over_the_store_is_the_memory_ranking(tmp_path):
    """0.5 similarity + 0.3 importance + 0.2 recency(now) with a static recency_base column: the query-time factor
    folds into the column's weight."""
    s = make_store(tmp_path)
    chunks, x, imp, rec = memory_chunks()
    run(s.add_chunks(chunks))
    qv = x[5].tolist()

    class E:
        async def embed_query(self, q):
            return qv

    decay = 2.0 ** -1.5  # now is 36 h after the epoch
    ret = VectorRetriever(s, E(), RetrieverConfig(top_k=6, similarity_threshold=0.0))
    res = run(ret.retrieve_boosted("q", boost_weights={"importance_score": 0.3, "recency_base": 0.2 * decay},
                                   sim_weight=0.5))
    (hits, blended), = want(s, qv, 6, 0.5, [0.3, 0.2 * decay], [imp, rec])
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, v, i + 1)
                                                           for i, ((cid, _), v) in enumerate(zip(hits, blended))]
