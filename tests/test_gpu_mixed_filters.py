"""GPU: mixed-filter batches -- hr_index_search_masks (one row mask PER QUERY, one exact scan per 64 queries) against
the CPU oracle run per query with that query's mask, and against B single-mask calls of the existing search.

Bar, everywhere: ids, order (canonical fp64 score desc, row asc) and fp32 score bits identical; slots past the live,
allowed rows hold -inf / -1."""
import asyncio

import numpy as np
import pytest

import hostile_data as H
import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid], s_ref[valid].astype(np.float32))
    assert np.all(np.isneginf(s_gpu[~valid]))


def _pack(allowed):
    """(D, n) bool -> (D, words) uint64 bitmaps"""
    return np.stack([oracle.mask_from_bool(a) for a in allowed])


def _oracle(stored, dtype, qp, k, allowed, mask_of, metric="cosine", live=None):
    """The oracle per query with that query's mask (queries sharing a mask in one call); -inf / -1 past the rows"""
    B, n = len(qp), len(stored)
    s = np.full((B, k), -np.inf)
    r = np.full((B, k), -1, np.int64)
    for d in np.unique(mask_of):
        sel = np.nonzero(mask_of == d)[0]
        a = np.ones(n, bool) if d < 0 else allowed[d].copy()
        if live is not None:
            a &= live
        kk = min(k, int(a.sum()))
        if kk:
            s[sel, :kk], r[sel, :kk] = oracle.c_search(stored, dtype, qp[sel], kk, oracle.mask_from_bool(a), nthreads=4,
                                                       metric=metric)
    return s, r


def _singles(idx, q, k, masks, mask_of):
    """B single-mask calls of the existing search"""
    s = np.empty((len(q), k), np.float32)
    r = np.empty((len(q), k), np.int64)
    for i, d in enumerate(mask_of):
        s[i], r[i] = (x[0] for x in idx.search(q[i], k, None if d < 0 else masks[d]))
    return s, r


def _mask_kinds(rng, n, D, few=7):
    """D masks cycling through the kinds a batch mixes: 50 % random, 3 % random, one contiguous range, all ones, an
    empty mask, fewer rows than any k > `few`.  (-1 = no mask at all is a mask_of value, not a bitmap.)"""
    out = np.zeros((D, n), bool)
    for d in range(D):
        kind = d % 6
        if kind == 0:
            out[d] = rng.random(n) < 0.5
        elif kind == 1:
            out[d] = rng.random(n) < 0.03
        elif kind == 2:
            lo = int(rng.integers(0, n - 300))
            out[d, lo:lo + int(rng.integers(40, 300))] = True
        elif kind == 3:
            out[d] = True
        elif kind == 5:
            out[d, rng.choice(n, few, replace=False)] = True
    return out


# ---------------------------------------------------------------- small parity matrix
N_SMALL, DIM_SMALL, B_MAX, K_MAX = 3001, 64, 130, 100  # 94 tiles, the last one partial


@pytest.mark.parametrize("metric", ["cosine", "ip", "l2"])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_parity_matrix(native, dtype, metric):
    """B in {1, 5, 33, 64, 65, 130} (one query block, both, both lane halves, the chunk boundary) x k in {1, 10, 40,
    100} (row parts 1, 2, 4) x D in {1, 2, B}.  The references are taken once per D at B = 130, k = 100: an exact
    top-k is the prefix of the exact top-100 in the canonical order, and the first B queries keep their masks."""
    rng = np.random.default_rng([N_SMALL, ("bf16", "f16", "f32").index(dtype), ("cosine", "ip", "l2").index(metric)])
    # (the generator's elements reach 1.3e5: scaled by a power of two into f16's range for the raw ip / l2 rows)
    raw = R.gen_rows(3, 0, N_SMALL, DIM_SMALL) * np.float32(2.0 ** -17)
    idx = native.NativeIndex(DIM_SMALL, dtype, metric)
    idx.add(raw)
    stored = R.process_rows(raw, metric, dtype)
    pick = rng.choice(N_SMALL, B_MAX // 2, replace=False)
    q = np.concatenate([raw[pick] + 0.05 * rng.standard_normal((len(pick), DIM_SMALL)),
                        rng.standard_normal((B_MAX - len(pick), DIM_SMALL))]).astype(np.float32)
    q = q[rng.permutation(B_MAX)]
    qp = R.process_queries(q, metric)
    for D in ("1", "2", "B"):
        if D == "1":  # one bitmap, every query on it
            allowed, mask_of = _mask_kinds(rng, N_SMALL, 1), np.zeros(B_MAX, np.int32)
        elif D == "2":  # a 3 % mask, a contiguous range and no mask, by turns
            allowed = _mask_kinds(rng, N_SMALL, 3)[1:]
            mask_of = (np.arange(B_MAX, dtype=np.int32) % 3) - 1
        else:  # a bitmap of its own per query, every kind in every chunk, and -1 at every 7th query
            allowed = _mask_kinds(rng, N_SMALL, B_MAX)
            mask_of = np.arange(B_MAX, dtype=np.int32)
            mask_of[6::7] = -1
        masks = _pack(allowed)
        s_ref, r_ref = _oracle(stored, dtype, qp, K_MAX, allowed, mask_of, metric)
        s_one, r_one = _singles(idx, q, K_MAX, masks, mask_of)
        _check(s_one, r_one, s_ref, r_ref)
        for B in (1, 5, 33, 64, 65, 130):
            for k in (1, 10, 40, 100):
                s, r = idx.search_masks(q[:B], k, masks, mask_of[:B])
                _check(s, r, s_ref[:B, :k], r_ref[:B, :k])
                np.testing.assert_array_equal(s.view(np.uint32), s_one[:B, :k].view(np.uint32))
    # D = 0 and every entry -1: the unmasked search
    s0, r0 = idx.search(q[:64], 10)
    for masks, of in ((np.zeros((0, 0), np.uint64), np.full(64, -1)), (_pack(_mask_kinds(rng, N_SMALL, 2)), np.full(64, -1))):
        s, r = idx.search_masks(q[:64], 10, masks, of)
        np.testing.assert_array_equal(r, r0)
        np.testing.assert_array_equal(s.view(np.uint32), s0.view(np.uint32))
    idx.close()


# ---------------------------------------------------------------- strided SAMPLE, tile list
@pytest.fixture(scope="module")
def big(native):
    n, dim, B = 70_001, 64, 64  # 2188 tiles: the SAMPLE reads every 2nd tile (sample_target: 1024 tiles)
    rng = np.random.default_rng(70)
    raw = R.gen_rows(11, 0, n, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(raw)
    pick = rng.choice(n, B, replace=False)
    q = (raw[pick] + 0.3 * rng.standard_normal((B, dim))).astype(np.float32)
    yield idx, R.process_rows(raw, "cosine", "bf16"), q, R.process_queries(q, "cosine"), n
    idx.close()


@pytest.mark.parametrize("case", ["disjoint_documents", "shared_documents", "random_1pct"])
def test_strided_sample_and_tile_list(native, big, case):
    idx, stored, q, qp, n = big
    B, k = 64, 10
    rng = np.random.default_rng(5)
    if case == "disjoint_documents":  # 64 contiguous documents covering the index: a dense union, the full scan
        edges = np.linspace(0, n, B + 1).astype(np.int64)
        allowed = np.zeros((B, n), bool)
        for d in range(B):
            allowed[d, edges[d]:edges[d + 1]] = True
        mask_of = np.arange(B, dtype=np.int32)
    elif case == "shared_documents":  # 8 documents of 500 rows: the union is ~6 % of the tiles, the tile-list path
        allowed = np.zeros((8, n), bool)
        for d in range(8):
            lo = 3_000 + d * 8_111
            allowed[d, lo:lo + 500] = True
        mask_of = (np.arange(B, dtype=np.int32) * 5) % 8
    else:
        allowed = rng.random((B, n)) < 0.01
        mask_of = np.arange(B, dtype=np.int32)
    masks = _pack(allowed)
    launches = idx.qmask_launches()
    s, r = idx.search_masks(q, k, masks, mask_of)
    assert idx.qmask_launches() == launches + 1
    tiles = idx.wave_tiles()  # (of that FILTER launch)
    s_ref, r_ref = _oracle(stored, "bf16", qp, k, allowed, mask_of)
    _check(s, r, s_ref, r_ref)
    s_one, r_one = _singles(idx, q, k, masks, mask_of)
    np.testing.assert_array_equal(r, r_one)
    np.testing.assert_array_equal(s.view(np.uint32), s_one.view(np.uint32))
    if case == "shared_documents":  # the union's tiles only: 8 x (500 / 32 + 2) at most
        assert 0 < int(tiles.sum()) <= 8 * 18


# ---------------------------------------------------------------- thresholds are per query
def _threshold_inputs():
    """8000 Gaussian rows, 16 disjoint masks of 500 rows; 40 near-copies of query i sit in mask (i + 1) % 16 -- rows
    query i may NOT see, scoring ~0.99 against it while its allowed rows score ~N(0, 1/64)."""
    n, dim, B = 8_000, 64, 16
    rng = np.random.default_rng(16)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    allowed = np.zeros((B, n), bool)
    for d in range(B):
        allowed[d, d * 500:(d + 1) * 500] = True
    for i in range(B):
        lo = ((i + 1) % B) * 500 + 100
        raw[lo:lo + 40] = q[i] + 0.1 * rng.standard_normal((40, dim)).astype(np.float32)
    return raw, q, allowed


def test_thresholds_are_per_query(native):
    """250 tiles: the SAMPLE visits every tile, so thresholds do not depend on sampling.  A scan that took its group
    maxima over the union would start every query's threshold at its planted copies' scores, reject all of its
    allowed rows and fail every guard.  Confirmed on the CPU with the oracle's scores (f16, cosine): the 10th-to-32nd
    allowed score gap is 0.018 to 0.098 over the 16 queries, against a guard term of ~2^-10 for unit vectors in f16
    (planted copies score 0.99, the best allowed row 0.3 to 0.4)."""
    raw, q, allowed = _threshold_inputs()
    n, B, k = len(raw), len(q), 10
    idx = native.NativeIndex(raw.shape[1], "f16", "cosine")
    idx.add(raw)
    stored, qp = R.process_rows(raw, "cosine", "f16"), R.process_queries(q, "cosine")
    masks, mask_of = _pack(allowed), np.arange(B, dtype=np.int32)
    s_ref, r_ref = _oracle(stored, "f16", qp, k, allowed, mask_of)
    st0 = idx.stats()
    _check(*_singles(idx, q, k, masks, mask_of), s_ref, r_ref)
    st1 = idx.stats()
    single = {key: st1[key] - st0[key] for key in ("guard_failures", "exhaustive")}
    assert single == {"guard_failures": 0, "exhaustive": 0}
    s, r = idx.search_masks(q, k, masks, mask_of)
    st2 = idx.stats()
    _check(s, r, s_ref, r_ref)
    for key in single:
        assert st2[key] - st1[key] <= single[key], (key, st2[key] - st1[key])
    idx.close()


# ---------------------------------------------------------------- deletions
def test_deletions_inside_and_outside_the_masks(native):
    n, dim, B, k = 5_000, 64, 40, 10
    rng = np.random.default_rng(9)
    raw = R.gen_rows(4, 0, n, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(raw)
    pick = rng.choice(n, B, replace=False)
    q = (raw[pick] + 0.05 * rng.standard_normal((B, dim))).astype(np.float32)
    allowed = _mask_kinds(rng, n, 12)
    mask_of = (np.arange(B, dtype=np.int32) % 13) - 1
    gone = np.unique(np.concatenate([pick[::2], rng.choice(n, 700, replace=False), np.arange(96, 160)]))
    idx.remove(gone)
    live = np.ones(n, bool)
    live[gone] = False
    masks = _pack(allowed)
    s, r = idx.search_masks(q, k, masks, mask_of)
    assert not np.isin(r, gone).any()
    _check(s, r, *_oracle(R.process_rows(raw, "cosine", "bf16"), "bf16", R.process_queries(q, "cosine"), k, allowed,
                          mask_of, live=live))
    s_one, r_one = _singles(idx, q, k, masks, mask_of)
    np.testing.assert_array_equal(r, r_one)
    np.testing.assert_array_equal(s.view(np.uint32), s_one.view(np.uint32))
    idx.close()


# ---------------------------------------------------------------- guards fail: the grouped single-mask fallbacks
def test_fallback_route_on_a_duplicate_heavy_corpus(native):
    """200 rows within 1e-9 of each other (hostile_data.neardup): no guard certifies k of them, so every query aimed
    at the cluster leaves the main pass and the single-mask fallback answers it, once per distinct mask."""
    n, dim, B, k = 6_000, 128, 24, 10
    rows, pos, centre = H.corpus("neardup", 1, n, dim, "cosine", "bf16")
    q, _ = H.queries("neardup", 3, rows, B, "cosine", centre)
    q[::3] = centre  # every third query sits on the cluster, each with another mask
    rng = np.random.default_rng(2)
    allowed = rng.random((6, n)) < 0.5
    allowed[5] = True
    mask_of = (np.arange(B, dtype=np.int32) % 7) - 1
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    st0 = idx.stats()
    s, r = idx.search_masks(q, k, _pack(allowed), mask_of)
    st1 = idx.stats()
    _check(s, r, *_oracle(R.process_rows(rows, "cosine", "bf16"), "bf16", R.process_queries(q, "cosine"), k, allowed,
                          mask_of))
    assert st1["guard_failures"] > st0["guard_failures"]
    assert np.isin(r[0], pos).all()
    idx.close()


# ---------------------------------------------------------------- k beyond HR_MAX_K
def test_large_k_takes_the_exhaustive_pass_per_query(native):
    n, dim, B, k = 3_001, 64, 9, 200
    assert k > native.HR_MAX_K
    rng = np.random.default_rng(12)
    raw = R.gen_rows(6, 0, n, dim)
    idx = native.NativeIndex(dim, "f16", "cosine")
    idx.add(raw)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    allowed = _mask_kinds(rng, n, 6)
    mask_of = (np.arange(B, dtype=np.int32) % 7) - 1
    s, r = idx.search_masks(q, k, _pack(allowed), mask_of)
    _check(s, r, *_oracle(R.process_rows(raw, "cosine", "f16"), "f16", R.process_queries(q, "cosine"), k, allowed, mask_of))
    idx.close()


# ---------------------------------------------------------------- the device entry point
def test_device_entry_point_on_a_side_stream(native):
    torch = pytest.importorskip("torch")
    n, dim, B, k = 9_001, 96, 70, 10
    rng = np.random.default_rng(13)
    raw = R.gen_rows(8, 0, n, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(raw)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    allowed = _mask_kinds(rng, n, 10)
    mask_of = (np.arange(B, dtype=np.int32) % 11) - 1
    masks = _pack(allowed)
    s_host, r_host = idx.search_masks(q, k, masks, mask_of)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        q_d = torch.from_numpy(q).to(dev)
        m_d = torch.from_numpy(masks.view(np.int64)).to(dev)
        of_d = torch.from_numpy(mask_of).to(dev)
        s_d = torch.empty((B, k), dtype=torch.float32, device=dev)
        r_d = torch.empty((B, k), dtype=torch.int64, device=dev)
        idx.search_masks_device(q_d.data_ptr(), B, k, s_d.data_ptr(), r_d.data_ptr(), m_d.data_ptr(), masks.shape[0],
                                masks.shape[1], of_d.data_ptr(), stream=st.cuda_stream)
        s, r = s_d.cpu().numpy(), r_d.cpu().numpy()
    np.testing.assert_array_equal(r, r_host)
    np.testing.assert_array_equal(s.view(np.uint32), s_host.view(np.uint32))
    _check(s, r, *_oracle(R.process_rows(raw, "cosine", "bf16"), "bf16", R.process_queries(q, "cosine"), k, allowed, mask_of))
    idx.close()


# ---------------------------------------------------------------- errors
def test_errors(native):
    n, dim = 1_000, 64
    raw = R.gen_rows(2, 0, n, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(raw)
    q = raw[:4].copy()
    masks = _pack(np.ones((2, n), bool))
    for bad in ([0, 1, 2, 0], [0, -2, 1, 0]):
        with pytest.raises(ValueError):
            idx.search_masks(q, 5, masks, bad)
    with pytest.raises(ValueError):
        idx.search_masks(q, 5, masks, [0, 1, 0])  # one entry per query
    with pytest.raises(ValueError, match="row mask has 15 words"):
        idx.search_masks(q, 5, masks[:, :-1], [0, 1, 0, -1])
    with pytest.raises(ValueError):  # the library's own length check
        native._check(idx.lib.hr_index_search_masks(idx._h, native._ptr(q), 4, 5, native._ptr(masks), 2, 15,
                                                    native._ptr(np.zeros(4, np.int32)),
                                                    native._ptr(np.empty((4, 5), np.float32)),
                                                    native._ptr(np.empty((4, 5), np.int64))))
    idx.close()


def test_multi_device_handle_refuses_and_the_store_groups(native, tmp_path):
    from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig

    n, dim = 2_000, 64
    raw = R.gen_rows(5, 0, n, dim)
    nd = native.device_count()
    grp = native.NativeIndex(dim, "bf16", "cosine", devices=[i % nd for i in range(2)])
    grp.add(raw)
    with pytest.raises(NotImplementedError):
        grp.search_masks(raw[:3], 5, _pack(np.ones((1, n), bool)), [0, -1, 0])
    grp.close()
    cfg = VectorStoreConfig(backend="hip", collection_name="grp", persist_directory=str(tmp_path),
                            index_params={"dtype": "bf16", "persist": False, "devices": [i % nd for i in range(2)],
                                          "mixed_filters": True})
    store = HipVectorStore(cfg)
    store.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 250}", content=str(i), chunk_index=i % 250,
                                 metadata={"source": f"s{i // 250}"}, embedding=raw[i].tolist()) for i in range(n)])
    rng = np.random.default_rng(1)
    q = rng.standard_normal((20, dim)).astype(np.float32)
    flt = [None if i % 5 == 4 else {"source": f"s{i % 4}"} for i in range(20)]
    got = store.search_batch(q, 5, flt)
    assert store.mixed_launches == 0 and store.grouped_launches == 5
    stored, qp = R.process_rows(raw, "cosine", "bf16"), R.process_queries(q, "cosine")
    allowed = np.stack([np.arange(n) // 250 == d for d in range(4)])
    mask_of = np.array([-1 if f is None else int(f["source"][1:]) for f in flt], np.int32)
    s_ref, r_ref = _oracle(stored, "bf16", qp, 5, allowed, mask_of)
    assert [[c.id for c, _ in res] for res in got] == [[f"c{x}" for x in row] for row in r_ref]
    np.testing.assert_array_equal(np.array([[s for _, s in res] for res in got], np.float32), s_ref.astype(np.float32))
    store.close()


# ---------------------------------------------------------------- the store and the fused retriever
def _store(tmp_path, name, raw, **params):
    from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig

    cfg = VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path),
                            index_params={"dtype": "bf16", "persist": False, **params})
    store = HipVectorStore(cfg)
    store.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 500}", content=f"text {i}", chunk_index=i % 500,
                                 metadata={"source": f"s{i // 500}"}, embedding=raw[i].tolist())
                           for i in range(len(raw))])
    return store


def test_store_with_mixed_filters(native, tmp_path):
    """64 concurrent search calls, 8 source filters and None, differing top_k: the sequential calls' results, one
    per-query-mask launch for the one 64-query chunk; the same store without the option gives the same results."""
    n, dim = 4_000, 64
    raw = R.gen_rows(9, 0, n, dim)
    rng = np.random.default_rng(3)
    q = (raw[rng.choice(n, 64, replace=False)] + 0.2 * rng.standard_normal((64, dim))).astype(np.float32)
    flt = [None if i % 9 == 8 else {"source": f"s{i % 9}"} for i in range(64)]
    ks = [3 + i % 6 for i in range(64)]
    on = _store(tmp_path, "on", raw, mixed_filters=True)
    off = _store(tmp_path, "off", raw)

    def concurrent(store):
        async def go():
            return await asyncio.gather(*[store.search(query_embedding=q[i].tolist(), top_k=ks[i], filters=flt[i])
                                          for i in range(64)])
        return asyncio.run(go())

    want = [asyncio.run(off.search(query_embedding=q[i].tolist(), top_k=ks[i], filters=flt[i])) for i in range(64)]
    launches = on._index.qmask_launches()
    got = concurrent(on)
    assert on._index.qmask_launches() == launches + 1 and on._batcher.launches == 1
    ident = lambda res: [[(c.id, s) for c, s in r] for r in res]  # noqa: E731
    assert ident(got) == ident(want)
    assert [len(r) for r in got] == ks
    assert ident(concurrent(off)) == ident(want) and off._index.qmask_launches() == 0 and off._batcher.launches >= 9 + 64
    on.close()
    off.close()


def test_fused_retriever_keeps_filtered_calls_in_the_cohort(native, tmp_path):
    """Concurrent filtered retrieve() calls on a mixed_filters store: one cohort, one per-query-mask search on the
    device queries; results equal the unfused path's (rank before threshold)."""
    torch = pytest.importorskip("torch")
    import threading

    from hiprag.rag import RetrieverConfig, VectorRetriever

    n, dim = 4_000, 64
    raw = R.gen_rows(10, 0, n, dim)
    rng = np.random.default_rng(4)
    names = [f"q{i}" for i in range(40)]
    table = {nm: (raw[rng.integers(n)] + 0.2 * rng.standard_normal(dim)).astype(np.float32) for nm in names}

    class Emb:  # the in-process embedder's surface the fused path needs
        batch_size, fused_retrieve, _fwd_lock = 64, True, threading.Lock()

        async def embed_query(self, text):
            return table[text].tolist()

        def encode_queries(self, texts):
            return torch.from_numpy(np.stack([table[t] for t in texts])).to("cuda:0")

    store = _store(tmp_path, "fused", raw, mixed_filters=True)
    flt = [None if i % 5 == 4 else {"source": f"s{i % 4}"} for i in range(40)]
    cfg = RetrieverConfig(top_k=5, similarity_threshold=0.3)
    fused = VectorRetriever(store, Emb(), cfg)
    assert fused._fused is not None

    class Plain(Emb):
        fused_retrieve = False

    plain = VectorRetriever(store, Plain(), cfg)
    assert plain._fused is None
    want = [asyncio.run(plain.retrieve(nm, top_k=3 + i % 4, filters=flt[i])) for i, nm in enumerate(names)]
    launches, mixed = store._index.qmask_launches(), store.mixed_launches

    async def go():
        return await asyncio.gather(*[fused.retrieve(nm, top_k=3 + i % 4, filters=flt[i]) for i, nm in enumerate(names)])

    got = asyncio.run(go())
    ident = lambda res: [[(r.chunk.id, r.score, r.rank) for r in x] for x in res]  # noqa: E731
    assert ident(got) == ident(want)
    assert store.mixed_launches == mixed + 1 and store._index.qmask_launches() == launches + 1
    fused._fused.close()  # (the worker counts a cohort after it has posted its results)
    assert fused._fused.cohorts == 1 and fused._fused.queries == 40
    store.close()
