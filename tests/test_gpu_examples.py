"""GPU: search by example (hr_examples.hip) against tests/examples_ref.py -- the built query as the
ordered float64 sum cast once, then the oracle's exact top-k over the allowed rows minus the query's own examples.
Built queries equal as fp32 bit patterns; rows equal and scores equal as fp32 bit patterns: every dtype and metric, row
counts at the tile and wave edges, examples at the tile edges, long rows, lists of 0 to 32 examples in one batch,
duplicates, cancelling weights, deletes and masks, k + M on both sides of HR_MAX_K, the device entry points, the errors,
and the store and retriever on a real index."""
import asyncio

import numpy as np
import pytest

import oracle
from examples_ref import assert_same, assert_same_bits, build_ref, examples_ref
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 2, 31, 32, 33, 64, 65, 1000, 4099]
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


def _build(native, x, dtype="bf16", metric="cosine"):
    idx = native.NativeIndex(x.shape[1], dtype, metric)
    idx.add(x)
    return idx, R.process_rows(x, metric, dtype)


def _dup_rows(rng, n, dim=64, spread=0.5):
    """Near-duplicate runs of 2..7 rows: unit(centre of the run + spread * unit noise)."""
    run_of, runs = [], 0
    while len(run_of) < n:
        run_of += [runs] * int(rng.integers(2, 8))
        runs += 1
    run_of = np.asarray(run_of[:n])
    centres = _unit(rng.standard_normal((runs, dim)).astype(np.float32))
    return _unit(centres[run_of] + spread * _unit(rng.standard_normal((n, dim)).astype(np.float32)))


def _weights(rng, examples):
    """fp32 weights of mixed sign, none of them zero."""
    return [[np.float32(v) for v in rng.uniform(0.2, 1.5, len(e)) * rng.choice([-1.0, 1.0, 1.0], len(e))]
            for e in examples]


def _lists(rng, n, B, m_max=3):
    """B example lists of 1..m_max distinct rows of an n-row index."""
    return [rng.choice(n, min(n, 1 + b % m_max), replace=False).tolist() for b in range(B)]


# ---------------------------------------------------------------- the builder alone
@pytest.mark.parametrize("dtype,dim", [("f32", 64), ("bf16", 64), ("f16", 64), ("bf16", 100), ("f32", 100),
                                       ("f16", 1024), ("f32", 1024), ("bf16", 2048), ("f32", 2048)])
def test_build_queries_bits(native, dtype, dim):
    """Rows 0, 31, 32, 33 and n - 1, two examples of one tile, one row twice, lists of 0 (base only), 1, 7 and 32
    examples in one batch, weights of mixed sign, with and without base vectors, before and after deletes."""
    rng = np.random.default_rng(dim + DTYPES.index(dtype))
    n = 203
    metric = "cosine" if dim in (64, 2048) else "ip"
    x = _dup_rows(rng, n, dim) * (1.0 if metric == "cosine" else rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
    idx, stored = _build(native, x, dtype, metric)
    ex = [[0], [31, 32], [33, n - 1], [40, 41], [5, 5], [], rng.choice(n, 7, replace=False).tolist(),
          rng.choice(n, 32, replace=False).tolist(), [n - 1, 0, 31]]
    w = _weights(rng, ex)
    q = rng.standard_normal((len(ex), dim)).astype(np.float32)
    q[0, :3] = [-0.0, 0.0, -0.0]
    for round_ in range(2):
        assert_same_bits(idx.build_queries(ex, w, q), build_ref(stored, dtype, ex, w, q))
        some = [e for e in ex if e]
        w_some = [v for v in w if v]
        assert_same_bits(idx.build_queries(some, w_some), build_ref(stored, dtype, some, w_some))
        assert_same_bits(idx.build_queries(some), build_ref(stored, dtype, some))  # default weights 1 / m
        one = idx.build_queries([[n - 1]], [[1.0]])  # weight 1: the stored row itself
        assert_same_bits(one, idx.get_rows([n - 1]) + np.float32(0.0))  # (0.0 + x: a stored -0.0 comes out +0.0)
        used = {r for e in ex for r in e}
        idx.remove([r for r in range(n) if r not in used][: 20 + 20 * round_])  # deletes elsewhere change nothing
    assert_same_bits(idx.build_queries([[]], q=q[:1]), q[:1])  # no example: the base vector's own bits, -0.0 kept
    idx.close()


# ---------------------------------------------------------------- the whole search
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_row_counts_dtypes_metrics(native, dtype, metric):
    """Every row count at a tile / wave edge, k = 1 and 10: n < k + M pads; default and mixed-sign weights."""
    rng = np.random.default_rng(10 * DTYPES.index(dtype) + METRICS.index(metric))
    dropped = 0
    for n in ROW_COUNTS:
        x = _dup_rows(rng, n) * (1.0 if metric == "cosine" else rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
        idx, stored = _build(native, x, dtype, metric)
        ex = _lists(rng, n, 3)
        for k in (1, 10):
            for w in (None, _weights(rng, ex)):
                got = idx.search_examples(ex, k, w)
                assert_same(got, examples_ref(stored, dtype, ex, k, w, metric=metric))
                for b in range(3):
                    assert not np.isin(got[1][b], ex[b]).any()
                if w is None and n >= 1000:
                    kept = idx.search_examples(ex, k, keep=True)[1]
                    dropped += int(sum(np.isin(kept[b], ex[b]).any() for b in range(3)))
        idx.close()
    assert dropped >= 4  # a single positive example is its own best match: the drop had something to do


@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2"), ("f16", "ip")])
def test_keep_is_the_plain_search_of_the_stored_row(native, dtype, metric):
    rng = np.random.default_rng(1)
    x = _dup_rows(rng, 1000)
    idx, stored = _build(native, x, dtype, metric)
    rows = [0, 33, 999]
    for k in (1, 10, 128):
        for r in rows:
            s0, r0 = idx.search(idx.get_rows([r]) + np.float32(0.0), k)
            assert_same(idx.search_examples([[r]], k, [[1.0]], keep=True), (s0, r0))
            if k < 128:
                s1, r1 = idx.search(idx.get_rows([r]) + np.float32(0.0), k + 1)
                stay = r1[0] != r
                assert (~stay).sum() == 1  # a stored row is among its own k + 1 best
                assert_same(idx.search_examples([[r]], k, [[1.0]]), (s1[:, stay], r1[:, stay]))
    idx.close()


def test_a_far_negative_example_drops_nothing(native):
    rng = np.random.default_rng(2)
    x = _dup_rows(rng, 1000)
    idx, stored = _build(native, x)
    q = (x[[10, 500]] + 0.05 * _unit(rng.standard_normal((2, 64)).astype(np.float32))).astype(np.float32)
    far = [int(np.argmin(x @ q[b])) for b in range(2)]  # the row least like the query, as a weak negative
    ex, w = [[far[0]], [far[1]]], [[-0.05], [-0.05]]
    got = idx.search_examples(ex, 10, w, q)
    assert_same(got, examples_ref(stored, "bf16", ex, 10, w, q))
    assert_same(got, idx.search_examples(ex, 10, w, q, keep=True))  # nothing in the way: the first k of the k + 1
    idx.close()


def test_exact_copies_of_the_example_stay_in_row_order(native):
    rng = np.random.default_rng(3)
    x = _dup_rows(rng, 500)
    x[200:241] = x[200]  # the example and 40 exact copies of it
    for dtype, metric in (("bf16", "cosine"), ("f32", "ip")):
        idx, stored = _build(native, x, dtype, metric)
        got = idx.search_examples([[200]], 45)
        assert_same(got, examples_ref(stored, dtype, [[200]], 45, metric=metric))
        assert got[1][0, :40].tolist() == list(range(201, 241))  # equal scores: rows ascending, only row 200 left
        assert len(set(got[0][0, :40].tolist())) == 1
        idx.close()


def test_weights_that_cancel_give_the_zero_query(native):
    rng = np.random.default_rng(4)
    x = _dup_rows(rng, 300)
    for dtype, metric in (("bf16", "cosine"), ("f32", "ip")):
        idx, stored = _build(native, x, dtype, metric)
        ex, w = [[7, 7], [3, 100, 3, 100]], [[1.0, -1.0], [0.5, 0.25, -0.5, -0.25]]
        assert not idx.build_queries(ex, w).any()
        got = idx.search_examples(ex, 10, w)
        assert_same(got, examples_ref(stored, dtype, ex, 10, w, metric=metric))
        assert got[1][0].tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10] and not got[0].any()  # score 0: rows ascending
        assert got[1][1].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]
        idx.close()


def test_masks_and_deletes(native):
    rng = np.random.default_rng(5)
    n = 500
    x = _dup_rows(rng, n)
    idx, stored = _build(native, x)
    ex = [[250], [260, 261], [270, 100]]
    w = [[1.0], [0.5, 0.5], [1.0, -0.3]]
    allowed = np.ones(n, bool)
    allowed[[250, 260, 100]] = False  # a row the mask forbids is still a legal example
    allowed[::7] = False
    got = idx.search_examples(ex, 10, w, mask=oracle.mask_from_bool(allowed))
    assert_same(got, examples_ref(stored, "bf16", ex, 10, w, allowed=allowed))
    assert allowed[got[1]].all()
    live = np.ones(n, bool)
    gone = np.unique(idx.search_examples(ex, 10, w)[1][:, :2])  # every query's two best go
    idx.remove(gone)
    live[gone] = False
    got = idx.search_examples(ex, 10, w)
    assert_same(got, examples_ref(stored, "bf16", ex, 10, w, allowed=live))
    assert not np.isin(got[1], gone).any()
    got = idx.search_examples(ex, 10, w, mask=oracle.mask_from_bool(allowed))
    assert_same(got, examples_ref(stored, "bf16", ex, 10, w, allowed=allowed & live))
    few = np.zeros(n, bool)  # a mask that leaves fewer than k rows, one of them an example
    few[[7, 8, 9, 261]] = True
    s, r = idx.search_examples(ex, 10, w, mask=oracle.mask_from_bool(few))
    assert_same((s, r), examples_ref(stored, "bf16", ex, 10, w, allowed=few & live))
    assert (np.sort(r[1, :3]) == [7, 8, 9]).all() and (r[1, 3:] == -1).all() and np.isneginf(s[1, 3:]).all()
    assert (np.sort(r[0, :4]) == [7, 8, 9, 261]).all()
    idx.close()


@pytest.mark.parametrize("B", [1, 3, 64, 65, 130])
def test_batch_sizes(native, B):
    rng = np.random.default_rng(B)
    x = _dup_rows(rng, 2000)
    idx, stored = _build(native, x)
    ex = _lists(rng, 2000, B, 4)
    w = _weights(rng, ex)
    q = 0.3 * _unit(rng.standard_normal((B, 64)).astype(np.float32))
    assert_same(idx.search_examples(ex, 10, w, q), examples_ref(stored, "bf16", ex, 10, w, q))
    idx.close()


def test_k_plus_m_on_both_sides_of_the_largest_k(native):
    """k = 120 with M = 8 (K' = 128: the scan path at its largest k), k = 120 with M = 16 (K' = 136: the exhaustive
    pass), and k = 128 with keep (K' = 128), on 1000 rows."""
    rng = np.random.default_rng(6)
    x = _dup_rows(rng, 1000)
    idx, stored = _build(native, x)
    before = idx.stats()["exhaustive"] if hasattr(idx, "stats") else None
    for k, m, keep in ((120, 8, False), (120, 16, False), (128, 16, True), (128, 1, False)):
        ex = [rng.choice(1000, m, replace=False).tolist(), rng.choice(1000, max(1, m // 2), replace=False).tolist()]
        got = idx.search_examples(ex, k, keep=keep)
        assert_same(got, examples_ref(stored, "bf16", ex, k, keep=keep))
        assert (got[1] >= 0).all()
    if before is not None:
        assert idx.stats()["exhaustive"] - before == 4  # K' = 136 and 129: two queries each
    idx.close()


def test_device_entry_points(native):
    import torch

    rng = np.random.default_rng(7)
    n = 300
    x = _dup_rows(rng, n)
    idx, stored = _build(native, x)
    ex = [[1], [33, 34, 35], [], [299, 0], [7, 7]]
    w = _weights(rng, ex)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)  # a non-default stream
    allowed = np.ones(n, bool)
    allowed[::3] = False
    with torch.cuda.stream(stream):
        qd = torch.from_numpy(q).to(dev)
        md = torch.from_numpy(oracle.mask_from_bool(allowed).view(np.int64)).to(dev)
        built = torch.empty((5, 64), dtype=torch.float32, device=dev)
        s = torch.empty((5, 7), dtype=torch.float32, device=dev)
        r = torch.empty((5, 7), dtype=torch.int64, device=dev)
        idx.build_queries_device(ex, built.data_ptr(), w, q_ptr=qd.data_ptr(), stream=stream.cuda_stream)
        assert_same_bits(built.cpu().numpy(), build_ref(stored, "bf16", ex, w, q))
        # the built queries feed any device search: the plain one is the keep form
        idx.search_device(built.data_ptr(), 5, 7, s.data_ptr(), r.data_ptr(), stream=stream.cuda_stream)
        assert_same((s.cpu().numpy(), r.cpu().numpy()), idx.search_examples(ex, 7, w, q, keep=True))
        for mask, ok in ((0, None), (md.data_ptr(), allowed)):
            idx.search_examples_device(ex, 7, s.data_ptr(), r.data_ptr(), w, q_ptr=qd.data_ptr(), mask_ptr=mask,
                                       stream=stream.cuda_stream)
            got = (s.cpu().numpy(), r.cpu().numpy())
            assert_same(got, examples_ref(stored, "bf16", ex, 7, w, q, ok))
            assert_same(got, idx.search_examples(ex, 7, w, q, mask=None if ok is None else oracle.mask_from_bool(ok)))
        some = [e for e in ex if e]
        idx.build_queries_device(some, built.data_ptr(), stream=stream.cuda_stream)  # no base vectors
        assert_same_bits(built.cpu().numpy()[:4], build_ref(stored, "bf16", some))
        idx.search_examples_device(some, 7, s.data_ptr(), r.data_ptr(), keep=True, stream=stream.cuda_stream)
        assert_same((s.cpu().numpy()[:4], r.cpu().numpy()[:4]), examples_ref(stored, "bf16", some, 7, keep=True))
    idx.close()


def test_errors_leave_the_handle_working(native):
    rng = np.random.default_rng(8)
    n = 100
    x = _dup_rows(rng, n)
    idx, stored = _build(native, x)
    idx.remove([50])
    q = rng.standard_normal((1, 64)).astype(np.float32)
    bad = [dict(examples=[[50]]),  # a removed example
           dict(examples=[[n]]), dict(examples=[[-1]]),  # out of range
           dict(examples=[[1]], weights=[[float("nan")]]), dict(examples=[[1]], weights=[[float("inf")]]),
           dict(examples=[[]]),  # no example and no base vector
           dict(examples=[list(range(33))])]  # m_b = 33
    for kw in bad:
        with pytest.raises(ValueError):
            idx.search_examples(k=5, **kw)
        with pytest.raises(ValueError):
            idx.build_queries(**kw)
    with pytest.raises(ValueError):
        idx.search_examples([[1], [50]], 5)  # one bad list fails the batch
    with pytest.raises(ValueError):
        idx.search_examples([[1]], 0)
    with pytest.raises(ValueError):
        idx.search_examples([[1]], 5, q=np.zeros((2, 64), np.float32))
    live = np.ones(n, bool)
    live[50] = False
    full = [list(range(32))]
    assert_same(idx.search_examples(full, 5), examples_ref(stored, "bf16", full, 5, allowed=live))
    assert_same(idx.search_examples([[]], 5, q=q), examples_ref(stored, "bf16", [[]], 5, q=q, allowed=live))
    s0, r0 = idx.search(q, 5)  # the handle still answers a plain search
    ws, wr = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 5, oracle.mask_from_bool(live), nthreads=2)
    assert_same((s0, r0), (ws.astype(np.float32), wr))
    idx.remove(np.arange(n))  # an empty index pads (only a base vector passes the checks)
    s, r = idx.search_examples([[]], 3, q=q)
    assert (r == -1).all() and np.isneginf(s).all()
    idx.close()
    two = native.NativeIndex(64, "bf16", "cosine", devices=[0, 0])  # a multi-device handle is out of scope
    two.add(x)
    with pytest.raises(NotImplementedError):
        two.search_examples([[1]], 5)
    with pytest.raises(NotImplementedError):
        two.build_queries([[1]])
    assert (two.search(q, 5)[1] >= 0).all()
    two.close()


# ---------------------------------------------------------------- the store and the retriever
def _corpus(n=240):
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


def _want(x, ex, w, k, q=None, allowed=None):
    s, r = examples_ref(R.process_rows(x, "cosine", "bf16"), "bf16", ex, k, w, q, allowed)
    return [[(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0] for b in range(len(ex))]


def _ids(res):
    return [[(c.id, s) for c, s in hits] for hits in res]


def test_store_search_similar(native, tmp_path):
    from hash_embed import vec

    chunks, x = _corpus()
    store = _store(tmp_path, "kb")
    asyncio.run(store.add_chunks(chunks))
    third, half = np.float32(np.float64(1.0) / 3), np.float32(0.5)
    got = _ids(store.search_similar_batch([["c8", "c9", "c10"], "c40"], top_k=6))
    assert got == _want(x, [[8, 9, 10], [40]], [[third] * 3, [1.0]], 6)
    assert {cid for cid, _ in got[0][:5]} == {"c11", "c12", "c13", "c14", "c15"}  # the rest of document 1
    neg = _ids(store.search_similar_batch([["c8", "c9"]], [["c16", "c24"]], top_k=6, neg_weight=0.5))
    assert neg == _want(x, [[8, 9, 16, 24]], [[half, half, np.float32(-0.25), np.float32(-0.25)]], 6)
    assert not {"c8", "c9", "c16", "c24"} & {cid for cid, _ in neg[0]}
    part = np.arange(len(chunks)) % 3
    flt = _ids(store.search_similar_batch(["c8"], top_k=5, filters={"part": 1}))
    assert flt == _want(x, [[8]], [[1.0]], 5, allowed=part == 1) and part[8] != 1
    qv = vec("query: what is in document 3")
    one = asyncio.run(store.search_similar(["c24", "c25"], 5, negative_ids=["c0"], query_embedding=qv.tolist()))
    assert _ids([one]) == _want(x, [[24, 25, 0]], [[half, half, np.float32(-1.0)]], 5, qv[None])
    with pytest.raises(ValueError, match="'nope'"):
        store.search_similar_batch([["c8", "nope"]])
    store.close()


def test_ivf_store_composes_on_the_host(native, tmp_path):
    """IVF_FLAT has no native search_examples: get_rows, the float64 sum, its own search at k + M, the drop."""
    from hiprag.rag.storage import search_examples_host

    chunks, x = _corpus()
    store = _store(tmp_path, "kb_ivf", index_type="IVF_FLAT", nlist=4, nprobe=4, ivf_train_rows=64, ivf_seed=1)
    asyncio.run(store.add_chunks(chunks))
    assert store._index.trained and not hasattr(store._index, "search_examples")
    got = store.search_similar_batch([["c8", "c9"]], top_k=6)
    s, r = search_examples_host(store._index, [[8, 9]], 6, [[np.float32(0.5)] * 2])
    assert _ids(got) == [[(f"c{row}", float(sc)) for sc, row in zip(s[0], r[0])]]
    assert _ids(got) == _want(x, [[8, 9]], [[0.5, 0.5]], 6)  # (every list probed: the exact answer)
    store.close()


def test_retrieve_similar_with_a_threshold(native, tmp_path):
    from hash_embed import HashEmbedder
    from hiprag.rag import RetrieverConfig
    from hiprag.rag.retriever import VectorRetriever

    chunks, x = _corpus()
    store = _store(tmp_path, "kb_r")
    asyncio.run(store.add_chunks(chunks))
    full = _want(x, [[8]], [[1.0]], 12)[0]
    th = (full[6][1] + full[7][1]) / 2  # between document 1's passages and everything else
    assert full[6][1] > th > full[7][1]
    ret = VectorRetriever(store, HashEmbedder(), RetrieverConfig(top_k=12, similarity_threshold=th))
    res = asyncio.run(ret.retrieve_similar("c8"))
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(full[:7])]
    assert {r.chunk.id for r in res} == {f"c{i}" for i in range(9, 16)}
    emb = HashEmbedder()
    qv = np.asarray(asyncio.run(emb.embed_query("passage")), np.float32)
    ret0 = VectorRetriever(store, emb, RetrieverConfig(top_k=4, similarity_threshold=0.0))
    res = asyncio.run(ret0.retrieve_similar(["c8", "c9"], negative_ids=["c100"], query="passage"))
    w = _want(x, [[8, 9, 100]], [[0.5, 0.5, -1.0]], 4, qv[None])[0]
    assert [(r.chunk.id, r.score, r.rank) for r in res] == [(cid, sc, i + 1) for i, (cid, sc) in enumerate(w)]
    store.close()
