"""GPU: MMR search (hr_mmr.hip) against tests/mmr_ref.py -- the oracle's exact top-P pool, the pool's
canonical similarities with the selected row in the query role, and the greedy loop in float64.  Rows equal, scores
equal as fp32 bit patterns: every dtype and metric, row counts at the tile and wave edges, pools larger than the
corpus, the largest register and LDS form, exact duplicates, a zero row, deletes and masks, the device entry point,
batch sizes, and the store."""
import asyncio
import os

import numpy as np
import pytest

import oracle
from mmr_ref import assert_same, mmr_ref
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


def _planted(rng, x, B, noise=0.05):
    pick = rng.choice(len(x), B, replace=len(x) < B)
    e = rng.standard_normal((B, x.shape[1])).astype(np.float32)
    return (_unit(x[pick]) + noise * _unit(e)).astype(np.float32)


def _ref(stored, dtype, metric, q, k, lam, fetch_k=0, allowed=None):
    return mmr_ref(stored, dtype, R.process_queries(q, metric), k, lam, fetch_k, allowed, metric)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_row_counts_dtypes_metrics(native, dtype, metric):
    """Every row count at a tile / wave edge; pools of k, 32, 128 rows and the default: fetch_k > n, padded pools and
    k > n among them; lambda 0, 0.3, 0.5, 1."""
    rng = np.random.default_rng(10 * DTYPES.index(dtype) + METRICS.index(metric))
    differs = 0
    for n in ROW_COUNTS:
        x = _dup_rows(rng, n) * (1.0 if metric == "cosine" else rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
        idx, stored = _build(native, x, dtype, metric)
        q = _planted(rng, x, 3)
        for k in (1, 10):
            plain = idx.search(q, min(k, n))[1]
            for fetch_k in (k, 32, 128, 0):
                for lam in (0.0, 0.3, 0.5, 1.0):
                    got = idx.search_mmr(q, k, lam, fetch_k=fetch_k)
                    assert_same(got, _ref(stored, dtype, metric, q, k, lam, fetch_k))
                    if n >= 1000 and k == 10 and fetch_k == 32 and lam == 0.5:
                        differs += int((got[1] != plain).any(axis=1).sum())
        idx.close()
    assert differs == 6  # the penalty changed every query's list at n = 1000 and 4099


def test_lambda_one_is_the_plain_search(native):
    rng = np.random.default_rng(1)
    x = _dup_rows(rng, 1000)
    for dtype, metric in (("bf16", "cosine"), ("f32", "l2")):
        idx, _ = _build(native, x, dtype, metric)
        q = _planted(rng, x, 5)
        for k, fetch_k in ((10, 0), (10, 10), (128, 128), (1, 32)):
            s0, r0 = idx.search(q, k)
            s1, r1 = idx.search_mmr(q, k, 1.0, fetch_k=fetch_k)
            np.testing.assert_array_equal(r1, r0)
            np.testing.assert_array_equal(s1.view(np.uint32), s0.view(np.uint32))
        idx.close()


def test_prefix_stability(native):
    rng = np.random.default_rng(2)
    x = _dup_rows(rng, 1000)
    idx, stored = _build(native, x)
    q = _planted(rng, x, 4)
    for fetch_k in (32, 128):
        s20, r20 = idx.search_mmr(q, 20, 0.5, fetch_k=fetch_k)
        s5, r5 = idx.search_mmr(q, 5, 0.5, fetch_k=fetch_k)
        np.testing.assert_array_equal(r5, r20[:, :5])
        np.testing.assert_array_equal(s5.view(np.uint32), s20[:, :5].view(np.uint32))
        assert_same((s20, r20), _ref(stored, "bf16", "cosine", q, 20, 0.5, fetch_k))


@pytest.mark.parametrize("dim,dtype", [(100, "bf16"), (100, "f32"), (1024, "bf16"), (1024, "f32"), (2048, "bf16"),
                                       (2048, "f32")])
def test_dims_and_the_largest_form(native, dim, dtype):
    """dim 100 (no multiple of 64), 1024 and 2048 at k = fetch_k = 128 on 4099 rows: 127 rounds over 128 candidates,
    16 waves, the longest rows in LDS."""
    rng = np.random.default_rng(dim)
    x = _dup_rows(rng, 4099, dim)
    metric = "l2" if dim == 100 else "cosine"
    idx, stored = _build(native, x, dtype, metric)
    q = _planted(rng, x, 2)
    assert_same(idx.search_mmr(q, 128, 0.5, fetch_k=128), _ref(stored, dtype, metric, q, 128, 0.5, 128))
    assert_same(idx.search_mmr(q, 10, 0.3), _ref(stored, dtype, metric, q, 10, 0.3))
    idx.close()


def test_exact_duplicates_break_ties_by_pool_position(native):
    rng = np.random.default_rng(3)
    x = _dup_rows(rng, 500)
    x[200:240] = x[200]  # 40 identical rows
    idx, stored = _build(native, x, "f32", "ip")
    q = np.concatenate([x[200:201] + 0.01 * _unit(rng.standard_normal((1, 64)).astype(np.float32)), _planted(rng, x, 2)])
    for k, fetch_k, lam in ((10, 32, 0.5), (64, 64, 0.5), (20, 128, 0.0), (20, 128, 0.9)):
        got = idx.search_mmr(q, k, lam, fetch_k=fetch_k)
        assert_same(got, _ref(stored, "f32", "ip", q, k, lam, fetch_k))
    s, r = idx.search_mmr(q[:1], 64, 0.5, fetch_k=64)
    dup = [int(v) for v in r[0] if 200 <= v < 240]
    assert len(dup) >= 30 and dup == sorted(dup)  # equal in every term: they come out in pool order (row ascending)
    idx.close()


def test_golden_duplicate_block(native, golden_dir):
    d = np.load(os.path.join(golden_dir, "ties.npz"))
    corpus = R.gen_rows(7, 0, 20000, 256)
    for s_, dst in zip(d["dup_src"], d["dup_dst"]):
        corpus[dst] = corpus[s_]
    idx, stored = _build(native, corpus)
    q = np.asarray(d["queries"], np.float32)[:4]
    for k, fetch_k, lam in ((10, 32, 0.5), (20, 128, 0.3)):
        assert_same(idx.search_mmr(q, k, lam, fetch_k=fetch_k), _ref(stored, "bf16", "cosine", q, k, lam, fetch_k))
    idx.close()


def test_zero_row_under_cosine(native):
    rng = np.random.default_rng(4)
    x = _dup_rows(rng, 40)
    x[5] = 0.0  # stays zero through the normalisation: score 0 against everything
    for dtype in DTYPES:
        idx, stored = _build(native, x, dtype)
        q = _planted(rng, x[6:], 3)
        for lam in (0.0, 0.5):
            got = idx.search_mmr(q, 40, lam, fetch_k=64)
            assert_same(got, _ref(stored, dtype, "cosine", q, 40, lam, 64))
            assert (np.sort(got[1], axis=1) == np.arange(40)).all()
        idx.close()


def test_deletes_and_masks(native):
    rng = np.random.default_rng(5)
    n = 500
    x = _dup_rows(rng, n)
    idx, stored = _build(native, x)
    q = _planted(rng, x[200:], 3)  # (their first picks lie beyond the rows the last mask below names)
    live = np.ones(n, bool)
    top = idx.search_mmr(q, 10, 0.5)[1]
    assert (top[:, 0] >= 200).all()
    idx.remove(top[:, 0])  # every query's first pick goes
    live[top[:, 0]] = False
    got = idx.search_mmr(q, 10, 0.5)
    assert_same(got, _ref(stored, "bf16", "cosine", q, 10, 0.5, 0, live))
    assert not np.isin(got[1], top[:, 0]).any()
    allowed = live.copy()
    allowed[got[1][0, 1]] = False
    allowed[300:] = False
    for fetch_k in (0, 10):
        assert_same(idx.search_mmr(q, 10, 0.5, mask=oracle.mask_from_bool(allowed), fetch_k=fetch_k),
                    _ref(stored, "bf16", "cosine", q, 10, 0.5, fetch_k, allowed))
    few = np.zeros(n, bool)  # a mask that leaves fewer than k rows
    few[[7, 8, 9, 100, int(top[0, 0])]] = True
    s, r = idx.search_mmr(q, 10, 0.5, mask=oracle.mask_from_bool(few))
    assert_same((s, r), _ref(stored, "bf16", "cosine", q, 10, 0.5, 0, few & live))
    assert (np.sort(r[:, :4], axis=1) == [7, 8, 9, 100]).all() and (r[:, 4:] == -1).all() and np.isneginf(s[:, 4:]).all()
    idx.remove(np.arange(n))  # an empty index pads
    s, r = idx.search_mmr(q, 3, 0.5)
    assert (r == -1).all() and np.isneginf(s).all()
    idx.close()


def test_device_entry_point_and_errors(native):
    import torch

    rng = np.random.default_rng(6)
    x = _dup_rows(rng, 300)
    idx, stored = _build(native, x)
    q = _planted(rng, x, 5)
    for bad in (dict(k=0, lam=0.5), dict(k=129, lam=0.5), dict(k=10, lam=0.5, fetch_k=9),
                dict(k=10, lam=0.5, fetch_k=129), dict(k=5, lam=-0.01), dict(k=5, lam=1.01), dict(k=5, lam=float("nan"))):
        with pytest.raises(ValueError):
            idx.search_mmr(q, **bad)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)  # a non-default stream
    allowed = np.ones(300, bool)
    allowed[::3] = False
    with torch.cuda.stream(stream):
        qd = torch.from_numpy(q).to(dev)
        md = torch.from_numpy(oracle.mask_from_bool(allowed).view(np.int64)).to(dev)
        s = torch.empty((5, 7), dtype=torch.float32, device=dev)
        r = torch.empty((5, 7), dtype=torch.int64, device=dev)
        for fetch_k, mask, ok in ((0, 0, None), (7, 0, None), (32, md.data_ptr(), allowed)):
            idx.search_mmr_device(qd.data_ptr(), 5, 7, 0.5, s.data_ptr(), r.data_ptr(), mask_ptr=mask, fetch_k=fetch_k,
                                  stream=stream.cuda_stream)
            got = (s.cpu().numpy(), r.cpu().numpy())
            assert_same(got, _ref(stored, "bf16", "cosine", q, 7, 0.5, fetch_k, ok))
            assert_same(got, idx.search_mmr(q, 7, 0.5, fetch_k=fetch_k,
                                            mask=None if ok is None else oracle.mask_from_bool(ok)))
        with pytest.raises(ValueError):
            idx.search_mmr_device(qd.data_ptr(), 5, 7, 2.0, s.data_ptr(), r.data_ptr(), stream=stream.cuda_stream)
    idx.set_mmr_timing(True)
    idx.search_mmr(q, 7, 0.5)
    ms = idx.mmr_last_ms()
    assert ms["probe_ms"] > 0.0 and ms["select_ms"] > 0.0
    idx.close()
    two = native.NativeIndex(64, "bf16", "cosine", devices=[0, 0])  # a multi-device handle is out of scope
    two.add(x)
    with pytest.raises(NotImplementedError):
        two.search_mmr(q, 5, 0.5)
    two.close()


@pytest.mark.parametrize("B", [1, 70])
def test_batch_sizes(native, B):
    rng = np.random.default_rng(B)
    x = _dup_rows(rng, 2000)
    idx, stored = _build(native, x)
    q = _planted(rng, x, B)
    assert_same(idx.search_mmr(q, 10, 0.5), _ref(stored, "bf16", "cosine", q, 10, 0.5))
    idx.close()


# ---------------------------------------------------------------- the store
def _chunks(rng, n=400, dim=64):
    from hiprag.rag import Chunk

    x = _dup_rows(rng, n, dim)
    return [Chunk(id=f"c{i}", document_id=f"d{i // 7}", content=f"text {i}", chunk_index=i, metadata={"part": i % 3},
                  embedding=x[i].tolist()) for i in range(n)], x


def _store(tmp_path, name, **kw):
    from hiprag.rag import HipVectorStore, VectorStoreConfig

    index_type = kw.pop("index_type", None)
    return HipVectorStore(VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                                            index_type=index_type,
                                            index_params={"dtype": "bf16", "fsync": False, **kw}))


def _want(x, q, k, lam, fetch_k=0, allowed=None):
    s, r = _ref(R.process_rows(x, "cosine", "bf16"), "bf16", "cosine", np.asarray(q, np.float32), k, lam, fetch_k, allowed)
    return [[(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0] for b in range(len(s))]


def _ids(res):
    return [[(c.id, s) for c, s in hits] for hits in res]


def test_store_mmr(native, tmp_path):
    rng = np.random.default_rng(12)
    chunks, x = _chunks(rng)
    store = _store(tmp_path, "kb")
    asyncio.run(store.add_chunks(chunks))
    q = _planted(rng, x, 4)
    got = _ids(store.search_batch(q, 10, mmr_lambda=0.5))
    assert got == _want(x, q, 10, 0.5, 40) and got != _ids(store.search_batch(q, 10))
    assert _ids(store.search_batch(q, 5, mmr_lambda=0.3, fetch_k=128)) == _want(x, q, 5, 0.3, 128)
    # a per-query filter list: one launch per distinct filter
    flt = [{"part": 1}, None, {"part": 1}, {"part": 2}]
    part = np.arange(len(chunks)) % 3
    got = _ids(store.search_batch(q, 6, flt, mmr_lambda=0.5))
    for i, f in enumerate(flt):
        assert got[i] == _want(x, q[i:i + 1], 6, 0.5, 32, None if f is None else part == f["part"])[0]

    # 8 concurrent callers of mixed top_k: one launch, each its prefix
    async def callers():
        return await asyncio.gather(*[store.search(q[0].tolist(), k, mmr_lambda=0.5, fetch_k=64)
                                      for k in (3, 12, 1, 7, 12, 5, 2, 9)])

    before = store._batcher.launches
    res = asyncio.run(callers())
    assert store._batcher.launches - before == 1
    full = _want(x, q[:1], 12, 0.5, 64)[0]
    assert _ids(res) == [full[:k] for k in (3, 12, 1, 7, 12, 5, 2, 9)]
    store.close()


def test_ivf_store_answers_mmr_through_its_exact_index(native, tmp_path):
    rng = np.random.default_rng(13)
    chunks, x = _chunks(rng)
    store = _store(tmp_path, "kb_ivf", index_type="IVF_FLAT", nlist=4, nprobe=1, ivf_train_rows=64, ivf_seed=1)
    asyncio.run(store.add_chunks(chunks))
    assert store._index.trained
    q = _planted(rng, x, 3)
    assert _ids(store.search_batch(q, 8, mmr_lambda=0.5)) == _want(x, q, 8, 0.5, 32)  # (nprobe = 1 would miss rows)
    store.close()
