"""GPU: collapsed search (hr_collapse.hip) -- the best row of each of the k best groups -- against
tests/collapse_ref.py: the oracle's full ranking de-duplicated by first occurrence.  Rows equal, scores equal as fp32
bit patterns, through the probe stage, the all-rows stage, ties, deletes, masks, column growth and the store."""
import asyncio
import json

import numpy as np
import pytest

import oracle  # noqa: F401
from collapse_ref import assert_same, collapse_ref
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 31, 32, 33, 64, 65, 1000, 4099]


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


def _runs(rng, n, lo=2, hi=7):
    """Group ids in runs of lo..hi rows, as a document's chunks are appended."""
    g, ids = [], 0
    while len(g) < n:
        g += [ids] * int(rng.integers(lo, hi + 1))
        ids += 1
    return np.asarray(g[:n], np.int32)


def _doc_rows(rng, groups, dim=64, spread=0.5):
    """Rows that resemble the other rows of their run: unit(centre of the run + spread * unit noise)."""
    groups = np.asarray(groups)
    run = np.concatenate([[0], np.cumsum(groups[1:] != groups[:-1])])
    centres = _unit(rng.standard_normal((run[-1] + 1, dim)).astype(np.float32))
    return _unit(centres[run] + spread * _unit(rng.standard_normal((len(groups), dim)).astype(np.float32)))


def _planted(rng, x, B, noise=0.05):
    pick = rng.choice(len(x), B, replace=len(x) < B)
    e = rng.standard_normal((B, x.shape[1])).astype(np.float32)
    return (_unit(x[pick]) + noise * _unit(e)).astype(np.float32)


def _ref(stored, dtype, metric, q, groups, k, allowed=None):
    return collapse_ref(stored, dtype, R.process_queries(q, metric), groups, k, allowed, metric)


def _incomplete(stored, dtype, metric, q, groups, k, P, allowed=None):
    """Which queries stage 1 cannot answer: the probe is full and its P rows hold fewer than k groups."""
    n = len(stored)
    mask = None if allowed is None else oracle.mask_from_bool(allowed)
    _, r = oracle.c_search(stored, dtype, R.process_queries(q, metric), min(P, n), mask, nthreads=2, metric=metric)
    out = []
    for b in range(len(q)):
        full = n >= P and r[b, P - 1] >= 0
        rows = r[b][r[b] >= 0]
        g = np.asarray([groups[x] if x < len(groups) else -1 for x in rows])
        out.append(bool(full and len(set(g[g >= 0].tolist())) < k))
    return np.asarray(out)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("metric", ["cosine", "ip", "l2"])
def test_row_counts_dtypes_metrics(native, dtype, metric):
    """Every row count at a tile / wave edge, default probe and probe = k (where any duplicate in the top k sends
    the query through the all-rows stage); k above the number of groups pads."""
    rng = np.random.default_rng(10 * ["f32", "bf16", "f16"].index(dtype) + ["cosine", "ip", "l2"].index(metric))
    for n in ROW_COUNTS:
        groups = _runs(rng, n)
        x = _doc_rows(rng, groups) * (1.0 if metric == "cosine" else rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32))
        idx, stored = _build(native, x, dtype, metric)
        idx.set_groups(0, groups)
        q = _planted(rng, x, 3)
        for k, probe in ((10, 0), (10, 10), (3, 3)):
            assert_same(idx.search_collapsed(q, k, probe=probe), _ref(stored, dtype, metric, q, groups, k))
        idx.close()


@pytest.mark.parametrize("k", [1, 10, 128])
def test_singleton_groups_equal_plain_search(native, k):
    rng = np.random.default_rng(k)
    x = rng.standard_normal((1000, 64)).astype(np.float32)
    idx, stored = _build(native, x)
    idx.set_groups(0, np.arange(1000, dtype=np.int32))
    q = _planted(rng, x, 5)
    s0, r0 = idx.search(q, k)
    s1, r1 = idx.search_collapsed(q, k)
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(s1.view(np.uint32), s0.view(np.uint32))
    assert idx.collapse_stats() == {"probe": 5, "all_rows": 0}


def test_one_group_and_k_above_groups(native):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((1000, 64)).astype(np.float32)
    idx, stored = _build(native, x)
    q = _planted(rng, x, 4)
    idx.set_groups(0, np.zeros(1000, np.int32))
    s, r = idx.search_collapsed(q, 5)
    assert_same((s, r), _ref(stored, "bf16", "cosine", q, np.zeros(1000, np.int32), 5))
    assert (r[:, 0] >= 0).all() and (r[:, 1:] == -1).all() and np.isneginf(s[:, 1:]).all()
    assert idx.collapse_stats()["all_rows"] == 4  # the probe saw one group and came back full
    groups = (np.arange(1000) % 7).astype(np.int32)  # 7 interleaved groups, k = 10: padding after the 7th
    idx.set_groups(0, groups)
    s, r = idx.search_collapsed(q, 10)
    assert_same((s, r), _ref(stored, "bf16", "cosine", q, groups, 10))
    assert (r[:, :7] >= 0).all() and (r[:, 7:] == -1).all()


@pytest.mark.parametrize("n_groups", [5000, 3])
def test_forced_all_rows_stage(native, n_groups):
    """probe = k over runs of 2-7 rows: 5000 groups (more than the selector's 1024 outputs per segment) and 3."""
    rng = np.random.default_rng(n_groups)
    groups = _runs(rng, 10 ** 6)
    n = int(np.searchsorted(groups, n_groups))  # the rows of the first n_groups groups
    groups = groups[:n]
    x = _doc_rows(rng, groups)
    idx, stored = _build(native, x)
    idx.set_groups(0, groups)
    q = _planted(rng, x, 4, noise=0.5)
    for k in (10, 128):
        need = _incomplete(stored, "bf16", "cosine", q, groups, k, k)
        before = idx.collapse_stats()["all_rows"]
        assert_same(idx.search_collapsed(q, k, probe=k), _ref(stored, "bf16", "cosine", q, groups, k))
        assert idx.collapse_stats()["all_rows"] - before == int(need.sum())
    assert idx.collapse_stats()["all_rows"] > 0


def _big_document(rng, n=1000, dim=128, members=200, first=300):
    """n rows, `members` of them normalise(q + 0.05 noise) for one query direction q, contiguous, in one group."""
    x = rng.standard_normal((n, dim)).astype(np.float32)
    c = _unit(rng.standard_normal(dim).astype(np.float32))
    x[first:first + members] = _unit(c + 0.05 * rng.standard_normal((members, dim)).astype(np.float32))
    groups = np.arange(n, dtype=np.int32)
    groups[first:first + members] = 0
    groups[0] = first  # (id 0 went to the document)
    return x, c, groups


def test_natural_all_rows_stage(native):
    """The default probe's rows are all one document: the all-rows stage answers."""
    rng = np.random.default_rng(4)
    x, c, groups = _big_document(rng)
    idx, stored = _build(native, x, "f32")
    idx.set_groups(0, groups)
    q = c[None, :]
    _, top = idx.search(q, 128)
    assert (groups[top[0]] == 0).all()  # the top 128 rows are one document
    got = idx.search_collapsed(q, 5)
    assert_same(got, _ref(stored, "f32", "cosine", q, groups, 5))
    assert (got[1][0] >= 0).all() and len(set(groups[got[1][0]].tolist())) == 5
    assert idx.collapse_stats() == {"probe": 0, "all_rows": 1}


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_mixed_batches(native, B):
    """Some queries complete in the probe, some do not: the flags are per query."""
    rng = np.random.default_rng(B)
    x, c, groups = _big_document(rng, n=2000, dim=64)
    idx, stored = _build(native, x)
    idx.set_groups(0, groups)
    q = _planted(rng, x, B, noise=0.3)
    hit = np.arange(B) % 3 == 0  # every third query asks for the big document
    q[hit] = c + 0.02 * rng.standard_normal((int(hit.sum()), 64)).astype(np.float32)
    need = _incomplete(stored, "bf16", "cosine", q, groups, 5, 128)  # (the default probe)
    assert need[hit].all() and (B == 1 or not need.all())
    assert_same(idx.search_collapsed(q, 5), _ref(stored, "bf16", "cosine", q, groups, 5))
    assert idx.collapse_stats() == {"probe": int((~need).sum()), "all_rows": int(need.sum())}


def _axis_rows(scores, dim=64):
    """fp32 rows score * e0: with q = e0 and the ip metric the scores are exactly `scores` (equal values tie)."""
    x = np.zeros((len(scores), dim), np.float32)
    x[:, 0] = np.asarray(scores, np.float32)
    q = np.zeros((1, dim), np.float32)
    q[0, 0] = 1.0
    return x, q


def test_ties(native):
    # identical vectors in different groups (rows 1, 2: the lower row ranks first), inside one group (rows 3, 4: the
    # lower represents it), and a tie that straddles the last slot of a 4-row probe (rows 5 | 6)
    scores = [0.9, 0.8, 0.8, 0.7, 0.7, 0.6, 0.6, 0.5, 0.4, 0.3]
    groups = np.asarray([0, 1, 2, 0, 0, 0, 3, 4, 5, 6], np.int32)
    x, q = _axis_rows(scores)
    idx, stored = _build(native, x, "f32", "ip")
    idx.set_groups(0, groups)
    for k, probe in ((4, 4), (4, 6), (4, 0), (7, 7), (3, 3)):
        got = idx.search_collapsed(q, k, probe=probe)
        assert_same(got, _ref(stored, "f32", "ip", q, groups, k))
    assert idx.search_collapsed(q, 4, probe=4)[1][0].tolist() == [0, 1, 2, 6]
    # the all-rows stage on its own: equal best scores inside a group and across groups
    groups2 = np.asarray([3, 1, 1, 2, 2, 3, 0, 0, 0, 0], np.int32)
    scores2 = [0.5, 0.8, 0.8, 0.8, 0.8, 0.5, 0.5, 0.5, 0.1, 0.5]
    x2, _ = _axis_rows(scores2)
    idx2, stored2 = _build(native, x2, "f32", "ip")
    idx2.set_groups(0, groups2)
    got = idx2.search_collapsed(q, 4, probe=4)
    assert_same(got, _ref(stored2, "f32", "ip", q, groups2, 4))
    assert got[1][0].tolist() == [1, 3, 0, 6] and idx2.collapse_stats()["all_rows"] == 1
    # many ties, interleaved ids: few score levels over 20 groups
    rng = np.random.default_rng(7)
    scores3 = rng.integers(1, 10, 300) / 10.0
    groups3 = rng.integers(0, 20, 300).astype(np.int32)
    x3, _ = _axis_rows(scores3)
    idx3, stored3 = _build(native, x3, "f32", "ip")
    idx3.set_groups(0, groups3)
    for k, probe in ((10, 10), (20, 0), (25, 128)):
        assert_same(idx3.search_collapsed(q, k, probe=probe), _ref(stored3, "f32", "ip", q, groups3, k))


def test_runs_and_interleaved_ids(native):
    rng = np.random.default_rng(8)
    n = 1000
    x = rng.standard_normal((n, 64)).astype(np.float32)
    idx, stored = _build(native, x)
    q = _planted(rng, x, 6, noise=0.4)
    # runs that cross lane 63 | 64 and the 256-row workgroup boundary, then runs of 40
    groups = np.empty(n, np.int32)
    groups[:60], groups[60:71], groups[71:251], groups[251:261] = 0, 1, 2, 3
    groups[261:] = 4 + (np.arange(n - 261) // 40)
    # ... set over several calls, row0 no multiple of 32
    idx.set_groups(0, groups[:37])
    idx.set_groups(37, groups[37:501])
    idx.set_groups(501, groups[501:])
    for k, probe in ((10, 10), (10, 0), (24, 24)):
        assert_same(idx.search_collapsed(q, k, probe=probe), _ref(stored, "bf16", "cosine", q, groups, k))
    for period in (2, 7):  # a, b, a, b, ...: every lane its own run
        inter = (np.arange(n) % period).astype(np.int32)
        idx.set_groups(0, inter)
        assert_same(idx.search_collapsed(q, 10, probe=10), _ref(stored, "bf16", "cosine", q, inter, 10))
    assert idx.collapse_stats()["all_rows"] >= 12


def test_deletes_and_masks(native):
    rng = np.random.default_rng(9)
    n = 500
    groups = (np.arange(n) // 5).astype(np.int32)
    x = _doc_rows(rng, groups)
    idx, stored = _build(native, x)
    groups[400:420] = -1  # rows without a group are never returned
    idx.set_groups(0, groups)
    q = _unit(x[[102, 250, 405]]) + 0.01 * rng.standard_normal((3, 64)).astype(np.float32)
    live = np.ones(n, bool)
    got = idx.search_collapsed(q, 8)
    assert_same(got, _ref(stored, "bf16", "cosine", q, groups, 8, live))
    assert got[1][0, 0] == 102 and got[1][1, 0] == 250 and not np.isin(got[1], np.arange(400, 420)).any()
    idx.remove([102])  # the group's best row goes: the next one represents it
    live[102] = False
    got = idx.search_collapsed(q, 8, probe=8)
    assert_same(got, _ref(stored, "bf16", "cosine", q, groups, 8, live))
    assert groups[got[1][0, 0]] == 20 and got[1][0, 0] != 102
    idx.remove(np.arange(250, 255))  # a whole group goes
    live[250:255] = False
    got = idx.search_collapsed(q, 8)
    assert_same(got, _ref(stored, "bf16", "cosine", q, groups, 8, live))
    assert 50 not in groups[got[1][1]].tolist()
    allowed = live.copy()  # a mask that hides a group's best row, and most of the corpus
    allowed[got[1][0, 0]] = False
    allowed[300:] = False
    mask = oracle.mask_from_bool(allowed)
    for probe in (0, 8):
        assert_same(idx.search_collapsed(q, 8, mask=mask, probe=probe),
                    _ref(stored, "bf16", "cosine", q, groups, 8, allowed))


def test_rows_added_later_and_column_growth(native):
    rng = np.random.default_rng(10)
    x = rng.standard_normal((100, 64)).astype(np.float32)
    idx, stored = _build(native, x)
    groups = (np.arange(100) // 4).astype(np.int32)
    idx.set_groups(0, groups)
    q = _planted(rng, x, 3)
    # an add that grows the index (and outruns the column): the new rows have no group until they are given one
    more = np.concatenate([_unit(q), rng.standard_normal((5000, 64)).astype(np.float32)])
    idx.add(more)
    x2 = np.concatenate([x, more])
    stored2 = R.process_rows(x2, "cosine", "bf16")
    got = idx.search_collapsed(q, 6)
    assert_same(got, _ref(stored2, "bf16", "cosine", q, groups, 6))
    assert (got[1] < 100).all()
    groups2 = np.concatenate([groups, 25 + (np.arange(len(more)) // 3)]).astype(np.int32)
    idx.set_groups(100, groups2[100:150])  # inside the doubled column
    idx.set_groups(150, groups2[150:])     # beyond it: grown with its contents kept
    for probe in (0, 6):
        got = idx.search_collapsed(q, 6, probe=probe)
        assert_same(got, _ref(stored2, "bf16", "cosine", q, groups2, 6))
    assert got[1][:, 0].tolist() == [100, 101, 102]


def test_device_entry_point_and_errors(native):
    import torch

    rng = np.random.default_rng(11)
    x = rng.standard_normal((300, 64)).astype(np.float32)
    idx, stored = _build(native, x)
    q = _planted(rng, x, 5)
    with pytest.raises(ValueError):  # no group column yet
        idx.search_collapsed(q, 5)
    groups = _runs(rng, 300)
    with pytest.raises(ValueError):
        idx.set_groups(0, np.asarray([0, -2], np.int32))
    with pytest.raises(ValueError):
        idx.set_groups(299, np.asarray([0, 1], np.int32))
    idx.set_groups(0, groups)
    for bad in (dict(k=0), dict(k=129), dict(k=10, probe=9), dict(k=10, probe=129)):
        with pytest.raises(ValueError):
            idx.search_collapsed(q, **bad)
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(q).to(dev)
    s = torch.empty((5, 7), dtype=torch.float32, device=dev)
    r = torch.empty((5, 7), dtype=torch.int64, device=dev)
    for probe in (0, 7):
        idx.search_collapsed_device(qd.data_ptr(), 5, 7, s.data_ptr(), r.data_ptr(), probe=probe,
                                    stream=torch.cuda.current_stream(dev).cuda_stream)
        assert_same((s.cpu().numpy(), r.cpu().numpy()), _ref(stored, "bf16", "cosine", q, groups, 7))
    # an empty index with a column pads; a multi-device handle is out of scope
    idx.remove(np.arange(300))
    s0, r0 = idx.search_collapsed(q, 3)
    assert (r0 == -1).all() and np.isneginf(s0).all()
    two = native.NativeIndex(64, "bf16", "cosine", devices=[0, 0])
    two.add(x)
    with pytest.raises(NotImplementedError):
        two.set_groups(0, groups)
    with pytest.raises(NotImplementedError):
        two.search_collapsed(q, 5)
    two.close()


# ---------------------------------------------------------------- the store
def _doc_chunks(rng, dim=64):
    """Documents of 1..60 chunks; every third document's chunks lack `source`, two documents share one."""
    from hiprag.rag import Chunk

    out, vecs = [], []
    for d, n in enumerate([60, 1, 7, 33, 2, 12, 5, 40, 3, 9, 1, 6]):
        center = _unit(rng.standard_normal(dim).astype(np.float32))
        for i in range(n):
            v = _unit(center + 0.5 * _unit(rng.standard_normal(dim).astype(np.float32)))
            meta = {"index_type": "index_summary"}
            if d % 3:
                meta["source"] = "shared.pdf" if d in (4, 5) else f"file_{d}.pdf"
            out.append(Chunk(id=f"d{d}_c{i}", document_id=f"doc{d}", content=f"text {d}.{i}", chunk_index=i,
                             metadata=meta, embedding=v.tolist()))
            vecs.append(v)
    return out, np.asarray(vecs, np.float32)


def _host_dedup(store, q, k, key, filters=None):
    """The reference's way with an unbounded fetch: the full ranking, first hit per key."""
    out = []
    for hits in store.search_batch(q, store.count_sync(), filters):
        seen, res = set(), []
        for c, s in hits:
            name = key(c)
            if name in seen:
                continue
            seen.add(name)
            res.append((c.id, s))
        out.append(res[:k])
    return out


def _ids(res):
    return [[(c.id, s) for c, s in hits] for hits in res]


def _store(tmp_path, name, **kw):
    from hiprag.rag import HipVectorStore, VectorStoreConfig

    index_type = kw.pop("index_type", None)
    return HipVectorStore(VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                                            index_type=index_type,
                                            index_params={"dtype": "bf16", "fsync": False, **kw}))


@pytest.mark.parametrize("field", ["document_id", "source"])
def test_store_collapse(native, tmp_path, field):
    rng = np.random.default_rng(12)
    chunks, vecs = _doc_chunks(rng)
    store = _store(tmp_path, "kb_" + field, collapse_field=field)
    asyncio.run(store.add_chunks(chunks[:100]))
    q = vecs[[0, 61, 70, 150]] + 0.05 * rng.standard_normal((4, 64)).astype(np.float32)
    key = (lambda c: c.document_id) if field == "document_id" else \
        (lambda c: c.metadata.get("source", c.document_id))
    assert _ids(store.search_batch(q, 4, collapse=True)) == _host_dedup(store, q, 4, key)
    asyncio.run(store.add_chunks(chunks[100:]))  # the column follows the adds
    for k in (1, 5, 50):
        got = _ids(store.search_batch(q, k, collapse=True))
        assert got == _host_dedup(store, q, k, key)
    assert len(got[0]) == (12 if field == "document_id" else 11)  # (two documents share a source)
    flt = {"source": {"$ne": "file_1.pdf"}}
    assert _ids(store.search_batch(q, 5, flt, collapse=True)) == _host_dedup(store, q, 5, key, flt)
    one = asyncio.run(store.search(q[0].tolist(), 5, collapse=True))
    assert [(c.id, s) for c, s in one] == _host_dedup(store, q[:1], 5, key)[0]
    assert asyncio.run(store.delete_by_document_id("doc0")) == 60
    assert _ids(store.search_batch(q, 5, collapse=True)) == _host_dedup(store, q, 5, key)
    store.close()
    again = _store(tmp_path, "kb_" + field, collapse_field=field)  # reload: the ids are derived again
    assert again.count_sync() == len(chunks) - 60
    assert _ids(again.search_batch(q, 5, collapse=True)) == _host_dedup(again, q, 5, key)
    again.close()


def test_ivf_store_collapses_through_its_exact_index(native, tmp_path):
    rng = np.random.default_rng(13)
    chunks, vecs = _doc_chunks(rng)
    store = _store(tmp_path, "kb_ivf", index_type="IVF_FLAT", nlist=4, nprobe=1, ivf_train_rows=64, ivf_seed=1)
    asyncio.run(store.add_chunks(chunks))
    assert store._index.trained
    q = vecs[[0, 61, 150]] + 0.05 * rng.standard_normal((3, 64)).astype(np.float32)
    exact = _store(tmp_path, "kb_flat")
    asyncio.run(exact.add_chunks(chunks))
    want = _host_dedup(exact, q, 6, lambda c: c.document_id)  # (the exact store's ranking: nprobe = 1 would miss rows)
    assert _ids(store.search_batch(q, 6, collapse=True)) == want
    store.close()
    exact.close()


def test_kb_file_search_returns_top_k_files(native, tmp_path, monkeypatch):
    from hiprag.rag import kb_tools as K

    def no_reranker(backend):
        raise RuntimeError("no reranker")

    monkeypatch.setattr(K, "_reranker_from", no_reranker)
    rng = np.random.default_rng(14)
    chunks, vecs = _doc_chunks(rng)
    qv = vecs[0] + 0.02 * rng.standard_normal(64).astype(np.float32)  # the 60-chunk document's direction

    class Embedder:
        async def embed_query(self, q):
            return qv.tolist()

    out = {}
    for collapse in (False, True):
        cfg = {"vector_store": {"backend": "hip", "persist_directory": str(tmp_path / f"c{int(collapse)}"),
                                "index_params": {"dtype": "bf16", "persist": False}}, "collapse_files": collapse}
        tk = K.KBSearchToolkit(config=cfg, kb_resolver=lambda kb: ("coll", "KB"))
        tk._embedder_cache = Embedder()
        store = tk._get_or_create_vector_store("coll", cfg["vector_store"]["persist_directory"])
        assert store.collapse_field == ("source" if collapse else "document_id")
        asyncio.run(store.add_chunks(chunks))
        out[collapse] = json.loads(asyncio.run(tk.kb_file_search(1, "q", top_k=5, auto_rerank=False)))
        store.close()
    assert out[False]["total_files"] == 1  # five rows fetched, all of one file
    assert out[True]["total_files"] == 5 and len({f["file_name"] for f in out[True]["files"]}) == 5
    assert out[True]["files"][0] == out[False]["files"][0]
