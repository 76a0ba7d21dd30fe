"""GPU: HipVectorStore with index_type "IVF_FLAT" (hiprag/rag/ivf_store.py): exact below the training threshold,
then the oracle's IVF restatement (oracle/ref_numpy.ivf_search) over the store's own centroids and list assignment --
through adds, deletes, where-filters, concurrent single-query searches, snapshots and the journal.  Exact
comparisons throughout."""
import asyncio
import os
import shutil

import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import ref_numpy as R

from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig

pytestmark = pytest.mark.gpu

DIM, NLIST, NPROBE, TRAIN = 64, 8, 2, 256
CUTS = [0, 200, 400, 850, 1300]     # four add_chunks calls; the second crosses 256 live rows in its middle


def _clustered(rng, n, dim, n_centers=40, spread=0.35):
    centers = rng.standard_normal((n_centers, dim)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    lab = rng.integers(0, n_centers, n)
    x = centers[lab] + spread * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    return x.astype(np.float32)


def _chunks(x, a, b):
    return [Chunk(id=f"c{r}", document_id=f"d{r % 13}", content=f"text {r}", chunk_index=r // 13,
                  metadata={"group": f"g{r % 10}"}, embedding=x[r].tolist()) for r in range(a, b)]


def _store(tmp_path, name, dtype, ivf, **params):
    p = {"include_embeddings": True, "fsync": False, **params}
    if dtype:
        p["dtype"] = dtype
    if ivf:
        p = {"nlist": NLIST, "nprobe": NPROBE, "ivf_train_rows": TRAIN, "ivf_seed": 3, **p}
    return HipVectorStore(VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                                            index_type="IVF_FLAT" if ivf else None, index_params=p))


def _hits(res):
    return [[(c.id, s) for c, s in per_q] for per_q in res]


def _check_restatement(store, stored, dtype, q, k=10, filters=None, allowed=None, nprobe=NPROBE):
    """search_batch against the restatement over the store's own centroids and lists (dead rows: list -1)."""
    idx = store._index
    assert idx.trained
    row_list = idx.lists_of_rows.copy()
    n = len(row_list)
    dead = np.array([store._records[r] is None for r in range(n)])
    assert ((row_list < 0) == dead).all()                       # every live row is in a list, no dead one is
    if allowed is not None:
        row_list[~allowed[:n]] = -1
    s_ref, r_ref, _ = R.ivf_search(stored[:n], dtype, R.process_queries(q, "cosine"), idx.centroids, row_list,
                                   nprobe, k)
    got = store.search_batch(q, k, filters)
    for b in range(len(q)):
        keep = r_ref[b] >= 0
        assert [c.id for c, _ in got[b]] == [f"c{r}" for r in r_ref[b][keep]]
        np.testing.assert_array_equal(np.array([s for _, s in got[b]], np.float32), s_ref[b][keep].astype(np.float32))
    return got


@pytest.mark.parametrize("dtype", ["bf16", None])
def test_ivf_store(tmp_path, dtype):
    rng = np.random.default_rng(11)
    n = CUTS[-1]
    x = _clustered(rng, n, DIM)
    sd = dtype or "f32"
    stored = R.process_rows(x, "cosine", sd)
    j = rng.choice(n, 8, replace=False)
    q = np.concatenate([x[j] + 0.02 * rng.standard_normal((8, DIM)).astype(np.float32),
                        rng.standard_normal((4, DIM)).astype(np.float32)]).astype(np.float32)
    store, plain = _store(tmp_path, "ivf", dtype, True), _store(tmp_path, "plain", dtype, False)
    full = _store(tmp_path, "full", dtype, True, nprobe=NLIST, persist=False)      # nprobe = nlist
    assert store.ivf and store.dtype == sd and not plain.ivf

    def add(a, b):
        for s in (store, plain, full):
            s.add_chunks_sync(_chunks(x, a, b))

    # ---- before the threshold: exact, the plain store's answers
    add(CUTS[0], CUTS[1])
    assert not store._index.trained
    assert _hits(store.search_batch(q, 10)) == _hits(plain.search_batch(q, 10))
    assert _hits(store.search_batch(q, 10, {"group": "g4"})) == _hits(plain.search_batch(q, 10, {"group": "g4"}))
    # ---- the add that crosses the threshold in its middle trains and places every row
    add(CUTS[1], CUTS[2])
    assert store._index.trained and store._index.ivf.n == CUTS[2]
    _check_restatement(store, stored, sd, q)
    store.flush()                                    # a snapshot that holds the trained lists
    import torch

    for s in (store, plain, full):                   # (embeddings that are already on the GPU: add_device)
        assert s.add_chunks_device(_chunks(x, CUTS[2], CUTS[3]), torch.from_numpy(x[CUTS[2]:CUTS[3]]).cuda()) == 450
    _check_restatement(store, stored, sd, q)
    add(CUTS[3], CUTS[4])
    got = _check_restatement(store, stored, sd, q, k=100)
    assert _hits(got) != _hits(plain.search_batch(q, 100))          # (two of eight lists: not the exact answer)
    # ---- delete_by_document_id tombstones both structures
    for s in (store, plain, full):
        assert asyncio.run(s.delete_by_document_id("d3")) == 100
    assert store._index.ivf.n == n - 100 and store._index.size() == (n, n - 100)
    _check_restatement(store, stored, sd, q)
    # ---- where-filters: about a tenth of the rows, and none
    groups = np.array([r % 10 for r in range(n)])
    got = _check_restatement(store, stored, sd, q, filters={"group": "g4"}, allowed=groups == 4)
    assert all(c.metadata["group"] == "g4" for res in got for c, _ in res) and any(got)
    assert store.search_batch(q, 10, {"group": "nope"}) == [[] for _ in q]
    _check_restatement(store, stored, sd, q, filters={"group": "nope"}, allowed=np.zeros(n, bool))
    # ---- 32 concurrent single-query searches = one search_batch
    q32 = np.concatenate([q, q[::-1], q[:8]])[:32]

    async def many():
        return await asyncio.gather(*[store.search(v.tolist(), 10) for v in q32])

    assert _hits(asyncio.run(many())) == _hits(store.search_batch(q32, 10))
    # ---- nprobe = nlist and top_k beyond the IVF search's 1024: the plain store's answers
    assert full._index.trained
    assert _hits(full.search_batch(q, 10)) == _hits(plain.search_batch(q, 10))
    assert _hits(full.search_batch(q, 10, {"group": "g4"})) == _hits(plain.search_batch(q, 10, {"group": "g4"}))
    big = store.search_batch(q[:3], 1100)
    assert _hits(big) == _hits(plain.search_batch(q[:3], 1100)) and len(big[0]) == 1100
    # ---- get_by_id and include_embeddings give the exact index's vectors
    for cid in ("c0", "c399", "c1299"):
        a, b = asyncio.run(store.get_by_id(cid)), asyncio.run(plain.get_by_id(cid))
        assert a.embedding == b.embedding and a.embedding == stored_row(stored, sd, int(cid[1:]))
    res = store.search_batch(q[:2], 5)
    for per_q in res:
        for c, _ in per_q:
            assert c.embedding == stored_row(stored, sd, int(c.id[1:]))
    # ---- persistence: the adds and the delete since the snapshot are in the journal
    before = _hits(store.search_batch(q, 10))
    before_f = _hits(store.search_batch(q, 10, {"group": "g4"}))
    lists_before = store._index.lists_of_rows.copy()
    d = str(tmp_path / "ivf")
    assert any(f.endswith(".journal") and os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    shutil.copytree(d, str(tmp_path / "crash" / "ivf"))            # the files as a crash would leave them
    replayed = _store(tmp_path / "crash", "ivf", dtype, True)      # snapshot + journal replay
    assert replayed._index.trained and replayed.count_sync() == n - 100
    np.testing.assert_array_equal(replayed._index.lists_of_rows, lists_before)
    assert _hits(replayed.search_batch(q, 10)) == before
    assert _hits(replayed.search_batch(q, 10, {"group": "g4"})) == before_f
    replayed.close()
    store.close()                                                  # folds the journal into a new generation
    side = sorted(f for f in os.listdir(d) if f.endswith(".ivf.npz"))
    assert len(side) == 1 and not any(f.endswith(".journal") and os.path.getsize(os.path.join(d, f))
                                      for f in os.listdir(d))
    again = _store(tmp_path, "ivf", dtype, True)
    assert again._index.trained
    np.testing.assert_array_equal(again._index.lists_of_rows, lists_before)
    assert _hits(again.search_batch(q, 10)) == before
    _check_restatement(again, stored, sd, q)
    again.flush()
    side2 = sorted(f for f in os.listdir(d) if f.endswith(".ivf.npz"))
    assert len(side2) == 1 and side2 != side                       # the old generation's side file is gone
    # ---- rebuild_ivf retrains on the rows stored now
    again.rebuild_ivf()
    _check_restatement(again, stored, sd, q)
    with pytest.raises(ValueError):
        plain.rebuild_ivf()
    for s in (again, plain, full):
        s.close()


def stored_row(stored, dtype, r):
    """The stored (normalised, quantised) row as the fp32 list get_rows returns."""
    return R.dequantize(stored[r:r + 1], dtype)[0].astype(np.float32).tolist()
