"""GPU: the store's device-query route (search_device_sync / search_masks_device_sync: queries read in place on the
GPU, scores and rows back in one packed buffer) against search_batch on the same queries from the host, bit for bit --
with B * k odd, so the rows' 8-byte alignment pad of the packed buffer is there, and even."""
import numpy as np
import pytest

from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

N, DIM = 4096, 64


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from hiprag import _native
    from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    raw = R.gen_rows(21, 0, N, DIM)
    cfg = VectorStoreConfig(backend="hip", collection_name="route", distance_metric="cosine",
                            persist_directory=str(tmp_path_factory.mktemp("route")),
                            index_params={"dtype": "bf16", "persist": False})
    s = HipVectorStore(cfg)
    s.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 512}", content=f"text {i}", chunk_index=i % 512,
                             metadata={"source": f"s{i // 512}"}, embedding=raw[i].tolist()) for i in range(N)])
    s.raw = raw
    yield s
    s.close()


def _queries(store, B, seed):
    rng = np.random.default_rng(seed)
    return (store.raw[rng.choice(N, B, replace=False)] + 0.2 * rng.standard_normal((B, DIM))).astype(np.float32)


def _pairs(res):
    return [[(c.id, s) for c, s in r] for r in res]


def _same_raw(got, want):
    (gs, gr), (ws, wr) = got, want
    assert gs.dtype == np.float32 and gr.dtype == np.int64 and gs.shape == gr.shape == ws.shape
    np.testing.assert_array_equal(gr, wr)
    np.testing.assert_array_equal(gs.view(np.uint32), np.asarray(ws, np.float32).view(np.uint32))


@pytest.mark.parametrize("B,k", [(3, 5), (2, 4)])
def test_device_queries_equal_host_queries(store, B, k):
    torch = pytest.importorskip("torch")
    q = _queries(store, B, 100 + B)
    q_dev = torch.from_numpy(q).to(f"cuda:{store.device}")
    assert hasattr(store._index, "search_device") and q_dev.is_cuda  # (the device route, not its host fallback)
    prep = store._prep_search(q, k, None)
    raw, tables = store.search_device_sync(q_dev, k)
    _same_raw(raw, store._run_search(prep)[0])
    got = store._assemble(prep, (raw, tables))
    assert [len(r) for r in got] == [k] * B
    assert _pairs(got) == _pairs(store.search_batch(q, k))


@pytest.mark.parametrize("B,k", [(3, 5), (2, 4)])
def test_device_queries_with_one_filter_each(store, B, k):
    torch = pytest.importorskip("torch")
    q = _queries(store, B, 200 + B)
    q_dev = torch.from_numpy(q).to(f"cuda:{store.device}")
    flt = [{"source": "s1"}, None, {"source": "s6"}][:B]
    assert hasattr(store._index, "search_masks_device")
    mixed, launches = store.mixed_launches, store._index.qmask_launches()
    raw, tables = store.search_masks_device_sync(q_dev, k, flt)
    assert store.mixed_launches == mixed + 1 and store._index.qmask_launches() == launches + 1
    prep = store._prep_search(q, k, flt)
    _same_raw(raw, store._run_search(prep)[0])
    got = store._assemble(prep, (raw, tables))
    assert _pairs(got) == _pairs(store.search_batch(q, k, flt))
    for r, f in zip(got, flt):
        assert len(r) == k and (f is None or all(c.metadata["source"] == f["source"] for c, _ in r))


def test_nothing_to_search(store, tmp_path):
    torch = pytest.importorskip("torch")
    from hiprag.rag import HipVectorStore, VectorStoreConfig

    q_dev = torch.zeros((3, DIM), device=f"cuda:{store.device}")
    flt = [{"source": "s1"}, None, {"source": "s6"}]
    empty = HipVectorStore(VectorStoreConfig(backend="hip", collection_name="none", persist_directory=str(tmp_path),
                                             index_params={"dtype": "bf16", "persist": False}))
    for s, k in ((store, 0), (empty, 5)):
        for raw, tables in (s.search_device_sync(q_dev, k), s.search_masks_device_sync(q_dev, k, flt)):
            assert raw is None and len(tables) == 3 and tables[2] == s._epoch
            assert s._assemble(s._prep_search(np.zeros((3, DIM), np.float32), k, None), (raw, tables)) == [[], [], []]
    empty.close()
