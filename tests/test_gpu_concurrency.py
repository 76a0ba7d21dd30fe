"""GPU: concurrency and resource-lifetime cases of the host layer.

* the query coalescer's first forward of a new shape is CAPTURED into a HIP graph on its worker thread
  while the event loop's thread launches the store's native searches -- with an empty graph cache, many concurrent
  VectorRetriever.retrieve calls (embed_query -> store.search, base_retriever.py:57-63) must return what the same
  vectors return searched one by one, and the vectors must be the embedder's.
* a CU-masked stream (hr_stream_create_cu_mask) used for the embedder and the search (the bench's
  CU split) and then destroyed (hr_stream_destroy) while tensors made on it are still alive: the process exits 0.
"""
import asyncio
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.mark.timeout(300)
def test_concurrent_retrieve_with_cold_graph_capture(tmp_path):
    from hiprag.rag import HipVectorStore, VectorStoreConfig
    from hiprag.rag.base import Chunk
    from hiprag.rag.rocm_embedder import TorchRocmEmbedder

    emb = TorchRocmEmbedder(preset="tiny", dtype="bfloat16", batch_size=32, max_length=128, seed=3)
    assert emb.graphed is not None and not emb.graphed.graphs  # cold: the first coalesced forward captures
    rng = np.random.default_rng(4)
    n, dim = 50_000, emb.dim
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    cfg = VectorStoreConfig(backend="hip", collection_name="conc", persist_directory=str(tmp_path),
                            index_params={"dtype": "bf16", "persist": False, "max_batch": 16})
    store = HipVectorStore(cfg)
    store.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 50}", content=str(i), chunk_index=i % 50,
                                 metadata={}, embedding=rows[i].tolist()) for i in range(n)])
    texts = [f"question {i} about topic w{i % 17} and w{(i * 5) % 23}" for i in range(96)]

    async def retrieve(t):  # VectorRetriever.retrieve's two awaits (base_retriever.py:57-63), vector kept
        v = await emb.embed_query(t)
        return v, await store.search(query_embedding=v, top_k=10)

    async def many():
        return await asyncio.gather(*[retrieve(t) for t in texts])

    out = asyncio.run(many())
    assert emb.graphed.graphs and emb._coalescer.forwards < len(texts)  # coalesced forwards, graphs captured
    # the vectors are the embedder's (a batch of another size only changes GEMM rounding)
    ref = emb.encode_queries(texts).cpu().numpy()
    v = np.asarray([x for x, _ in out], np.float32)
    assert float((v * ref).sum(1).min()) > 0.999

    async def alone(x):
        return await store.search(query_embedding=x, top_k=10)

    for x, res in out:  # each concurrent answer == the same vector searched alone, on a quiet loop
        want = asyncio.run(alone(x))
        assert [c.id for c, _ in res] == [c.id for c, _ in want]
        assert [s for _, s in res] == [s for _, s in want]
    store.close()
    emb._coalescer.close()


@pytest.mark.timeout(200)
def test_cu_masked_streams_destroyed_then_clean_exit():
    proc = subprocess.run([sys.executable, "-u", os.path.join(REPO, "tools", "cu_stream_probe.py"), "split", "lib",
                           "alive"], timeout=150, capture_output=True, text=True)
    print(proc.stdout[-2000:], proc.stderr[-3000:])
    assert proc.returncode == 0, (proc.returncode, proc.stderr[-3000:])
    assert "destroyed" in proc.stdout and "exiting" in proc.stdout


@pytest.mark.timeout(300)
def test_fused_retrieve_on_gpu_matches_two_step(tmp_path):
    """The retriever's fused cohorts on the GPU (one bf16 forward whose (B, dim) output feeds hr_index_search_device
    directly) vs the reference's two awaits (embed_query lists -> store.search) over the same store: the same top-k
    wherever the two forwards' roundings do not reorder a near tie, scores within the bf16 forward's rounding."""
    from hiprag.rag import HipVectorStore, RetrieverConfig, VectorRetriever, VectorStoreConfig
    from hiprag.rag.base import Chunk
    from hiprag.rag.rocm_embedder import TorchRocmEmbedder

    emb = TorchRocmEmbedder(preset="tiny", dtype="bfloat16", batch_size=32, max_length=128, seed=5)
    docs = [f"passage {i} on subject w{i % 41} with w{(i * 11) % 97} and w{(i * 5) % 13}" for i in range(3000)]
    vecs = emb.encode_passages(docs).cpu().numpy()
    cfg = VectorStoreConfig(backend="hip", collection_name="fused", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": False, "max_batch": 32})
    store = HipVectorStore(cfg)
    store.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 30}", content=docs[i], chunk_index=i % 30,
                                 metadata={}, embedding=vecs[i].tolist()) for i in range(len(docs))])
    rc = RetrieverConfig(top_k=8, similarity_threshold=0.0)
    ret, two = VectorRetriever(store, emb, rc), VectorRetriever(store, emb, rc)
    two._fused = None
    assert ret._fused is not None
    qs = [f"what is said on subject w{i % 41} and w{(i * 3) % 97}" for i in range(100)]

    async def many(r):
        return await asyncio.gather(*[r.retrieve(q) for q in qs])

    got, want = asyncio.run(many(ret)), asyncio.run(many(two))
    assert ret._fused.cohorts >= 4 and ret._fused.queries == len(qs)
    same = sum([x.chunk.id for x in g] == [x.chunk.id for x in w] for g, w in zip(got, want))
    assert same >= 0.9 * len(qs), same
    for g, w in zip(got, want):
        assert len(g) == 8 and abs(g[0].score - w[0].score) < 2e-2
    store.close()
    ret._fused.close()


@pytest.mark.timeout(300)
def test_fused_retriever_cohorts_of_mixed_top_k(tmp_path):
    """Four cohorts whose k are 10, 50, 200, 10 -- the pipelined submit, a k above the searcher's kc (32) while the
    first cohort is in flight, a k above HR_MAX_K (the store's synchronous search, no searcher), the pipelined submit
    again -- all queued before the worker's first forward returns (the stub embedder holds it until they are), twice
    on one retriever.  No call raises; every call's (chunk id, score, rank) list is the unfused retriever's."""
    import threading

    from hiprag.rag import HipVectorStore, RetrieverConfig, VectorRetriever, VectorStoreConfig
    from hiprag.rag.base import Chunk
    from oracle import ref_numpy as R

    n, dim, nq = 4_000, 64, 128
    raw = R.gen_rows(12, 0, n, dim)
    rng = np.random.default_rng(6)
    names = [f"q{i}" for i in range(nq)]
    table = {nm: (raw[rng.integers(n)] + 0.2 * rng.standard_normal(dim)).astype(np.float32) for nm in names}
    ks = [(10, 50, 200, 10)[i // 32] for i in range(nq)]

    class Emb:  # the in-process embedder's surface the fused path needs; the vectors come from the table
        batch_size, fused_retrieve, _fwd_lock = 32, True, threading.Lock()
        hold, entered, gate = False, threading.Event(), threading.Event()

        async def embed_query(self, text):
            return table[text].tolist()

        def encode_queries(self, texts):
            if Emb.hold:  # the first forward of a run waits until every cohort is queued behind it
                Emb.hold = False
                Emb.entered.set()
                if not Emb.gate.wait(timeout=120):
                    raise RuntimeError("the cohorts were never all queued")
            return torch.from_numpy(np.stack([table[t] for t in texts])).to("cuda:0")

    class Plain(Emb):
        fused_retrieve = False

    cfg = VectorStoreConfig(backend="hip", collection_name="mixedk", persist_directory=str(tmp_path),
                            index_params={"persist": False})
    store = HipVectorStore(cfg)
    store.add_chunks_sync([Chunk(id=f"c{i}", document_id=f"d{i // 500}", content=f"text {i}", chunk_index=i % 500,
                                 metadata={}, embedding=raw[i].tolist()) for i in range(n)])
    rc = RetrieverConfig(top_k=5, similarity_threshold=0.0)
    fused, plain = VectorRetriever(store, Emb(), rc), VectorRetriever(store, Plain(), rc)
    assert fused._fused is not None and fused._fused.max_batch == 32 and plain._fused is None
    ident = lambda res: [[(r.chunk.id, r.score, r.rank) for r in x] for x in res]  # noqa: E731
    want = ident([asyncio.run(plain.retrieve(nm, top_k=k)) for nm, k in zip(names, ks)])
    assert [len(w) for w in want] == ks
    fr = fused._fused

    async def go():
        loop = asyncio.get_running_loop()
        Emb.entered.clear()
        Emb.gate.clear()
        Emb.hold = True
        all_calls = asyncio.gather(*[fused.retrieve(nm, top_k=k) for nm, k in zip(names, ks)], return_exceptions=True)

        def release():  # cohort 1 is in the held forward and the other three wait in the worker's queue
            if Emb.entered.is_set() and fr._work.qsize() == 3:
                Emb.gate.set()
            elif not all_calls.done():
                loop.call_later(0.001, release)

        loop.call_soon(release)
        return await all_calls

    searchers = []
    for run in range(2):
        got = asyncio.run(go())
        raised = [g for g in got if isinstance(g, BaseException)]
        assert not raised, raised[:3]
        assert Emb.gate.is_set() and ident(got) == want
        searchers.append(fr._searcher[1])
    assert searchers[0] is searchers[1] and searchers[0].kc == 32  # one searcher served both runs
    fr.close()  # (the worker counts a cohort after it has posted its results)
    # every cohort but a run's last was finalized with its successor already submitted
    assert fr.cohorts == 8 and fr.queries == 2 * nq and fr.pipelined == 6
    store.close()
