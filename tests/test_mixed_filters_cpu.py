"""CPU: host logic of mixed-filter batches -- per-query filters in search_batch, the micro-batcher's merge across
filter keys under index_params.mixed_filters, the grouping fallbacks, the retrievers' pass-through.  The device index
is the oracle-backed tests/fake_index_masks.MaskOracleIndex (its search_masks counts as ONE launch)."""
import asyncio
import os
import subprocess

import numpy as np
import pytest

from fake_index import OracleIndex
from fake_index_masks import GroupMaskOracleIndex, MaskOracleIndex
from hiprag.rag import (BatchedVectorRetriever, Chunk, HipVectorStore, RetrieverConfig, VectorRetriever,
                        VectorStoreConfig)

DIM = 16


def run(coro):
    return asyncio.run(coro)


def make_store(tmp_path, index_cls=MaskOracleIndex, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "f32", "persist": False, **params})
    return HipVectorStore(cfg, index_factory=lambda dim: index_cls(dim, "f32"))


def fill(store, docs=8, per_doc=40):
    rng = np.random.default_rng(0)
    cs = [Chunk(id=f"d{d}_{i}", document_id=f"d{d}", content=f"{d} {i}", chunk_index=i,
                metadata={"source": f"src_{d}", "index_type": "index_content"},
                embedding=rng.standard_normal(DIM).astype(np.float32).tolist())
          for d in range(docs) for i in range(per_doc)]
    run(store.add_chunks(cs))
    return cs


def ids(res):
    return [[(c.id, s) for c, s in r] for r in res]


def queries(n, seed=1):
    return np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)


def filters_for(n, docs=8):
    """source filters of `docs` documents and None, by turns"""
    return [None if i % (docs + 1) == docs else {"source": f"src_{i % (docs + 1)}"} for i in range(n)]


def test_search_batch_list_form_results_and_validation(tmp_path):
    s = make_store(tmp_path)
    fill(s)
    q, flt = queries(20), filters_for(20)
    want = [s.search_batch(q[i:i + 1], 5, flt[i])[0] for i in range(20)]
    before = s._index.searches
    got = s.search_batch(q, 5, flt)
    assert ids(got) == ids(want)
    assert s._index.searches - before == 1 and s._index.mask_calls[-1] == (20, 8) and s.mixed_launches == 1
    for r, f in zip(got, flt):
        assert f is None or all(c.metadata["source"] == f["source"] for c, _ in r)
    with pytest.raises(ValueError):
        s.search_batch(q, 5, flt[:-1])
    with pytest.raises(ValueError):
        s.search_batch(q[:3], 5, flt[:4])
    # the dict and None forms are unchanged, and one distinct predicate takes the single-mask search
    n_mask = len(s._index.mask_calls)
    one = {"source": "src_3"}
    assert ids(s.search_batch(q, 5, [one] * 20)) == ids(s.search_batch(q, 5, one))
    assert ids(s.search_batch(q, 5, [None] * 20)) == ids(s.search_batch(q, 5, None)) == ids(s.search_batch(q, 5))
    assert len(s._index.mask_calls) == n_mask
    # a filter nothing matches and top_k beyond the allowed rows
    got = s.search_batch(q[:3], 100, [{"source": "nowhere"}, {"source": "src_0"}, None])
    assert [len(r) for r in got] == [0, 40, 100]


@pytest.mark.parametrize("index_cls", [OracleIndex, GroupMaskOracleIndex])
def test_list_form_groups_where_the_index_takes_no_masks(tmp_path, index_cls):
    """An index without search_masks, and a multi-device handle that refuses it: one launch per distinct filter."""
    s = make_store(tmp_path, index_cls)
    fill(s)
    q, flt = queries(20), filters_for(20)
    want = [s.search_batch(q[i:i + 1], 5, flt[i])[0] for i in range(20)]
    before = s._index.searches
    assert ids(s.search_batch(q, 5, flt)) == ids(want)
    assert s._index.searches - before == 9 and s.grouped_launches == 9 and s.mixed_launches == 0


def _concurrent(s, q, flt, ks, collapse=None):
    async def go():
        return await asyncio.gather(*[
            s.search(query_embedding=q[i].tolist(), top_k=ks[i], filters=flt[i],
                     **({"collapse": True} if collapse and collapse[i] else {})) for i in range(len(q))])
    return run(go())


def test_batcher_merges_across_filters_only_with_the_option(tmp_path):
    q, flt = queries(64), filters_for(64)
    ks = [3 + i % 5 for i in range(64)]
    off = make_store(tmp_path / "off")
    on = make_store(tmp_path / "on", mixed_filters=True)
    assert not off.mixed_filters and on.mixed_filters
    fill(off)
    fill(on)
    want = [run(off.search(query_embedding=q[i].tolist(), top_k=ks[i], filters=flt[i])) for i in range(64)]
    # default: one launch per filter group (8 sources and None), as before
    b0, l0 = off._index.searches, off._batcher.launches
    assert ids(_concurrent(off, q, flt, ks)) == ids(want)
    assert off._index.searches - b0 == 9 and off._batcher.launches - l0 == 9 and not off._index.mask_calls
    # mixed_filters: one launch, one per-query-mask search
    b0, l0 = on._index.searches, on._batcher.launches
    assert ids(_concurrent(on, q, flt, ks)) == ids(want)
    assert on._index.searches - b0 == 1 and on._batcher.launches - l0 == 1 and on._index.mask_calls == [(64, 8)]
    # 130 calls: chunks of max_batch
    q2, f2 = queries(130, 2), filters_for(130)
    l0 = on._batcher.launches
    got = _concurrent(on, q2, f2, [4] * 130)
    assert on._batcher.launches - l0 == 3
    assert ids(got) == ids([off.search_batch(q2[i:i + 1], 4, f2[i])[0] for i in range(130)])
    # one filter for every call: the single-mask search, no per-query masks
    n_mask = len(on._index.mask_calls)
    _concurrent(on, q[:10], [{"source": "src_1"}] * 10, [3] * 10)
    assert len(on._index.mask_calls) == n_mask


def test_collapsed_queries_never_share_a_launch_with_plain_ones(tmp_path):
    launches = []

    class Recording(MaskOracleIndex):
        def set_groups(self, row0, groups):
            pass

        def search_collapsed(self, q, k, mask=None, probe=0):
            launches.append(("collapsed", len(np.atleast_2d(q))))
            return self.search(q, k, mask)

        def search_masks(self, q, k, masks, mask_of):
            launches.append(("masks", len(q)))
            return super().search_masks(q, k, masks, mask_of)

    s = make_store(tmp_path, Recording, mixed_filters=True)
    fill(s)
    q = queries(12)
    flt = [{"source": f"src_{i % 3}"} for i in range(12)]
    collapse = [i % 2 == 0 for i in range(12)]
    _concurrent(s, q, flt, [3] * 12, collapse)
    # the six plain calls share one per-query-mask launch; the collapsed ones keep one launch per filter group
    assert sorted(launches) == [("collapsed", 2)] * 3 + [("masks", 6)]


def test_batched_retriever_passes_per_query_filters(tmp_path):
    s = make_store(tmp_path)
    cs = fill(s)
    table = {f"q{i}": np.asarray(cs[i * 7].embedding, np.float32) for i in range(12)}

    class Emb:
        async def embed_query(self, q):
            return table[q].tolist()

    names = list(table)
    flt = filters_for(12, docs=3)
    cfg = RetrieverConfig(top_k=4, similarity_threshold=0.0)
    ret = BatchedVectorRetriever(s, Emb(), cfg)
    before = s._index.searches
    got = run(ret.batch_retrieve(names, top_k=4, filters=flt))
    assert s._index.searches - before == 1
    one = VectorRetriever(s, Emb(), cfg)
    want = [run(one.retrieve(n, top_k=4, filters=f)) for n, f in zip(names, flt)]
    assert [[(r.chunk.id, r.score, r.rank) for r in x] for x in got] == \
        [[(r.chunk.id, r.score, r.rank) for r in x] for x in want]
    with pytest.raises(ValueError):
        run(ret.batch_retrieve(names, top_k=4, filters=flt[:5]))


def test_new_symbols_are_exported_and_the_abi_version_stays():
    from hiprag import _native

    new = {"hr_index_search_masks", "hr_index_search_masks_device", "hr_index_qmask_launches"}
    assert new <= set(_native.EXPORTS)
    assert callable(_native.NativeIndex.search_masks) and callable(_native.NativeIndex.search_masks_device)
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libhiprag.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert new <= exported
    assert _native.load_library().hr_abi_version() == 2
