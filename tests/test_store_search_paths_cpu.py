"""CPU: a differential pin of the store's search layer -- every search form x every shape of ``filters`` x an index with
and without the native per-query-mask / derived calls.  The batch answer must equal the same queries issued one at a
time, each with its own filter (ids, scores, counts and member bits with ==), and the mixed_launches / grouped_launches
counters must advance by the literals below, read from a run of the commit before the search layer was refactored.
The async forms and the micro-batcher's grouping rules are pinned the same way."""
import asyncio

import numpy as np
import pytest

from collapse_ref import collapse_ref
from fake_index_examples import ExamplesOracleIndex
from fake_index_fused import FusedOracleIndex
from fake_index_masks import MaskOracleIndex
from fake_index_mmr import MmrOracleIndex
from fake_index_range import RangeOracleIndex
from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
from oracle import ref_numpy as R

DIM, N, B = 16, 200, 5


class CollapsedCalls:
    """The group column and the collapsed search of NativeIndex over an OracleIndex, by tests/collapse_ref.py."""

    groups = np.zeros(0, np.int32)

    def set_groups(self, row0, groups):
        g = np.asarray(groups, np.int32).reshape(-1)
        if len(self.groups) < row0 + len(g):
            self.groups = np.concatenate([self.groups, np.full(row0 + len(g) - len(self.groups), -1, np.int32)])
        self.groups[row0:row0 + len(g)] = g

    def search_collapsed(self, q, k, mask=None, probe=0):
        allowed = self.live.copy()
        if mask is not None:
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        return collapse_ref(self.rows, self.dtype, R.process_queries(np.atleast_2d(q), self.metric), self.groups, k,
                            allowed, self.metric)


class NativeIndex(CollapsedCalls, MaskOracleIndex, MmrOracleIndex, RangeOracleIndex, ExamplesOracleIndex,
                  FusedOracleIndex):
    """Every native call of a single-device exact index."""


class HostIndex(CollapsedCalls, MmrOracleIndex, RangeOracleIndex):
    """No search_masks, search_examples or search_fused: the store groups per where-clause and composes by-example and
    fused searches on the host (collapsed, MMR and range searches have no host form)."""


INDEXES = {"native": NativeIndex, "host": HostIndex}


def make_store(index_cls, **params):
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory="unused",
                            index_params={"dtype": "f32", "persist": False, "mixed_filters": True, **params})
    s = HipVectorStore(cfg, index_factory=lambda dim: index_cls(dim, "f32"))
    rng = np.random.default_rng(0)
    asyncio.run(s.add_chunks([
        Chunk(id=f"c{i}", document_id=f"d{i % 7}", content=f"text {i}", chunk_index=i // 7,
              metadata={"source": f"src_{i % 3}"}, embedding=rng.standard_normal(DIM).astype(np.float32).tolist())
        for i in range(N)]))
    return s


@pytest.fixture(scope="module", params=list(INDEXES))
def store(request):
    s = make_store(INDEXES[request.param])
    s.kind = request.param
    return s


A, C = {"source": "src_0"}, {"source": "src_2"}
FILTERS = {"none": None, "dict": A, "equal": [dict(A) for _ in range(B)], "mixed": [A, None, C, A, None]}
Q = np.random.default_rng(1).standard_normal((B, DIM)).astype(np.float32)
POS = [["c3"], ["c10", "c11"], ["c20"], [], ["c40", "c41", "c42"]]
NEG = [[], ["c12"], ["c21", "c22"], ["c30"], []]
SIZES = [2, 3]  # the fused forms: the B queries as two groups
T = np.float32(0.3)


def per_query(filters, i):
    return filters[i] if isinstance(filters, list) else filters


def pairs(hits):
    return [(c.id, s) for c, s in hits]


def topk(**kw):
    def batch(s, flt):
        return [pairs(r) for r in s.search_batch(Q, 5, flt, **kw)]

    def single(s, flt):
        return [pairs(s.search_batch(Q[i:i + 1], 5, per_query(flt, i), **kw)[0]) for i in range(B)]
    return batch, single


def range_form():
    def shape(r):
        return pairs(r.hits), r.total, r.truncated

    def batch(s, flt):
        return [shape(r) for r in s.search_range_batch(Q, T, 10, flt)]

    def single(s, flt):
        return [shape(s.search_range_batch(Q[i:i + 1], T, 10, per_query(flt, i))[0]) for i in range(B)]
    return batch, single


def count_form():
    def batch(s, flt):
        return s.count_above_batch(Q, T, flt)

    def single(s, flt):
        return [s.count_above_batch(Q[i:i + 1], T, per_query(flt, i))[0] for i in range(B)]
    return batch, single


def similar_form():
    def batch(s, flt):
        return [pairs(r) for r in s.search_similar_batch(POS, NEG, 5, flt, Q)]

    def single(s, flt):
        return [pairs(s.search_similar_batch([POS[i]], [NEG[i]], 5, per_query(flt, i), Q[i:i + 1])[0])
                for i in range(B)]
    return batch, single


def fused_form(fusion):
    starts = np.cumsum([0] + SIZES)
    groups = [Q[a:b] for a, b in zip(starts[:-1], starts[1:])]

    def shape(r):
        return pairs(r.hits), r.members

    def batch(s, flt):
        return [shape(r) for r in s.search_fused_batch(groups, 5, fusion=fusion, filters=flt)]

    def single(s, flt):
        out = []
        for g, (a, b) in zip(groups, zip(starts[:-1], starts[1:])):
            f = flt[a:b] if isinstance(flt, list) else flt
            out.append(shape(s.search_fused_batch([g], 5, fusion=fusion, filters=f)[0]))
        return out
    return batch, single


FORMS = {"plain": topk(), "collapse": topk(collapse=True), "mmr": topk(mmr_lambda=0.5), "range": range_form(),
         "count": count_form(), "similar": similar_form(), "fused_rrf": fused_form("rrf"),
         "fused_max": fused_form("max")}

# (mixed_launches, grouped_launches) one batch call adds for the "mixed" filter list (three distinct clauses); every
# other shape of `filters` is one clause for the whole batch and adds (0, 0)
LAUNCHES = {
    "native": {"plain": (1, 0), "collapse": (0, 3), "mmr": (0, 3), "range": (0, 3), "count": (0, 3),
               "similar": (0, 3), "fused_rrf": (1, 0), "fused_max": (1, 0)},
    "host": {"plain": (0, 3), "collapse": (0, 3), "mmr": (0, 3), "range": (0, 3), "count": (0, 3),
             "similar": (0, 3), "fused_rrf": (0, 3), "fused_max": (0, 3)},
}


@pytest.mark.parametrize("flt", list(FILTERS))
@pytest.mark.parametrize("form", list(FORMS))
def test_batch_equals_one_at_a_time(store, form, flt):
    batch, single = FORMS[form]
    want = single(store, FILTERS[flt])
    before = store.mixed_launches, store.grouped_launches
    got = batch(store, FILTERS[flt])
    added = store.mixed_launches - before[0], store.grouped_launches - before[1]
    print(store.kind, form, flt, added)
    assert got == want
    assert len(got) == (len(SIZES) if form.startswith("fused") else B)
    if form != "count":  # something was found, so the comparison says something
        assert all(len(r[0] if isinstance(r, tuple) else r) for r in got)
    assert added == (LAUNCHES[store.kind][form] if flt == "mixed" else (0, 0))


def test_async_forms_equal_the_batch_forms(store):
    q = Q[0].tolist()
    for kw in ({}, {"collapse": True}, {"mmr_lambda": 0.5}):
        got = asyncio.run(store.search(q, 5, A, **kw))
        assert pairs(got) == pairs(store.search_batch(Q[:1], 5, A, **kw)[0]) and len(got) == 5
    r = asyncio.run(store.search_range(q, float(T), 10, A))
    w = store.search_range_batch(Q[:1], T, 10, A)[0]
    assert (pairs(r.hits), r.total) == (pairs(w.hits), w.total) and r.total > 0
    got = asyncio.run(store.search_similar(POS[1], 5, A, negative_ids=NEG[1], query_embedding=q))
    assert pairs(got) == pairs(store.search_similar_batch([POS[1]], [NEG[1]], 5, A, Q[:1])[0]) and len(got) == 5
    for flt in (A, [A, None, C]):
        f = asyncio.run(store.search_fused(Q[:3], 5, flt, fusion="max"))
        w = store.search_fused_batch([Q[:3]], 5, fusion="max", filters=flt)[0]
        assert (pairs(f.hits), f.members) == (pairs(w.hits), w.members) and len(f.hits) == 5


def test_concurrent_searches_group_by_mode(store):
    """Eight concurrent calls -- plain, collapsed and two MMR lambdas, two of each with different top_k -- are four
    launches, and every caller's list is its own top_k long and equals its own synchronous answer."""
    calls = [({}, 3), ({}, 6), ({"collapse": True}, 2), ({"collapse": True}, 4), ({"mmr_lambda": 0.5}, 3),
             ({"mmr_lambda": 0.5}, 7), ({"mmr_lambda": 0.25}, 4), ({"mmr_lambda": 0.25}, 5)]

    async def go():
        return await asyncio.gather(*[store.search(Q[i % B].tolist(), k, None, **kw)
                                      for i, (kw, k) in enumerate(calls)])

    before = store._batcher.launches
    got = asyncio.run(go())
    assert store._batcher.launches - before == 4
    for i, ((kw, k), r) in enumerate(zip(calls, got)):
        assert len(r) == k
        if "mmr_lambda" in kw:  # (the default pool follows top_k: ask for the pool the shared launch ran with)
            kw = dict(kw, fetch_k=32)
        assert pairs(r) == pairs(store.search_batch(Q[i % B][None], k, None, **kw)[0])


def test_concurrent_plain_searches_fill_across_filters_only_with_the_option():
    flt = [A, None, C, A, None]
    for mixed, launches in ((True, 1), (False, 3)):
        s = make_store(NativeIndex, mixed_filters=mixed)

        async def go():
            return await asyncio.gather(*[s.search(Q[i].tolist(), 4, flt[i]) for i in range(B)])

        got = asyncio.run(go())
        assert s._batcher.launches == launches and s.mixed_launches == (1 if mixed else 0)
        assert [pairs(r) for r in got] == [pairs(s.search_batch(Q[i:i + 1], 4, flt[i])[0]) for i in range(B)]
