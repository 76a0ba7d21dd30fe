"""CPU: every bad search request against its exact exception type and text, raised before any index call (the stand-in
index records zero calls).  Where one request trips two checks, the table fixes which one wins."""
import asyncio

import numpy as np
import pytest
import torch

from fake_index import OracleIndex
from test_store_search_paths_cpu import DIM, NEG, POS, A, B, C, NativeIndex, Q, make_store

CALLS = ("search", "search_masks", "search_mmr", "search_collapsed", "set_groups", "search_range", "search_examples",
         "build_queries", "search_fused", "get_rows")


class Recording(NativeIndex):
    """NativeIndex of the paths test, every search-side call written down."""


def _recorded(name):
    def call(self, *a, **kw):
        self.calls.append(name)
        return getattr(super(Recording, self), name)(*a, **kw)
    return call


for _name in CALLS:
    setattr(Recording, _name, _recorded(_name))


@pytest.fixture(scope="module")
def stores():
    out = {"single": make_store(Recording), "unmixed": make_store(Recording, mixed_filters=False),
           "multi": make_store(Recording)}
    out["multi"]._index.devices = [0, 0]
    for s in out.values():
        s._index.calls = []
    return out


W = np.zeros((B, DIM + 1), np.float32)  # the wrong dim
MIXED = [A, None, C, A, None]
SHORT = [A, None, C, A]
GROUPS = [Q[:2], Q[2:]]
NAN = float("nan")
DIM_MSG = "query dim 17 != collection dim 16"
FLT_MSG = "4 filters for 5 queries"
K_MSG = "a collapsed search returns at most 128 groups (top_k = 129)"
ONE_DEV = "a %s search needs a single-device store"
MMR_DEV = "an MMR search needs a single-device store"


def aw(method, *a, **kw):
    return lambda s: asyncio.run(getattr(s, method)(*a, **kw))


def sy(method, *a, **kw):
    return lambda s: getattr(s, method)(*a, **kw)


CASES = [
    # ---- wrong dim, every form
    ("dim plain", "single", sy("search_batch", W, 5), ValueError, DIM_MSG),
    ("dim collapse", "single", sy("search_batch", W, 5, collapse=True), ValueError, DIM_MSG),
    ("dim mmr", "single", sy("search_batch", W, 5, mmr_lambda=0.5), ValueError, DIM_MSG),
    ("dim search", "single", aw("search", W[0].tolist(), 5), ValueError, DIM_MSG),
    ("dim search mmr", "single", aw("search", W[0].tolist(), 5, mmr_lambda=0.5), ValueError, DIM_MSG),
    ("dim range", "single", sy("search_range_batch", W, 0.3), ValueError, DIM_MSG),
    ("dim count", "single", sy("count_above_batch", W, 0.3), ValueError, DIM_MSG),
    ("dim search_range", "single", aw("search_range", W[0].tolist(), 0.3), ValueError, DIM_MSG),
    ("dim similar", "single", sy("search_similar_batch", POS, NEG, 5, None, W), ValueError, DIM_MSG),
    ("dim search_similar", "single", aw("search_similar", "c1", 5, query_embedding=W[0].tolist()), ValueError, DIM_MSG),
    ("dim fused", "single", sy("search_fused_batch", [W[:2], W[2:]], 5), ValueError, "query dim != collection dim 16"),
    ("dim search_fused", "single", aw("search_fused", W[:2], 5), ValueError, "query dim != collection dim 16"),
    ("dim device", "single", sy("search_device_sync", torch.zeros(B, DIM + 1), 5), ValueError,
     "queries must be (B, 16)"),
    ("dim masks device", "single", sy("search_masks_device_sync", torch.zeros(B, DIM + 1), 5, MIXED), ValueError,
     "queries must be (B, 16)"),
    ("1-d device", "single", sy("search_device_sync", torch.zeros(DIM), 5), ValueError, "queries must be (B, 16)"),
    # ---- one filter per query, the wrong number of them
    ("filters plain", "single", sy("search_batch", Q, 5, SHORT), ValueError, FLT_MSG),
    ("filters tuple", "single", sy("search_batch", Q, 5, tuple(SHORT)), ValueError, FLT_MSG),
    ("filters collapse", "single", sy("search_batch", Q, 5, SHORT, collapse=True), ValueError, FLT_MSG),
    ("filters mmr", "single", sy("search_batch", Q, 5, SHORT, mmr_lambda=0.5), ValueError, FLT_MSG),
    ("filters range", "single", sy("search_range_batch", Q, 0.3, 10, SHORT), ValueError, FLT_MSG),
    ("filters count", "single", sy("count_above_batch", Q, 0.3, SHORT), ValueError, FLT_MSG),
    ("filters similar", "single", sy("search_similar_batch", POS, NEG, 5, SHORT), ValueError, FLT_MSG),
    ("filters fused", "single", sy("search_fused_batch", GROUPS, 5, filters=SHORT), ValueError, FLT_MSG),
    ("filters masks device", "single", sy("search_masks_device_sync", torch.zeros(B, DIM), 5, SHORT), ValueError,
     FLT_MSG),
    ("dim before filters", "single", sy("search_batch", W, 5, SHORT), ValueError, DIM_MSG),
    ("dim before filters, range", "single", sy("search_range_batch", W, 0.3, 10, SHORT), ValueError, DIM_MSG),
    ("dim before filters, masks device", "single", sy("search_masks_device_sync", torch.zeros(B, DIM + 1), 5, SHORT),
     ValueError, "queries must be (B, 16)"),
    # ---- MMR
    ("lambda high", "single", sy("search_batch", Q, 5, mmr_lambda=1.5), ValueError,
     "mmr_lambda must be in [0, 1] (got 1.5)"),
    ("lambda negative", "single", aw("search", Q[0].tolist(), 5, mmr_lambda=-0.1), ValueError,
     "mmr_lambda must be in [0, 1] (got -0.1)"),
    ("lambda nan", "single", sy("search_batch", Q, 5, mmr_lambda=NAN), ValueError,
     "mmr_lambda must be in [0, 1] (got nan)"),
    ("lambda nan, search", "single", aw("search", Q[0].tolist(), 5, mmr_lambda=NAN), ValueError,
     "mmr_lambda must be in [0, 1] (got nan)"),
    ("lambda with collapse", "single", sy("search_batch", Q, 5, mmr_lambda=0.5, collapse=True), ValueError,
     "mmr_lambda and collapse=True do not combine"),
    ("lambda with collapse, search", "single", aw("search", Q[0].tolist(), 5, mmr_lambda=0.5, collapse=True),
     ValueError, "mmr_lambda and collapse=True do not combine"),
    ("collapse before a bad lambda", "single", sy("search_batch", Q, 5, mmr_lambda=7, collapse=True), ValueError,
     "mmr_lambda and collapse=True do not combine"),
    ("fetch_k low", "single", sy("search_batch", Q, 5, mmr_lambda=0.5, fetch_k=3), ValueError,
     "fetch_k must be in [top_k, 128] (got 3, top_k = 5)"),
    ("fetch_k high", "single", aw("search", Q[0].tolist(), 5, mmr_lambda=0.5, fetch_k=129), ValueError,
     "fetch_k must be in [top_k, 128] (got 129, top_k = 5)"),
    ("mmr top_k", "single", sy("search_batch", Q, 129, mmr_lambda=0.5), ValueError,
     "an MMR search returns at most 128 hits (top_k = 129)"),
    ("lambda before dim", "single", sy("search_batch", W, 5, mmr_lambda=2), ValueError,
     "mmr_lambda must be in [0, 1] (got 2)"),
    ("lambda before top_k <= 0", "single", aw("search", Q[0].tolist(), 0, mmr_lambda=2), ValueError,
     "mmr_lambda must be in [0, 1] (got 2)"),
    # ---- collapsed top_k
    ("collapsed k, search", "single", aw("search", Q[0].tolist(), 129, collapse=True), ValueError, K_MSG),
    ("collapsed k, search_batch", "single", sy("search_batch", Q, 129, collapse=True), ValueError, K_MSG),
    ("collapsed k, one dict", "single", sy("search_batch", Q, 129, A, collapse=True), ValueError, K_MSG),
    ("collapsed k, mixed filters", "single", sy("search_batch", Q, 129, MIXED, collapse=True), ValueError, K_MSG),
    ("collapsed k before dim, search", "single", aw("search", W[0].tolist(), 129, collapse=True), ValueError, K_MSG),
    ("dim before collapsed k, search_batch", "single", sy("search_batch", W, 129, collapse=True), ValueError, DIM_MSG),
    ("collapsed k before a bad where-clause", "single", sy("search_batch", Q, 129, {"$nope": 1}, collapse=True),
     ValueError, K_MSG),
    ("a bad where-clause before collapsed k, mixed", "single",
     sy("search_batch", Q, 129, [A, None, {"$nope": 1}, A, None], collapse=True), ValueError,
     "unsupported top-level operator '$nope'"),
    ("devices before a bad where-clause", "multi", sy("search_batch", Q, 5, {"$nope": 1}, mmr_lambda=0.5), ValueError,
     MMR_DEV),
    ("collapsed k before devices", "multi", sy("search_batch", Q, 129, collapse=True), ValueError, K_MSG),
    ("collapsed k before devices, mixed", "multi", sy("search_batch", Q, 129, MIXED, collapse=True), ValueError, K_MSG),
    # ---- range
    ("max_hits negative", "single", sy("search_range_batch", Q, 0.3, -1), ValueError,
     "max_hits must be in [0, 65536] (got -1)"),
    ("max_hits high", "single", aw("search_range", Q[0].tolist(), 0.3, 65537), ValueError,
     "max_hits must be in [0, 65536] (got 65537)"),
    ("min_score nan", "single", sy("search_range_batch", Q, NAN), ValueError, "min_score must not be NaN"),
    ("min_score nan, count", "single", sy("count_above_batch", Q, [0.1, 0.2, NAN, 0.3, 0.4]), ValueError,
     "min_score must not be NaN"),
    ("threshold count", "single", sy("search_range_batch", Q, [0.1, 0.2]), ValueError, "2 thresholds for 5 queries"),
    ("dim before max_hits", "single", sy("search_range_batch", W, 0.3, -1), ValueError, DIM_MSG),
    ("max_hits before nan", "single", sy("search_range_batch", Q, NAN, -1), ValueError,
     "max_hits must be in [0, 65536] (got -1)"),
    ("threshold count before nan", "single", sy("search_range_batch", Q, [NAN, 0.2]), ValueError,
     "2 thresholds for 5 queries"),
    ("nan before filters", "single", sy("search_range_batch", Q, NAN, 10, SHORT), ValueError,
     "min_score must not be NaN"),
    # ---- by example
    ("too many examples", "single", sy("search_similar_batch", [[f"x{i}" for i in range(30)]], [["y1", "y2", "y3"]]),
     ValueError, "a query takes at most 32 example chunks (got 33)"),
    ("unknown id", "single", sy("search_similar_batch", [["c1", "nope"]]), ValueError, "unknown chunk id 'nope'"),
    ("unknown id, search_similar", "single", aw("search_similar", "nope"), ValueError, "unknown chunk id 'nope'"),
    ("unknown negative id", "single", aw("search_similar", "c1", negative_ids="gone"), ValueError,
     "unknown chunk id 'gone'"),
    ("nothing to go by", "single", sy("search_similar_batch", [["c1"], []]), ValueError,
     "a query without example chunks needs a query embedding"),
    ("negative lists", "single", sy("search_similar_batch", [["c1"], ["c2"]], [["c3"]]), ValueError,
     "1 negative lists for 2 queries"),
    ("query embeddings", "single", sy("search_similar_batch", [["c1"], ["c2"]], None, 5, None, Q[:1]), ValueError,
     "1 query embeddings for 2 queries"),
    ("query embeddings before dim", "single", sy("search_similar_batch", [["c1"], ["c2"]], None, 5, None, W[:1]),
     ValueError, "1 query embeddings for 2 queries"),
    ("weights", "single", sy("search_similar_batch", [["c1"]], pos_weight=float("inf")), ValueError,
     "pos_weight and neg_weight must be finite"),
    ("filters before unknown id", "single", sy("search_similar_batch", [["nope"]] * B, None, 5, SHORT), ValueError,
     FLT_MSG),
    ("dim before filters, similar", "single", sy("search_similar_batch", POS, NEG, 5, SHORT, W), ValueError, DIM_MSG),
    # ---- fused
    ("fusion", "single", sy("search_fused_batch", GROUPS, 5, fusion="avg"), ValueError,
     "fusion must be 'rrf' or 'max' (got 'avg')"),
    ("fusion, search_fused", "single", aw("search_fused", Q[:2], 5, fusion="avg"), ValueError,
     "fusion must be 'rrf' or 'max' (got 'avg')"),
    ("fusion before dim", "single", sy("search_fused_batch", [W[:2]], 5, fusion="avg"), ValueError,
     "fusion must be 'rrf' or 'max' (got 'avg')"),
    ("members", "single", sy("search_fused_batch", [np.zeros((17, DIM), np.float32)], 5), ValueError,
     "a group takes 1 to 16 query embeddings"),
    ("fused top_k", "single", sy("search_fused_batch", GROUPS, 129), ValueError,
     "a fused search returns at most 128 hits (top_k = 129)"),
    ("dim before fused top_k", "single", sy("search_fused_batch", [W[:2]], 129), ValueError,
     "query dim != collection dim 16"),
    ("rrf_k", "single", sy("search_fused_batch", GROUPS, 5, rrf_k=-1), ValueError,
     "rrf_k must be finite and not negative (got -1)"),
    ("fused fetch_k", "single", sy("search_fused_batch", GROUPS, 5, fetch_k=4), ValueError,
     "fetch_k must be in [top_k, 128] (got 4, top_k = 5)"),
    ("weights with max", "single", sy("search_fused_batch", GROUPS, 5, fusion="max", weights=[[1, 1], [1, 1, 1]]),
     ValueError, "max fusion takes no weights"),
    ("weights shape", "single", sy("search_fused_batch", GROUPS, 5, weights=[[1, 1], [1, 1]]), ValueError,
     "weights must have the shape of query_groups"),
    ("weights shape, search_fused", "single", aw("search_fused", Q[:3], 5, weights=[1, 1]), ValueError,
     "weights must have the shape of query_groups"),
    ("weights finite", "single", sy("search_fused_batch", GROUPS, 5, weights=[[1, NAN], [1, 1, 1]]), ValueError,
     "weights must be finite"),
    ("weights with max before filters", "single",
     sy("search_fused_batch", GROUPS, 5, fusion="max", weights=[[1, 1], [1, 1, 1]], filters=SHORT), ValueError,
     "max fusion takes no weights"),
    ("member filters", "unmixed", sy("search_fused_batch", GROUPS, 5, filters=MIXED), ValueError,
     "one filter per member needs index_params.mixed_filters = true"),
    ("member filters, search_fused", "unmixed", aw("search_fused", Q[:3], 5, [A, None, C]), ValueError,
     "one filter per member needs index_params.mixed_filters = true"),
    ("filter count before member filters", "unmixed", sy("search_fused_batch", GROUPS, 5, filters=SHORT), ValueError,
     FLT_MSG),
    # ---- the single-device forms on a multi-device handle
    ("devices mmr", "multi", sy("search_batch", Q, 5, mmr_lambda=0.5), ValueError, MMR_DEV),
    ("devices mmr, mixed", "multi", sy("search_batch", Q, 5, MIXED, mmr_lambda=0.5), ValueError, MMR_DEV),
    ("devices mmr, search", "multi", aw("search", Q[0].tolist(), 5, mmr_lambda=0.5), ValueError, MMR_DEV),
    ("devices collapsed", "multi", sy("search_batch", Q, 5, collapse=True), ValueError, ONE_DEV % "collapsed"),
    ("devices collapsed, mixed", "multi", sy("search_batch", Q, 5, MIXED, collapse=True), ValueError,
     ONE_DEV % "collapsed"),
    ("devices collapsed, search", "multi", aw("search", Q[0].tolist(), 5, A, collapse=True), ValueError,
     ONE_DEV % "collapsed"),
    ("devices range", "multi", sy("search_range_batch", Q, 0.3), ValueError, ONE_DEV % "range"),
    ("devices count", "multi", sy("count_above_batch", Q, 0.3, MIXED), ValueError, ONE_DEV % "range"),
    ("devices search_range", "multi", aw("search_range", Q[0].tolist(), 0.3), ValueError, ONE_DEV % "range"),
    ("filters before devices, range", "multi", sy("search_range_batch", Q, 0.3, 10, SHORT), ValueError, FLT_MSG),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bad_request(stores, case):
    _, which, request, exc, text = case
    s = stores[which]
    with pytest.raises(exc) as e:
        request(s)
    assert type(e.value) is exc and str(e.value) == text
    assert s._index.calls == []
    assert not s._batcher.pending and not s._batcher.running


def test_an_index_without_the_native_call():
    """Collapsed, MMR and range searches have no host form: the index's type is named, nothing is searched."""
    s = make_store(OracleIndex)
    for request, what in ((sy("search_batch", Q, 5, mmr_lambda=0.5), "MMR"),
                          (sy("search_batch", Q, 5, [A, None, C, A, None], mmr_lambda=0.5), "MMR"),
                          (sy("search_batch", Q, 5, collapse=True), "collapsed"),
                          (aw("search", Q[0].tolist(), 5, collapse=True), "collapsed"),
                          (sy("search_range_batch", Q, 0.3), "range"),
                          (sy("count_above_batch", Q, 0.3, [A, None, C, A, None]), "range")):
        with pytest.raises(NotImplementedError) as e:
            request(s)
        assert str(e.value) == f"OracleIndex has no {what} search"
    assert s._index.searches == 0


def test_the_multi_device_forms_that_do_run(stores):
    """Plain, by-example and fused searches take a multi-device handle (grouped / composed on the host)."""
    s = stores["multi"]
    try:
        assert len(s.search_batch(Q, 5, MIXED)) == B and "search_masks" not in s._index.calls
        assert len(s.search_similar_batch(POS, NEG, 5, MIXED, Q)) == B and "search_examples" not in s._index.calls
        assert len(s.search_fused_batch(GROUPS, 5, filters=MIXED)) == 2 and "search_fused" not in s._index.calls
    finally:
        s._index.calls.clear()
