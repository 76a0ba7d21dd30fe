"""GPU: boosted search (hr_boost.hip) against tests/boost_ref.py -- rows equal, blended values equal as
fp64 bit patterns, scores equal as fp32 bit patterns.

Which stage answered is asserted too, and never from the library's own numbers: boost_ref.mechanism restates the pilot
pool, tau, the columns' extrema, the bisection for the floor and the exact window count, so every query's stage (1 iff
the count is <= window) is known before the GPU result is looked at, and the boost_stats deltas must equal the class
counts exactly."""
import asyncio

import numpy as np
import pytest

import boost_ref as BR
import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 31, 32, 33, 64, 65, 1000, 4099]
DTYPES = ["f32", "bf16", "f16"]
METRICS = ["cosine", "ip", "l2"]
WEIGHTS = [(1.0, 0.0), (1.0, 0.05), (1.0, 0.25), (0.5, 0.5), (1.0, -0.25), (1.0, 2.0)]


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


# ---------------------------------------------------------------- inputs and the reference (CPU only)
def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def make_rows(rng, n, metric, dim=64):
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    if metric != "cosine":
        x = x * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32)


def planted(rng, x, B, noise=0.05):
    pick = rng.choice(len(x), B, replace=len(x) < B)
    e = rng.standard_normal((B, x.shape[1])).astype(np.float32)
    return np.ascontiguousarray(_unit(x[pick]) + np.float32(noise) * _unit(e), np.float32)


class Ref:
    """The fp64 score matrix of one (rows, queries) pair, computed once and shared by every weight, k and window."""

    def __init__(self, x, q, dtype, metric):
        self.dtype, self.metric = dtype, metric
        self.stored = R.process_rows(x, metric, dtype)
        self.qp = R.process_queries(q, metric)
        self.s = np.concatenate([R.exact_scores(self.stored, dtype, self.qp[b:b + 32], metric)
                                 for b in range(0, len(self.qp), 32)]) if len(x) else np.zeros((len(q), 0))
        self.B, self.n = len(q), len(x)

    def ref(self, k, alpha, betas, cols, allowed=None):
        return BR.boost_ref(self.stored, self.dtype, self.qp, k, alpha, betas, cols, allowed, self.metric, scores=self.s)

    def mech(self, k, alpha, betas, cols, allowed=None, probe=0, window=0):
        return BR.mechanism(self.stored, self.dtype, self.qp, k, alpha, betas, cols, allowed, self.metric, probe, window,
                            scores=self.s)


def build(native, x, dtype="bf16", metric="cosine", cols=()):
    idx = native.NativeIndex(x.shape[1], dtype, metric)
    idx.add(x)
    for c, col in enumerate(cols):
        idx.set_boost(c, 0, col)
    return idx


def check(idx, ref, q, k, alpha, betas, cols, allowed=None, probe=0, window=0, need=None):
    """One host-form call against the reference; the stage of every query comes from the reference first.  need: 1 / 2
    = every query must be answered by that stage.  Returns (result, stage-1 queries, stage-2 queries)."""
    stage = ref.mech(k, alpha, betas, cols, allowed, probe, window)["stage"]
    one, two = int((stage == 1).sum()), int((stage == 2).sum())
    if need is not None:
        assert (one, two) == ((ref.B, 0) if need == 1 else (0, ref.B)), (one, two)
    want = ref.ref(k, alpha, betas, cols, allowed)
    st0 = idx.boost_stats()
    got = idx.search_boosted(q, k, alpha, betas, None if allowed is None else oracle.mask_from_bool(allowed), probe,
                             window)
    st1 = idx.boost_stats()
    BR.assert_same(got, want)
    assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (one, two)
    return got, one, two


# ---------------------------------------------------------------- 1. every row count x dtype x metric
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_row_counts_dtypes_metrics(native, dtype, metric):
    """The issue's weight grid on one U[0, 1) column at k = 10, and k = 1 / 128 at (0.5, 0.5); windows 0 (the default)
    and 16, which sends the larger row counts through stage 2."""
    rng = np.random.default_rng(10 * DTYPES.index(dtype) + METRICS.index(metric))
    staged = [0, 0]
    for n in ROW_COUNTS:
        x = make_rows(rng, n, metric)
        q = planted(rng, x, 3)
        col = rng.random(n).astype(np.float32)
        ref = Ref(x, q, dtype, metric)
        idx = build(native, x, dtype, metric, [col])
        for alpha, beta in WEIGHTS:
            for window in (0, 16):
                _, one, two = check(idx, ref, q, 10, alpha, [beta], [col], window=window)
                staged[0] += one
                staged[1] += two
        for k in (1, 128):
            check(idx, ref, q, k, 0.5, [0.5], [col])
        # alpha = 1, beta = 0 is the plain search, bit for bit
        v, s, r = idx.search_boosted(q, 10, 1.0, [0.0])
        ps, pr = idx.search(q, 10)
        assert (r == pr).all() and (s.view(np.uint32) == ps.view(np.uint32)).all()
        idx.close()
    assert staged[0] > 100 and staged[1] >= 9  # both stages were asserted


# ---------------------------------------------------------------- 2. the plain search's forms, batch sizes, padded dims
@pytest.mark.parametrize("B", [1, 3, 65])
def test_identity_forms_equal_the_plain_search(native, B):
    rng = np.random.default_rng(20 + B)
    x = make_rows(rng, 4099, "cosine")
    q = planted(rng, x, B)
    col = rng.random(4099).astype(np.float32)
    idx = build(native, x, "bf16", "cosine", [col])
    idx.set_boost(1, 0, np.zeros(10, np.float32))  # column 1: all zero; column 2: never set
    for k in (1, 10, 128):
        ps, pr = idx.search(q, k)
        for betas in ([], [0.0], [0.0, 0.7], [0.0, 0.7, -3.0]):
            v, s, r = idx.search_boosted(q, k, 1.0, betas)
            assert (r == pr).all() and (s.view(np.uint32) == ps.view(np.uint32)).all()
            assert (v.astype(np.float32) == ps).all()  # v = 1 * s + 0 = s
    ref = Ref(x, q, "bf16", "cosine")
    check(idx, ref, q, 10, 0.5, [0.5], [col], need=1)
    check(idx, ref, q, 10, 0.5, [0.5], [col], probe=128, window=32, need=2)
    idx.close()


def test_padded_dims(native):
    rng = np.random.default_rng(31)
    x = make_rows(rng, 1000, "l2", dim=200)
    q = planted(rng, x, 3)
    col = rng.random(1000).astype(np.float32)
    ref = Ref(x, q, "f16", "l2")
    idx = build(native, x, "f16", "l2", [col])
    for window in (0, 10):
        check(idx, ref, q, 10, 1.0, [0.25], [col], window=window)
    idx.close()


# ---------------------------------------------------------------- 3. one to four columns, mixed signs
def test_columns_and_mixed_sign_weights(native):
    rng = np.random.default_rng(3)
    n = 4099
    x = make_rows(rng, n, "ip")
    q = planted(rng, x, 3)
    cols = [rng.random(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.integers(0, 5, n) / 4).astype(np.float32), np.exp2(rng.uniform(-8, 0, n)).astype(np.float32)]
    ref = Ref(x, q, "f32", "ip")
    idx = build(native, x, "f32", "ip", cols)
    betas = [0.3, -0.05, 0.125, -0.2]
    staged = [0, 0]
    for m in (1, 2, 3, 4):
        for window in (0, 64):
            _, one, two = check(idx, ref, q, 10, 0.5, betas[:m], cols[:m], window=window)
            staged[0] += one
            staged[1] += two
    assert staged[0] >= 12 and staged[1] >= 3
    idx.close()


# ---------------------------------------------------------------- 4. masks, deletes, columns set twice, rows added later
def test_mask_deletes_reset_and_added_rows(native):
    rng = np.random.default_rng(4)
    n = 4099
    x = make_rows(rng, n, "cosine")
    q = planted(rng, x, 3)
    col = rng.random(n).astype(np.float32)
    col[777] = 1.5  # the column's maximum
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x, "bf16", "cosine", [col])
    allowed = rng.random(n) < 0.6
    check(idx, ref, q, 10, 1.0, [0.25], [col], allowed)
    check(idx, ref, q, 10, 1.0, [0.25], [col], allowed, window=16)
    # deletes: the best rows and the row holding the column's maximum (bext still counts it: every row [0, n))
    (_, _, r), _, _ = check(idx, ref, q, 10, 1.0, [0.25], [col])
    gone = np.unique(np.concatenate([r[:, :3].reshape(-1), [777]]))
    idx.remove(gone)
    live = np.ones(n, bool)
    live[gone] = False
    (_, _, r2), _, _ = check(idx, ref, q, 10, 1.0, [0.25], [col], live)
    assert not set(gone.tolist()) & set(r2.reshape(-1).tolist())
    check(idx, ref, q, 10, 1.0, [0.25], [col], live & allowed, window=16)
    # a range set again: the cached extrema are dropped with it
    col2 = col.copy()
    col2[1000:2000] = rng.random(1000).astype(np.float32) * 4
    idx.set_boost(0, 1000, col2[1000:2000])
    check(idx, ref, q, 10, 1.0, [0.25], [col2], live)
    check(idx, ref, q, 10, 1.0, [-0.25], [col2], live)
    # rows added after the set read 0.0 until set
    extra = make_rows(rng, 300, "cosine")
    idx.add(extra)
    x3 = np.concatenate([x, extra])
    ref3 = Ref(x3, q, "bf16", "cosine")
    live3 = np.concatenate([live, np.ones(300, bool)])
    check(idx, ref3, q, 10, 1.0, [0.25], [col2], live3)  # (boost_ref pads the column with 0.0)
    check(idx, ref3, q, 10, 1.0, [0.25], [col2], live3, window=16)
    tail = rng.random(300).astype(np.float32)
    idx.set_boost(0, n, tail)
    check(idx, ref3, q, 10, 1.0, [0.25], [np.concatenate([col2, tail])], live3)
    idx.close()


# ---------------------------------------------------------------- 5. padding and the empty index
def test_padding_and_empty_index(native):
    rng = np.random.default_rng(5)
    x = make_rows(rng, 65, "cosine")
    q = planted(rng, x, 3)
    col = rng.random(65).astype(np.float32)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x, "bf16", "cosine", [col])
    allowed = np.zeros(65, bool)
    allowed[[3, 40, 64]] = True
    (v, s, r), _, _ = check(idx, ref, q, 10, 1.0, [0.5], [col], allowed)
    assert (r[:, 3:] == -1).all() and np.isneginf(v[:, 3:]).all() and np.isneginf(s[:, 3:]).all()
    assert (np.sort(r[:, :3], axis=1) == [3, 40, 64]).all()
    check(idx, ref, q, 128, 1.0, [0.5], [col])  # k beyond the rows
    idx.remove(np.arange(65))
    v, s, r = idx.search_boosted(q, 10, 1.0, [0.5])
    assert (r == -1).all() and np.isneginf(v).all() and np.isneginf(s).all()
    idx.close()
    empty = native.NativeIndex(64, "bf16", "cosine")
    st0 = empty.boost_stats()
    v, s, r = empty.search_boosted(q, 10, 1.0, [])
    assert (r == -1).all() and np.isneginf(v).all() and np.isneginf(s).all()
    assert empty.boost_stats()["window"] - st0["window"] == 3
    for bad in (dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=2.0 ** 65), dict(betas=[2.0 ** 65]),
                dict(betas=[float("nan")]), dict(window=9), dict(window=8193), dict(probe=9), dict(probe=129)):
        kw = dict(alpha=1.0, betas=[0.5])
        kw.update(bad)
        with pytest.raises(ValueError):
            empty.search_boosted(q, 10, **kw)
    with pytest.raises(ValueError):
        empty.set_boost(0, 0, [1.0])  # no such row
    with pytest.raises(ValueError):
        empty.set_boost(4, 0, [])
    empty.close()


# ---------------------------------------------------------------- 6. the stages, from the reference alone
def test_stages_and_the_boundary_pair(native):
    """n = 4099, (0.5, 0.5), probe 128: the reference windows hold 67 to 466 rows, so window = 32 sends every query to
    stage 2 and window = 4096 every query to stage 1; for one query, window = its count is stage 1, one less stage 2."""
    rng = np.random.default_rng(6)
    n, B = 4099, 65
    x = make_rows(rng, n, "cosine")
    q = planted(rng, x, B)
    col = rng.random(n).astype(np.float32)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x, "bf16", "cosine", [col])
    count = ref.mech(10, 0.5, [0.5], [col], probe=128)["count"]
    assert count.min() > 32 and count.max() <= 4096
    check(idx, ref, q, 10, 0.5, [0.5], [col], probe=128, window=32, need=2)
    check(idx, ref, q, 10, 0.5, [0.5], [col], probe=128, window=4096, need=1)
    b = int(np.argmin(count))
    ref1 = Ref(x, q[b:b + 1], "bf16", "cosine")
    c = int(count[b])
    assert ref1.mech(10, 0.5, [0.5], [col], probe=128)["count"][0] == c
    check(idx, ref1, q[b:b + 1], 10, 0.5, [0.5], [col], probe=128, window=c, need=1)
    check(idx, ref1, q[b:b + 1], 10, 0.5, [0.5], [col], probe=128, window=c - 1, need=2)
    # a mixed batch: the median count as the window splits the queries between the stages
    mid = int(np.median(count))
    _, one, two = check(idx, ref, q, 10, 0.5, [0.5], [col], probe=128, window=mid)
    assert one >= 1 and two >= 1
    idx.close()


# ---------------------------------------------------------------- 7. exact ties on dyadic data
def test_exact_ties(native):
    """ip / f32, rows a_r * e_0 and the query e_0 with dyadic a_r and boosts: s and v are exact.  Rows outside the pilot
    pool whose v equals tau enter and win by lower row; duplicates of one vector are ordered by boost, then row; boosts
    one fp32 ulp apart are ordered correctly.  Both stages give the same list."""
    n = 200
    a = np.full(n, 0.5, np.float32)
    b = np.zeros(n, np.float32)
    a[100:140] = 1.0                      # 40 rows with v = 1.0: they fill the pilot pool behind rows 160, 161: tau = 1.0 at k = 10
    b[[5, 7]] = 0.5                       # outside the pool, v = 0.5 + 0.5 = tau
    a[150:156] = 0.75                     # duplicates of one vector
    b[150:156] = [0.5, 0.75, 0.5, 0.75, 0.25, 0.75]
    a[160:162] = 2.0
    b[160] = 1.0
    b[161] = np.nextafter(np.float32(1.0), np.float32(2.0))
    x = np.zeros((n, 64), np.float32)
    x[:, 0] = a
    q = np.zeros((1, 64), np.float32)
    q[0, 0] = 1.0
    ref = Ref(x, q, "f32", "ip")
    want_rows = [161, 160, 151, 153, 155, 150, 152, 5, 7, 100]
    assert ref.ref(10, 1.0, [1.0], [b])[2][0].tolist() == want_rows
    idx = build(native, x, "f32", "ip", [b])
    # the pilot at probe 32: the top 32 by similarity = rows 160, 161 and 100..129 -- rows 5, 7 and 150..155 are outside
    for probe, window, need in ((32, 0, 1), (32, 10, 2), (0, 0, 1), (128, 16, 2)):
        (v, s, r), _, _ = check(idx, ref, q, 10, 1.0, [1.0], [b], probe=probe, window=window, need=need)
        assert r[0].tolist() == want_rows
        assert v[0].tolist() == [3.0 + 2.0 ** -23, 3.0, 1.5, 1.5, 1.5, 1.25, 1.25, 1.0, 1.0, 1.0]
        assert s[0].tolist() == [2.0, 2.0, 0.75, 0.75, 0.75, 0.75, 0.75, 0.5, 0.5, 1.0]
    idx.close()


# ---------------------------------------------------------------- 8. the device form
def test_device_form(native):
    import torch

    rng = np.random.default_rng(8)
    n = 4099
    x = make_rows(rng, n, "cosine")
    q = planted(rng, x, 5)
    cols = [rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)]
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x, "bf16", "cosine", cols)
    allowed = np.ones(n, bool)
    allowed[::5] = False
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        qt = torch.from_numpy(q).to(dev)
        md = torch.from_numpy(oracle.mask_from_bool(allowed).view(np.int64)).to(dev)
        for window, mask, ok in ((0, 0, None), (16, 0, None), (0, md.data_ptr(), allowed), (16, md.data_ptr(), allowed)):
            stage = ref.mech(10, 1.0, [0.25, -0.1], cols, ok, window=window)["stage"]
            v = torch.full((5, 10), 7.0, dtype=torch.float64, device=dev)
            s = torch.full((5, 10), 7.0, dtype=torch.float32, device=dev)
            r = torch.full((5, 10), 7, dtype=torch.int64, device=dev)
            st0 = idx.boost_stats()
            idx.search_boosted_device(qt.data_ptr(), 5, 10, 1.0, [0.25, -0.1], v.data_ptr(), s.data_ptr(), r.data_ptr(),
                                      mask_ptr=mask, window=window, stream=stream.cuda_stream)
            assert stream.query()  # the stream is idle on return
            st1 = idx.boost_stats()
            BR.assert_same((v.cpu().numpy(), s.cpu().numpy(), r.cpu().numpy()), ref.ref(10, 1.0, [0.25, -0.1], cols, ok))
            assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (
                int((stage == 1).sum()), int((stage == 2).sum()))
        with pytest.raises(ValueError):
            idx.search_boosted_device(qt.data_ptr(), 5, 10, 0.0, [0.25], v.data_ptr(), s.data_ptr(), r.data_ptr(),
                                      stream=stream.cuda_stream)
    idx.close()


# ---------------------------------------------------------------- 9. the store and the retriever on the real index
def test_store_and_retriever(native, tmp_path):
    from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig
    from hiprag.rag.config import RetrieverConfig
    from hiprag.rag.retriever import VectorRetriever
    from hiprag.rag.storage import BoostedHits

    rng = np.random.default_rng(9)
    n, dim = 300, 32
    x = make_rows(rng, n, "cosine", dim)
    imp = rng.random(n).astype(np.float32)
    rec = np.exp2(-rng.uniform(0, 6, n)).astype(np.float32)
    chunks = [Chunk(id=f"c{i}", document_id=f"d{i % 7}", content=f"t{i}", chunk_index=i,
                    metadata={"part": i % 3, "importance_score": float(imp[i]), "recency_base": float(rec[i])},
                    embedding=x[i].tolist()) for i in range(n)]
    cfg = VectorStoreConfig(backend="hip", collection_name="kb", persist_directory=str(tmp_path),
                            index_params={"dtype": "bf16", "persist": False,
                                          "boost_fields": ["importance_score", "recency_base"]})
    store = HipVectorStore(cfg)
    asyncio.run(store.add_chunks(chunks))
    q = planted(rng, x, 3)
    ref = Ref(x, q, "bf16", "cosine")
    weights = {"importance_score": 0.3, "recency_base": 0.2}
    allowed = np.arange(n) % 3 == 1
    res = store.search_boosted_batch(q.tolist(), 5, boost_weights=weights, sim_weight=0.5, filters={"part": 1})
    wv, ws, wr = ref.ref(5, 0.5, [0.3, 0.2], [imp, rec], allowed)
    assert all(isinstance(h, BoostedHits) for h in res)
    for b, h in enumerate(res):
        assert [c.id for c, _ in h.hits] == [f"c{r}" for r in wr[b]]
        assert [np.float32(sc) for _, sc in h.hits] == ws[b].tolist()
        assert list(h.blended) == wv[b].tolist()
    qv = q[0].tolist()

    class E:
        async def embed_query(self, _):
            return qv

    ret = VectorRetriever(store, E(), RetrieverConfig(top_k=5, similarity_threshold=0.0))
    out = asyncio.run(ret.retrieve_boosted("q", boost_weights=weights, sim_weight=0.5))
    wv, ws, wr = ref.ref(5, 0.5, [0.3, 0.2], [imp, rec])
    assert [(r.chunk.id, r.score, r.rank) for r in out] == [(f"c{row}", float(v), i + 1)
                                                           for i, (row, v) in enumerate(zip(wr[0], wv[0]))]
