"""GPU: range search (hr_range.hip) against tests/range_ref.py -- the canonical fp64 scores, hits by the
fp32 cast, (score desc, row asc) order, exact counts.  Rows equal, scores equal as fp32 bit patterns, counts equal.

Which stage answered is asserted too, and never from the library's own numbers.  Before the GPU result is looked at,
every query of such an assertion is put, on the CPU reference, into exactly one of two classes:
  must be stage 1   the allowed rows with canonical score >= t - MARGIN number at most cap / 2
  must be stage 2   the hits exceed cap
(cap = max(1024, 2 max_hits)).  MARGIN = 0.05 is 2.5 to 5 times the largest guard window E_q these shapes give (about
0.009 for ip and 0.018 for l2 on fp32 rows through the bf16 shadow with norms up to 1.5, less elsewhere): every row the
window scan may append scores at least t - E_q, so a stage-1 query's region cannot overflow, and a stage-2 query's
must.  The stats deltas must equal the class counts exactly: nothing reaches the right answer through a stage it did
not need."""
import asyncio

import numpy as np
import pytest

import oracle
from oracle import ref_numpy as R
from range_ref import assert_same, range_ref, thresholds

pytestmark = pytest.mark.gpu

ROW_COUNTS = [1, 31, 32, 33, 64, 65, 1000, 4099]
DTYPES = ["f32", "bf16", "f16"]
METRICS = ["cosine", "ip", "l2"]
MARGIN = 0.05
INF = np.float32(np.inf)


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
    """Isotropic rows: unit-normalised for cosine, scaled by U(0.5, 1.5) per row for ip / l2."""
    x = _unit(rng.standard_normal((n, dim)).astype(np.float32))
    if metric != "cosine":
        x = x * rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    return np.ascontiguousarray(x, np.float32)


def planted(rng, x, B, noise=0.05):
    pick = rng.choice(len(x), B, replace=len(x) < B)
    e = rng.standard_normal((B, x.shape[1])).astype(np.float32)
    return np.ascontiguousarray(_unit(x[pick]) + np.float32(noise) * _unit(e), np.float32)


def cap_of(max_hits):
    return max(1024, 2 * max_hits)


class Ref:
    """The fp64 score matrix of one (rows, queries) pair, computed once and shared by every threshold and cut."""

    def __init__(self, x, q, dtype, metric):
        self.dtype, self.metric = dtype, metric
        self.stored = R.process_rows(x, metric, dtype)
        qp = R.process_queries(q, metric)
        self.s = np.concatenate([R.exact_scores(self.stored, dtype, qp[b:b + 32], metric)  # (blocks bound the products)
                                 for b in range(0, len(qp), 32)])
        self.B, self.n = self.s.shape
        self.s32 = self.s.astype(np.float32)
        self.qp = R.process_queries(q, metric)

    def ranked(self, allowed=None):
        """fp32 scores of the allowed rows in search order, one list per query."""
        rows = np.arange(self.n) if allowed is None else np.nonzero(allowed)[0]
        return [self.s32[b, rows[np.lexsort((rows, -self.s[b, rows]))]] for b in range(self.B)]

    def at_rank(self, j, allowed=None):
        """Per query the fp32 score at rank j (the last rank where there are fewer rows)."""
        return np.asarray([r[min(j, len(r) - 1)] for r in self.ranked(allowed)], np.float32)

    def ref(self, t, max_hits, allowed=None):
        return range_ref(self.stored, self.dtype, self.qp, t, max_hits, allowed, self.metric, scores=self.s)

    def classes(self, t, max_hits, allowed=None):
        """(stage-1 queries, stage-2 queries, unclassified queries) of a call, from the reference alone."""
        t = thresholds(t, self.B)
        ok = np.ones(self.n, bool) if allowed is None else np.asarray(allowed, bool)
        cap = cap_of(max_hits)
        window = (ok[None, :] & (self.s >= t.astype(np.float64)[:, None] - MARGIN)).sum(axis=1)
        hits = (ok[None, :] & (self.s32 >= t[:, None])).sum(axis=1)
        one, two = window <= cap // 2, hits > cap
        assert not (one & two).any()
        return int(one.sum()), int(two.sum()), int((~one & ~two).sum())


def build(native, x, dtype="bf16", metric="cosine"):
    idx = native.NativeIndex(x.shape[1], dtype, metric)
    idx.add(x)
    return idx


def check(idx, ref, q, t, max_hits, allowed=None, need=None):
    """One host-form call against the reference.  need: 1 / 2 = every query must be in that class (asserted before the
    call); None: the stage is asserted only when every query falls into a class.  Returns the call's result."""
    one, two, neither = ref.classes(t, max_hits, allowed)
    if need is not None:
        assert (one, two, neither) == ((ref.B, 0, 0) if need == 1 else (0, ref.B, 0)), (one, two, neither)
    want = ref.ref(t, max_hits, allowed)
    st0, top0 = idx.range_stats(), idx.stats()
    got = idx.search_range(q, t, max_hits, None if allowed is None else oracle.mask_from_bool(allowed))
    st1 = idx.range_stats()
    if max_hits == 0:
        assert got[0] is None and got[1] is None
    assert_same(got, want if max_hits else (None, None, want[2]))
    if neither == 0:
        assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (one, two)
    assert st1["window"] + st1["all_rows"] - st0["window"] - st0["all_rows"] == ref.B
    assert idx.stats() == top0  # the top-k search's counters do not move
    return got


# ---------------------------------------------------------------- 1. every row count x dtype x metric
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_row_counts_dtypes_metrics(native, dtype, metric):
    """Thresholds taken from the reference ranking itself: the fp32 score at rank j (the boundary row is in), one ulp
    above it (it is out), a value between two ranks, above the best score, -inf and +inf; max_hits 1, 10, 512."""
    rng = np.random.default_rng(10 * DTYPES.index(dtype) + METRICS.index(metric))
    staged = [0, 0]
    for n in ROW_COUNTS:
        x = make_rows(rng, n, metric)
        q = planted(rng, x, 3)
        ref = Ref(x, q, dtype, metric)
        idx = build(native, x, dtype, metric)
        ts = [-INF, INF, ref.at_rank(0) + np.float32(1.0)]
        for j in sorted({0, min(9, n - 1), min(99, n - 1), min(199, n - 1)}):
            t_in = ref.at_rank(j)
            ts += [t_in, np.nextafter(t_in, INF)]
            if j == min(9, n - 1) and j + 1 < n:
                ts.append(((t_in.astype(np.float64) + ref.at_rank(j + 1)) / 2).astype(np.float32))
        for t in ts:
            for max_hits in (1, 10, 512):
                one, two, _ = ref.classes(t, max_hits)
                staged[0] += one
                staged[1] += two
                got = check(idx, ref, q, t, max_hits)
                if np.ndim(t) and (t > ref.at_rank(0)).all():
                    assert (got[2] == 0).all() and (got[1] == -1).all() and np.isneginf(got[0]).all()
        assert (idx.search_range(q, -INF, 10)[2] == n).all()
        idx.close()
    assert staged[0] > 400 and staged[1] >= 9  # both stages were asserted (stage 2: t = -inf at n = 4099)


# ---------------------------------------------------------------- 2. ties
def tie_case(rng):
    x = make_rows(rng, 4099, "cosine")
    tied = np.sort(rng.choice(4099, 40, replace=False))
    x[tied] = x[tied[0]]
    q = planted(rng, x[tied[:1]], 2)
    return x, tied, q


def test_ties(native):
    """40 bit-identical rows scattered through 4099, the threshold exactly at their score and one ulp above it; a
    max_hits cut inside the block keeps the lowest rows; the count is the full block."""
    x, tied, q = tie_case(np.random.default_rng(2))
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(0)
    assert (ref.s32[:, tied] == t[:, None]).all() and (ref.at_rank(39) == t).all() and (ref.at_rank(40) < t).all()
    for max_hits in (10, 40, 64):
        s, r, c = check(idx, ref, q, t, max_hits, need=1)
        assert (c == 40).all()
        m = min(max_hits, 40)
        assert (r[:, :m] == tied[None, :m]).all() and (r[:, m:] == -1).all()
    s, r, c = check(idx, ref, q, np.nextafter(t, INF), 10, need=1)
    assert (c == 0).all() and (r == -1).all()
    # the block below other hits: a cut inside it still takes its lowest rows
    t_low = ref.at_rank(60)
    s, r, c = check(idx, ref, q, t_low, 50, need=1)
    assert (c >= 61).all() and (r[:, :40] == tied[None, :]).all()
    idx.close()


# ---------------------------------------------------------------- 3. deletes and masks
def test_deletes_and_masks(native):
    rng = np.random.default_rng(3)
    n = 4099
    x = make_rows(rng, n, "ip")
    q = planted(rng, x, 4)
    ref = Ref(x, q, "f16", "ip")
    idx = build(native, x, "f16", "ip")
    t = ref.at_rank(199)
    s, r, c = check(idx, ref, q, t, 512, need=1)
    assert (c >= 200).all()
    hits = np.unique(r[r >= 0])
    gone, hidden = hits[0::3], hits[1::3]
    masked = np.ones(n, bool)
    masked[hidden] = False
    check(idx, ref, q, t, 512, masked, need=1)  # a third of the hits masked out
    idx.remove(gone)
    live = np.ones(n, bool)
    live[gone] = False
    s, r, c = idx.search_range(q, t, 512)
    assert_same((s, r, c), ref.ref(t, 512, live))  # a third tombstoned
    assert not np.isin(r, gone).any()
    s, r, c = idx.search_range(q, t, 512, oracle.mask_from_bool(masked))
    assert_same((s, r, c), ref.ref(t, 512, live & masked))  # both
    assert not np.isin(r, np.concatenate([gone, hidden])).any()
    # a mask that allows 5 rows in 3 tiles: the selective tile list
    few = np.zeros(n, bool)
    few[[40, 41, 2000, 2001, 4098]] = True
    for tt, mh in ((-INF, 10), (-INF, 0), (t, 10)):
        got = idx.search_range(q, tt, mh, oracle.mask_from_bool(few))
        assert_same(got, ref.ref(tt, mh, live & few) if mh else (None, None, ref.ref(tt, 0, live & few)[2]))
    assert (idx.search_range(q, -INF, 10, oracle.mask_from_bool(few))[2] == int((live & few).sum())).all()
    none = np.zeros(n, bool)
    assert (idx.search_range(q, -INF, 10, oracle.mask_from_bool(none))[2] == 0).all()
    with pytest.raises(ValueError):
        idx.search_range(q, t, 10, np.zeros(n // 64 - 1, np.uint64))  # shorter than the index, as search()
    assert_same(idx.search_range(q, t, 512), ref.ref(t, 512, live))
    idx.close()


# ---------------------------------------------------------------- 4., 5. stage 2
def cluster_case(rng, B=3):
    """3000 rows unit(c + 0.01 noise) inside 4099 isotropic ones; queries near c, and planted background queries."""
    n = 4099
    x = make_rows(rng, n, "cosine")
    c = _unit(rng.standard_normal((1, 64)).astype(np.float32))
    inside = np.sort(rng.choice(n, 3000, replace=False))
    x[inside] = _unit(c + np.float32(0.01) * _unit(rng.standard_normal((3000, 64)).astype(np.float32)))
    q_dense = np.ascontiguousarray(_unit(c + np.float32(0.01) * _unit(rng.standard_normal((B, 64)).astype(np.float32))))
    outside = np.setdiff1d(np.arange(n), inside)
    q_sparse = planted(rng, x[outside], B)
    return x, inside, q_dense, q_sparse


def test_forced_stage_two(native):
    rng = np.random.default_rng(4)
    x, inside, qd, _ = cluster_case(rng)
    ref = Ref(x, qd, "bf16", "cosine")
    idx = build(native, x)
    idx.remove([5, 77, int(inside[3])])
    live = np.ones(len(x), bool)
    live[[5, 77, int(inside[3])]] = False
    some = live.copy()
    some[::7] = False
    # t = -inf: every live, allowed row; the lists are the plain search's
    for allowed in (live, some):
        mask = oracle.mask_from_bool(allowed)
        assert ref.classes(-INF, 10, allowed) == (0, 3, 0)
        st0 = idx.range_stats()
        s, r, c = idx.search_range(qd, -INF, 10, mask)
        assert_same((s, r, c), ref.ref(-INF, 10, allowed))
        assert (c == int(allowed.sum())).all()
        ps, pr = idx.search(qd, 10, mask)
        np.testing.assert_array_equal(r, pr)
        np.testing.assert_array_equal(s.view(np.uint32), ps.view(np.uint32))
        assert_same(idx.search_range(qd, -INF, 0, mask), (None, None, c))  # the same as a count-only call
        st1 = idx.range_stats()
        assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (0, 6)
    # the dense cluster: ~3000 hits against cap 1024
    assert ref.classes(0.9, 100, live) == (0, 3, 0)
    st0 = idx.range_stats()
    s, r, c = idx.search_range(qd, 0.9, 100)
    assert_same((s, r, c), ref.ref(0.9, 100, live))
    assert (c >= 2990).all() and (c <= 3000).all()
    ps, pr = idx.search(qd, 100)
    np.testing.assert_array_equal(r, pr)
    np.testing.assert_array_equal(s.view(np.uint32), ps.view(np.uint32))
    assert_same(idx.search_range(qd, 0.9, 0), (None, None, c))
    st1 = idx.range_stats()
    assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (0, 6)
    assert st1["scans"] - st0["scans"] == 2  # one window scan per call: stage 2 follows an overflowed region
    idx.close()


def test_one_batch_mixing_both_stages(native):
    rng = np.random.default_rng(5)
    x, inside, qd, qs = cluster_case(rng)
    q = np.ascontiguousarray(np.stack([qd[0], qs[0], qs[1], qd[1], qs[2]]))
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(0)  # the background queries: their planted row and what sits within MARGIN of it
    t[[0, 3]] = 0.9     # the cluster queries: the whole cluster
    assert ref.classes(t, 100) == (3, 2, 0)
    s, r, c = check(idx, ref, q, t, 100)
    assert (c[[0, 3]] >= 2990).all() and (c[[1, 2, 4]] >= 1).all() and (c[[1, 2, 4]] < 50).all()
    check(idx, ref, q, t, 0)
    idx.close()


# ---------------------------------------------------------------- 6., 7. count-only, identities
def test_count_only_on_the_window_path(native):
    rng = np.random.default_rng(6)
    x = make_rows(rng, 4099, "l2")
    q = planted(rng, x, 5)
    ref = Ref(x, q, "f32", "l2")
    idx = build(native, x, "f32", "l2")
    for j in (0, 9, 99):
        got = check(idx, ref, q, ref.at_rank(j), 0, need=1)  # max_hits = 0: NULL outputs
        assert (got[2] >= j + 1).all()
    idx.close()


def test_identities(native):
    """For a fixed t the max_hits = m' answer is the prefix of the max_hits = m answer; where count <= k the answer is
    the first count entries of search(k)."""
    rng = np.random.default_rng(7)
    x = make_rows(rng, 4099, "cosine")
    q = planted(rng, x, 4)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(99)
    full = check(idx, ref, q, t, 512, need=1)
    for m in (1, 17, 100, 101):
        s, r, c = idx.search_range(q, t, m)
        np.testing.assert_array_equal(c, full[2])
        np.testing.assert_array_equal(r, full[1][:, :m])
        np.testing.assert_array_equal(s.view(np.uint32), full[0][:, :m].view(np.uint32))
    ps, pr = idx.search(q, 128)
    for b in range(4):
        cnt = int(full[2][b])
        assert 100 <= cnt <= 128
        np.testing.assert_array_equal(full[1][b, :cnt], pr[b, :cnt])
        np.testing.assert_array_equal(full[0][b, :cnt].view(np.uint32), ps[b, :cnt].view(np.uint32))
        assert ps[b, cnt] < t[b]
    # a prefix across the stages: t = -inf is answered by stage 2, its first rows are search's
    s, r, c = idx.search_range(q, -INF, 128)
    np.testing.assert_array_equal(r, pr)
    idx.close()


def test_regions_beyond_the_lds(native):
    """max_hits = 5000 and 65536: regions of 10,000 and 131,072 records.  9000 rows at t = -inf put 9000 records into
    a region -- more than one workgroup orders in LDS (8192), fewer than cap, so the region cannot overflow (n <= cap:
    stage 1 whatever E_q is) and is ordered through rocPRIM; 40 bit-identical rows pin the row order there."""
    rng = np.random.default_rng(14)
    n = 9000
    x = make_rows(rng, n, "cosine")
    tied = np.sort(rng.choice(n, 40, replace=False))
    x[tied] = x[tied[0]]
    q = np.ascontiguousarray(np.concatenate([planted(rng, x[tied[:1]], 1), planted(rng, x, 2)]))
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    allowed = np.ones(n, bool)
    allowed[::9] = False
    for t in (-INF, ref.at_rank(8500)):
        for max_hits, ok in ((5000, None), (65536, None), (5000, allowed)):
            st0 = idx.range_stats()
            got = check(idx, ref, q, t, max_hits, ok)
            st1 = idx.range_stats()
            assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (3, 0)
            assert (got[2] > 7000).all()
    s, r, c = idx.search_range(q, -INF, 5000)
    assert (r[0, :40] == tied).all() and (c == n).all()
    # a cut at max_hits = 5000 of 9000 hits is the prefix of the uncut list
    full = idx.search_range(q, -INF, 65536)
    np.testing.assert_array_equal(r, full[1][:, :5000])
    np.testing.assert_array_equal(s.view(np.uint32), full[0][:, :5000].view(np.uint32))
    assert (full[1][:, n:] == -1).all()
    idx.close()


# ---------------------------------------------------------------- 8. more queries than one pass takes
# At dim 64 a pass of 16-bit rows takes up to four query groups of 64 (make_plan: QB = 2, NG <= 4): 256 queries.
PASS_QUERIES = 256


def test_three_query_groups_the_last_one_partial(native):
    """130 queries: one pass of three 64-query groups, the last one of 2."""
    rng = np.random.default_rng(8)
    x = make_rows(rng, 4099, "cosine")
    q = planted(rng, x, 130)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(9)
    st0 = idx.range_stats()
    check(idx, ref, q, t, 64, need=1)
    assert idx.range_stats()["scans"] - st0["scans"] == 1
    t[::3] = -INF  # every third query through stage 2, in all three groups
    assert ref.classes(t, 64) == (86, 44, 0)
    check(idx, ref, q, t, 64)
    idx.close()


def test_three_chunks_the_last_one_partial(native):
    """600 queries: chunks of 256 + 256 + 88, the last one planned on its own (two groups).  Thresholds, outputs,
    counts and flags are offset per chunk and the regions are reused by every chunk; every fifth query goes through
    stage 2, in every chunk, after the last chunk's scan."""
    B = 600
    rng = np.random.default_rng(15)
    x = make_rows(rng, 2000, "cosine")
    q = planted(rng, x, B)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(9)
    t[1::2] = ref.at_rank(29)[1::2]  # neighbours differ in threshold and count: a shifted offset shows
    st0 = idx.range_stats()
    got = check(idx, ref, q, t, 64, need=1)
    assert idx.range_stats()["scans"] - st0["scans"] == -(-B // PASS_QUERIES) == 3
    assert (got[2][0::2] >= 10).all() and (got[2][1::2] >= 30).all() and (got[2][0::2] < 30).all()
    t[::5] = -INF
    for b0 in range(0, B, PASS_QUERIES):
        assert np.isneginf(t[b0:b0 + PASS_QUERIES]).sum() >= 17  # stage-2 queries in every chunk
    assert ref.classes(t, 64) == (480, 120, 0)
    st0 = idx.range_stats()
    got = check(idx, ref, q, t, 64)
    assert idx.range_stats()["scans"] - st0["scans"] == 3
    assert (got[2][::5] == 2000).all()
    check(idx, ref, q, t, 0)  # count-only over the same chunks
    idx.close()


def test_regions_beyond_the_lds_in_a_later_chunk(native):
    """260 queries at max_hits = 5000 (regions of 10,000 records): chunks of 256 + 4.  Two queries of each chunk take
    t = -inf over 8500 rows -- 8500 records in the region, beyond the LDS and below cap (n <= cap: stage 1 whatever
    E_q is) -- so the per-chunk ordering through rocPRIM runs for the first chunk and for the second."""
    B, n = 260, 8500
    rng = np.random.default_rng(16)
    x = make_rows(rng, n, "cosine")
    q = planted(rng, x, B)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(9)
    t[[0, 100, 257, 259]] = -INF
    st0 = idx.range_stats()
    got = check(idx, ref, q, t, 5000)
    st1 = idx.range_stats()
    assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"], st1["scans"] - st0["scans"]) == (B, 0, 2)
    assert (got[2][[0, 100, 257, 259]] == n).all() and (np.delete(got[2], [0, 100, 257, 259]) < 100).all()
    idx.close()


# ---------------------------------------------------------------- 9. steady state
N_SCAN = 245_747  # 7680 tiles: 24 tiles per wave with a quarter to spare under a 16-CU mask
CUS16 = list(range(16))


def test_steady_state_under_a_cu_mask(native):
    """The window scan in its steady state: 245,747 synthetic rows under the smallest legal CU mask, so every wave of
    the collect pass streams 24 or more tiles against its fixed floor (range_wave_tiles: counted by the pass itself;
    every tile once)."""
    from hiprag import synth

    seed, dim, B = 31, 64, 64
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add_synthetic(seed, 0, N_SCAN)
    rng = np.random.default_rng(9)
    rows = synth.corpus_rows(seed, rng.choice(N_SCAN, B, replace=False), dim)
    q = np.ascontiguousarray(_unit(rows) + np.float32(0.05) * _unit(rng.standard_normal((B, dim)).astype(np.float32)))
    qp = R.process_queries(q, "cosine")
    s_ref, r_ref = oracle.c_search_synthetic(seed, 0, N_SCAN, dim, "bf16", "cosine", qp, 512)
    s32 = s_ref.astype(np.float32)
    t = s32[:, 9].copy()
    assert (s_ref[:, 511] < t.astype(np.float64) - MARGIN).all()  # at most 511 rows within MARGIN: must be stage 1
    cut = (s32 >= t[:, None]).sum(axis=1)
    assert (cut >= 10).all() and (cut < 512).all()
    want_s = np.full((B, 512), -np.inf, np.float32)
    want_r = np.full((B, 512), -1, np.int64)
    for b in range(B):
        want_s[b, :cut[b]], want_r[b, :cut[b]] = s32[b, :cut[b]], r_ref[b, :cut[b]]
    idx.set_cu_mask(CUS16)
    st0, top0 = idx.range_stats(), idx.stats()
    first = idx.search_range(q, t, 512)
    wt = idx.range_wave_tiles()  # of the collect pass itself
    assert len(wt) > 0 and int(wt.min()) >= 24 and int(wt.sum()) == (N_SCAN + 31) // 32
    assert_same(first, (want_s, want_r, cut))
    st1 = idx.range_stats()
    assert (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"], st1["scans"] - st0["scans"]) == (B, 0, 1)
    assert idx.stats() == top0
    again = idx.search_range(q, t, 512)
    assert_same(again, first)
    assert_same(idx.search_range(q, t, 0), (None, None, cut))
    idx.set_cu_mask(None)
    idx.close()


# ---------------------------------------------------------------- 10. the device form
def test_device_form(native):
    import torch

    rng = np.random.default_rng(10)
    x, inside, qd, qs = cluster_case(rng)
    q = np.ascontiguousarray(np.stack([qs[0], qd[0], qs[1], qs[2], qd[1]]))
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(0)
    t[[1, 4]] = 0.9
    allowed = np.ones(len(x), bool)
    allowed[::5] = False
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        qt = torch.from_numpy(q).to(dev)
        tt = torch.from_numpy(t).to(dev)
        md = torch.from_numpy(oracle.mask_from_bool(allowed).view(np.int64)).to(dev)
        for max_hits, mask, ok in ((100, 0, None), (7, md.data_ptr(), allowed), (0, 0, None)):
            s = torch.full((5, max(max_hits, 1)), 7.0, dtype=torch.float32, device=dev)
            r = torch.full((5, max(max_hits, 1)), 7, dtype=torch.int64, device=dev)
            c = torch.full((5,), 7, dtype=torch.int64, device=dev)
            st0 = idx.range_stats()
            idx.search_range_device(qt.data_ptr(), 5, tt.data_ptr(), max_hits, s.data_ptr() if max_hits else 0,
                                    r.data_ptr() if max_hits else 0, c.data_ptr(), mask_ptr=mask,
                                    stream=stream.cuda_stream)
            assert stream.query()  # the stream is idle on return
            st1 = idx.range_stats()
            got = (s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()) if max_hits else (None, None, c.cpu().numpy())
            want = ref.ref(t, max_hits, ok)
            assert_same(got, want if max_hits else (None, None, want[2]))
            host = idx.search_range(q, t, max_hits, None if ok is None else oracle.mask_from_bool(ok))
            assert_same(got, host)
            one, two, neither = ref.classes(t, max_hits, ok)
            assert neither == 0 and (st1["window"] - st0["window"], st1["all_rows"] - st0["all_rows"]) == (one, two)
        bad = torch.from_numpy(np.asarray([0.5, np.nan, 0.5, 0.5, 0.5], np.float32)).to(dev)
        with pytest.raises(ValueError):
            idx.search_range_device(qt.data_ptr(), 5, bad.data_ptr(), 7, s.data_ptr(), r.data_ptr(), c.data_ptr(),
                                    stream=stream.cuda_stream)
    idx.close()


# ---------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_handle_usable(native):
    import ctypes

    rng = np.random.default_rng(11)
    x = make_rows(rng, 1000, "cosine")
    q = planted(rng, x, 3)
    ref = Ref(x, q, "bf16", "cosine")
    idx = build(native, x)
    t = ref.at_rank(9)
    with pytest.raises(ValueError):
        idx.search_range(q, [0.5, np.nan, 0.5], 10)
    with pytest.raises(ValueError):
        idx.search_range(q, 0.5, 65537)
    with pytest.raises(ValueError):
        idx.search_range(q, 0.5, -1)
    with pytest.raises(ValueError):
        idx.search_range(q, [0.5, 0.5], 10)
    with pytest.raises(ValueError):
        idx.search_range(q[:, :32], 0.5, 10)
    # the library's own checks, past the Python wrapper's
    p = ctypes.c_void_p
    s, r, c = np.empty((3, 8), np.float32), np.empty((3, 8), np.int64), np.empty(3, np.int64)
    tq = t.copy()

    def args(B, mh):
        return (idx._h, q.ctypes.data_as(p), B, tq.ctypes.data_as(p), mh, None, s.ctypes.data_as(p),
                r.ctypes.data_as(p), c.ctypes.data_as(p))

    assert idx.lib.hr_index_search_range(*args(3, 65537)) == native.E_INVALID
    assert idx.lib.hr_index_search_range(*args(3, -1)) == native.E_INVALID
    assert idx.lib.hr_index_search_range(*args(0, 8)) == native.E_INVALID
    tq[1] = np.nan
    assert idx.lib.hr_index_search_range(*args(3, 8)) == native.E_INVALID
    assert idx.lib.hr_index_search_range(idx._h, q.ctypes.data_as(p), 3, t.ctypes.data_as(p), 8, None, None, None,
                                         c.ctypes.data_as(p)) == native.E_INVALID  # lists asked for, none given
    check(idx, ref, q, t, 10, need=1)  # the handle still answers
    assert_same(idx.search_range(q, INF, 4), ref.ref(INF, 4))
    idx.close()
    two = native.NativeIndex(64, "bf16", "cosine", devices=[0, 0])  # a multi-device handle is out of scope
    two.add(x)
    with pytest.raises(NotImplementedError):
        two.search_range(q, t, 10)
    assert two.search(q, 5)[1].shape == (3, 5)
    two.close()
    empty = native.NativeIndex(64, "bf16", "cosine")
    s, r, c = empty.search_range(q, -INF, 4)
    assert (c == 0).all() and (r == -1).all() and np.isneginf(s).all()
    assert (empty.search_range(q, -INF, 0)[2] == 0).all()
    empty.close()


# ---------------------------------------------------------------- 11. the store
def _chunks(x):
    from hiprag.rag import Chunk

    return [Chunk(id=f"c{i}", document_id=f"d{i // 7}", content=f"text {i}", chunk_index=i, metadata={"part": i % 3},
                  embedding=x[i].tolist()) for i in range(len(x))]


def _store(tmp_path, name, **kw):
    from hiprag.rag import HipVectorStore, VectorStoreConfig

    index_type = kw.pop("index_type", None)
    return HipVectorStore(VectorStoreConfig(backend="hip", collection_name=name, persist_directory=str(tmp_path / name),
                                            index_type=index_type,
                                            index_params={"dtype": "bf16", "fsync": False, **kw}))


def _want(ref, t, max_hits, allowed=None):
    s, r, c = ref.ref(t, max_hits, allowed)
    return [([(f"c{row}", float(sc)) for sc, row in zip(s[b], r[b]) if row >= 0], int(c[b])) for b in range(len(c))]


def _got(res):
    return [([(c.id, s) for c, s in h.hits], h.total) for h in res]


@pytest.mark.parametrize("index_type", [None, "IVF_FLAT"])
def test_store_range(native, tmp_path, index_type):
    rng = np.random.default_rng(12)
    x = make_rows(rng, 400, "cosine")
    kw = dict(index_type="IVF_FLAT", nlist=4, nprobe=1, ivf_train_rows=64, ivf_seed=1) if index_type else {}
    store = _store(tmp_path, "kb", **kw)
    asyncio.run(store.add_chunks(_chunks(x)))
    if index_type:
        assert store._index.trained  # above its training threshold: plain searches probe one list of four
    q = planted(rng, x, 4)
    ref = Ref(x, q, "bf16", "cosine")
    part = np.arange(400) % 3
    t = ref.at_rank(19)
    assert _got(store.search_range_batch(q, t, 50)) == _want(ref, t, 50)  # exact: nprobe = 1 would miss rows
    assert _got(store.search_range_batch(q, float(t[0]), 8)) == _want(ref, t[0], 8)
    assert store.count_above_batch(q, t) == [w[1] for w in _want(ref, t, 0)]
    res = store.search_range_batch(q, t, 50, {"part": 1})
    assert _got(res) == _want(ref, t, 50, part == 1)
    flt = [{"part": 1}, None, {"part": 2}, {"part": 1}]
    res = store.search_range_batch(q, t, 5, flt)
    for i, f in enumerate(flt):
        assert _got([res[i]]) == [_want(ref, t, 5, None if f is None else part == f["part"])[i]]
    assert any(h.truncated for h in res)
    gone = [cid for cid, _ in _want(ref, t, 50)[0][0]][:3]
    asyncio.run(store.delete(gone))
    live = np.ones(400, bool)
    live[[int(g[1:]) for g in gone]] = False
    assert _got(store.search_range_batch(q, t, 50)) == _want(ref, t, 50, live)
    one = asyncio.run(store.search_range(q[1].tolist(), float(t[1]), 50, {"part": 2}))
    assert _got([one]) == [_want(ref, t, 50, live & (part == 2))[1]]
    assert store.count_above_batch(q, -np.inf) == [397] * 4
    store.close()
