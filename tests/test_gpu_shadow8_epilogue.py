"""GPU: the shadow-8 scan's epilogue and corpus ring (hr_kernels.hpp, scan_body with DT == I8S) against the CPU oracle,
with the scan forced on (set_shadow8(2)).  Bar, as in test_gpu_shadow8.py: rows equal to the oracle's, fp32 score bits
equal, -inf / -1 padding.

The epilogue folds the row scale and the lane's live / mask bit into one FMA (addend -0.0 or -inf) and masks the
threshold compare with one ballot of the allowed lanes per tile.  What can go wrong with that sits on single lanes:
a masked, deleted or padding row whose approximate score would be the best of its tile must reach neither a group
maximum nor a candidate region, also while the thresholds are still -inf (-inf >= -inf holds).  So the queries here
are planted on rows that are then forbidden, and the masks leave single lanes, whole tiles, fewer than k rows or
nothing.

The ring ladder runs the same epilogue behind every ring depth the shadow-8 kernels are built for (2, 4, 8, 16
entries), one to five spans per tile, the kernel with the per-wave refresh, and shards where every wave scans several
tiles -- the last span of a tile prefetches the next tile, or the first tile of the unit grabbed from the dynamic tail.
"""
import functools

import numpy as np
import pytest

import hostile_data as H
import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

N = 4096 + 37  # 130 tiles, the last one partial
KMAX = 40


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid].view(np.uint32), s_ref[valid].astype(np.float32).view(np.uint32))
    assert np.all(np.isneginf(s_gpu[~valid]))


def _oracle(rows, dtype, q, k, allowed):
    stored = R.process_rows(rows, "cosine", dtype)
    return oracle.c_search(stored, dtype, R.process_queries(q, "cosine"), k, oracle.mask_from_bool(allowed))


# ---------------------------------------------------------------- lane-level predicates
@functools.lru_cache(maxsize=2)
def _planted_corpus(dim):
    """Gaussian rows, 64 queries that are (almost) copies of 64 distinct rows, and which of those rows get deleted
    (the even queries'; the odd queries' rows stay live and are masked out instead)."""
    rows = R.gen_rows(7, 0, N, dim)
    rng = np.random.default_rng(dim)
    planted = rng.choice(N, 64, replace=False)
    q = (rows[planted] + rng.standard_normal((64, dim)).astype(np.float32) * 100).astype(np.float32)
    rows.setflags(write=False)
    return rows, q, planted


def _mask(kind, planted):
    tiles = (N + 31) // 32
    allowed = np.zeros(N, bool)
    if kind == "one_row_per_tile":  # a different lane in each tile
        r = np.arange(tiles) * 32 + (np.arange(tiles) * 7 + 3) % 32
        allowed[r[r < N]] = True
    elif kind == "alternate_tiles":
        allowed[(np.arange(N) // 32) % 2 == 1] = True
    elif kind == "fewer_than_k":  # 7 rows, in 7 tiles
        allowed[np.arange(7) * 577 + 11] = True
    elif kind != "none":
        raise KeyError(kind)
    allowed[planted] = False  # the best approximate score of every query sits on a forbidden lane
    return allowed


@pytest.mark.parametrize("kind", ["one_row_per_tile", "alternate_tiles", "fewer_than_k", "none"])
@pytest.mark.parametrize("dim", [64, 1024])
def test_forbidden_lanes_reach_neither_maxima_nor_candidates(native, dim, kind):
    rows, q, planted = _planted_corpus(dim)
    allowed = _mask(kind, planted)
    live = np.ones(N, bool)
    live[planted[0::2]] = False
    s_ref, r_ref = _oracle(rows, "bf16", q, KMAX, live & allowed)
    if kind == "fewer_than_k":
        assert (r_ref[:, 6] >= 0).all() and (r_ref[:, 7:] == -1).all()
    if kind == "none":
        assert (r_ref == -1).all()
    assert not np.isin(r_ref, planted).any()
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    idx.remove(planted[0::2])
    idx.set_shadow8(2)
    m = oracle.mask_from_bool(allowed)
    for B in (1, 64):
        for k in (10, KMAX):
            l0 = idx.shadow8_stats()["launches"]
            s, r = idx.search(q[:B], k, m)
            if kind != "none":  # (a mask without a row leaves no tile to scan: the host answers with the padding)
                assert idx.shadow8_stats()["launches"] > l0, (B, k)
            _check(s, r, s_ref[:B, :k], r_ref[:B, :k])
    idx.close()


@pytest.mark.parametrize("dim", [64, 1024])
def test_thresholds_that_never_leave_minus_inf(native, dim):
    """33 rows, all but 3 deleted: fewer live rows than groups, so every threshold stays -inf for the whole scan and
    only the allowed-lane mask keeps the 30 deleted rows (the queries' own among them) and the padding lanes of the
    second tile out."""
    n = 33
    rows = R.gen_rows(9, 0, n, dim)
    rng = np.random.default_rng(dim + 1)
    q = (rows[rng.integers(0, n, 64)] + rng.standard_normal((64, dim)).astype(np.float32) * 100).astype(np.float32)
    live = np.zeros(n, bool)
    live[[2, 30, 32]] = True
    q[:3] = rows[[2, 30, 32]]  # ... and three queries on the rows that stay
    s_ref, r_ref = _oracle(rows, "bf16", q, 10, live)
    assert (r_ref[:, 2] >= 0).all() and (r_ref[:, 3:] == -1).all()
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    idx.remove(np.nonzero(~live)[0])
    idx.set_shadow8(2)
    for B in (1, 64):
        l0 = idx.shadow8_stats()["launches"]
        s, r = idx.search(q[:B], 10)
        assert idx.shadow8_stats()["launches"] > l0
        _check(s, r, s_ref[:B], r_ref[:B])
    idx.close()


# ---------------------------------------------------------------- ring ladder
N_LADDER = 3 * 2048 * 32 + 37  # three tiles and more for each of at most 2048 waves, a partial last tile


def _ladder_case(native, n, dim, B, k, seed):
    stored = oracle.c_build_synthetic(1, 0, n, dim, "bf16", "cosine")
    rng = np.random.default_rng(seed)
    planted = np.concatenate([R.gen_rows(1, int(j), 1, dim) for j in rng.choice(n, B, replace=False)])
    q = planted + rng.standard_normal((B, dim)).astype(np.float32) * 20000  # near neighbours, not exact copies
    q[1::2] = rng.standard_normal((B // 2, dim))                            # and isotropic queries
    q = q.astype(np.float32)
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), k)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add_synthetic(1, 0, n)
    idx.set_shadow8(2)
    f0 = idx.stats()["guard_failures"]
    s, r = idx.search(q, k)
    assert idx.shadow8_stats()["launches"] > 0
    _check(s, r, s_ref, r_ref)
    assert idx.stats()["guard_failures"] == f0
    idx.close()


@pytest.mark.parametrize("dim,B", [(128, 64), (256, 64), (1024, 64), (1280, 64), (2048, 32)])
def test_ring_ladder(native, dim, B):
    """D = 128: a ring of 4; 256: 8; 1024: 16, two spans per tile; 1280 at B = 64: 8, five spans, the kernel with the
    per-wave refresh (no room for the threshold row in LDS); 2048 at B = 32: 16, four spans."""
    _ladder_case(native, N_LADDER, dim, B, 10, dim)


def test_dynamic_tail_1p2m_x128(native):
    """1.2M x 128 (a ring of 4): 18 or more tiles per wave, so waves leave their static runs for the dynamic tail and a
    run's last tile prefetches the first tile of the unit grabbed from the pool; mid-scan refreshes in every wave."""
    _ladder_case(native, 1_200_000, 128, 64, 10, 5)


def test_dynamic_tail_1p2m_x64(native):
    """The same at D = 64 (a ring of 2), the shard of test_gpu_shadow8_cadence.py."""
    _ladder_case(native, 1_200_000, 64, 64, 10, 6)


# ---------------------------------------------------------------- value families
N_FAM = 20_011


def _family(name, dim):
    rng = np.random.default_rng(11)
    if name == "identical":  # every row the same vector
        rows = np.repeat(H.anisotropic(rng, 1, dim), N_FAM, axis=0)
        return rows, H.queries("anisotropic", 2, rows, 32)[0]
    rows = H.corpus(name, 1, N_FAM, dim)[0]  # sparse: all-zero and one-hot rows; wide: one huge element among tiny ones
    return rows, H.queries(name, 2, rows, 32)[0]


@pytest.mark.parametrize("name", ["sparse", "wide", "identical"])
def test_value_families_through_the_masked_filter(native, name):
    """The families int8 treats worst, under a row mask that forbids two lanes in three: where the shadow's error makes
    the guard fail the collect pass answers, and the result is the oracle's either way."""
    dim, k = 256, 10
    rows, q = _family(name, dim)
    allowed = np.arange(N_FAM) % 3 == 0
    s_ref, r_ref = _oracle(rows, "bf16", q, k, allowed)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    idx.set_shadow8(2)
    l0 = idx.shadow8_stats()["launches"]
    s, r = idx.search(q, k, oracle.mask_from_bool(allowed))
    assert idx.shadow8_stats()["launches"] > l0
    _check(s, r, s_ref, r_ref)
    idx.close()
