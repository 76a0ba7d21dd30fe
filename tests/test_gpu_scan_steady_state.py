"""GPU: the scans' steady state -- many tiles per wave -- reached through a 16-CU mask (DESIGN.md "Steady-state
tests").

Every grid is sized min(CUs x blocks per CU, units / 8), so on a 256-CU device a corpus below ~65k rows is one tile per
wave: no mid-scan threshold refresh, no second trip round the corpus ring, no dynamic tail, and below 2048 tiles no
strided SAMPLE and no starting floor.  hr_index_set_cu_mask (the serving setup where the embedder shares the GPU) sets
the CU count the grids are sized from; with the smallest legal mask (16 CUs) a k_scan launch has 128-256 waves, a
128-query launch 128, a 256-query launch 64, and ~250k rows give every wave 24 tiles or more.

Every case, in this order:
  regime   wave_tiles().min() >= 24 (>= 48 for the shadow-8 scan: three refreshes at its cadence), or tiles // waves
           for the 128- and 256-query FILTERs, which do not fill wave_tiles; and >= 4096 tiles (strided SAMPLE, floor).
  path     the counter of the kernel the case is named after moved, the others did not.
  parity   rows equal to the oracle's, scores equal to its canonical fp64 scores cast to fp32, -inf / -1 padding.
  no hidden fallback   results are exact through the guard whatever the scan does, so a scan whose steady state is
           wrong still passes `parity` -- through the collect pass.  At least kj rows lie at or above the final
           threshold t, so the kj-th largest approximate score is >= t and t <= s_kj + E_q; the guard (s_k > t + E_q)
           must therefore pass whenever the oracle's exact s_k - s_kj > 2 E_q.  E_q is restated here in float64
           (_guard_e) from the test's own rounding of the query, never read back from the library, and taken 0.1 %
           larger than the formula: the library normalises the query in fp32 on the device, so its E_q may differ from
           this one in the last bits, and the demand is only valid with an E_q at least as large as the library's.
           The guard-failure delta may not exceed the number of queries that do not qualify, at most 1/8 of a batch may
           fail to qualify, and the exhaustive pass never runs.  fp32 rows under ip / l2 scan a bf16 shadow (u_x =
           2^-8) and mostly do not qualify: those cases assert regime, path and parity only.
  replay   the same batch again (the captured graph of the (B, k) shape) returns identical outputs.

What these cases found (hr_index.hip region_slots): the private candidate regions held 32 slots per (wave, query)
whatever the grid, so with 16x fewer waves every plan of four or more row parts (k = 100, the shadow-8 scan) overflowed
them and answered through the collect pass -- 1-6 of 64 queries in one group, all of them with query groups, over a
tile list, pipelined, and for the shadow-8 scan at k = 40.  Each printed line gives the case's tiles per wave, launch
counters, candidates per query, qualifying share and fallback deltas (pytest -s).
"""
import numpy as np
import pytest

import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

CUS16 = list(range(16))
# 16 CUs x 2 workgroups x 8 waves: the most waves a masked k_scan launch has (one workgroup per CU where the query
# tile takes more than half the LDS: 128)
MAX_WAVES = 256
KREF = 152           # deepest rank any case needs: kj8 of the shadow-8 scan at k = 40
QSEED = 4242


def _rows_for(tiles_per_wave, waves=MAX_WAVES):
    """Rows that give every one of `waves` waves `tiles_per_wave` tiles with a quarter to spare: the dynamic tail hands
    the last 10 % of a wave's share out from a counter and row-part teams split waves and tiles unevenly, so a wave may
    end up to ~12 % below the mean.  At least 4096 tiles (4 x the SAMPLE's 1024); the last tile is partial."""
    tiles = max(4 * 1024, (tiles_per_wave * 5 + 3) // 4 * waves)
    return tiles * 32 - 13


N_SCAN = _rows_for(24)      # 245,747 rows, 7680 tiles
N_SHADOW8 = _rows_for(48)   # 491,507 rows, 15360 tiles
N_2048 = _rows_for(24, 64)  # 131,059 rows, 4096 tiles: 2 groups x 64 waves at one workgroup per CU
N_BIG = 17_000 * 32 - 13    # 543,987 rows: early SAMPLE (>= 16384 tiles), tile lists of ~7.6k tiles


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid], s_ref[valid].astype(np.float32))
    assert np.all(np.isneginf(s_gpu[~valid]))


# ---------------------------------------------------------------- queries, guard window (CPU, reference only)
def _queries(seed, n, dim, metric, B=256, planted_only=False):
    """Planted (even) and isotropic (odd) queries.  cosine: unit row + 0.05 unit noise / N(0, 1); ip and l2 keep the
    rows raw, so both kinds are at the rows' own scale."""
    from hiprag import synth

    rng = np.random.default_rng([QSEED, seed, dim])
    pick = rng.choice(n, B, replace=False)
    x = synth.corpus_rows(seed, pick, dim)
    eps = rng.standard_normal((B, dim)).astype(np.float32)
    iso = rng.standard_normal((B, dim)).astype(np.float32)
    if metric == "cosine":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        eps /= np.linalg.norm(eps, axis=1, keepdims=True)
        q = x + np.float32(0.05) * eps
    else:
        sd = np.float32(x.std())
        q = x + np.float32(0.05) * sd * eps
        iso *= sd
    if not planted_only:
        q[1::2] = iso[1::2]
    return np.ascontiguousarray(q, np.float32)


def _mfma_type(dtype, metric):
    """What the scan rounds the queries to: the rows' own 16-bit type; fp32 rows scan an f16 shadow under cosine and
    a bf16 one under ip / l2."""
    if dtype != "f32":
        return dtype
    return "f16" if metric == "cosine" else "bf16"


def _max_norm(stored, dtype):
    mx = 0.0
    for lo in range(0, len(stored), 1 << 15):
        x = R.dequantize(stored[lo:lo + (1 << 15)], dtype).astype(np.float64)
        mx = max(mx, float(np.sqrt((x * x).sum(axis=1).max())))
    return mx


def _u_x8(stored, dtype, max_norm):
    """The shadow-8 storage term, restated: scale = max|x| / 127 (fp32), value = RNE(x / scale) clamped to +-127, the
    error norm ||x - scale * value|| in fp64, its maximum over the rows against the largest row norm."""
    worst = 0.0
    for lo in range(0, len(stored), 1 << 15):
        x = R.dequantize(stored[lo:lo + (1 << 15)], dtype).astype(np.float32)
        scale = (np.abs(x).max(axis=1, keepdims=True) / np.float32(127.0)).astype(np.float32)
        safe = np.where(scale > 0, scale, np.float32(1.0))
        v = np.clip(np.rint((x / safe).astype(np.float32)), -127.0, 127.0)
        d = x.astype(np.float64) - scale.astype(np.float64) * v.astype(np.float64)
        worst = max(worst, float(np.sqrt((d * d).sum(axis=1).max())))
    return worst / max_norm


def _guard_e(qp, dim, dtype, metric, max_norm, u_x8=None):
    """E_q of DESIGN.md "Exactness guard" per processed query, float64: max||x|| (||q - q^|| + (gamma + u_x) ||q^||),
    gamma = (dpad + 64) 2^-23; l2 (scan score 2 q^.x - |x|^2 in fp32) doubles it and adds the fp32 roundings of |x|^2
    and of the fused multiply-add (guard_e).  u_x8: the shadow-8 scan (f16 queries, its measured storage term, gamma
    with the scale multiply's rounding against the shadow's own norm)."""
    mt = "f16" if u_x8 is not None else _mfma_type(dtype, metric)
    qh = R.dequantize(R.quantize(qp, mt), mt).astype(np.float64)
    q64 = qp.astype(np.float64)
    dq = np.sqrt(((q64 - qh) ** 2).sum(axis=1))
    nq = np.sqrt((qh * qh).sum(axis=1))
    dpad = (dim + 63) // 64 * 64
    gamma = (dpad + 64) * 2.0 ** -23
    if u_x8 is not None:
        u = u_x8
        gamma = (gamma + 2.0 ** -23) * (1.0 + u_x8)
    elif dtype != "f32":
        u = 0.0
    elif mt == "bf16":
        u = 2.0 ** -8
    else:  # f16 shadow: 2^-11 relative, and the subnormal elements' absolute 2^-25 folded in (storage_u)
        u = 2.0 ** -11 + np.sqrt(dpad) * 2.0 ** -25 / max_norm
    e = max_norm * (dq * (1 + 1e-6) + (gamma + u) * nq) + 1e-9
    if metric == "l2":
        qn2 = (q64 * q64).sum(axis=1)
        e = 2.0 * e + 2.0 ** -22 * (max_norm ** 2 + 2.0 * max_norm * nq) + 1e-9
        e = e + 2.0 ** -50 * (1.0 + qn2 + max_norm ** 2 + 2.0 * max_norm * np.sqrt(qn2))  # euclid_slack
    return e * (1.0 + 1e-3)


def _kj(k, dim, shadow8=False):
    wide = (dim + 63) // 64 * 64 >= 2048
    margin = max(20, k) if wide else max(16, k // 2)
    return k + 4 * margin + 32 if shadow8 else k + margin


def _qualifies(s_ref, r_ref, k, kj, e):
    """Queries a correct scan must certify, from the reference alone: kj allowed rows exist and s_k - s_kj > 2 E_q"""
    return (r_ref[:, kj - 1] >= 0) & (s_ref[:, k - 1] - s_ref[:, kj - 1] > 2.0 * e)


class Corpus:
    """One synthetic corpus on the GPU with its 256 queries and, computed once per block of 64 queries and shared by
    every case, the oracle's top-KREF."""

    def __init__(self, native, dim, dtype, metric, n, seed, planted_only=False, no_shadows=False):
        self.dim, self.dtype, self.metric, self.n, self.seed = dim, dtype, metric, n, seed
        self.n_tiles = (n + 31) // 32
        # no_shadows: fp32 rows kept without their 16-bit scan shadow (as hiprag.ivf creates its indexes), so the scans
        # stream the fp32 rows as such -- the DT = F32 kernels.  The stored values, the oracle and E_q are the same.
        self.idx = native.NativeIndex(dim, dtype, metric, no_shadows=no_shadows)
        self.idx.add_synthetic(seed, 0, n)
        self.q = _queries(seed, n, dim, metric, planted_only=planted_only)
        self.qp = R.process_queries(self.q, metric)
        stored = self.stored()
        self.max_norm = _max_norm(stored, dtype)
        self.u_x8 = _u_x8(stored, dtype, self.max_norm) if metric == "cosine" else None
        self._blocks = {}
        self._ref_block(0, stored)

    def stored(self):
        return oracle.c_build_synthetic(self.seed, 0, self.n, self.dim, self.dtype, self.metric)

    def _ref_block(self, j, stored=None):
        if j not in self._blocks:
            stored = self.stored() if stored is None else stored
            self._blocks[j] = oracle.c_search(stored, self.dtype, self.qp[64 * j:64 * j + 64], KREF, metric=self.metric)
        return self._blocks[j]

    def ref(self, B):
        blocks = [self._ref_block(j) for j in range((B + 63) // 64)]
        return np.concatenate([b[0] for b in blocks])[:B], np.concatenate([b[1] for b in blocks])[:B]

    def e(self, B, shadow8=False):
        return _guard_e(self.qp[:B], self.dim, self.dtype, self.metric, self.max_norm, self.u_x8 if shadow8 else None)

    def benign_pick(self, B, k, kj, shadow8=False):
        """The first B of the 256 queries that qualify (s_k - s_kj > 2 E_q), chosen from the reference alone: a benign
        batch at a shape where the plain first B hold too many that no scan could be asked to certify"""
        s_ref, r_ref = self.ref(256)
        pick = np.nonzero(_qualifies(s_ref, r_ref, k, kj, self.e(256, shadow8)))[0][:B]
        assert len(pick) == B, f"only {len(pick)} of 256 queries qualify"
        return pick


@pytest.fixture(scope="module")
def corpora(native):
    cache = {}

    def get(dim, dtype, metric, n=N_SCAN, planted_only=False, no_shadows=False):
        key = (dim, dtype, metric, n, planted_only, no_shadows)
        if key not in cache:
            seed = 30 + 3 * ("bf16", "f16", "f32").index(dtype) + ("cosine", "ip", "l2").index(metric)
            cache[key] = Corpus(native, dim, dtype, metric, n, seed, planted_only, no_shadows)
        return cache[key]

    yield get
    for c in cache.values():
        c.idx.close()
    cache.clear()


# ---------------------------------------------------------------- the common frame
def _counters(idx):
    return {"wide": idx.wide_launches(), "q256": idx.q256_launches(), "qmask": idx.qmask_launches(),
            "shadow8": idx.shadow8_stats()["launches"]}


def _moved(before, after):
    return {name: after[name] - before[name] for name in before}


def _tiles_per_wave(idx, path, n_units):
    """Smallest number of tiles a wave of the last FILTER scanned: counted by k_scan; the 128- and 256-query FILTERs
    (16 workgroups of 8 resp. 4 waves, one tile per wave and round) do not count, so units // waves."""
    if path == "wide":
        return n_units // (16 * 8)
    if path == "q256":
        return n_units // (16 * 4)
    wt = idx.wave_tiles()
    assert len(wt) > 0, "no k_scan FILTER recorded its waves"
    assert len(wt) <= MAX_WAVES * 4, f"{len(wt)} waves: the grid was not sized from the 16-CU mask"
    return int(wt.min())


def _frame(label, idx, search, path, expect, s_ref, r_ref, k, kj, e, *, min_tiles=24, n_units, cus=CUS16, extra_fail=0):
    """regime, path, parity, no hidden fallback, replay (module docstring).  search() -> (scores, rows); expect: the
    launches by counter; e None: no fallback demand (fp32 rows under ip / l2); extra_fail: queries allowed to leave the
    main pass besides the non-qualifying ones."""
    idx.set_cu_mask(cus)
    assert n_units >= 4 * 1024, "SAMPLE not strided: the floor kernels would not run"
    c0, st0 = _counters(idx), idx.stats()
    s, r = search()
    c1, st1 = _counters(idx), idx.stats()
    cand_total, cand_max = idx.last_candidates()
    tiles = _tiles_per_wave(idx, path, n_units)
    moved = _moved(c0, c1)
    dg, dx = st1["guard_failures"] - st0["guard_failures"], st1["exhaustive"] - st0["exhaustive"]
    B = len(r)
    qual = _qualifies(s_ref, r_ref, k, kj, e) if e is not None else None
    share = "n/a (fp32 rows, bf16 shadow)" if qual is None else f"{int(qual.sum())}/{B}"
    print(f"\n[{label}] tiles/wave >= {tiles}, launches {moved}, candidates/query {cand_total / B:.1f} (max {cand_max}), "
          f"qualifying {share}, guard failures +{dg}, exhaustive +{dx}")
    assert tiles >= min_tiles, f"not the steady state: a wave scanned {tiles} tiles"
    assert moved == expect, f"path: launches {moved}, expected {expect}"
    _check(s, r, s_ref[:, :k], r_ref[:, :k])
    if qual is not None:
        nonq = int((~qual).sum())
        assert nonq * 8 <= B, f"inputs not benign: {nonq} of {B} queries do not qualify"
        assert dg <= nonq + extra_fail, f"hidden fallback: {dg} guard failures, {nonq} queries may fail"
        assert dx == 0, f"hidden fallback: {dx} exhaustive passes"
    s2, r2 = search()
    np.testing.assert_array_equal(r2, r)
    np.testing.assert_array_equal(s2.view(np.uint32), s.view(np.uint32))
    return s, r


def _expect(**kw):
    out = {"wide": 0, "q256": 0, "qmask": 0, "shadow8": 0}
    out.update(kw)
    return out


def _benign(dtype, metric):
    """fp32 rows under ip / l2 reach the MFMA as bf16 (their shadow, or converted when streamed): u_x = 2^-8 puts 2 E_q above most top-k gaps (0-84 % of the queries
    qualify, by dim and k), so no fallback demand can be made of them"""
    return not (dtype == "f32" and metric != "cosine")


def _plain(c, B, k, label, path="scan", expect=None, **kw):
    s_ref, r_ref = c.ref(B)
    e = c.e(B) if _benign(c.dtype, c.metric) else None
    return _frame(label, c.idx, lambda: c.idx.search(c.q[:B], k), path, expect or _expect(), s_ref, r_ref, k,
                  _kj(k, c.dim), e, n_units=c.n_tiles, **kw)


# ---------------------------------------------------------------- k_scan, one query group
# ring depth P = 4 / 8 / 16 at 64 / 128 / 256 dims; B = 20 is one query block (QB = 1), B = 64 two; k = 10 one row
# part, k = 32 two (team dealing), k = 100 five (early_refresh, k_floor_kth_parts)
SCAN_SHAPES = [(20, 10), (64, 10), (64, 32), (64, 100)]
SCAN_COSINE = [(dim, dtype, "cosine", B, k) for dim in (64, 128, 256) for dtype in ("bf16", "f16", "f32")
               for B, k in SCAN_SHAPES]
# ip / l2 keep the generator's raw rows (elements up to 1.3e5: beyond f16's range), so bf16 and f32 rows
SCAN_RAW = [(dim, dtype, metric, B, k)
            for dim, dtype, metric in ((128, "bf16", "ip"), (64, "f32", "ip"), (64, "bf16", "l2"), (128, "f32", "l2"))
            for B, k in ((64, 10), (20, 32), (64, 100))]
SCAN_PAD = [(200, "bf16", "cosine", 64, 10), (200, "bf16", "cosine", 20, 100)]  # 56 padding columns


@pytest.mark.parametrize("dim,dtype,metric,B,k", SCAN_COSINE + SCAN_RAW + SCAN_PAD,
                         ids=lambda v: str(v))
def test_k_scan_one_group(corpora, dim, dtype, metric, B, k):
    c = corpora(dim, dtype, metric)
    _plain(c, B, k, f"k_scan {dim} {dtype} {metric} B={B} k={k}")


def test_k_scan_2048_dims_two_32_query_groups(corpora):
    """2048 dims leave LDS for one 32-query block: B = 64 is two 32-query groups in one launch, and the margin is the
    wider max(20, k).  Half the rows: one workgroup per CU and two groups leave 64 waves per group."""
    c = corpora(2048, "bf16", "cosine", N_2048)
    _plain(c, 64, 10, "k_scan 2048 bf16 cosine B=64 k=10 (2 x 32-query groups)")
    assert len(c.idx.wave_tiles()) % 2 == 0


@pytest.mark.parametrize("B", [100, 256])
@pytest.mark.parametrize("k", [10, 100])
def test_k_scan_query_groups(corpora, B, k):
    """384 dims (24 k-steps: not a dim the 128-query FILTER takes): B = 100 is two 64-query groups, B = 256 four, each
    group's workgroups covering all tiles"""
    c = corpora(384, "bf16", "cosine")
    _plain(c, B, k, f"k_scan groups 384 bf16 B={B} k={k}")
    wt = c.idx.wave_tiles()
    groups = 2 if B == 100 else 4
    assert len(wt) % groups == 0 and int(wt.sum()) == groups * c.n_tiles


# ---------------------------------------------------------------- masks and deletions
@pytest.fixture(scope="module")
def masked(native, corpora):
    """543,987 x 64 bf16 rows; the oracle passes with the two masks are taken once.  `ranges`: three contiguous
    document ranges, 45 % of the rows (a tile list of ~7.6k tiles); `dense`: half the rows at random, and 2 % of all
    rows deleted from a second index over the same rows."""
    c = corpora(64, "bf16", "cosine", N_BIG)
    n = c.n
    rng = np.random.default_rng(9)
    ranges = np.zeros(n, bool)
    for lo in (20_011, 210_000, 400_003):
        ranges[lo:lo + n * 15 // 100] = True
    dense = rng.random(n) < 0.5
    dead = np.unique(rng.integers(0, n, n // 50))
    live = np.ones(n, bool)
    live[dead] = False
    idx2 = native.NativeIndex(c.dim, c.dtype, c.metric)
    idx2.add_synthetic(c.seed, 0, n)
    idx2.remove(dead)
    stored = c.stored()
    refs = {"ranges": oracle.c_search(stored, c.dtype, c.qp[:64], KREF, oracle.mask_from_bool(ranges)),
            "dense": oracle.c_search(stored, c.dtype, c.qp[:64], KREF, oracle.mask_from_bool(dense & live))}
    yield c, idx2, {"ranges": ranges, "dense": dense}, refs
    idx2.close()


@pytest.mark.parametrize("k", [10, 100])
def test_dense_bitmap_and_tombstones(masked, k):
    """A dense bitmap keeps the full scan with the mask fused into it; 2 % of the rows are tombstones"""
    c, idx2, masks, refs = masked
    m = oracle.mask_from_bool(masks["dense"])
    s_ref, r_ref = refs["dense"]
    _frame(f"k_scan dense bitmap + tombstones k={k}", idx2, lambda: idx2.search(c.q[:64], k, m), "scan", _expect(),
           s_ref, r_ref, k, _kj(k, c.dim), c.e(64), n_units=c.n_tiles)
    assert int(idx2.wave_tiles().sum()) == c.n_tiles  # (the full scan, not a list)


@pytest.mark.parametrize("k", [10, 100])
def test_tile_list_of_document_ranges(masked, k):
    """Contiguous document ranges become a tile list; it is long enough for the steady state, and every listed tile
    is scanned exactly once"""
    c, _, masks, refs = masked
    m = oracle.mask_from_bool(masks["ranges"])
    listed = len(np.unique(np.nonzero(masks["ranges"])[0] // 32))
    assert listed * 2 <= c.n_tiles  # (at most half the tiles: the list is used)
    s_ref, r_ref = refs["ranges"]
    _frame(f"k_scan tile list of {listed} tiles k={k}", c.idx, lambda: c.idx.search(c.q[:64], k, m), "scan", _expect(),
           s_ref, r_ref, k, _kj(k, c.dim), c.e(64), n_units=listed)
    assert int(c.idx.wave_tiles().sum()) == listed


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_per_query_masks(corpora, dtype):
    """search_masks, B = 64: two dense bitmaps, a sparse one (1 % of the rows) and unmasked queries by turns -- the
    per-query-mask (QM) scan bodies over a dense union.  Each query equals its single-mask oracle answer.  The strided
    SAMPLE sees almost none of a sparse mask's rows (the known hazard), so the sparse mask's 16 queries may
    leave the main pass.  The library counts fallbacks per call, not per query, so the other 48 queries -- dense masks
    and none -- are also searched in a call of their own, where none that qualifies may fall back."""
    c = corpora(64, dtype, "cosine")
    B, k, n = 64, 10, c.n
    rng = np.random.default_rng(12)
    allowed = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.01, rng.random(n) < 0.7])
    mask_of = (np.arange(B, dtype=np.int32) % 4) - 1  # -1 (none), 0, 1 (sparse), 2
    masks = np.stack([oracle.mask_from_bool(a) for a in allowed])
    stored = c.stored()
    s_ref = np.full((B, KREF), -np.inf)
    r_ref = np.full((B, KREF), -1, np.int64)
    for d in range(-1, 3):
        sel = np.nonzero(mask_of == d)[0]
        s_ref[sel], r_ref[sel] = oracle.c_search(stored, dtype, c.qp[sel], KREF,
                                                 None if d < 0 else oracle.mask_from_bool(allowed[d]))
    _frame(f"k_scan per-query masks 64 {dtype}", c.idx, lambda: c.idx.search_masks(c.q[:B], k, masks, mask_of), "scan",
           _expect(qmask=1), s_ref, r_ref, k, _kj(k, c.dim), c.e(B), n_units=c.n_tiles,
           extra_fail=int((mask_of == 1).sum()))
    rest = np.nonzero(mask_of != 1)[0]
    q_rest, of_rest = np.ascontiguousarray(c.q[rest]), np.ascontiguousarray(mask_of[rest])
    _frame(f"k_scan per-query masks 64 {dtype}, the 48 dense / unmasked queries", c.idx,
           lambda: c.idx.search_masks(q_rest, k, masks, of_rest), "scan", _expect(qmask=1), s_ref[rest], r_ref[rest], k,
           _kj(k, c.dim), c.e(B)[rest], n_units=c.n_tiles)


# ---------------------------------------------------------------- the 128-query FILTER (hr_wide.hip)
# (dim, dtype, metric, k, no_shadows).  Row parts: k = 32 is two; k = 100 is five, more than the three the 128-query
# FILTER takes on 16-bit rows -- and fp32 rows that scan their 16-bit shadow plan alike -- so the five-part cases keep
# the fp32 rows without a shadow (streamed as such: up to seven parts, the DT = F32 eight-wave form).
# (512 dims in f16: with bf16 queries 21 of these 128 queries have s_32 - s_48 <= 2 E_q there, more than the 1/8 a
# benign batch may hold.)
WIDE = [(256, dtype, "cosine", k, False) for dtype in ("bf16", "f16", "f32") for k in (10, 32)] + \
       [(512, "f16", "cosine", 10, False), (512, "f16", "cosine", 32, False), (256, "bf16", "l2", 10, False),
        (256, "bf16", "l2", 32, False), (512, "f32", "l2", 10, False),
        (256, "f32", "cosine", 100, True), (512, "f32", "l2", 100, True)]


@pytest.mark.parametrize("dim,dtype,metric,k,no_shadows", WIDE, ids=lambda v: str(v))
def test_wide_filter(corpora, dim, dtype, metric, k, no_shadows):
    """B = 128 at the dims the 128-query FILTER takes: one launch of 16 workgroups x 8 waves, 60 tiles per wave, with
    one, two and five row parts"""
    c = corpora(dim, dtype, metric, no_shadows=no_shadows)
    _plain(c, 128, k, f"wide8 {dim} {dtype}{' streamed' if no_shadows else ''} {metric} B=128 k={k}", path="wide",
           expect=_expect(wide=1))


# ---------------------------------------------------------------- the 256-query FILTER (hr_q256.hip)
@pytest.mark.parametrize("dtype,no_shadows", [("bf16", False), ("f16", False), ("f32", False), ("f32", True)],
                         ids=["bf16", "f16", "f32-shadow", "f32-streamed"])
def test_q256_filter(corpora, dtype, no_shadows):
    """B = 256, k = 10 at 256 dims: one 256-query launch (16 workgroups x 4 waves, 120 tiles per wave); with the
    256-query FILTER off, two 128-query launches return the same bits.  fp32 rows scan their f16 shadow by default
    (the 16-bit kernel again); without the shadow they are streamed as such: k_filter_q256's DT = F32 body."""
    c = corpora(256, dtype, "cosine", no_shadows=no_shadows)
    dtype = dtype + (" streamed" if no_shadows else "")
    s, r = _plain(c, 256, 10, f"q256 256 {dtype} B=256 k=10", path="q256", expect=_expect(q256=1))
    c.idx.set_q256(False)
    try:
        s2, r2 = _plain(c, 256, 10, f"q256 off: 2 x wide8 256 {dtype} B=256 k=10", path="wide", expect=_expect(wide=2))
    finally:
        c.idx.set_q256(True)
    np.testing.assert_array_equal(r2, r)
    np.testing.assert_array_equal(s2.view(np.uint32), s.view(np.uint32))


# ---------------------------------------------------------------- the shadow-8 scan
def _shadow8(c, B, k, label, kc8, pick=None):
    pick = np.arange(B) if pick is None else pick
    s_ref, r_ref = c.ref(int(pick.max()) + 1)
    q = np.ascontiguousarray(c.q[pick])
    c.idx.set_shadow8(2)
    try:
        _frame(label, c.idx, lambda: c.idx.search(q, k), "scan", _expect(shadow8=1), s_ref[pick], r_ref[pick], k,
               _kj(k, c.dim, shadow8=True), c.e(int(pick.max()) + 1, shadow8=True)[pick], min_tiles=48,
               n_units=c.n_tiles)
        assert c.idx.shadow8_stats()["kc8"] == kc8
    finally:
        c.idx.set_shadow8(1)


SHADOW8 = [(dim, dtype, k) for dim in (128, 256) for dtype in ("bf16", "f16", "f32") for k in (10, 40)]


@pytest.mark.parametrize("dim,dtype,k", SHADOW8, ids=lambda v: str(v))
def test_shadow8_scan(corpora, dim, dtype, k):
    """set_shadow8(2): the int8 shadow's scan (ring of 4 / 8 paired k-steps at 128 / 256 dims) with its 16-tile
    cadence and the thresholds shared through the LDS row; kc8 = 128 / 160 are four / five row parts.  256 dims, fp32
    rows, k = 40: E_q of the int8 shadow is ~0.009 whatever the dim while the top-k gaps shrink with it, and 9 of the
    first 64 queries have s_40 - s_152 <= 2 E_q -- more than a benign batch may hold -- so that case takes the first 64
    of the corpus's 256 queries that qualify by the reference."""
    c = corpora(dim, dtype, "cosine", N_SHADOW8)
    pick = c.benign_pick(64, k, _kj(k, dim, shadow8=True), shadow8=True) if (dim, dtype, k) == (256, "f32", 40) else None
    _shadow8(c, 64, k, f"shadow-8 {dim} {dtype} B=64 k={k}", 128 if k == 10 else 160, pick)


def test_shadow8_scan_refresh_from_the_table(corpora):
    """1280 dims at B = 64 (QB = 2): the query tile fills the 160 KiB of LDS, no room is left for the shared threshold
    row (launch_scan8: lds + QB * 32 * 4 <= 160 KiB fails), so every wave refreshes all its thresholds from the table
    -- the shadow-8 body without THL.  One workgroup per CU: 128 waves.  At 1280 dims the background scores lie within
    2 E_q of each other (28 of 64 mixed queries qualify at k = 10), so the batch is planted queries at k = 1: the
    planted row stands 0.9 above the background, every query qualifies, and the plan is the same four row parts."""
    c = corpora(1280, "bf16", "cosine", _rows_for(48, 128), planted_only=True)
    _shadow8(c, 64, 1, "shadow-8 1280 bf16 B=64 k=1 (refresh from the table)", 128)


# ---------------------------------------------------------------- fallbacks inside the regime
def test_fallbacks_on_the_masked_grid(native):
    """100 duplicates of one row (more than kc = 32 candidates tie: the guard must fail, and the collect pass runs on
    the 16-CU grid) and 3000 of another (more than the collect buffer holds: the exhaustive pass).  Here the counters
    must rise, and the results are still the oracle's: the lowest duplicate rows first."""
    dim, n, B, k = 64, N_SCAN, 64, 10
    rng = np.random.default_rng(17)
    raw = oracle.c_gen_rows(41, 0, n, dim)
    pos = rng.choice(n, 3100, replace=False)
    few, many = np.sort(pos[:100]), np.sort(pos[100:])
    raw[few] = raw[few[0]]
    raw[many] = raw[many[0]]
    q = _queries(41, n, dim, "cosine", B)
    q[0], q[1] = raw[few[0]], raw[many[0]]
    idx = native.NativeIndex(dim, "bf16", "cosine")
    try:
        idx.add(raw)
        stored = oracle.c_quantize(oracle.c_normalize_rows(raw), "bf16")
        qp = R.process_queries(q, "cosine")
        s_ref, r_ref = oracle.c_search(stored, "bf16", qp, KREF)
        e = _guard_e(qp, dim, "bf16", "cosine", _max_norm(stored, "bf16"))
        qual = _qualifies(s_ref, r_ref, k, _kj(k, dim), e)
        assert not qual[0] and not qual[1] and int((~qual).sum()) * 8 <= B
        idx.set_cu_mask(CUS16)

        def run(qs):
            c0, st0 = _counters(idx), idx.stats()
            s, r = idx.search(qs, k)
            c1, st1 = _counters(idx), idx.stats()
            assert _moved(c0, c1) == _expect()  # (k_scan, its collect pass and the exhaustive pass)
            return s, r, st1["guard_failures"] - st0["guard_failures"], st1["exhaustive"] - st0["exhaustive"]

        # each planted query alone (B = 1: one query block on the same grid), tied to its own counter ...
        for j, rows, want in ((0, few, (1, 0)), (1, many, (1, 1))):
            s, r, dg, dx = run(q[j:j + 1])
            assert int(idx.wave_tiles().min()) >= 24
            _check(s, r, s_ref[j:j + 1, :k], r_ref[j:j + 1, :k])
            np.testing.assert_array_equal(r[0], rows[:k])
            assert (dg, dx) == want, f"query {j}: guard failures +{dg}, exhaustive +{dx}, expected {want}"
        # ... and in the batch of 64, where only queries that do not qualify may join them
        s, r, dg, dx = run(q)
        tiles = int(idx.wave_tiles().min())
        nonq = int((~qual).sum())
        print(f"\n[fallbacks] tiles/wave >= {tiles}, candidates {idx.last_candidates()}, qualifying {int(qual.sum())}/{B}, "
              f"guard failures +{dg}, exhaustive +{dx}")
        assert tiles >= 24
        _check(s, r, s_ref[:, :k], r_ref[:, :k])
        np.testing.assert_array_equal(r[0], few[:k])
        np.testing.assert_array_equal(r[1], many[:k])
        assert 2 <= dg <= nonq
        assert 1 <= dx <= nonq - 1
        s2, r2, dg2, dx2 = run(q)  # replay: the same answers through the same fallbacks
        np.testing.assert_array_equal(r2, r)
        np.testing.assert_array_equal(s2.view(np.uint32), s.view(np.uint32))
        assert (dg2, dx2) == (dg, dx)
    finally:
        idx.close()


# ---------------------------------------------------------------- pipelined batches under the mask
@pytest.mark.parametrize("k,max_k", [(10, 16), (100, 100)])
def test_pipelined_batches(corpora, k, max_k):
    """ShardedSearch.submit / finalize_all with four batches in flight, queries ready by event: dual FILTER streams,
    the early SAMPLE (>= 16384 tiles) and early_refresh; the pipelined FILTER leaves half the 16 CUs to the tail, so
    its grid is smaller still.  Every batch equals the oracle, and no qualifying query reaches the fallback."""
    torch = pytest.importorskip("torch")
    from hiprag.dist import ShardedSearch

    c = corpora(64, "bf16", "cosine", N_BIG)
    s_ref, r_ref = c.ref(256)
    qual = _qualifies(s_ref, r_ref, k, _kj(k, c.dim), c.e(256))
    assert int((~qual).sum()) * 8 <= 256
    c.idx.set_cu_mask(CUS16)
    qd = torch.from_numpy(c.q).cuda().view(4, 64, c.dim)
    ready = torch.cuda.Event()
    ready.record()
    ss = ShardedSearch(c.idx, 0, max_batch=64, max_k=max_k, depth=4, device=torch.device("cuda", 0))
    s_out = torch.empty((4, 64, k), dtype=torch.float32, device="cuda")
    r_out = torch.empty((4, 64, k), dtype=torch.int64, device="cuda")
    x0, c0 = c.idx.stats()["exhaustive"], _counters(c.idx)
    for rep in range(2):  # every workspace a second time
        for i in range(4):
            ss.submit(qd[i], k, s_out=s_out[i], r_out=r_out[i], q_ready=ready)
        ss.finalize_all()
        torch.cuda.synchronize()
        for i in range(4):
            _check(s_out[i].cpu().numpy(), r_out[i].cpu().numpy(), s_ref[64 * i:64 * i + 64, :k],
                   r_ref[64 * i:64 * i + 64, :k])
    tiles = int(c.idx.wave_tiles().min())
    dx = c.idx.stats()["exhaustive"] - x0
    print(f"\n[pipelined k={k}] tiles/wave >= {tiles}, candidates (last batch) {c.idx.last_candidates()}, qualifying "
          f"{int(qual.sum())}/256, fallback queries {ss.fallback_queries} in 2 rounds, exhaustive +{dx}")
    assert tiles >= 24
    assert _moved(c0, _counters(c.idx)) == _expect()  # (k_scan FILTERs: no other kernel's counter moved)
    assert ss.fallback_queries <= 2 * int((~qual).sum()) and dx == 0
    ss.close()


# ---------------------------------------------------------------- which CUs, and lifting the mask
def test_mask_choice_and_lifting_the_mask(corpora):
    """The same k_scan case on the first 16 CUs, on 16 CUs spread over the device (every 16th of 256), and with the
    mask lifted: identical bits each time, and wave_tiles shows the full-device grid again"""
    torch = pytest.importorskip("torch")

    c = corpora(128, "bf16", "cosine")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    spread = list(range(0, n_cu, n_cu // 16))[:16]
    s_ref, r_ref = c.ref(64)
    args = (s_ref, r_ref, 10, _kj(10, c.dim), c.e(64))
    search = lambda: c.idx.search(c.q[:64], 10)  # noqa: E731
    s0, r0 = _frame("k_scan first 16 CUs", c.idx, search, "scan", _expect(), *args, n_units=c.n_tiles)
    waves16 = len(c.idx.wave_tiles())
    s1, r1 = _frame(f"k_scan CUs {spread[:3]}...", c.idx, search, "scan", _expect(), *args, n_units=c.n_tiles, cus=spread)
    assert len(c.idx.wave_tiles()) == waves16
    c.idx.set_cu_mask(None)
    s2, r2 = search()
    wt = c.idx.wave_tiles()
    print(f"\n[mask lifted] {len(wt)} waves (masked: {waves16}), tiles/wave {int(wt.min())}..{int(wt.max())}")
    assert len(wt) > waves16 and int(wt.sum()) == c.n_tiles
    for s, r in ((s1, r1), (s2, r2)):
        np.testing.assert_array_equal(r, r0)
        np.testing.assert_array_equal(s.view(np.uint32), s0.view(np.uint32))
