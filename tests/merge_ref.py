"""Plain numpy restatements of the three kernels every exact answer leaves the GPU through, and the crafted
inputs that pin them (shared by tests/test_merge_ref_cpu.py and tests/test_gpu_merge_kernels.py):

  ref_merge         k_merge         (hr_merge_candidates[_strided]): top-k of G ranks' candidates + exactness guard
  ref_merge_sorted  k_merge_sorted  (hr_merge_sorted): top-k of G ranks' sorted lists
  ref_topk          k_topk_cand     (hr_topk_records): top-m of one segment
  topk_path         which of k_topk_cand's four paths a segment takes (a restatement of its control flow)

A record is {float64 score, int64 row}; an array of records is a float64 array with a last axis of 2 whose second
element holds the row's bits (pack / unpack).  The order everywhere is (score desc, row asc) with -0.0 == +0.0;
records with row < 0 are absent whatever their score; padding is (-inf, -1).  No GPU, no torch.
"""
import numpy as np

NI = -np.inf
PATHS = ("all", "level1", "full", "full+ids")
TOPK_MAX = 1024  # k_topk_cand's LDS capacity, in records
_ABSENT_ROWS = np.array([-1, -7, -2 ** 63], np.int64)


def pack(scores, rows):
    scores, rows = np.asarray(scores, np.float64), np.asarray(rows, np.int64)
    rec = np.empty(scores.shape + (2,), np.float64)
    rec[..., 0] = scores
    rec.view(np.int64)[..., 1] = rows
    return rec


def unpack(rec):
    rec = np.ascontiguousarray(rec)
    assert rec.dtype == np.float64 and rec.shape[-1] == 2
    return rec[..., 0], rec.view(np.int64)[..., 1]


def _sorted_valid(scores, rows):
    scores, rows = np.asarray(scores, np.float64).reshape(-1), np.asarray(rows, np.int64).reshape(-1)
    keep = rows >= 0
    scores, rows = scores[keep], rows[keep]
    order = np.lexsort((rows, -scores))  # -(+-0.0) compare equal, -(-inf) sorts last
    return scores[order], rows[order]


# ---------------------------------------------------------------- references
def ref_merge(cand, bounds, k):
    """cand [G, B, kc] records, bounds [G, B] -> scores f32 [B, k], rows i64 [B, k], kth f64 [B], fail i32 [B]."""
    sc, rw = unpack(cand)
    bounds = np.asarray(bounds, np.float64)
    B = sc.shape[1]
    s_out = np.full((B, k), NI, np.float32)
    r_out = np.full((B, k), -1, np.int64)
    kth = np.full(B, NI)
    fail = np.zeros(B, np.int32)
    for q in range(B):
        s, r = _sorted_valid(sc[:, q], rw[:, q])
        n = min(k, len(r))
        s_out[q, :n], r_out[q, :n] = s[:n], r[:n]
        if len(r) >= k:
            kth[q] = s[k - 1]
        maxb = bounds[:, q].max()
        fail[q] = int(maxb > NI and (len(r) < k or not kth[q] > maxb))
    return s_out, r_out, kth, fail


def ref_merge_sorted(cand, k):
    """cand [G, B, m] records (each rank's list sorted, absent records at its tail) -> scores f32 [B, k], rows i64
    [B, k]: the top-k of the union."""
    sc, rw = unpack(cand)
    B = sc.shape[1]
    s_out = np.full((B, k), NI, np.float32)
    r_out = np.full((B, k), -1, np.int64)
    for q in range(B):
        s, r = _sorted_valid(sc[:, q], rw[:, q])
        n = min(k, len(r))
        s_out[q, :n], r_out[q, :n] = s[:n], r[:n]
    return s_out, r_out


def ref_topk(scores, ids, m):
    """One segment -> scores f64 [m], ids i64 [m]."""
    s, r = _sorted_valid(scores, ids)
    out_s = np.full(m, NI)
    out_r = np.full(m, -1, np.int64)
    n = min(m, len(r))
    out_s[:n], out_r[:n] = s[:n], r[:n]
    return out_s, out_r


def d2key(x):
    """The kernels' order-preserving float64 -> uint64 key: +0.0 replaces -0.0, a negative value is ~bits, any other
    bits | sign."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.where(x == 0.0, 0.0, x).view(np.uint64)
    sign = np.uint64(1 << 63)
    return np.where((u & sign) != 0, ~u, u | sign)


def topk_path(scores, ids, m):
    """The path k_topk_cand takes on one segment: "all" (no selection: n_valid <= m), "level1" (the records whose
    upper 32 key bits are at or above the m-th's fit in LDS), "full" (they do not; 64-bit select, every tie at the
    m-th key wins), "full+ids" (they do not; the ties at the m-th key exceed the need, radix select over ids)."""
    scores, ids = np.asarray(scores, np.float64).reshape(-1), np.asarray(ids, np.int64).reshape(-1)
    keys = d2key(scores[ids >= 0])
    if len(keys) <= m:
        return "all"
    hi = keys >> np.uint64(32)
    mth_hi = np.sort(hi)[::-1][m - 1]
    if int((hi >= mth_hi).sum()) <= TOPK_MAX:
        return "level1"
    kth = np.sort(keys)[::-1][m - 1]
    need_ties = m - int((keys > kth).sum())
    n_ties = int((keys == kth).sum())
    return "full+ids" if n_ties > need_ties else "full"


# ---------------------------------------------------------------- k_merge: the guard table
def _scatter(rng, G, kc, recs, ranks=None):
    """recs (a list of (score, row)) at random slots of a [G, kc] grid whose other slots are absent records that
    would win: score +inf, a negative row.  ranks: {index in recs: rank} pins a record to one rank's list."""
    scores = np.full((G, kc), np.inf)
    rows = rng.choice(_ABSENT_ROWS, size=(G, kc))
    free = rng.permutation(G * kc).tolist()
    assert len(recs) <= len(free)
    ranks = ranks or {}
    for i in sorted(range(len(recs)), key=lambda i: i not in ranks):  # pinned records first
        if i in ranks:
            slot = next(x for x in free if x // kc == ranks[i])
            free.remove(slot)
        else:
            slot = free.pop()
        scores[slot // kc, slot % kc], rows[slot // kc, slot % kc] = recs[i]
    return scores, rows


def merge_cases(G, kc, k, seed=0):
    """The guard table of k_merge for one geometry and one k: a list of dicts (name, scores [G, kc], rows [G, kc],
    bounds [G], fail, kth, rows_at) with the expected fail / kth written out by hand; rows_at pins single positions
    of the expected rows ({position: row}, or "ascending")."""
    assert G >= 2 and 1 <= k <= kc and kc >= 8
    rng = np.random.default_rng([seed, G, kc, k])
    n = G * kc
    cases = []

    def rows_for(cnt, base=0):
        return [base + int(r) for r in rng.permutation(16 * n)[:cnt]]

    def ladder(cnt, base=0):  # scores 5000, 4999, ...: the k-th is 5001 - k
        return [(5000.0 - j, r) for j, r in enumerate(rows_for(cnt, base))]

    def below(cnt):  # losers, rows disjoint from rows_for's
        return [(-5.0 - j, 16 * n + 1 + j) for j in range(cnt)]

    def add(name, recs, bounds, fail, kth, ranks=None, rows_at=None):
        s, r = _scatter(rng, G, kc, recs, ranks)
        cases.append(dict(name=name, scores=s, rows=r, bounds=np.asarray(bounds, np.float64), fail=fail, kth=kth,
                          rows_at=rows_at or {}))

    kth_l = 5001.0 - k
    nob = [NI] * G
    low = [kth_l - 50.0 - g for g in range(G)]  # finite bounds, all below the ladder's k-th

    add("no_bounds_enough", ladder(k + 5), nob, 0, kth_l)
    add("no_bounds_short", ladder(k - 1), nob, 0, NI, rows_at={k - 1: -1})
    add("bound_short", ladder(k - 1), [-1e300] * G, 1, NI, rows_at={k - 1: -1})
    add("bounds_below", ladder(k + 5), low, 0, kth_l)
    b = list(low)
    b[G // 2] = kth_l
    add("kth_eq_maxb", ladder(k + 5), b, 1, kth_l)
    up, down = float(np.nextafter(0.3, np.inf)), float(np.nextafter(0.3, NI))
    b = [0.1] * G
    b[1] = 0.3
    add("kth_one_ulp_above_maxb", ladder(k - 1) + [(up, 16 * n)] + below(5), b, 0, up, rows_at={k - 1: 16 * n})
    add("kth_one_ulp_below_maxb", ladder(k - 1) + [(down, 16 * n)] + below(5), b, 1, down, rows_at={k - 1: 16 * n})
    b = list(low)
    b[G - 1] = kth_l + 0.5
    add("last_rank_bound_only", ladder(k + 5), b, 1, kth_l)
    b = list(low)
    b[0] = kth_l + 0.5
    add("first_rank_bound_only", ladder(k + 5), b, 1, kth_l)
    b = list(low)
    b[G // 2] = np.inf
    add("bound_overflow_marker", ladder(k + 5), b, 1, kth_l)
    # k-th and (k+1)-th tied across two ranks: the lower row, in the last rank, wins
    r_hi, r_lo = 16 * n + 900, 16 * n + 800
    add("tie_at_k_across_ranks", ladder(k - 1) + [(50.0, r_hi), (50.0, r_lo)] + below(5), nob, 0, 50.0,
        ranks={k - 1: 0, k: G - 1}, rows_at={k - 1: r_lo})
    add("all_tied", [(7.25, r) for r in rows_for(n)], [7.0] * G, 0, 7.25, rows_at="ascending")
    # _scatter's absents, (+inf, row < 0), between the valid records of every list: four losers pinned to each rank
    add("absent_inf_scattered", ladder(k + 5) + below(4 * G), low, 0, kth_l,
        ranks={k + 5 + j: j % G for j in range(4 * G)})
    # a valid -inf record: last among the valid, ahead of the padding; -inf never clears a finite bound
    add("valid_neg_inf_no_bounds", ladder(k - 1) + [(NI, 16 * n + 3)], nob, 0, NI, rows_at={k - 1: 16 * n + 3})
    add("valid_neg_inf_bound", ladder(k - 1) + [(NI, 16 * n + 3)], [-1e308] * G, 1, NI, rows_at={k - 1: 16 * n + 3})
    zr = sorted(rows_for(k + 4))
    add("signed_zeros", [((0.0, -0.0)[(j * 7 // 3) % 2], r) for j, r in enumerate(zr)], [-1.0] * G, 0, 0.0,
        rows_at={0: zr[0], k - 1: zr[k - 1]})
    big = ladder(k + 5, base=2 ** 40)
    big[0] = (big[0][0], 2 ** 62 + 5)
    big[k - 1] = (big[k - 1][0], 2 ** 62)
    add("big_rows", big, low, 0, kth_l, rows_at={0: 2 ** 62 + 5, k - 1: 2 ** 62})
    return cases


def stack_merge_cases(cases):
    """One query per case: scores [G, B, kc], rows [G, B, kc], bounds [G, B]."""
    return (np.stack([c["scores"] for c in cases], 1), np.stack([c["rows"] for c in cases], 1),
            np.stack([c["bounds"] for c in cases], 1))


_FUZZ_VALUES = np.array([NI, -1e30, -2.5, -0.0, 0.0, 0.5, 1.0, float(np.nextafter(1.0, 2.0)), 3.0])


def merge_fuzz(G, kc, B, seed):
    """Random k_merge input: scores from a small set (ties everywhere) or normals, absents interleaved at a rate
    from none to all, bounds from the same set.  -> scores [G, B, kc], rows [G, B, kc], bounds [G, B]."""
    rng = np.random.default_rng([seed, G, kc, B])
    n = G * kc
    scores = np.empty((G, B, kc))
    rows = np.empty((G, B, kc), np.int64)
    bounds = np.empty((G, B))
    for q in range(B):
        s = rng.choice(_FUZZ_VALUES, n) if q % 3 else np.round(rng.standard_normal(n), 1)
        r = rng.permutation(4 * n)[:n].astype(np.int64) + (2 ** 41 if q % 5 == 0 else 0)
        absent = rng.random(n) < rng.choice([0.0, 0.05, 0.5, 0.95, 1.0])
        s[absent & (rng.random(n) < 0.5)] = np.inf
        r[absent] = rng.choice(_ABSENT_ROWS, int(absent.sum()))
        scores[:, q], rows[:, q] = s.reshape(G, kc), r.reshape(G, kc)
        bounds[:, q] = NI if q % 2 else rng.choice(np.concatenate([_FUZZ_VALUES, [NI, NI, np.inf]]), G)
    return scores, rows, bounds


# ---------------------------------------------------------------- k_merge_sorted
def merge_sorted_case(G, m, k, seed=0):
    """B = 5 queries of G sorted lists of m records -> scores [G, 5, m], rows [G, 5, m]:
      0  tied scores from a small set, lists of different lengths, one list all padding (G >= 2)
      1  every record of every list tied
      2  distinct scores but for one run of ties that straddles positions k-1 and k, consecutive rows in different lists
      3  few valid records, valid -inf scores ahead of padding whose score is +inf
      4  nothing valid"""
    rng = np.random.default_rng([seed, G, m, k])
    B = 5
    scores = np.full((G, B, m), NI)
    rows = np.full((G, B, m), -1, np.int64)

    def put(q, g, s, r):
        s, r = _sorted_valid(s, r)
        scores[g, q, :len(r)], rows[g, q, :len(r)] = s, r

    def split(q, s, r, lens):
        perm = rng.permutation(len(r))
        at = 0
        for g in range(G):
            idx = perm[at:at + lens[g]]
            put(q, g, s[idx], r[idx])
            at += lens[g]

    # 0
    lens = rng.integers(m // 2, m + 1, G)
    lens[0] = m if G >= 2 else m - 3
    if G >= 2:
        lens[G // 2] = 0
    if G >= 3:
        lens[G - 1] = 1
    tot = int(lens.sum())
    split(0, rng.choice(_FUZZ_VALUES, tot), rng.permutation(8 * tot)[:tot].astype(np.int64) + 2 ** 40, lens)
    # 1
    tot = G * m
    r = rng.permutation(4 * tot)[:tot].astype(np.int64)
    split(1, np.full(tot, -1.5), r, [m] * G)
    # 2: round-robin over the lists in the union's order, so neighbours of the tie run sit in different lists
    tot = G * m
    s = 1000.0 - np.arange(tot)
    t = min(k - 1, tot - 2)
    s[max(0, t - 2):t + 4] = s[max(0, t - 2)]
    r = np.sort(rng.permutation(4 * tot)[:tot].astype(np.int64))
    for g in range(G):
        put(2, g, s[g::G], r[g::G])
    # 3
    lens = np.minimum(m, rng.integers(2, 9, G))
    tot = int(lens.sum())
    s = rng.choice(np.array([NI, NI, 2.0, -3.0]), tot)
    split(3, s, rng.permutation(4 * tot)[:tot].astype(np.int64), lens)
    scores[:, 3][rows[:, 3] < 0] = np.inf
    return scores, rows


# ---------------------------------------------------------------- k_topk_cand
TOPK_LENGTHS = (1023, 1024, 1025, 4095, 4096, 4097, 8 * 1024 + 3)  # around for_each_record's 4 x 1024 unroll


def _mix_absents(rng, scores, ids, n_abs):
    """n_abs absent records (+inf, row < 0) at random positions among the given ones."""
    n = len(ids) + n_abs
    s = np.full(n, np.inf)
    r = rng.choice(_ABSENT_ROWS, n)
    pos = np.sort(rng.permutation(n)[:len(ids)])
    s[pos], r[pos] = scores, ids
    return s, r


def topk_cases(seed=0):
    """The crafted segments of k_topk_cand: a list of dicts (name, path, m, scores, ids), path being the one of PATHS
    the case is built to take (tests/test_merge_ref_cpu.py holds topk_path to it)."""
    rng = np.random.default_rng([seed, 77])
    cases = []

    def add(name, path, m, scores, ids, n_abs=None):
        scores, ids = np.asarray(scores, np.float64), np.asarray(ids, np.int64)
        if n_abs is None:
            n_abs = len(ids) // 16 + 3
        if n_abs:
            scores, ids = _mix_absents(rng, scores, ids, n_abs)
        cases.append(dict(name=name, path=path, m=m, scores=scores, ids=ids))

    def perm_ids(n, mult=1, base=0):
        return rng.permutation(n).astype(np.int64) * mult + base

    # all records fit
    for m in (100, 1024):
        for nv in (0, 1, m - 1, m):
            s = np.round(rng.standard_normal(nv), 1)  # ties
            if nv > 1:
                s[:2] = NI  # valid -inf records
            add(f"all_m{m}_valid{nv}", "all", m, s, perm_ids(nv, 3, 11))
    # level 1
    normals = rng.standard_normal(5000)
    assert len(np.unique(normals)) == 5000
    for m in (1, 100, 1024):
        add(f"level1_normals_m{m}", "level1", m, normals, perm_ids(5000))
    add("level1_m1024_valid1025", "level1", 1024, rng.permutation(1025) * 0.001 - 0.5, perm_ids(1025))
    z = np.concatenate([np.tile([0.0, -0.0, -0.0], 100), -1.0 - rng.random(300)])
    add("level1_signed_zeros_m100", "level1", 100, z, perm_ids(600))
    # level-1 overflow, all ties at the m-th key needed: 3000 distinct scores sharing the upper 32 key bits
    j = rng.permutation(3000).astype(np.float64)
    for m in (1, 100, 1024):
        add(f"full_pos_m{m}", "full", m, 1.0 + j * 2.0 ** -45, perm_ids(3000))
        add(f"full_neg_m{m}", "full", m, -1.0 - j * 2.0 ** -45, perm_ids(3000))
    # overflow + id select: 3000 records of one score, three id sets
    id_sets = {
        "lowbits": lambda: perm_ids(3000, 1, (0x1234567 << 32) | 0x89AB0000),  # a common high part, 12 low bits
        "highbits": lambda: perm_ids(3000, 2 ** 33, 5),  # perm * 2^33 + c: the high radix passes decide
        "wide": lambda: np.concatenate([[0, 2 ** 62], rng.integers(1, 2 ** 62, 2998)])[rng.permutation(3000)],
    }
    for m in (1, 100, 1024):
        for name, ids in id_sets.items():
            ids = ids()
            assert len(np.unique(ids)) == 3000
            add(f"ids_{name}_m{m}", "full+ids", m, np.full(3000, 0.625), ids)
    # 50 above, 2000 tied at the m-th place, 500 below: need_ties = 50 of 2000
    s = np.concatenate([2.0 + np.arange(50), np.full(2000, 1.5), -np.arange(500.0)])
    p = rng.permutation(2550)
    add("ids_mixed_50_of_2000_m100", "full+ids", 100, s[p], perm_ids(2550, 2 ** 20, 1))
    # 50 above, 256 tied at the m-th place whose ids differ in the low byte only, 1700 below; one upper key word
    t = 1.0 + 2000 * 2.0 ** -45
    s = np.concatenate([t + (1 + np.arange(50)) * 2.0 ** -45, np.full(256, t), t - (1 + np.arange(1700)) * 2.0 ** -45])
    ids = np.concatenate([10 ** 12 + np.arange(50), (0x7654321 << 8) + rng.permutation(256), 10 ** 13 + np.arange(1700)])
    p = rng.permutation(2006)
    add("ids_low_byte_50_of_256_m100", "full+ids", 100, s[p], ids[p])
    add("ids_signed_zeros_m100", "full+ids", 100, np.tile([0.0, -0.0, -0.0], 1000), perm_ids(3000))
    s = np.concatenate([rng.standard_normal(900), np.full(2100, NI)])  # the 1024-th is a valid -inf: 124 of 2100
    p = rng.permutation(3000)
    add("ids_valid_neg_inf_m1024", "full+ids", 1024, s[p], perm_ids(3000)[p])
    # exact segment lengths around the unroll, m = 10, the winners in the last three records
    for L in TOPK_LENGTHS:
        n_abs = L // 20
        s, r = _mix_absents(rng, rng.standard_normal(L - 3 - n_abs), perm_ids(L - 3 - n_abs, 1, 50), n_abs)
        add(f"len{L}_level1_m10", "level1", 10, np.concatenate([s, [100.0, 102.0, 101.0]]),
            np.concatenate([r, [7, 8, 9]]), n_abs=0)
        # every record tied, no absents: the three lowest ids last; up to 1024 records still fit level 1
        add(f"len{L}_tied_m10", "level1" if L <= TOPK_MAX else "full+ids", 10, np.full(L, -2.0),
            np.concatenate([perm_ids(L - 3, 1, 50), [2, 0, 1]]), n_abs=0)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases
