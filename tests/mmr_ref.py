"""Reference for the MMR search (include/hiprag.h): the exact top-P pool from the C oracle (or the numpy
reference), the pool's similarities from R.exact_scores with the SELECTED row in the query role, and the greedy loop
in float64 exactly as the header states it -- ``lam * rel - (1 - lam) * maxsim`` as three roundings (numpy never fuses),
NaN mapped to -inf, first maximum.  Scores out are the pool's canonical fp64 scores cast to fp32, as hr_index_search
casts them; rows come in selection order; slots after the last pick hold -inf / -1."""
import numpy as np

import oracle
from oracle import ref_numpy as R


def default_fetch_k(k):
    return min(128, max(32, 4 * k))


def pool_sim(stored, dtype, pool_rows, metric):
    """sim[s, j] of the pool's rows (all >= 0): row index = the selected row s in the query role, column = j."""
    rows = stored[np.asarray(pool_rows, np.int64)]
    return R.exact_scores(rows, dtype, R.dequantize(rows, dtype), metric)


def greedy(rel, sim, k, lam):
    """Positions picked from a pool of len(rel) candidates: rel float64, sim[s, j] float64."""
    rel = np.asarray(rel, np.float64)
    P = len(rel)
    lam = np.float64(lam)
    om = np.float64(1.0) - lam  # computed once
    taken = np.zeros(P, bool)
    maxsim = np.full(P, -np.inf)
    picks = []
    for t in range(min(k, P)):
        if t == 0:
            pick = 0
        else:
            s = sim[picks[-1]]
            maxsim = np.where(s > maxsim, s, maxsim)
            with np.errstate(invalid="ignore", over="ignore"):
                v = lam * rel - om * maxsim
            v = np.where(np.isnan(v), -np.inf, v)
            cand = np.nonzero(~taken)[0]
            pick = int(cand[np.argmax(v[cand])])  # the first maximum: ties to the lowest position
        taken[pick] = True
        picks.append(pick)
    return picks


def mmr_ref(stored, dtype, q, k, lam, fetch_k=0, allowed=None, metric="cosine", use_c=True):
    """stored: the rows as the index keeps them (R.process_rows); q: processed queries (R.process_queries); allowed:
    bool per row (live and unmasked).  Returns (scores f32 B x k, rows i64 B x k)."""
    q = np.asarray(q, np.float32)
    if q.ndim == 1:
        q = q[None]
    P = fetch_k or default_fetch_k(k)
    assert 1 <= k <= P <= 128 and 0.0 <= lam <= 1.0
    B, n = q.shape[0], len(stored)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    if n == 0:
        return out_s, out_r
    P = min(P, n)  # (slots beyond the rows would be padding, and padding is no candidate)
    if use_c:
        mask = None if allowed is None else oracle.mask_from_bool(np.asarray(allowed, bool))
        s, r = oracle.c_search(stored, dtype, q, P, mask, nthreads=2, metric=metric)
    else:
        s, r = R.search(stored, dtype, q, P, None if allowed is None else np.asarray(allowed, bool), metric=metric)
    for b in range(B):
        valid = r[b] >= 0  # (a prefix: padding sits at the end of the pool)
        rows, rel32 = r[b][valid], np.asarray(s[b][valid], np.float64).astype(np.float32)
        if len(rows) == 0:
            continue
        picks = greedy(rel32.astype(np.float64), pool_sim(stored, dtype, rows, metric), k, lam)
        out_s[b, : len(picks)], out_r[b, : len(picks)] = rel32[picks], rows[picks]
    return out_s, out_r


def assert_same(got, ref):
    """Rows equal; scores equal as fp32 bit patterns."""
    (gs, gr), (rs, rr) = got, ref
    np.testing.assert_array_equal(np.asarray(gr), rr)
    np.testing.assert_array_equal(np.asarray(gs, np.float32).view(np.uint32), rs.view(np.uint32))
