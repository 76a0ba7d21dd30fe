"""Reference for the collapsed search: the FULL exact ranking of every query (k = n, from the C oracle
or the numpy reference), de-duplicated by group at first occurrence.  Rows without a group (-1, or beyond the ids
given) are left out; slots after the last kept row hold -inf / -1; scores are the canonical fp64 ones cast to fp32,
as hr_index_search casts them."""
import numpy as np

import oracle
from oracle import ref_numpy as R


def dedup(scores, rows, groups, k):
    """First occurrence per group of one query's ranking (rows < 0: padding) -> (scores f32[k], rows i64[k])."""
    groups = np.asarray(groups, np.int64)
    out_s = np.full(k, -np.inf, np.float32)
    out_r = np.full(k, -1, np.int64)
    seen, m = set(), 0
    for s, r in zip(scores, rows):
        if m == k:
            break
        if r < 0:
            continue
        g = groups[r] if r < len(groups) else -1
        if g < 0 or g in seen:
            continue
        seen.add(int(g))
        out_s[m], out_r[m] = np.float32(s), r
        m += 1
    return out_s, out_r


def collapse_ref(stored, dtype, q, groups, k, allowed=None, metric="cosine", use_c=True):
    """stored: the rows as the index keeps them (R.process_rows); q: processed queries (R.process_queries);
    groups: int ids per row (shorter than the rows: the rest have none); allowed: bool per row (live and unmasked).
    Returns (scores f32 B x k, rows i64 B x k)."""
    q = np.asarray(q, np.float32)
    if q.ndim == 1:
        q = q[None]
    n = len(stored)
    B = q.shape[0]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    if n == 0:
        return out_s, out_r
    if use_c:
        mask = None if allowed is None else oracle.mask_from_bool(np.asarray(allowed, bool))
        s, r = oracle.c_search(stored, dtype, q, n, mask, nthreads=2, metric=metric)
    else:
        s, r = R.search(stored, dtype, q, n, None if allowed is None else np.asarray(allowed, bool), metric=metric)
    for b in range(B):
        out_s[b], out_r[b] = dedup(s[b], r[b], groups, k)
    return out_s, out_r


def assert_same(got, ref):
    """Rows equal; scores equal as fp32 bit patterns."""
    (gs, gr), (rs, rr) = got, ref
    np.testing.assert_array_equal(np.asarray(gr), rr)
    np.testing.assert_array_equal(np.asarray(gs, np.float32).view(np.uint32), rs.view(np.uint32))
