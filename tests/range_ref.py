"""Reference for the range search (include/hiprag.h): the canonical fp64 scores of R.exact_scores, a row
a hit iff it is allowed and its score cast to fp32 is >= the fp32 threshold (a NaN score never is), the hits ordered by
(fp64 score desc, row asc), the first ``max_hits`` out with scores cast to fp32 and -inf / -1 after them, and the exact
count of the hits whatever ``max_hits`` is."""
import numpy as np

from oracle import ref_numpy as R


def thresholds(t, B):
    """One fp32 threshold per query from a scalar or a per-query sequence."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (B,)))


def range_ref(stored, dtype, q_processed, t, max_hits, allowed=None, metric="cosine", scores=None):
    """stored: the rows as the index keeps them (R.process_rows); q_processed: R.process_queries' output; t: scalar or
    one value per query; allowed: bool per row (live and unmasked), None = every row; scores: the fp64 score matrix
    when the caller computed it already (R.exact_scores: it is the expensive part and never changes).  Returns (scores
    f32 B x max_hits, rows i64 B x max_hits, counts i64 B)."""
    q = np.asarray(q_processed, np.float32)
    if q.ndim == 1:
        q = q[None]
    B, n = q.shape[0], len(stored)
    t = thresholds(t, B)
    out_s = np.full((B, max_hits), -np.inf, np.float32)
    out_r = np.full((B, max_hits), -1, np.int64)
    counts = np.zeros(B, np.int64)
    if n == 0:
        return out_s, out_r, counts
    s = R.exact_scores(stored, dtype, q, metric) if scores is None else scores
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    with np.errstate(over="ignore", invalid="ignore"):
        s32 = s.astype(np.float32)
    for b in range(B):
        rows = np.nonzero(ok & (s32[b] >= t[b]))[0].astype(np.int64)  # (NaN >= t is False)
        counts[b] = len(rows)
        order = np.lexsort((rows, -s[b, rows]))[:max_hits]
        out_s[b, : len(order)] = s32[b, rows[order]]
        out_r[b, : len(order)] = rows[order]
    return out_s, out_r, counts


def assert_same(got, ref):
    """Rows equal, scores equal as fp32 bit patterns, counts equal; a count-only answer is (None, None, counts)."""
    (gs, gr, gc), (rs, rr, rc) = got, ref
    np.testing.assert_array_equal(np.asarray(gc, np.int64), np.asarray(rc, np.int64))
    if gs is None or rs is None:
        assert gs is None and gr is None, "a count-only call returns no lists"
        return
    np.testing.assert_array_equal(np.asarray(gr), rr)
    np.testing.assert_array_equal(np.asarray(gs, np.float32).view(np.uint32),
                                  np.asarray(rs, np.float32).view(np.uint32))
