"""Reference for the boosted search (include/hiprag.h), in numpy fp64.

The answer: the canonical scores of R.exact_scores, the blend v = (...((alpha * s) + beta[0] * b_0) + beta[1] * b_1 ...)
with one rounding per product and per sum in column order (numpy evaluates every operation on its own: nothing is
fused), a row with a NaN v dropped, the rest ordered by (v desc, row asc), the first k out as (v f64, (float)s f32,
row i64) with -inf / -inf / -1 after them; -0.0 is written as 0.0, as the library's order-preserving keys do.

The mechanism (``mechanism``), also from the contract alone: the pilot pool (exact top-P by (s desc, row asc)), tau =
the k-th largest v of the pool (-inf below k rows), bext over ALL rows of every column, the bisection over the ordered
fp32 bit patterns for t0 = the smallest fp32 with Vmax(t0) >= tau, t = nextafter(t0, -inf), and the exact count of the
allowed rows with (float)s >= t: a query is answered by stage 1 iff that count is <= window."""
import numpy as np

from oracle import ref_numpy as R

DEFAULT_WINDOW = 4096
MAX_K = 128


def default_probe(k):
    return min(MAX_K, max(32, 4 * k))


def columns(cols, n):
    """The columns as the index reads them: float32, n entries each, 0.0 where nothing was set."""
    out = []
    for c in cols:
        a = np.zeros(n, np.float32)
        c = np.asarray(c, np.float32).reshape(-1)[:n]
        a[: len(c)] = c
        out.append(a)
    return out


def blend(alpha, s, betas, cols):
    """v of fp64 scores ``s`` (any shape) against per-row column values ``cols`` (broadcastable to it)."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float64(alpha) * np.asarray(s, np.float64)
        for beta, b in zip(betas, cols):
            p = np.float64(beta) * np.asarray(b, np.float32).astype(np.float64)
            v = v + p
    return v


def boost_ref(stored, dtype, q_processed, k, alpha, betas, cols, allowed=None, metric="cosine", scores=None):
    """stored: R.process_rows' output; q_processed: R.process_queries' output; cols: one array per beta (shorter than n:
    the rest reads 0.0); allowed: bool per row (live and unmasked); scores: R.exact_scores when already computed.
    Returns (blended f64 B x k, scores f32 B x k, rows i64 B x k)."""
    q = np.asarray(q_processed, np.float32)
    if q.ndim == 1:
        q = q[None]
    B, n = q.shape[0], len(stored)
    out_v = np.full((B, k), -np.inf, np.float64)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    if n == 0:
        return out_v, out_s, out_r
    s = R.exact_scores(stored, dtype, q, metric) if scores is None else scores
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    cs = columns(cols, n)
    assert len(cs) == len(betas)
    with np.errstate(over="ignore", invalid="ignore"):
        s32 = s.astype(np.float32)
    s32 = np.where(s32 == 0, np.float32(0.0), s32)
    for b in range(B):
        v = blend(alpha, s[b], betas, cs)
        v = np.where(v == 0, 0.0, v)
        rows = np.nonzero(ok & ~np.isnan(v))[0].astype(np.int64)
        order = np.lexsort((rows, -v[rows]))[:k]
        out_v[b, : len(order)] = v[rows[order]]
        out_s[b, : len(order)] = s32[b, rows[order]]
        out_r[b, : len(order)] = rows[order]
    return out_v, out_s, out_r


# ---------------------------------------------------------------- the mechanism
def f2key(f):
    f = np.float32(f)
    u = int(np.float32(0.0 if f == 0 else f).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def key2f(key):
    u = (key & 0x7FFFFFFF) if key & 0x80000000 else (~key & 0xFFFFFFFF)
    return np.uint32(u).view(np.float32)


def vmax(alpha, betas, bext, x):
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float64(alpha) * np.float64(x)
        for beta, e in zip(betas, bext):
            v = v + np.float64(beta) * np.float64(e)
    return v


def floor_of(alpha, betas, bext, tau):
    """t = nextafter(t0, -inf), t0 the smallest fp32 with Vmax(t0) >= tau (bisection over the ordered bit patterns)."""
    lo, hi = f2key(-np.inf), f2key(np.inf)
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if vmax(alpha, betas, bext, key2f(mid)) >= tau:
            hi = mid
        else:
            lo = mid + 1
    return np.nextafter(key2f(lo), np.float32(-np.inf))


def mechanism(stored, dtype, q_processed, k, alpha, betas, cols, allowed=None, metric="cosine", probe=0, window=0,
              scores=None):
    """Per query: tau, the floor t, the exact window count and the answering stage (1 or 2).  Corpora without NaN
    scores.  Returns a dict of arrays."""
    q = np.asarray(q_processed, np.float32)
    if q.ndim == 1:
        q = q[None]
    B, n = q.shape[0], len(stored)
    P = probe or default_probe(k)
    W = window or max(k, DEFAULT_WINDOW)
    s = R.exact_scores(stored, dtype, q, metric) if scores is None else scores
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    cs = columns(cols, n)
    bext = [float(c.max()) if beta >= 0 else float(c.min()) for beta, c in zip(betas, cs)]  # all rows, dead included
    s32 = s.astype(np.float32)
    tau = np.full(B, -np.inf)
    t = np.full(B, -np.inf, np.float32)
    count = np.zeros(B, np.int64)
    rows = np.nonzero(ok)[0]
    for b in range(B):
        pool = rows[np.lexsort((rows, -s[b, rows]))[:P]]
        v = blend(alpha, s[b, pool], betas, [c[pool] for c in cs])
        v = np.sort(v[~np.isnan(v)])[::-1]
        if len(v) >= k:
            tau[b] = v[k - 1]
        t[b] = floor_of(alpha, betas, bext, tau[b])
        count[b] = int((ok & (s32[b] >= t[b])).sum())
    return {"tau": tau, "t": t, "count": count, "stage": np.where(count <= W, 1, 2), "window": W}


def assert_same(got, ref):
    """Rows equal, blended equal as fp64 bit patterns, scores equal as fp32 bit patterns."""
    (gv, gs, gr), (rv, rs, rr) = got, ref
    np.testing.assert_array_equal(np.asarray(gr), rr)
    np.testing.assert_array_equal(np.asarray(gv, np.float64).view(np.uint64), np.asarray(rv, np.float64).view(np.uint64))
    np.testing.assert_array_equal(np.asarray(gs, np.float32).view(np.uint32),
                                  np.asarray(rs, np.float32).view(np.uint32))
