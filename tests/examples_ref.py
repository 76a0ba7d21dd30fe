"""Reference for the search by example (include/hiprag.h): the built query as the header states it -- per
component ``acc = float64(q)`` (or 0.0), then per example in list order ``acc = acc + float64(w) * float64(x)`` (numpy
never fuses; the product of two fp32 values is exact in float64 anyway), one cast to fp32 -- then R.process_queries and
the C oracle's exact top-k over the allowed rows minus the query's own examples.  Scores out are the canonical fp64
scores cast to fp32, as hr_index_search casts them; slots after the last row hold -inf / -1."""
import numpy as np

import oracle
from oracle import ref_numpy as R


def default_weights(examples):
    """1 / m_b per example, computed in float64 and cast to fp32 (NativeIndex's default)."""
    return [[np.float32(np.float64(1.0) / np.float64(max(len(e), 1)))] * len(e) for e in examples]


def build_ref(stored, dtype, examples, weights=None, q=None):
    """stored: the rows as the index keeps them (R.process_rows).  Returns the B built queries, fp32."""
    if weights is None:
        weights = default_weights(examples)
    x = R.dequantize(stored, dtype)
    B, dim = len(examples), x.shape[1]
    out = np.zeros((B, dim), np.float32)
    for b in range(B):
        acc = np.zeros(dim, np.float64) if q is None else np.asarray(q[b], np.float32).astype(np.float64)
        for r, w in zip(examples[b], weights[b]):
            acc = acc + np.float64(np.float32(w)) * x[int(r)].astype(np.float64)
        with np.errstate(over="ignore"):
            out[b] = acc.astype(np.float32)
    return out


def examples_ref(stored, dtype, examples, k, weights=None, q=None, allowed=None, metric="cosine", keep=False):
    """allowed: bool per row (live and unmasked; None = every row).  Returns (scores f32 B x k, rows i64 B x k)."""
    built = R.process_queries(build_ref(stored, dtype, examples, weights, q), metric)
    B, n = len(examples), len(stored)
    out_s = np.full((B, k), -np.inf, np.float32)
    out_r = np.full((B, k), -1, np.int64)
    if n == 0:
        return out_s, out_r
    base = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    kk = min(k, n)
    for b in range(B):
        ok = base.copy()
        if not keep:
            ok[np.asarray(examples[b], np.int64)] = False
        s, r = oracle.c_search(stored, dtype, built[b:b + 1], kk, oracle.mask_from_bool(ok), nthreads=2, metric=metric)
        valid = r[0] >= 0
        out_s[b, :kk][valid] = s[0][valid].astype(np.float32)
        out_r[b, :kk][valid] = r[0][valid]
    return out_s, out_r


def assert_same(got, ref):
    """Rows equal; scores equal as fp32 bit patterns."""
    (gs, gr), (rs, rr) = got, ref
    np.testing.assert_array_equal(np.asarray(gr), rr)
    np.testing.assert_array_equal(np.asarray(gs, np.float32).view(np.uint32), rs.view(np.uint32))


def assert_same_bits(got, ref):
    np.testing.assert_array_equal(np.asarray(got, np.float32).view(np.uint32),
                                  np.asarray(ref, np.float32).view(np.uint32))
