"""Reference for the fused multi-query search (include/hiprag.h), in plain Python float arithmetic.

Input: Q ranked lists of P slots (rows int64, -1 = padding; scores fp32), the rows of one list distinct; group g owns
``groups[g]`` consecutive lists, its members.  Per group, over the distinct rows that appear in any member:

  rrf    ``fused(r)`` starts at 0.0; then, for the members i in member order that hold r, at 1-based position p_i,
         ``fused = fused + float(w_i) / (rrf_k + float(p_i))`` -- Python floats are IEEE doubles, one division and one
         addition per term, each rounded once, nothing reassociated.  w_i = fp32 ``weights[i]``, 1.0 without weights.
  max    ``fused(r)`` = the largest fp32 score among the members holding r, widened; NaN counts as -inf.
  order  fused descending, then row ascending; the first min(k, distinct rows) are kept, the remaining slots hold
         -inf / -1 / 0.
  members  bit j: member j of the group holds the row.

``search_fused_ref`` takes the pools from the C oracle's exact top-``fetch_k`` of every member (scores cast to fp32 as
hr_index_search casts them), never from the library's own search."""
import math

import numpy as np

import oracle
from oracle import ref_numpy as R

MAX_K, MAX_MEMBERS = 128, 16


def default_fetch(k, mode):
    return k if mode == "max" else min(MAX_K, max(4 * k, 50))


def check_args(groups, k, P, mode, rrf_k, weights):
    """Every refusal of hr_fuse_lists, as ValueError."""
    groups = [int(m) for m in groups]
    if mode not in ("rrf", "max"):
        raise ValueError("mode must be 'rrf' or 'max'")
    if not groups:
        raise ValueError("at least one group")
    if any(m < 1 or m > MAX_MEMBERS for m in groups):
        raise ValueError("a group takes 1 to 16 members")
    if not 1 <= P <= MAX_K or not 1 <= k <= P:
        raise ValueError("need 1 <= k <= P <= 128")
    if not (math.isfinite(rrf_k) and rrf_k >= 0):
        raise ValueError("rrf_k must be finite and not negative")
    if weights is not None:
        if mode == "max":
            raise ValueError("max fusion takes no weights")
        if len(weights) != sum(groups):
            raise ValueError("one weight per list")
        if not all(math.isfinite(float(np.float32(w))) for w in weights):
            raise ValueError("weights must be finite")
    return groups


def fuse_ref(rows, scores, groups, k, mode="rrf", rrf_k=60.0, weights=None):
    """rows (Q, P) int64, scores (Q, P) fp32.  Returns (fused f64 (G, k), rows i64 (G, k), members u32 (G, k))."""
    rows = np.asarray(rows, np.int64)
    scores = np.asarray(scores, np.float32)
    groups = check_args(groups, k, rows.shape[1], mode, rrf_k, weights)
    G, P = len(groups), rows.shape[1]
    out_f = np.full((G, k), -np.inf, np.float64)
    out_r = np.full((G, k), -1, np.int64)
    out_m = np.zeros((G, k), np.uint32)
    q0 = 0
    for g, m in enumerate(groups):
        acc: dict = {}  # row -> [fused, member bits]
        for j in range(m):
            i = q0 + j
            w = 1.0 if weights is None else float(np.float32(weights[i]))
            for p in range(P):
                r = int(rows[i, p])
                if r < 0:
                    continue
                if mode == "rrf":
                    cur = acc.setdefault(r, [0.0, 0])
                    cur[0] = cur[0] + w / (float(rrf_k) + float(p + 1))
                else:
                    cur = acc.setdefault(r, [-math.inf, 0])
                    s = float(scores[i, p])
                    if s != s:
                        s = -math.inf
                    if s > cur[0]:
                        cur[0] = s
                cur[1] |= 1 << j
        ranked = sorted(acc.items(), key=lambda kv: (-kv[1][0], kv[0]))[:k]
        for t, (r, (f, bits)) in enumerate(ranked):
            out_f[g, t], out_r[g, t], out_m[g, t] = f, r, bits
        q0 += m
    return out_f, out_r, out_m


def pools_ref(stored, dtype, q, P, allowed=None, metric="cosine"):
    """The exact top-P of every query from the C oracle, scores cast to fp32, -inf / -1 past the allowed rows.
    allowed: None, one bool array for every query, or a list with one bool array (or None) per query."""
    q = R.process_queries(np.asarray(q, np.float32), metric)
    Q, n = len(q), len(stored)
    out_s = np.full((Q, P), -np.inf, np.float32)
    out_r = np.full((Q, P), -1, np.int64)
    if n == 0:
        return out_s, out_r
    kk = min(P, n)
    per_query = isinstance(allowed, (list, tuple))
    for i in range(Q):
        ok = allowed[i] if per_query else allowed
        mask = None if ok is None else oracle.mask_from_bool(np.asarray(ok, bool))
        s, r = oracle.c_search(stored, dtype, q[i:i + 1], kk, mask, nthreads=2, metric=metric)
        valid = r[0] >= 0
        out_s[i, :kk][valid] = s[0][valid].astype(np.float32)
        out_r[i, :kk][valid] = r[0][valid]
    return out_s, out_r


def search_fused_ref(stored, dtype, q, groups, k, fetch_k=0, mode="rrf", rrf_k=60.0, weights=None, allowed=None,
                     metric="cosine"):
    if not 1 <= k <= MAX_K or (fetch_k != 0 and not k <= fetch_k <= MAX_K):
        raise ValueError("need 1 <= k <= fetch_k <= 128")
    P = fetch_k or default_fetch(k, mode)
    check_args(groups, k, P, mode, rrf_k, weights)
    s, r = pools_ref(stored, dtype, q, P, allowed, metric)
    return fuse_ref(r, s, groups, k, mode, rrf_k, weights)


def assert_same(got, ref):
    """Rows and member bits equal; fused scores equal as fp64 bit patterns.  got may lack the member bits."""
    np.testing.assert_array_equal(np.asarray(got[1]), ref[1])
    np.testing.assert_array_equal(np.asarray(got[0], np.float64).view(np.uint64), ref[0].view(np.uint64))
    if len(got) > 2 and got[2] is not None:
        np.testing.assert_array_equal(np.asarray(got[2]), ref[2])
