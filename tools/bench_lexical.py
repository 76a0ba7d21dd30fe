#!/usr/bin/env python3
"""Keyword (BM25) search timing: the forward-index scan of hr_lex_search against its streaming bound.

Corpus: synthetic Zipf term ids, --rows rows of --tokens tokens each (about 80 distinct terms per row at the
defaults).  Batches of B = 1 and B = 64 queries of 4 Zipf-drawn terms, k = 10.  Times are HIP-event times inside the
library (hr_lex_last_ms: scan = k_lex_score + segment padding, select = the top-k), the median of --iters calls after
--warmup.  The bound is the bytes the scan must stream once per sub-batch -- entries (4 B) and row offsets (8 B) --
over the 8 TB/s HBM peak.  For context the pure-Python reference (tests/lex_ref.py) is timed on the first --ref-rows
rows.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "youtu-rag_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12  # bytes / s


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--qterms", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ref-rows", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    from hiprag import _native

    rng = np.random.default_rng(a.seed)
    p = 1.0 / np.arange(1, a.vocab + 1)
    cdf = np.cumsum(p / p.sum())
    vocab = rng.choice(1 << 22, a.vocab, replace=False).astype(np.uint32)

    def draw(n):
        return vocab[np.minimum(np.searchsorted(cdf, rng.random(n)), a.vocab - 1)]

    idx = _native.NativeLexIndex(a.device)
    t0 = time.perf_counter()
    chunk = 100_000
    ref_rows, n_entries = [], 0
    for r0 in range(0, a.rows, chunk):
        n = min(chunk, a.rows - r0)
        tok = draw(n * a.tokens)
        off = np.arange(n + 1, dtype=np.int64) * a.tokens
        idx.add((tok, off))
        srt = np.sort(tok.reshape(n, a.tokens), axis=1)
        n_entries += n + int((srt[:, 1:] != srt[:, :-1]).sum())  # distinct terms per row = the row's entries
        if r0 < a.ref_rows:
            m = min(n, a.ref_rows - r0)
            ref_rows += tok[: m * a.tokens].reshape(m, a.tokens).tolist()
    build_s = time.perf_counter() - t0
    n_rows, _ = idx.size()
    distinct = n_entries / max(n_rows, 1)
    stream_bytes = n_entries * 4 + (n_rows + 1) * 8
    bound_ms = stream_bytes / HBM_PEAK * 1e3
    out = {"rows": n_rows, "tokens_per_row": a.tokens, "distinct_terms_per_row": round(distinct, 1),
           "stream_bytes": int(stream_bytes), "bound_ms": round(bound_ms, 4), "build_s": round(build_s, 2),
           "k": a.k, "qterms": a.qterms, "batches": {}}
    for B in a.batches:
        queries = [draw(a.qterms).tolist() for _ in range(B)]
        scan, select, wall = [], [], []
        for it in range(a.warmup + a.iters):
            t0 = time.perf_counter()
            idx.search(queries, a.k)
            w = time.perf_counter() - t0
            s_ms, t_ms, n_sub = idx.last_ms()
            if it >= a.warmup:
                scan.append(s_ms)
                select.append(t_ms)
                wall.append(w * 1e3)
        scan_ms = statistics.median(scan)
        out["batches"][str(B)] = {
            "scan_ms": round(scan_ms, 4), "select_ms": round(statistics.median(select), 4),
            "wall_ms": round(statistics.median(wall), 4), "sub_batches": n_sub,
            "scan_fraction_of_bound": round(bound_ms * n_sub / scan_ms, 4) if scan_ms > 0 else None,
            "scan_GBps": round(stream_bytes * n_sub / scan_ms / 1e6, 1) if scan_ms > 0 else None}
    if a.ref_rows > 0 and ref_rows:
        import lex_ref

        ref = lex_ref.RefIndex()
        ref.add(ref_rows)
        q = [draw(a.qterms).tolist()]
        t0 = time.perf_counter()
        ref.search(q, a.k)
        dt = time.perf_counter() - t0
        out["lex_ref_host"] = {"rows": len(ref_rows), "ms_per_query": round(dt * 1e3, 2),
                               "ms_per_query_scaled_to_corpus": round(dt * 1e3 * n_rows / len(ref_rows), 1)}
    idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
