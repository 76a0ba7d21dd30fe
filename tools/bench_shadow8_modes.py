"""Shadow-8 mode 1 against mode 2 below mode 1's range: the synchronous search (hr_index_search, 64 queries, k = 10)
over a synthetic bf16 corpus with the shadow off for this size (mode 1: shards of <= 160k tiles keep the 16-bit rows)
and forced on (mode 2), alternating, wall time per call.  One JSON line per (rows, mode, repeat).
Usage: python tools/bench_shadow8_modes.py [rows ...]   (default 5000000 2500000)"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "youtu-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from hiprag import _native  # noqa: E402

DIM, B, K, STEPS, WARMUP, REPEATS = 1024, 64, 10, 200, 10, 3


def main():
    _native.load_library()
    sizes = [int(a) for a in sys.argv[1:]] or [5_000_000, 2_500_000]
    rng = np.random.default_rng(0)
    q = rng.standard_normal((B, DIM)).astype(np.float32)
    for n in sizes:
        idx = _native.NativeIndex(DIM, "bf16", "cosine")
        idx.add_synthetic(1, 0, n)
        ref = None
        for rep in range(REPEATS):
            for mode in (1, 2):
                idx.set_shadow8(mode)
                l0 = idx.shadow8_stats()["launches"]
                for _ in range(WARMUP):
                    s, r = idx.search(q, K)
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    s, r = idx.search(q, K)
                ms = (time.perf_counter() - t0) * 1e3 / STEPS
                if ref is None:
                    ref = (s.copy(), r.copy())
                same = bool(np.array_equal(s, ref[0]) and np.array_equal(r, ref[1]))
                print(json.dumps({"rows": n, "dim": DIM, "batch": B, "k": K, "mode": mode, "repeat": rep,
                                  "ms_per_search": round(ms, 4), "results_equal": same,
                                  "shadow8_filter_used": idx.shadow8_stats()["launches"] > l0,
                                  "guard_failures": idx.stats()["guard_failures"]}), flush=True)
        idx.close()


if __name__ == "__main__":
    main()
