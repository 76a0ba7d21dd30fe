"""Boosted search on one GPU (hr_index_search_boosted): what a batch costs beside the plain search of the
same queries, split into its parts, and how many queries the window cannot hold.

The corpus is bench.py's: synthetic rows (hr_index_add_synthetic), stored bf16 under cosine; the queries are planted
(unit(row) + 0.05 * unit noise), B = 64, k = 10, one fresh batch per step; one boost column of U[0, 1) values.  Device
entry points, a host clock around a synchronise; the calls of one shape alternate batch by batch in one process, so
they see the same clocks and the same queries.  Per boost weight (alpha = 1):
  boosted   hr_index_search_boosted_device, defaults (probe 40, window 4096)
  search    the plain search of the batch for k = 10 (what the parent commit offers)
  pilot     the plain search for the 40 rows of the pilot pool
  window    search_range at the call's floors with max_hits = 4096.  The floors are recomputed on the host from the
            pilot pool's fp32 scores (tests/boost_ref.py's bisection), so they can sit one fp32 step beside the
            library's, which blends the fp64 scores
  tail      boosted - pilot - window: the rescoring, the floor kernel, the LDS sort -- and, for a query whose count
            exceeds the window, its all-rows pass (one fp64 corpus pass per query), reported as ms per stage-2 query
            from the boost_stats delta
A shape whose queries all take stage 2 runs 1 warm-up and 2 timed batches (each query is a corpus pass of its own).
Usage: python tools/bench_boost.py [--rows 10000000] [--dim 1024] [--out profiles/boost_X.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import boost_ref as BR  # noqa: E402
from hiprag import _native, synth  # noqa: E402

B, K, P, WINDOW = 64, 10, 40, 4096
WEIGHTS = [0.02, 0.1, 0.5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    idx = _native.NativeIndex(a.dim, "bf16", "cosine")
    t0 = time.time()
    idx.add_synthetic(a.seed, 0, a.rows)
    col = np.random.default_rng(a.seed).random(a.rows).astype(np.float32)
    idx.set_boost(0, 0, col)
    torch.cuda.synchronize()
    print(f"{a.rows} x {a.dim} bf16 rows and one boost column built in {time.time() - t0:.1f}s", flush=True)
    nb = a.warmup + a.steps
    q = torch.from_numpy(np.stack([synth.planted_queries(a.seed, a.rows, a.dim, B, qseed=1000 + i)[0]
                                   for i in range(nb)])).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    bext = [float(col.max())]
    # the pilot pools of every batch, for the host-side floors
    sp = torch.empty((B, P), dtype=torch.float32, device=dev)
    rp = torch.empty((B, P), dtype=torch.int64, device=dev)
    pools = []
    for i in range(nb):
        idx.search_device(q[i].data_ptr(), B, P, sp.data_ptr(), rp.data_ptr(), stream=st)
        pools.append((sp.cpu().numpy().astype(np.float64), rp.cpu().numpy()))

    def floors(beta):
        t = np.zeros((nb, B), np.float32)
        for i, (s, r) in enumerate(pools):
            v = np.sort(BR.blend(1.0, s, [beta], [col[r]]), axis=1)[:, ::-1]
            t[i] = [BR.floor_of(1.0, [beta], bext, tau) for tau in v[:, K - 1]]
        return torch.from_numpy(t).to(dev)

    def plain(k):
        s = torch.empty((B, k), dtype=torch.float32, device=dev)
        r = torch.empty((B, k), dtype=torch.int64, device=dev)
        return lambda i: idx.search_device(q[i].data_ptr(), B, k, s.data_ptr(), r.data_ptr(), stream=st)

    counts = torch.zeros((B,), dtype=torch.int64, device=dev)

    def ranged(t):
        s = torch.empty((B, WINDOW), dtype=torch.float32, device=dev)
        r = torch.empty((B, WINDOW), dtype=torch.int64, device=dev)
        return lambda i: idx.search_range_device(q[i].data_ptr(), B, t[i].data_ptr(), WINDOW, s.data_ptr(),
                                                 r.data_ptr(), counts.data_ptr(), stream=st)

    def boosted(beta):
        v = torch.empty((B, K), dtype=torch.float64, device=dev)
        s = torch.empty((B, K), dtype=torch.float32, device=dev)
        r = torch.empty((B, K), dtype=torch.int64, device=dev)
        return lambda i: idx.search_boosted_device(q[i].data_ptr(), B, K, 1.0, [beta], v.data_ptr(), s.data_ptr(),
                                                   r.data_ptr(), stream=st)

    def alternate(fns, warmup, steps):
        ms = [[] for _ in fns]
        for i in range(warmup + steps):
            for j, fn in enumerate(fns):
                torch.cuda.synchronize()
                t_0 = time.perf_counter()
                fn(i)
                torch.cuda.synchronize()
                if i >= warmup:
                    ms[j].append((time.perf_counter() - t_0) * 1e3)
        return [{"median_ms": float(np.median(m)), "min_ms": float(np.min(m))} for m in ms]

    out = {"rows": a.rows, "dim": a.dim, "dtype": "bf16", "metric": "cosine", "B": B, "k": K, "probe": P,
           "window": WINDOW, "column": "U[0,1)", "alpha": 1.0, "weights": {}}
    for beta in WEIGHTS:
        t = floors(beta)
        # one untimed call tells which stage this weight's queries take
        s0 = idx.boost_stats()
        boosted(beta)(0)
        s1 = idx.boost_stats()
        all2 = s1["all_rows"] - s0["all_rows"] == B
        warmup, steps = (1, 2) if all2 else (a.warmup, a.steps)
        s0 = idx.boost_stats()
        res = alternate([boosted(beta), plain(K), plain(P), ranged(t)], warmup, steps)
        s1 = idx.boost_stats()
        e = dict(zip(["boosted", "search_k10", "pilot_search_k40", "range_at_the_floors"], res))
        calls = warmup + steps
        e["warmup"], e["steps"] = warmup, steps
        e["stage2_share"] = (s1["all_rows"] - s0["all_rows"]) / (calls * B)
        e["mean_window_count_last_batch"] = float(counts.double().mean().item())
        tail = e["boosted"]["median_ms"] - e["pilot_search_k40"]["median_ms"] - e["range_at_the_floors"]["median_ms"]
        e["tail_ms"] = tail
        n2 = e["stage2_share"] * B
        e["tail_ms_per_stage2_query"] = tail / n2 if n2 else None
        out["weights"][str(beta)] = e
        print(beta, json.dumps(e), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    idx.close()


if __name__ == "__main__":
    main()
