"""Collapsed search on one GPU (hr_index_search_collapsed): what the probe stage costs over a plain
search of the same depth, how often the all-rows stage runs at each probe size, and what it costs per query.

The corpus is document-like: rows in runs of 40 (a document's chunks), row = unit(centre of its run + spread * unit
noise), stored bf16; a run is one group.  Queries are planted: unit(row) + 0.05 * unit noise, B = 64, k = 10.
  1. singleton groups (every query completes in the probe): collapsed search at probe P beside the plain
     search(k = P) -- device entry points, wall time per batch and the library's own HIP-event times
     (probe search / prefix kernel);
  2. runs of 40 as groups: probe in {k, 2k, 4k, 8k, 128}, time per batch and the share of queries that reach the
     all-rows stage;
  3. a tight corpus (spread 0.3: a query's top rows are all its own document) at probe = k: every query takes the
     all-rows stage; its HIP-event time per query.
Usage: python tools/bench_collapse.py [--rows 1000000] [--dim 768] [--spread 2.0] [--out profiles/collapse_X.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hiprag import _native  # noqa: E402

RUN, B, K = 40, 64, 10


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def build(n, dim, spread, seed, dev):
    """The index and B planted queries (device tensors); rows are generated and added 100k at a time."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    idx = _native.NativeIndex(dim, "bf16", "cosine")
    idx.reserve(n)
    pick = torch.randint(0, n, (B,), generator=g, device=dev)
    q = torch.empty((B, dim), dtype=torch.float32, device=dev)
    step = 100_000 // RUN * RUN
    for lo in range(0, n, step):
        m = min(step, n - lo)
        centres = unit(torch.randn(((m + RUN - 1) // RUN, dim), generator=g, device=dev))
        x = unit(centres.repeat_interleave(RUN, 0)[:m] + spread * unit(torch.randn((m, dim), generator=g, device=dev)))
        idx.add_device(x.data_ptr(), m, torch.cuda.current_stream(dev).cuda_stream)
        here = (pick >= lo) & (pick < lo + m)
        q[here] = x[pick[here] - lo]
    q = (q + 0.05 * unit(torch.randn((B, dim), generator=g, device=dev))).contiguous()
    return idx, q


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run_collapsed(idx, q, k, probe, reps):
    """ms per batch (wall), the library's stage times of the last call, and the all-rows share."""
    dev = q.device
    s = torch.empty((B, k), dtype=torch.float32, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def go():
        idx.search_collapsed_device(q.data_ptr(), B, k, s.data_ptr(), r.data_ptr(), probe=probe, stream=st)

    go()
    before = idx.collapse_stats()
    idx.set_collapse_timing(False)
    ms = timed(go, reps)
    after = idx.collapse_stats()
    idx.set_collapse_timing(True)
    go()
    idx.set_collapse_timing(False)
    done = (after["probe"] - before["probe"]) + (after["all_rows"] - before["all_rows"])
    share = (after["all_rows"] - before["all_rows"]) / max(1, done)
    return {"probe": probe, "ms_per_batch": ms, "all_rows_share": share,
            "events_ms": idx.collapse_last_ms(), "distinct": int((r >= 0).sum().item()) / B}


def run_plain(idx, q, k, reps):
    dev = q.device
    s = torch.empty((B, k), dtype=torch.float32, device=dev)
    r = torch.empty((B, k), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    return timed(lambda: idx.search_device(q.data_ptr(), B, k, s.data_ptr(), r.data_ptr(), stream=st), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e6)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, dev = int(a.rows), torch.device("cuda", 0)
    out = {"rows": n, "dim": a.dim, "dtype": "bf16", "run": RUN, "B": B, "k": K, "spread": a.spread}
    t0 = time.perf_counter()
    idx, q = build(n, a.dim, a.spread, 0, dev)
    print(f"corpus {n} x {a.dim} bf16 in {time.perf_counter() - t0:.1f} s", flush=True)
    probes = [K, 2 * K, 4 * K, 8 * K, 128]

    # 1. the probe stage against the plain search of the same depth
    idx.set_groups(0, np.arange(n, dtype=np.int32))
    out["stage1"] = []
    for P in probes:
        plain = run_plain(idx, q, P, a.reps)
        c = run_collapsed(idx, q, K, P, a.reps)
        assert c["all_rows_share"] == 0.0
        c["plain_search_ms_per_batch"] = plain
        out["stage1"].append(c)
        ev = c["events_ms"]
        print(f"[1] probe {P:3d}: plain search(k={P}) {plain:7.3f} ms/batch, collapsed {c['ms_per_batch']:7.3f} "
              f"ms/batch (events: search {ev['probe_ms']:.3f}, prefix {ev['prefix_ms']:.4f})", flush=True)

    # 2. the probe sweep over documents of 40 chunks
    idx.set_groups(0, (np.arange(n) // RUN).astype(np.int32))
    out["sweep"] = []
    for P in probes:
        c = run_collapsed(idx, q, K, P, a.reps)
        out["sweep"].append(c)
        print(f"[2] probe {P:3d}: {c['ms_per_batch']:8.3f} ms/batch, all-rows share {c['all_rows_share']:.3f}, "
              f"events {c['events_ms']}", flush=True)
    idx.close()
    del idx

    # 3. every query through the all-rows stage
    idx, q = build(n, a.dim, 0.3, 1, dev)
    idx.set_groups(0, (np.arange(n) // RUN).astype(np.int32))
    c = run_collapsed(idx, q, K, K, max(2, a.reps // 3))
    assert c["all_rows_share"] == 1.0 and c["distinct"] == K
    c["all_rows_ms_per_query"] = c["events_ms"]["all_rows_ms"] / B
    out["stage2"] = c
    print(f"[3] all-rows stage: {c['all_rows_ms_per_query']:.3f} ms/query ({n // RUN} groups), "
          f"batch {c['ms_per_batch']:.2f} ms", flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
