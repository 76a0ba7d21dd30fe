"""MMR search on one GPU (hr_index_search_mmr): what the selection stage costs beside the probe.

The corpus is document-like: rows in runs of 40 (a document's chunks), row = unit(centre of its run + spread * unit
noise), stored bf16.  Queries are planted: unit(row) + 0.05 * unit noise, B = 64, k = 10, lambda = 0.5, fetch_k in
{32, 128}.  Per pool size: the library's own HIP-event times of the two stages -- the probe (a plain exact search for
fetch_k rows, the yardstick) and the selection kernel -- as the median over the timed calls, wall time per batch
through the device entry point with the timers off, queries/s from it, and how many of the 64 lists differ from the
plain top-k.
Usage: python tools/bench_mmr.py [--rows 1000000] [--dim 768] [--spread 2.0] [--out profiles/mmr_X.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO]
import torch  # noqa: E402

from hiprag import _native  # noqa: E402

RUN, B, K, LAM = 40, 64, 10, 0.5


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


def run_mmr(idx, q, fetch_k, reps):
    dev = q.device
    s = torch.empty((B, K), dtype=torch.float32, device=dev)
    r = torch.empty((B, K), dtype=torch.int64, device=dev)
    r0 = torch.empty((B, K), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def go():
        idx.search_mmr_device(q.data_ptr(), B, K, LAM, s.data_ptr(), r.data_ptr(), fetch_k=fetch_k, stream=st)

    for _ in range(3):  # warm-up: code objects, work buffers
        go()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        go()  # (returns with the stream idle)
    wall = (time.perf_counter() - t0) / reps * 1e3
    idx.set_mmr_timing(True)
    ev = []
    for _ in range(reps):
        go()
        ev.append(idx.mmr_last_ms())
    idx.set_mmr_timing(False)
    idx.search_device(q.data_ptr(), B, K, s.data_ptr(), r0.data_ptr(), stream=st)
    probe = statistics.median(e["probe_ms"] for e in ev)
    select = statistics.median(e["select_ms"] for e in ev)
    return {"fetch_k": fetch_k, "probe_ms": probe, "select_ms": select, "select_over_probe": select / probe,
            "select_ms_min_max": [min(e["select_ms"] for e in ev), max(e["select_ms"] for e in ev)],
            "wall_ms_per_batch": wall, "queries_per_s": B / wall * 1e3,
            "lists_changed": int((r != r0).any(dim=1).sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e6)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, dev = int(a.rows), torch.device("cuda", 0)
    out = {"rows": n, "dim": a.dim, "dtype": "bf16", "run": RUN, "B": B, "k": K, "lambda": LAM, "spread": a.spread,
           "reps": a.reps, "pools": []}
    t0 = time.perf_counter()
    idx, q = build(n, a.dim, a.spread, 0, dev)
    print(f"corpus {n} x {a.dim} bf16 in {time.perf_counter() - t0:.1f} s", flush=True)
    for P in (32, 128):
        c = run_mmr(idx, q, P, a.reps)
        out["pools"].append(c)
        print(f"fetch_k {P:3d}: probe {c['probe_ms']:.3f} ms, selection {c['select_ms']:.3f} ms "
              f"({c['select_over_probe']:.2f} x the probe), {c['wall_ms_per_batch']:.3f} ms/batch, "
              f"{c['queries_per_s']:.0f} queries/s, {c['lists_changed']}/{B} lists changed", flush=True)
    idx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
