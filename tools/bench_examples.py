"""Search by example on one GPU (hr_index_search_examples): what it costs beside the plain search it
contains.

The corpus is document-like: rows in runs of 40 (a document's chunks), row = unit(centre of its run + spread * unit
noise), stored bf16.  B = 64 queries, k = 10; query b's examples are the first m rows of a run (one document's chunks),
m in {1, 8}, weights 1 / m.  Per m, on the same handle in the same run: the wall time of search_examples_device (the
example lists to the device, the build kernel, the exact search for k + m rows, the drop kernel) and of search_device
at k + m on the SAME built queries (build_queries_device's output) -- the yardstick: the difference is what the feature
adds -- as medians over interleaved calls, build_queries_device alone, and the host's packing of the lists alone.
Every entry point returns with the stream idle, so wall time per call is the time of the call.
The measurement runs in a child process under a time limit (a hung GPU step ends the run instead of holding the
device); the parent never touches the GPU.
Usage: python tools/bench_examples.py [--rows 1000000] [--dim 768] [--limit 600] [--out profiles/examples_X.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO]

RUN, B, K = 40, 64, 10


def build(n, dim, spread, seed, dev):
    """The index; rows are generated and added 100k at a time."""
    import torch

    from hiprag import _native

    def unit(x):
        return x / x.norm(dim=-1, keepdim=True)

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    idx = _native.NativeIndex(dim, "bf16", "cosine")
    idx.reserve(n)
    step = 100_000 // RUN * RUN
    for lo in range(0, n, step):
        m = min(step, n - lo)
        centres = unit(torch.randn(((m + RUN - 1) // RUN, dim), generator=g, device=dev))
        x = unit(centres.repeat_interleave(RUN, 0)[:m] + spread * unit(torch.randn((m, dim), generator=g, device=dev)))
        idx.add_device(x.data_ptr(), m, torch.cuda.current_stream(dev).cuda_stream)
    return idx


def measure(idx, n, dim, m, reps, dev):
    import numpy as np
    import torch

    rng = np.random.default_rng(m)
    first = rng.choice(n // RUN, B, replace=False) * RUN
    ex = [list(range(int(f), int(f) + m)) for f in first]
    kp = K + m
    built = torch.empty((B, dim), dtype=torch.float32, device=dev)
    s = torch.empty((B, kp), dtype=torch.float32, device=dev)
    r = torch.empty((B, kp), dtype=torch.int64, device=dev)
    se = torch.empty((B, K), dtype=torch.float32, device=dev)
    re_ = torch.empty((B, K), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def examples():
        idx.search_examples_device(ex, K, se.data_ptr(), re_.data_ptr(), stream=st)

    def plain():
        idx.search_device(built.data_ptr(), B, kp, s.data_ptr(), r.data_ptr(), stream=st)

    def builder():
        idx.build_queries_device(ex, built.data_ptr(), stream=st)

    def pack():
        idx._example_lists(ex, None)  # the host's share of every call: the lists as three flat arrays

    for fn in (builder, examples, plain) * 3:  # warm-up: code objects, work buffers
        fn()
    torch.cuda.synchronize()
    t = {"examples": [], "plain": [], "build": [], "pack": []}
    for _ in range(reps):  # interleaved: clock and cache state drift alike for the three
        for name, fn in (("examples", examples), ("plain", plain), ("build", builder), ("pack", pack)):
            t0 = time.perf_counter()
            fn()  # (returns with the stream idle)
            t[name].append((time.perf_counter() - t0) * 1e3)
    examples()
    got = re_.cpu().numpy()
    hit = int(sum(np.isin(got[b], ex[b]).any() for b in range(B)))
    med = {name: statistics.median(v) for name, v in t.items()}
    return {"m": m, "k": K, "search_examples_device_ms": med["examples"], "plain_k": kp,
            "search_device_ms": med["plain"], "added_ms": med["examples"] - med["plain"],
            "build_queries_device_ms": med["build"], "list_pack_host_ms": med["pack"],
            "min_ms": {name: min(v) for name, v in t.items()}, "lists_holding_an_example": hit}


def child(a):
    import torch

    n, dev = int(a.rows), torch.device("cuda", 0)
    out = {"rows": n, "dim": a.dim, "dtype": "bf16", "run": RUN, "B": B, "k": K, "spread": a.spread, "reps": a.reps,
           "cases": []}
    t0 = time.perf_counter()
    idx = build(n, a.dim, a.spread, 0, dev)
    print(f"corpus {n} x {a.dim} bf16 in {time.perf_counter() - t0:.1f} s", flush=True)
    for m in (1, 8):
        c = measure(idx, n, a.dim, m, a.reps, dev)
        out["cases"].append(c)
        print(f"m = {m}: search_examples_device {c['search_examples_device_ms']:.3f} ms, search_device at k = "
              f"{c['plain_k']} {c['search_device_ms']:.3f} ms (added {c['added_ms']:.3f} ms), build alone "
              f"{c['build_queries_device_ms']:.3f} ms, of it packing the lists on the host "
              f"{c['list_pack_host_ms']:.3f} ms; {c['lists_holding_an_example']} lists hold an example", flush=True)
    idx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e6)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=600, help="seconds the measuring process may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
