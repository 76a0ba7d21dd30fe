"""Fused multi-query search on one GPU (hr_index_search_fused): what the fusion costs beside the scan
it follows, and what the host route costs instead.

The corpus is document-like: rows in runs of 40 (a document's chunks), row = unit(centre of its run + spread * unit
noise), stored bf16.  16 groups of 4 members (64 queries: one scan), every member a noisy copy of one row of its
group's document, k = 10, fetch_k = 50, both modes.  Per mode, on the same handle in the same run, medians over
interleaved calls of
  fused   search_fused_device: the 64 members searched for 50 rows, the pools fused on the device, 16 x 10 records out
  plain   search_device of the same 64 queries at k = 50: the floor -- the same scan is in both
  host    the host route: NativeIndex.search of the 64 host queries at k = 50 (64 x 50 records copied out), then the
          Python fusion (storage.fuse_lists_host).  The store's per-hit chunk lookups (64 x 50 of them on the host
          route, 16 x 10 on the fused one) are NOT included: the 10M-row corpus has no chunk table here
and of fuse_lists alone on the pools where search_device left them.  Every entry point returns with the stream idle,
so wall time per call is the time of the call.
The measurement runs in a child process under a time limit (a hung GPU step ends the run instead of holding the
device); the parent never touches the GPU.
Usage: python tools/bench_fused.py [--rows 1e7] [--dim 1024] [--limit 900] [--out profiles/fused_X.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO]

RUN, G, M, K, FETCH = 40, 16, 4, 10, 50


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


def measure(idx, n, dim, mode, reps, noise, dev):
    import numpy as np
    import torch

    from hiprag.rag.storage import fuse_lists_host

    rng = np.random.default_rng(7)
    anchors = rng.choice(n // RUN, G, replace=False) * RUN + rng.integers(0, RUN, G)  # one row per group
    base = np.repeat(idx.get_rows(anchors.tolist()), M, axis=0)
    eps = rng.standard_normal((G * M, dim)).astype(np.float32)
    q = (base + noise * eps / np.linalg.norm(eps, axis=1, keepdims=True)).astype(np.float32)
    groups = [M] * G
    qd = torch.from_numpy(q).to(dev)
    ps = torch.empty((G * M, FETCH), dtype=torch.float32, device=dev)
    pr = torch.empty((G * M, FETCH), dtype=torch.int64, device=dev)
    f = torch.empty((G, K), dtype=torch.float64, device=dev)
    r = torch.empty((G, K), dtype=torch.int64, device=dev)
    mb = torch.empty((G, K), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    host_out = {}

    def fused():
        idx.search_fused_device(qd.data_ptr(), groups, K, f.data_ptr(), r.data_ptr(), mb.data_ptr(), FETCH, mode,
                                stream=st)

    def plain():
        idx.search_device(qd.data_ptr(), G * M, FETCH, ps.data_ptr(), pr.data_ptr(), stream=st)

    def host():
        s_h, r_h = idx.search(q, FETCH)
        host_out["res"] = fuse_lists_host(s_h, r_h, groups, K, mode)

    def fuse_only():
        idx.fuse_lists(pr.data_ptr(), ps.data_ptr(), FETCH, groups, K, f.data_ptr(), r.data_ptr(), mb.data_ptr(), mode,
                       stream=st)

    for fn in (plain, fused, host, fuse_only) * 3:  # warm-up: code objects, work buffers, the graph of the host search
        fn()
    torch.cuda.synchronize()
    t = {"fused": [], "plain": [], "host": [], "fuse_only": []}
    for _ in range(reps):  # interleaved: clock and cache state drift alike for all
        for name, fn in (("fused", fused), ("plain", plain), ("host", host), ("fuse_only", fuse_only)):
            t0 = time.perf_counter()
            fn()  # (returns with the stream idle)
            t[name].append((time.perf_counter() - t0) * 1e3)
    fused()
    same = bool(np.array_equal(r.cpu().numpy(), host_out["res"][1]) and
                np.array_equal(f.cpu().numpy().view(np.uint64), host_out["res"][0].view(np.uint64)))
    held = mb.cpu().numpy().view(np.uint32)
    med = {name: statistics.median(v) for name, v in t.items()}
    return {"mode": mode, "groups": G, "members": M, "k": K, "fetch_k": FETCH,
            "search_fused_device_ms": med["fused"], "search_device_k50_ms": med["plain"],
            "host_route_ms": med["host"], "fuse_lists_alone_ms": med["fuse_only"],
            "fused_minus_plain_ms": med["fused"] - med["plain"], "host_minus_fused_ms": med["host"] - med["fused"],
            "min_ms": {name: min(v) for name, v in t.items()}, "fused_equals_host_route": same,
            "mean_members_per_hit": float(np.mean([bin(int(b)).count("1") for b in held.reshape(-1)]))}


def child(a):
    import torch

    n, dev = int(a.rows), torch.device("cuda", 0)
    out = {"rows": n, "dim": a.dim, "dtype": "bf16", "run": RUN, "spread": a.spread, "noise": a.noise, "reps": a.reps,
           "host_route": "NativeIndex.search (host queries in, 64 x 50 records out) + storage.fuse_lists_host; "
                         "no chunk lookups on either side", "cases": []}
    t0 = time.perf_counter()
    idx = build(n, a.dim, a.spread, 0, dev)
    print(f"corpus {n} x {a.dim} bf16 in {time.perf_counter() - t0:.1f} s", flush=True)
    for mode in ("rrf", "max"):
        c = measure(idx, n, a.dim, mode, a.reps, a.noise, dev)
        out["cases"].append(c)
        print(f"{mode}: search_fused_device {c['search_fused_device_ms']:.3f} ms, search_device at k = {FETCH} "
              f"{c['search_device_k50_ms']:.3f} ms (fusion adds {c['fused_minus_plain_ms']:.3f} ms; fuse_lists alone "
              f"{c['fuse_lists_alone_ms']:.3f} ms), host route {c['host_route_ms']:.3f} ms "
              f"({c['host_minus_fused_ms']:.3f} ms more); same answer: {c['fused_equals_host_route']}; "
              f"{c['mean_members_per_hit']:.2f} members per hit", flush=True)
    idx.close()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--noise", type=float, default=0.5, help="norm of the noise a member adds to its group's row")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring process may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
