"""Child process of tests/test_gpu_shadow8_pipelined.py (not a test module).

The spare-CU counts of the pipelined scans (HIPRAG_TAIL_CUS, HIPRAG_TAIL_CUS8) are read once when libhiprag.so loads,
so each setting runs here, in a fresh process that the parent test starts with the environment set.  argv[1] is the
.npz the parent wrote: the query batches and the oracle's answers.  Runs the cases in order, stops at the first failure
and prints one JSON line: {"ok": bool, "cases": [{"name", "ok", ...}], "env": {...}}.  Exit status 0 only if every case
passed."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "youtu-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

KNOBS = ("HIPRAG_TAIL_CUS", "HIPRAG_TAIL_CUS8")


def pipelined(native, torch, ShardedSearch, name, dim, segments, batches, k, s_ref, r_ref, max_k):
    """batches (nb, B, dim) submitted back to back through ShardedSearch(depth=2); s_ref / r_ref (nb, B, >= k)."""
    dev = torch.device("cuda", 0)
    idx = native.NativeIndex(dim, "bf16", "cosine", device=0)
    try:
        for seg in segments:
            if seg[0] == "syn":
                idx.add_synthetic(1, seg[1], seg[2])
            else:
                idx.add(seg[1])
        idx.set_shadow8(2)
        nb, B = batches.shape[:2]
        q_dev = torch.from_numpy(batches).to(dev)
        q_ready = torch.cuda.Event()
        q_ready.record()
        s_dev = torch.empty((nb, B, k), dtype=torch.float32, device=dev)
        r_dev = torch.empty((nb, B, k), dtype=torch.int64, device=dev)
        searcher = ShardedSearch(idx, 0, max_batch=B, device=dev, max_k=max_k, depth=2)
        f0 = idx.stats()["guard_failures"]
        l0 = idx.shadow8_stats()["launches"]
        fb0 = searcher.fallback_queries
        for i in range(nb):
            searcher.submit(q_dev[i], k, s_out=s_dev[i], r_out=r_dev[i], q_ready=q_ready)
        searcher.finalize_all()
        torch.cuda.synchronize()
        st = idx.shadow8_stats()
        out = {"name": name, "batches": int(nb), "launches": int(st["launches"] - l0), "kc8": int(st["kc8"]),
               "guard_failures": int(idx.stats()["guard_failures"] - f0),
               "fallback_queries": int(searcher.fallback_queries - fb0)}
        s, r = s_dev.cpu().numpy(), r_dev.cpu().numpy()
        searcher.close()
    finally:
        idx.close()
    rows = [bool(np.array_equal(r[i], r_ref[i][:, :k])) for i in range(nb)]
    bits = [bool(np.array_equal(s[i].view(np.uint32), s_ref[i][:, :k].astype(np.float32).view(np.uint32)))
            for i in range(nb)]
    out["rows_equal"], out["score_bits_equal"] = rows, bits
    out["ok"] = (all(rows) and all(bits) and out["launches"] == nb and out["guard_failures"] == 0
                 and out["fallback_queries"] == 0)
    return out


def main():
    import torch

    from hiprag import _native as native
    from hiprag.dist import ShardedSearch

    native.load_library()
    res = {"ok": False, "cases": [], "env": {k: os.environ.get(k) for k in KNOBS}}
    if native.device_count() < 1:
        res["error"] = "no HIP device visible"
        print(json.dumps(res))
        return 1
    ref = np.load(sys.argv[1])
    ok = True
    n64 = int(ref["n64"])
    for k in (10, 40):
        if ok:
            case = pipelined(native, torch, ShardedSearch, f"D64 1.2M rows, 6 x B64, k{k}", 64, [("syn", 0, n64)],
                             ref["q64"], k, ref["s64"], ref["r64"], 40)
            res["cases"].append(case)
            ok = case["ok"]
    if ok:
        a, b, n_syn = int(ref["dup_a_at"]), int(ref["dup_b_at"]), int(ref["n_syn"])
        segs = [("syn", 0, a), ("rows", ref["dup_a"]), ("syn", a, b - a), ("rows", ref["dup_b"]), ("syn", b, n_syn - b)]
        case = pipelined(native, torch, ShardedSearch, "D1024 300k rows, duplicates in parts 0 and 2, 6 x B64, k10", 1024,
                         segs, ref["q1024"], 10, ref["s1024"], ref["r1024"], 16)
        res["cases"].append(case)
        ok = case["ok"]
    res["ok"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
