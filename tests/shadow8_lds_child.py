"""Child process of tests/test_gpu_shadow8_lds_refresh.py (not a test module).

The shadow-8 FILTER's refresh cadence and its shared-refresh switch (HIPRAG_REFRESH_EVERY8, HIPRAG_REFRESH_LDS) are
read once when libhiprag.so loads, so the cases run here, in a fresh process that the parent test starts with the
environment set.  Runs the cases in order, stops at the first failure and prints one JSON line:
{"ok": bool, "cases": [{"name", "ok", ...}], "env": {...}}.  Exit status 0 only if every case passed."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "youtu-rag_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402

N = 300_000  # 9,375 tiles over at most 2,048 waves: 4-5 tiles per wave, two or more refreshes each at a 2-tile cadence


def make_queries(rng, dim, B, noise):
    """As tests/test_gpu_shadow8_cadence.py: half near neighbours of corpus rows, half isotropic."""
    planted = np.concatenate([R.gen_rows(1, int(j), 1, dim) for j in rng.choice(N, B, replace=False)])
    q = planted + rng.standard_normal((B, dim)).astype(np.float32) * noise
    q[1::2] = rng.standard_normal((B // 2, dim))
    return q.astype(np.float32)


def check(native, name, dim, q, k, s_ref, r_ref, segments, kc8):
    """segments: list of ("syn", row0, n) / ("rows", fp32 array) in corpus order."""
    idx = native.NativeIndex(dim, "bf16", "cosine")
    try:
        for seg in segments:
            if seg[0] == "syn":
                idx.add_synthetic(1, seg[1], seg[2])
            else:
                idx.add(seg[1])
        idx.set_shadow8(2)
        f0 = idx.stats()["guard_failures"]
        s, r = idx.search(q, k)
        st = idx.shadow8_stats()
        f1 = idx.stats()["guard_failures"]
    finally:
        idx.close()
    out = {"name": name, "launches": int(st["launches"]), "kc8": int(st["kc8"]), "guard_failures": int(f1 - f0),
           "rows_equal": bool(np.array_equal(r, r_ref[:, :k])),
           "scores_equal": bool(np.array_equal(s, s_ref[:, :k].astype(np.float32)))}
    out["ok"] = (out["launches"] > 0 and (kc8 is None or out["kc8"] == kc8) and out["guard_failures"] == 0 and out["rows_equal"]
                 and out["scores_equal"])
    return out


def main():
    from hiprag import _native as native

    native.load_library()
    res = {"ok": False, "cases": [],
           "env": {k: os.environ.get(k) for k in ("HIPRAG_REFRESH_EVERY8", "HIPRAG_REFRESH_LDS")}}
    if native.device_count() < 1:
        res["error"] = "no HIP device visible"
        print(json.dumps(res))
        return 1

    def run(case):
        res["cases"].append(case)
        return case["ok"]

    ok = True
    # ---- D = 64: one corpus, one oracle answer (k = 40) for the three cases
    rng = np.random.default_rng(3)
    stored = oracle.c_build_synthetic(1, 0, N, 64, "bf16", "cosine")
    q64 = make_queries(rng, 64, 64, 20000)
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q64, "cosine"), 40)
    syn = [("syn", 0, N)]
    ok = ok and run(check(native, "D64 B64 k10 (np=4, QB=2)", 64, q64, 10, s_ref, r_ref, syn, 128))
    ok = ok and run(check(native, "D64 B64 k40 (np=5)", 64, q64, 40, s_ref, r_ref, syn, 160))
    ok = ok and run(check(native, "D64 B20 k10 (QB=1)", 64, q64[:20], 10, s_ref[:20], r_ref[:20], syn, 128))
    del stored
    # ---- D = 1280 at QB = 2: the query tile fills the LDS, the kernel keeps the per-wave refresh
    if ok:
        rng = np.random.default_rng(4)
        stored = oracle.c_build_synthetic(1, 0, N, 1280, "bf16", "cosine")
        q = make_queries(rng, 1280, 64, 20000)
        s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 10)
        ok = run(check(native, "D1280 B64 k10 (LDS full: fallback)", 1280, q, 10, s_ref, r_ref, syn, None))
        del stored
    # ---- D = 1024: two near-duplicates of every query, in row parts 0 and 2 of the four (75,008 rows each): the
    # thresholds that keep the rest of the corpus out come from group maxima other waves published
    if ok:
        rng = np.random.default_rng(5)
        B, dim, a, b = 64, 1024, 40_000, 200_000
        q = make_queries(rng, dim, B, 20000)
        sd = q.std(axis=1, keepdims=True)
        dup_a = (q + rng.standard_normal(q.shape).astype(np.float32) * 0.05 * sd).astype(np.float32)
        dup_b = (q + rng.standard_normal(q.shape).astype(np.float32) * 0.07 * sd).astype(np.float32)
        n_syn = N - 2 * B
        segs = [("syn", 0, a), ("rows", dup_a), ("syn", a, b - a), ("rows", dup_b), ("syn", b, n_syn - b)]
        stored = np.concatenate([
            oracle.c_build_synthetic(1, 0, a, dim, "bf16", "cosine"),
            oracle.c_quantize(oracle.c_normalize_rows(dup_a), "bf16"),
            oracle.c_build_synthetic(1, a, b - a, dim, "bf16", "cosine"),
            oracle.c_quantize(oracle.c_normalize_rows(dup_b), "bf16"),
            oracle.c_build_synthetic(1, b, n_syn - b, dim, "bf16", "cosine")])
        assert stored.shape[0] == N
        s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 10)
        case = check(native, "D1024 B64 k10 planted duplicates in parts 0 and 2", dim, q, 10, s_ref, r_ref, segs, None)
        # the two duplicates lead every query's answer (the case is about what it says)
        want = np.stack([a + np.arange(B), b + B + np.arange(B)], axis=1)
        case["duplicates_lead"] = bool(np.array_equal(np.sort(r_ref[:, :2], axis=1), want))
        case["ok"] = case["ok"] and case["duplicates_lead"]
        ok = run(case)
    res["ok"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
