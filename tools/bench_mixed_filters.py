"""Mixed-filter batches on one GPU: ONE hr_index_search_masks call (a row mask per query, one exact scan per 64
queries) against the way without it -- one hr_index_search per distinct filter -- on the same index, in alternating
repeats.  B = 64, k = 10, bf16 cosine.

Sweep: D in {2, 8, 64} distinct filters x per-filter selectivity {one contiguous document (0.1 % of the rows), 1 %
random rows, 30 % random rows}, query i on filter i % D; plus, per selectivity, one mixed point with D = 8 and every
second query unfiltered.

Per point, one JSON line: ms per batch of the single call and of the per-filter launches (median and min..max over the
repeats), the union's share of tiles, the mask prep by HIP events (union + tile list, allow table), the share of
queries that left the main pass (guard failures + exhaustive passes over the timed single calls), the device-entry
time (bitmaps already on the GPU) and the upload time of the D bitmaps on their own.

Usage: python tools/bench_mixed_filters.py [--rows 1e6] [--dim 768] [--reps 7] [--out profiles/NAME.jsonl]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "youtu-rag_amd"), REPO]
import numpy as np  # noqa: E402

from hiprag import _native, synth  # noqa: E402

B, K = 64, 10


def pack(allowed):
    pad = (-len(allowed)) % 64
    return np.packbits(np.concatenate([allowed, np.zeros(pad, bool)]), bitorder="little").view(np.uint64).copy()


def make_masks(rng, n, D, kind):
    """(D, words) bitmaps and the OR of them as bools"""
    union = np.zeros(n, bool)
    rows = []
    doc = max(32, n // 1000)
    starts = rng.choice(n // doc, D, replace=False) * doc if kind == "document" else None
    for d in range(D):
        if kind == "document":
            a = np.zeros(n, bool)
            a[starts[d]:starts[d] + doc] = True
        else:
            a = rng.random(n) < (0.01 if kind == "1pct" else 0.30)
        union |= a
        rows.append(pack(a))
    return np.stack(rows), union


def tile_share(union, open_query):
    if open_query:
        return 1.0
    n = len(union)
    t = np.concatenate([union, np.zeros((-n) % 32, bool)]).reshape(-1, 32).any(axis=1)
    return float(t.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e6)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, dim, reps = int(args.rows), args.dim, args.reps
    try:
        import torch
    except ImportError:
        torch = None
    idx = _native.NativeIndex(dim, "bf16", "cosine")
    idx.reserve(n)
    idx.add_synthetic(0, 0, n)
    q, _ = synth.planted_queries(0, n, dim, B, qseed=7)
    rng = np.random.default_rng(0)
    out = open(args.out, "w") if args.out else None
    points = [(D, kind, False) for kind in ("document", "1pct", "30pct") for D in (2, 8, 64)]
    points += [(8, kind, True) for kind in ("document", "1pct", "30pct")]
    for D, kind, half_open in points:
        masks, union = make_masks(rng, n, D, kind)
        mask_of = (np.arange(B) % D).astype(np.int32)
        if half_open:  # the D filters over the even queries, the odd ones unfiltered
            mask_of = ((np.arange(B) // 2) % D).astype(np.int32)
            mask_of[1::2] = -1
        groups = [(d, np.nonzero(mask_of == d)[0]) for d in np.unique(mask_of)]

        def single():
            return idx.search_masks(q, K, masks, mask_of)

        def per_filter():
            for d, sel in groups:
                idx.search(q[sel], K, None if d < 0 else masks[d])

        for _ in range(2):
            single()
            per_filter()
        t_new, t_old = [], []
        left = 0
        for _ in range(reps):  # alternating repeats on the same box
            st0 = idx.stats()
            t0 = time.perf_counter()
            single()
            t_new.append((time.perf_counter() - t0) * 1e3)
            st1 = idx.stats()
            left += (st1["guard_failures"] - st0["guard_failures"]) + (st1["exhaustive"] - st0["exhaustive"])
            t0 = time.perf_counter()
            per_filter()
            t_old.append((time.perf_counter() - t0) * 1e3)
        idx.set_qmask_timing(True)
        single()
        prep = idx.qmask_last_ms()
        idx.set_qmask_timing(False)
        dev_ms = upload_ms = None
        if torch is not None:
            qd = torch.from_numpy(q).cuda()
            ofd = torch.from_numpy(mask_of).cuda()
            sd = torch.empty((B, K), dtype=torch.float32, device="cuda")
            rd = torch.empty((B, K), dtype=torch.int64, device="cuda")
            ups = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                md = torch.from_numpy(masks.view(np.int64)).cuda()
                torch.cuda.synchronize()
                ups.append((time.perf_counter() - t0) * 1e3)
            upload_ms = float(np.median(ups))
            devs = []
            for i in range(reps + 1):
                t0 = time.perf_counter()
                idx.search_masks_device(qd.data_ptr(), B, K, sd.data_ptr(), rd.data_ptr(), md.data_ptr(), D,
                                        masks.shape[1], ofd.data_ptr())
                if i:
                    devs.append((time.perf_counter() - t0) * 1e3)
            dev_ms = float(np.median(devs))
        rec = {"rows": n, "dim": dim, "B": B, "k": K, "D": D, "selectivity": kind, "half_unfiltered": half_open,
               "launches_per_filter_way": len(groups),
               "single_ms": float(np.median(t_new)), "single_range_ms": [min(t_new), max(t_new)],
               "per_filter_ms": float(np.median(t_old)), "per_filter_range_ms": [min(t_old), max(t_old)],
               "union_tile_share": tile_share(union, half_open),
               "union_tile_list_ms": prep["union_tile_list_ms"], "allow_table_ms": prep["allow_table_ms"],
               "left_main_pass_share": left / (reps * B), "device_entry_ms": dev_ms, "bitmap_upload_ms": upload_ms}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()
    idx.close()


if __name__ == "__main__":
    main()
