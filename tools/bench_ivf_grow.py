#!/usr/bin/env python3
"""Growable IVF lists: what growth costs the search (stage 1 of tools/bench_rerank.py, same corpus and queries).

  --leg bulk   the bulk-built index through hr_ivf_search (runs on older trees too: the A/B against a parent build)
  --leg grow   the same rows added in --batches equal add() calls, searched through hr_ivf_search_ext, before and
               after compact(): ms per batch, extents, the share of allocated slots that hold no live row
  --leg store  HipVectorStore search_batch of --batch queries, index_type IVF_FLAT against the exact store, and the
               recall@10 of the IVF answers against the exact ones

One JSON line per leg.  Times: device events around --steps batches after --warmup, repeated --repeats times.
Usage: python tools/bench_ivf_grow.py --leg bulk,grow [--rows 6250000 --dim 1024 --dtype f16 --nlist 8192 --nprobe 32]
       python tools/bench_ivf_grow.py --leg store --rows 1000000 --dim 768 --dtype bf16 --nlist 1024 --nprobe 16 --k 10
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.environ.get("HIPRAG_PKG_ROOT") or os.path.join(REPO, "youtu-rag_amd"), REPO]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--leg", default="bulk,grow")
    p.add_argument("--rows", type=int, default=6_250_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--dtype", default="f16")
    p.add_argument("--nlist", type=int, default=8192)
    p.add_argument("--nprobe", type=int, default=32)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--batches", type=int, default=64)
    p.add_argument("--centers", type=int, default=20000)
    p.add_argument("--spread", type=float, default=0.7)
    p.add_argument("--grow-time", default="both", help="grow leg: time the fragmented index, the compacted one or both")
    p.add_argument("--tag", default="")
    args = p.parse_args()

    import numpy as np
    import torch

    from hiprag import _native
    from hiprag.ivf import IvfIndex

    dev = torch.device("cuda", 0)
    N, D, B, K = args.rows, args.dim, args.batch, args.k
    st = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    t00 = time.time()
    log = lambda m: print(f"[{time.time() - t00:7.1f}s] {m}", file=sys.stderr, flush=True)  # noqa: E731
    centers = torch.empty((args.centers, D), dtype=torch.float32, device=dev)
    _native.gen_rows_device(7, 0, args.centers, D, centers.data_ptr(), st())
    centers = torch.nn.functional.normalize(centers, dim=1)

    def rows(i0, i1):  # the clustered corpus of tools/bench_ivf.py
        noise = torch.empty((i1 - i0, D), dtype=torch.float32, device=dev)
        _native.gen_rows_device(11, i0, i1 - i0, D, noise.data_ptr(), st())
        c = (torch.arange(i0, i1, device=dev, dtype=torch.int64) * 2654435761) % args.centers
        return centers[c] + args.spread * torch.nn.functional.normalize(noise, dim=1)

    g = torch.Generator(device=dev)
    g.manual_seed(5)
    qs = []
    for _ in range(8):
        j = torch.randint(0, N, (B // 2,), generator=g, device=dev)
        base = torch.cat([rows(int(r), int(r) + 1) for r in j.tolist()])
        qs.append(torch.cat([base + 0.1 * torch.randn(base.shape, generator=g, device=dev),
                             torch.randn((B - B // 2, D), generator=g, device=dev)]).contiguous())

    def time_ivf(ivf):
        cand = torch.empty((B, K, 2), dtype=torch.float64, device=dev)
        bound = torch.empty(B, dtype=torch.float64, device=dev)
        out = []
        for _ in range(args.repeats):
            for i in range(args.warmup):
                ivf.search_candidates(qs[i % len(qs)], K, args.nprobe, cand, bound)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                ivf.search_candidates(qs[i % len(qs)], K, args.nprobe, cand, bound)
            e1.record()
            torch.cuda.synchronize()
            out.append(round(e0.elapsed_time(e1) / args.steps, 4))
        ivf.search_candidates(qs[0], K, args.nprobe, cand, bound)
        torch.cuda.synchronize()
        return out, cand.view(torch.int64)[..., 1].cpu().numpy(), cand[..., 0].cpu().numpy()

    common = {"rows": N, "dim": D, "dtype": args.dtype, "nlist": args.nlist, "nprobe": args.nprobe, "batch": B, "k": K,
              "steps": args.steps, "tag": args.tag}
    sample = lambda: rows(0, min(N, args.nlist * 32))  # noqa: E731
    legs = args.leg.split(",")
    ref = None
    if "bulk" in legs:
        ivf = IvfIndex(D, args.nlist, dtype=args.dtype, metric="cosine")
        ivf.train(sample(), iters=10, seed=0)
        ivf.build(N, rows)
        torch.cuda.synchronize()
        log("bulk index built")
        ms, ids, sc = time_ivf(ivf)
        ref = (ids, sc)
        print(json.dumps({"leg": "bulk", **common, "ms_per_batch": ms,
                          "tiles": int(ivf.list_tiles[-1].item()), "ids_crc": int(np.bitwise_xor.reduce(ids.ravel())),
                          "score_sum": float(sc[np.isfinite(sc)].sum())}), flush=True)
        ivf.close()
        del ivf
        torch.cuda.empty_cache()
    if "grow" in legs:
        ivf = IvfIndex(D, args.nlist, dtype=args.dtype, metric="cosine")
        ivf.train(sample(), iters=10, seed=0)
        step = -(-N // args.batches)
        t0 = time.time()
        for i in range(0, N, step):
            ivf.add(rows(i, min(N, i + step)).contiguous())
        torch.cuda.synchronize()
        add_s = time.time() - t0
        log(f"{args.batches} adds done")

        def shape(ivf):
            slots = int(ivf.ntiles.sum()) * 32
            return {"n_ext": ivf.n_ext, "tiles": int(ivf.ntiles.sum()),
                    "dead_slot_fraction": round(1.0 - ivf.index.size()[1] / max(slots, 1), 5)}

        if args.grow_time == "compacted":     # (a profile of the compacted index alone)
            ivf.compact()
        ms_f, ids_f, sc_f = time_ivf(ivf)
        frag = shape(ivf)
        t0 = time.time()
        ivf.compact()
        torch.cuda.synchronize()
        compact_s = time.time() - t0
        ms_c, ids_c, sc_c = time_ivf(ivf) if args.grow_time == "both" else (ms_f, ids_f, sc_f)
        same = bool((ids_f == ids_c).all() and (sc_f == sc_c).all())
        # (the bulk build assigns lists in other GEMM shapes than the adds: a row between two centroids may differ)
        as_bulk = None if ref is None else bool((ids_c == ref[0]).all() and (sc_c == ref[1]).all())
        print(json.dumps({"leg": "grow", **common, "batches": args.batches, "add_s": round(add_s, 1),
                          "fragmented": {"ms_per_batch": ms_f, **frag},
                          "compacted": {"ms_per_batch": ms_c, **shape(ivf), "compact_s": round(compact_s, 1)},
                          "compact_keeps_results": same, "results_equal_bulk": as_bulk, "ids_crc": int(np.bitwise_xor.reduce(ids_c.ravel())),
                          "score_sum": float(sc_c[np.isfinite(sc_c)].sum())}), flush=True)
        ivf.close()
        del ivf
        torch.cuda.empty_cache()
    if "store" in legs:
        import tempfile

        from hiprag.rag import Chunk, HipVectorStore, VectorStoreConfig

        res = {}
        hits = {}
        qh = [q.cpu().numpy() for q in qs]
        for name, index_type in (("exact", None), ("ivf", "IVF_FLAT")):
            cfg = VectorStoreConfig(backend="hip", collection_name=name, persist_directory=tempfile.mkdtemp(),
                                    index_type=index_type,
                                    index_params={"dtype": args.dtype, "persist": False, "nlist": args.nlist,
                                                  "nprobe": args.nprobe, "capacity": N})
            store = HipVectorStore(cfg)
            t0 = time.time()
            for i in range(0, N, 1 << 16):
                j = min(N, i + (1 << 16))
                x = rows(i, j).contiguous()
                store.add_chunks_device([Chunk(id=str(r), document_id="d", content="", chunk_index=0, metadata={})
                                         for r in range(i, j)], x)
            log(f"{name} store filled in {time.time() - t0:.1f}s")
            out = []
            for _ in range(args.repeats):
                for i in range(args.warmup):
                    store.search_batch(qh[i % len(qh)], K)
                t0 = time.perf_counter()
                for i in range(args.steps):
                    store.search_batch(qh[i % len(qh)], K)     # (each call ends with its results on the host)
                out.append(round((time.perf_counter() - t0) * 1e3 / args.steps, 4))
            res[name] = out
            hits[name] = [[[c.id for c, _ in per_q] for per_q in store.search_batch(q, K)] for q in qh]
            store.close()
            torch.cuda.empty_cache()
        def recall(sl):  # queries sl of every batch: the first half is planted near stored rows, the rest isotropic
            return round(float(np.mean([len(set(a[:10]) & set(b[:10])) / 10 for qa, qb in zip(hits["ivf"], hits["exact"])
                                        for a, b in zip(qa[sl], qb[sl])])), 4)

        print(json.dumps({"leg": "store", **common, "exact_ms_per_search_batch": res["exact"],
                          "ivf_ms_per_search_batch": res["ivf"], "recall_at_10_vs_exact": recall(slice(None)),
                          "recall_at_10_planted_q": recall(slice(0, B // 2)),
                          "recall_at_10_isotropic_q": recall(slice(B // 2, None))}), flush=True)


if __name__ == "__main__":
    main()
