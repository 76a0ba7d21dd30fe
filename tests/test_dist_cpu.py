"""CPU, world_size 2 over gloo: the row-sharded orchestration (hiprag.dist.ShardedSearch)
-- candidate all-gather, exact merge, guard and collect-mode fallback -- returns the
single-index oracle answer.  Shard search/merge are oracle-backed stand-ins here (host
logic only); the same orchestration drives the HIP kernels and RCCL on the GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from merge_ref import ref_merge_sorted
from sharded_cpu import B_W, DUP_W, KS_W, NT_W, WIDE_CUTS, planted_rows

N, DIM, B, K, KC = 3000, 96, 12, 10, 32


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _numpy_merge(cand_all, bound_all, G, Bq, kc, k):
    """Reference semantics of k_merge (exact desc, row asc; guard)."""
    c = cand_all.numpy().reshape(G, Bq, kc, 2)
    rows_all = c.view(np.int64)[..., 1]
    s_out = np.full((Bq, k), -np.inf, np.float32)
    r_out = np.full((Bq, k), -1, np.int64)
    kth = np.full(Bq, -np.inf)
    fail = np.zeros(Bq, np.int32)
    for q in range(Bq):
        sc = c[:, q, :, 0].reshape(-1)
        rw = rows_all[:, q, :].reshape(-1)
        valid = rw >= 0
        sc, rw = sc[valid], rw[valid]
        order = np.lexsort((rw, -sc))
        sc, rw = sc[order], rw[order]
        n = min(k, len(rw))
        s_out[q, :n] = sc[:n]
        r_out[q, :n] = rw[:n]
        maxb = bound_all.numpy()[:, q].max()
        if len(rw) >= k:
            kth[q] = sc[k - 1]
        fail[q] = int(maxb > -np.inf and (len(rw) < k or not kth[q] > maxb))
    return s_out, r_out, kth, fail


def _worker(rank, world, port, result_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle
    from hiprag.dist import ShardedSearch
    from oracle import ref_numpy as R

    lo, hi = N * rank // world, N * (rank + 1) // world
    stored = oracle.c_build_synthetic(5, lo, hi - lo, DIM, "bf16", "cosine", 1)
    rng = np.random.default_rng(0)
    q = rng.standard_normal((B, DIM)).astype(np.float32)
    qn = R.process_queries(q, "cosine")
    e_fake = np.zeros(B)
    e_fake[[1, 7]] = 0.08  # force the guard to fail for two queries -> collect fallback

    class CpuSharded(ShardedSearch):
        def _stream(self):
            return 0

        def _shard_search(self, qt, k, cand, bound, mask_ptr, q_ready=None):
            s, r = oracle.c_search(stored, "bf16", qn[: qt.shape[0]], KC, row_offset=lo, nthreads=1)
            cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
            cand[..., 0] = torch.from_numpy(s)
            full = (hi - lo) > KC
            bound[:] = torch.from_numpy(np.where(full, s[:, -1] + e_fake[: qt.shape[0]], -np.inf))

        def _shard_collect(self, qt, kth, cap, cand, bound, mask_ptr):
            idx = [int(np.nonzero((q == qt[i].numpy()).all(1))[0][0]) for i in range(qt.shape[0])]
            s, r = oracle.c_search(stored, "bf16", qn[idx], cap, row_offset=lo, nthreads=1)
            keep = s >= (kth.numpy()[:, None] - e_fake[idx][:, None])
            s = np.where(keep, s, -np.inf)
            r = np.where(keep, r, -1)
            cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
            cand[..., 0] = torch.from_numpy(s)
            bound[:] = torch.from_numpy(np.where(keep.all(1), np.inf, -np.inf))

        def _merge(self, cand_all, bound_all, G, Bq, kc, k, s_out, r_out, kth, fail):
            s, r, kt, f = _numpy_merge(cand_all, bound_all, G, Bq, kc, k)
            s_out.copy_(torch.from_numpy(s))
            r_out.copy_(torch.from_numpy(r))
            kth.copy_(torch.from_numpy(kt))
            fail.copy_(torch.from_numpy(f))

    ss = CpuSharded(index=None, row_offset=lo, max_batch=B, device=torch.device("cpu"))
    s, r = ss.search(torch.from_numpy(q), K)
    # the same batch known only to rank 1: broadcast first (src_rank), identical results
    q_in = torch.from_numpy(q) if rank == 1 else torch.zeros((B, DIM))
    s2, r2 = ss.search(q_in, K, src_rank=1)
    assert torch.equal(s2, s) and torch.equal(r2, r)
    if rank == 0:
        np.savez(result_path, s=s.numpy(), r=r.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_search_matches_single_index(tmp_path):
    import oracle
    from oracle import ref_numpy as R

    path = str(tmp_path / "res.npz")
    mp.start_processes(_worker, args=(2, _free_port(), path), nprocs=2, join=True, start_method="spawn")
    got = np.load(path)
    stored = oracle.c_build_synthetic(5, 0, N, DIM, "bf16", "cosine", 2)
    q = np.random.default_rng(0).standard_normal((B, DIM)).astype(np.float32)
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), K)
    np.testing.assert_array_equal(got["r"], r_ref)
    np.testing.assert_array_equal(got["s"], s_ref.astype(np.float32))


def test_merge_guard_semantics():
    """Guard: fail iff some shard still hides rows that might beat the k-th result."""
    cand = torch.zeros((2, 1, 3, 2), dtype=torch.float64)
    cand[0, 0, :, 0] = torch.tensor([0.9, 0.5, 0.4], dtype=torch.float64)
    cand[1, 0, :, 0] = torch.tensor([0.8, 0.7, 0.1], dtype=torch.float64)
    cand.view(torch.int64)[0, 0, :, 1] = torch.tensor([3, 5, 9])
    cand.view(torch.int64)[1, 0, :, 1] = torch.tensor([100, 101, 102])
    s, r, kth, fail = _numpy_merge(cand, torch.tensor([[0.3], [-np.inf]]), 2, 1, 3, 2)
    assert r.tolist() == [[3, 100]] and kth[0] == 0.8 and fail[0] == 0
    s, r, kth, fail = _numpy_merge(cand, torch.tensor([[0.85], [-np.inf]]), 2, 1, 3, 2)
    assert fail[0] == 1


class StubRccl:
    """A ctypes-shaped stand-in for librccl.so (the entry points RcclComm binds, same argument conventions) that
    moves the bytes between the ranks with gloo on the host -- so RcclComm's G > 1 control flow (unique-id
    broadcast, ncclCommInitRank(G, uid, rank), rank-ordered all-gather, broadcast, destroy) runs on CPU.  Pointers
    are host addresses here (CPU tensors)."""

    def __init__(self, uid_bytes: bytes):
        import ctypes

        self.ct, self.uid_bytes, self.calls = ctypes, uid_bytes, []

        def get_error_string(rc):
            return b"stub error"

        def get_unique_id(uid_ref):
            ctypes.memmove(ctypes.addressof(uid_ref._obj), self.uid_bytes, 128)
            self.calls.append(("ncclGetUniqueId",))
            return 0

        def comm_init_rank(comm_ref, nranks, uid, rank):
            self.calls.append(("ncclCommInitRank", int(nranks), bytes(uid.internal), int(rank)))
            comm_ref._obj.value = 0x5EED
            return 0

        def all_gather(send, recv, count, dtype, comm, stream):
            n = int(count.value)
            assert dtype == 1 and comm.value == 0x5EED  # uint8, the communicator InitRank returned
            mine = torch.frombuffer(bytearray(ctypes.string_at(send.value, n)), dtype=torch.uint8)
            every = [torch.empty(n, dtype=torch.uint8) for _ in range(dist.get_world_size())]
            dist.all_gather(every, mine)
            for r, t in enumerate(every):  # rank r's bytes at offset r * count (ncclAllGather's layout)
                ctypes.memmove(recv.value + r * n, t.numpy().tobytes(), n)
            self.calls.append(("ncclAllGather", n))
            return 0

        def broadcast(send, recv, count, dtype, root, comm, stream):
            n = int(count.value)
            t = torch.frombuffer(bytearray(ctypes.string_at(send.value, n)), dtype=torch.uint8)
            dist.broadcast(t, int(root))
            ctypes.memmove(recv.value, t.numpy().tobytes(), n)
            self.calls.append(("ncclBroadcast", n, int(root)))
            return 0

        def comm_destroy(comm):
            self.calls.append(("ncclCommDestroy",))
            return 0

        self.ncclGetErrorString = get_error_string
        self.ncclGetUniqueId = get_unique_id
        self.ncclCommInitRank = comm_init_rank
        self.ncclAllGather = all_gather
        self.ncclBroadcast = broadcast
        self.ncclCommDestroy = comm_destroy


def _rccl_worker(rank, world, port, result_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import oracle
    from hiprag.dist import ShardedSearch, _record_len
    from oracle import ref_numpy as R

    lo, hi = N * rank // world, N * (rank + 1) // world
    bounds = [(N * g // world, N * (g + 1) // world) for g in range(world)]
    stored = oracle.c_build_synthetic(5, lo, hi - lo, DIM, "bf16", "cosine", 1)
    q = np.random.default_rng(0).standard_normal((B, DIM)).astype(np.float32)
    qn = R.process_queries(q, "cosine")
    stub = StubRccl(uid_bytes=bytes([rank * 7 + 3]) * 128 if rank == 0 else bytes(128))
    seen = {}

    class CpuRccl(ShardedSearch):
        def _stream(self):
            return 0

        def _shard_search(self, qt, k, cand, bound, mask_ptr, q_ready=None):
            s, r = oracle.c_search(stored, "bf16", qn[: qt.shape[0]], KC, row_offset=lo, nthreads=1)
            cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
            cand[..., 0] = torch.from_numpy(s)
            bound[:] = torch.from_numpy(s[:, -1])

        def _merge(self, cand_all, bound_all, G, Bq, kc, k, s_out, r_out, kth, fail):
            # the packed records as the product's k_merge reads them: rank g's record at g * (record bytes)
            assert cand_all.stride(0) * 8 == _record_len(Bq, kc) * 8 and bound_all.stride(0) == cand_all.stride(0)
            rows = cand_all.contiguous().view(torch.int64)[..., 1].numpy()
            for g, (a, b) in enumerate(bounds):  # rank order: row g of the gather holds rank g's shard rows
                assert ((rows[g] >= a) & (rows[g] < b)).all(), (g, rows[g].min(), rows[g].max())
            seen["merged"] = seen.get("merged", 0) + 1
            s, r, kt, f = _numpy_merge(cand_all, bound_all, G, Bq, kc, k)
            s_out.copy_(torch.from_numpy(s))
            r_out.copy_(torch.from_numpy(r))
            kth.copy_(torch.from_numpy(kt))
            fail.copy_(torch.from_numpy(f))

    ss = CpuRccl(index=None, row_offset=lo, max_batch=B, device=torch.device("cpu"), kc=KC, rccl_lib=stub)
    assert ss.rccl is not None and ss.transport.startswith("rccl") and ss.rccl.G == world
    s, r = ss.search(torch.from_numpy(q), K)
    q_in = torch.from_numpy(q) if rank == 1 else torch.zeros((B, DIM))
    s2, r2 = ss.search(q_in, K, src_rank=1)  # the batch known to rank 1 only: ncclBroadcast from root 1
    assert torch.equal(s2, s) and torch.equal(r2, r)
    ss.close()
    names = [c[0] for c in stub.calls]
    init = [c for c in stub.calls if c[0] == "ncclCommInitRank"][0]
    out = {"rank": rank, "names": names, "init_G": init[1], "init_rank": init[3], "uid": init[2].hex(),
           "merged": seen["merged"], "ag": [c[1] for c in stub.calls if c[0] == "ncclAllGather"],
           "bc": [c[1:] for c in stub.calls if c[0] == "ncclBroadcast"]}
    import json

    with open(f"{result_path}.{rank}.json", "w") as f:
        json.dump(out, f)
    if rank == 0:
        np.savez(result_path, s=s.numpy(), r=r.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_comm_two_ranks_with_stub_library(tmp_path):
    """RcclComm's G > 1 control flow on CPU -- the unique id rank 0 draws reaches rank 1 through
    the process-group broadcast, every rank calls ncclCommInitRank(G, that id, its rank), the all-gathered records
    arrive in rank order and the merge reads them with the packed record stride, and the answer is the single-index
    oracle's."""
    import json

    import oracle
    from hiprag.dist import _record_len
    from oracle import ref_numpy as R

    path = str(tmp_path / "rccl")
    mp.start_processes(_rccl_worker, args=(2, _free_port(), path), nprocs=2, join=True, start_method="spawn")
    per = [json.load(open(f"{path}.{r}.json")) for r in range(2)]
    uid0 = (bytes([3]) * 128).hex()
    for r, o in enumerate(per):
        assert o["init_G"] == 2 and o["init_rank"] == r and o["uid"] == uid0  # rank 1 never drew an id itself
        assert o["names"][-1] == "ncclCommDestroy"
        assert o["ag"] == [_record_len(B, KC) * 8] * 2  # one all-gather of the packed record per batch
        assert o["bc"] == [[B * DIM * 4, 1]]            # the src_rank batch: one broadcast from root 1
        assert o["merged"] == 2
    assert "ncclGetUniqueId" in per[0]["names"] and "ncclGetUniqueId" not in per[1]["names"]
    got = np.load(path + ".npz")
    stored = oracle.c_build_synthetic(5, 0, N, DIM, "bf16", "cosine", 2)
    q = np.random.default_rng(0).standard_normal((B, DIM)).astype(np.float32)
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), K)
    np.testing.assert_array_equal(got["r"], r_ref)
    np.testing.assert_array_equal(got["s"], s_ref.astype(np.float32))


# ---------------------------------------------------------------- ties across the shard boundary, k beyond kc
NT, DUP_LO, DUP_HI = 6000, 2000, 4000  # 2,000 copies of one row straddling the rank boundary at 3,000


def _ties_stored(lo, hi, dup_hi=DUP_HI):
    """Stored (bf16, cosine-processed) rows [lo, hi) of the ties corpus: the synthetic rows with rows
    [DUP_LO, dup_hi) replaced by copies of row 77.  lo == hi: an empty shard, (0, DIM)."""
    import oracle

    x = oracle.c_build_synthetic(5, lo, hi - lo, DIM, "bf16", "cosine", 1)
    dup = oracle.c_build_synthetic(5, 77, 1, DIM, "bf16", "cosine", 1)[0]
    a, b = max(lo, DUP_LO), min(hi, dup_hi)
    if a < b:
        x[a - lo:b - lo] = dup
    return x


def _ties_queries(nb=B, planted=()):
    """nb queries: the duplicated row itself, a near-tie, random ones -- and, from position 6 on, the stored rows
    `planted` (rows outside the tie block), so that the shards holding them own a top-1 answer."""
    import oracle
    from oracle import ref_numpy as R

    q = np.random.default_rng(3).standard_normal((nb, DIM)).astype(np.float32)
    dup = R.dequantize(oracle.c_build_synthetic(5, 77, 1, DIM, "bf16", "cosine", 1), "bf16")[0]
    q[0] = dup          # its top-k is all ties (2,000 equal scores)
    q[4] = dup + 0.01 * q[4]  # near-ties
    for i, row in enumerate(planted):
        q[6 + i] = R.dequantize(oracle.c_build_synthetic(5, row, 1, DIM, "bf16", "cosine", 1), "bf16")[0]
    return R.process_queries(q, "cosine")


def _numpy_merge_sorted(cand_all, G, Bq, m, k):
    """Reference semantics of k_merge_sorted: the top-k of the union of the ranks' sorted lists."""
    return ref_merge_sorted(cand_all.numpy().reshape(G, Bq, m, 2), k)


def _ties_worker(rank, world, port, result_path, cuts=None, dup_hi=DUP_HI, ks=(10, 100, 200), nb=B, src=1,
                 plant=False):
    """One rank of the ties corpus cut at `cuts` (default: equal parts): every k of `ks`, then the k = 200 batch
    known to rank `src` only.  Every rank writes its own answers, counters and stub log to result_path.<rank>.npz
    -- after its last collective, so a failing rank never leaves the others waiting in one."""
    from datetime import timedelta

    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    import oracle
    from hiprag.dist import ShardedSearch, _record_len

    cuts = list(cuts) if cuts is not None else [NT * g // world for g in range(world + 1)]
    assert len(cuts) == world + 1 and cuts[0] == 0 and cuts[-1] == NT
    lo, hi = cuts[rank], cuts[rank + 1]
    stored = _ties_stored(lo, hi, dup_hi)
    qn = _ties_queries(nb, planted_rows(cuts) if plant else ())
    stub = StubRccl(uid_bytes=bytes([9]) * 128 if rank == 0 else bytes(128))
    seen = {"scan_kc": [], "collect": 0, "exact_m": []}

    def qidx(qt):
        return [int(np.nonzero((qn == qt[i].numpy()).all(1))[0][0]) for i in range(qt.shape[0])]

    def in_cuts(cand_all, G):
        # rank order: record g of the gather holds rows of shard g only (padding aside)
        rows = cand_all.contiguous().view(torch.int64)[..., 1].numpy().reshape(G, -1)
        for g in range(G):
            real = rows[g][rows[g] >= 0]
            assert ((real >= cuts[g]) & (real < cuts[g + 1])).all(), (g, cuts[g], cuts[g + 1], real.min(), real.max())

    class CpuTies(ShardedSearch):
        """Shard pieces with the kernels' contracts: the scan's bound is the k-th candidate's score (ties at
        the boundary fail the guard), a collect window larger than its buffer returns the shard's exact top
        rows (bound -inf), the exhaustive pass returns the sorted exact top-m.  A shard with fewer rows than
        asked for pads (-inf / -1) and bounds nothing (-inf); an empty shard is all padding (the oracle over
        zero rows) -- and still takes part in every collective."""

        def _stream(self):
            return 0

        def _shard_search(self, qt, k, cand, bound, mask_ptr, q_ready=None, kc=None):
            kc = kc or self.kc
            seen["scan_kc"].append(kc)
            s, r = oracle.c_search(stored, "bf16", qn[qidx(qt)], kc, row_offset=lo, nthreads=1)
            assert hi > lo or ((r == -1).all() and np.isneginf(s).all())
            cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
            cand[..., 0] = torch.from_numpy(s)
            bound[:] = torch.from_numpy(np.where(r[:, -1] >= 0, s[:, -1], -np.inf))

        def _shard_collect(self, qt, kth, cap, cand, bound, mask_ptr):
            seen["collect"] += 1
            s, r = oracle.c_search(stored, "bf16", qn[qidx(qt)], cap, row_offset=lo, nthreads=1)
            keep = s >= kth.numpy()[:, None]
            full = keep[:, -1]  # the window reaches past the buffer: the shard's exact top-cap instead
            keep |= full[:, None]
            cand.view(torch.int64)[..., 1] = torch.from_numpy(np.where(keep, r, -1))
            cand[..., 0] = torch.from_numpy(np.where(keep, s, -np.inf))
            bound[:] = -np.inf

        def _shard_exact(self, qt, m, cand, mask_ptr):
            seen["exact_m"].append(m)
            s, r = oracle.c_search(stored, "bf16", qn[qidx(qt)], m, row_offset=lo, nthreads=1)
            cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
            cand[..., 0] = torch.from_numpy(s)

        def _merge(self, cand_all, bound_all, G, Bq, kc, k, s_out, r_out, kth, fail):
            assert G == world and cand_all.stride(0) == _record_len(Bq, kc) == bound_all.stride(0)
            in_cuts(cand_all, G)
            s, r, kt, f = _numpy_merge(cand_all, bound_all, G, Bq, kc, k)
            s_out.copy_(torch.from_numpy(s))
            r_out.copy_(torch.from_numpy(r))
            kth.copy_(torch.from_numpy(kt))
            fail.copy_(torch.from_numpy(f))

        def _merge_sorted(self, cand_all, G, Bq, m, k, s_out, r_out):
            assert G == world
            in_cuts(cand_all, G)
            s, r = _numpy_merge_sorted(cand_all.contiguous(), G, Bq, m, k)
            s_out.copy_(torch.from_numpy(s))
            r_out.copy_(torch.from_numpy(r))

    ss = CpuTies(index=None, row_offset=lo, max_batch=nb, device=torch.device("cpu"), max_k=16, rccl_lib=stub)
    assert ss.kc == 32 and ss.rccl is not None
    out = {}
    for k in ks:
        s, r = ss.search(torch.from_numpy(qn), k)
        out[f"s{k}"], out[f"r{k}"] = s.numpy(), r.numpy()
    s_b, r_b = ss.search(torch.from_numpy(qn) if rank == src else torch.zeros((nb, DIM)), 200, src_rank=src)
    out["s_src"], out["r_src"] = s_b.numpy(), r_b.numpy()
    ss.close()
    dist.barrier()
    dist.destroy_process_group()  # the last collective is behind this rank: what follows cannot stall another
    out["fallback"], out["exact"] = ss.fallback_queries, ss.exact_queries
    out["scan_kc"], out["collect"], out["exact_m"] = np.array(seen["scan_kc"]), seen["collect"], np.array(seen["exact_m"])
    # the collectives this rank issued, in order: name, bytes (and the root of a broadcast)
    out["log"] = np.array([" ".join(map(str, c)) for c in stub.calls if c[0] in ("ncclAllGather", "ncclBroadcast")])
    np.savez(f"{result_path}.{rank}.npz", **out)
    assert np.array_equal(out["r_src"], out["r200"]) and np.array_equal(out["s_src"], out["s200"])


def test_sharded_ties_and_large_k_match_oracle(tmp_path):
    """2,000 duplicate rows straddling the shard boundary and k in {10, 100, 200} -- k above
    the pipelined kc (32) and above HR_MAX_K -- through the stub-RCCL exchange, identical to the single-index
    oracle (ids and score bits) on both ranks; nothing raises."""
    import oracle

    path = str(tmp_path / "ties")
    mp.start_processes(_ties_worker, args=(2, _free_port(), path), nprocs=2, join=True, start_method="spawn")
    stored = _ties_stored(0, NT)
    qn = _ties_queries()
    for rank in range(2):
        got = np.load(f"{path}.{rank}.npz")
        for k in (10, 100, 200):
            s_ref, r_ref = oracle.c_search(stored, "bf16", qn, k)
            np.testing.assert_array_equal(got[f"r{k}"], r_ref, err_msg=f"rank {rank} k={k}")
            np.testing.assert_array_equal(got[f"s{k}"], s_ref.astype(np.float32), err_msg=f"rank {rank} k={k}")
        # (row 77 itself ties with its 2,000 copies and comes first)
        assert list(got["r10"][0]) == [77] + list(range(DUP_LO, DUP_LO + 9))
        assert list(got["r200"][0]) == [77] + list(range(DUP_LO, DUP_LO + 199))
        # k = 10: the pipelined scan (kc 32), ties -> collect fallback; k = 100: the scan at kc_for_k(100) = 160, its
        # fallback; k = 200 > HR_MAX_K: the exhaustive pass (twice: the plain and the broadcast batch)
        assert list(got["scan_kc"]) == [32, 160] and int(got["collect"]) >= 2 and int(got["fallback"]) >= 2
        assert list(got["exact_m"]) == [200, 200] and int(got["exact"]) == 2 * B


# ---------------------------------------------------------------- 3 and 8 ranks: tiny, empty and uneven shards
@pytest.mark.parametrize("name", sorted(WIDE_CUTS))
def test_sharded_wide_worlds_match_oracle_on_every_rank(tmp_path, name):
    """ShardedSearch at world sizes 3 and 8 over shards that are empty, smaller than kc, and uneven, with a block of
    2,200 exact ties crossing the cuts: k = 10 (pipelined, kc 32), 100 and 128 (the scans at kc 160 and 192) and
    200 (the exhaustive pass), then a k = 200 batch only the LAST rank knows (src_rank).  Every rank holds the
    oracle's answer, bit for bit; every rank issued the same collectives with the same byte counts in the same
    order (an empty rank included); record g of every gather held rows of cut g only (checked in the workers'
    merges); the tie query's fallback ran with fallback_cap(G) records per shard."""
    import oracle
    from hiprag.dist import _record_len, fallback_cap

    cuts = WIDE_CUTS[name]
    world = len(cuts) - 1
    stored = _ties_stored(0, NT_W, DUP_W[1])
    qn = _ties_queries(B_W, planted_rows(cuts))
    # every shard that holds copies holds more than kc of them: its scan returns kc tied candidates, its bound is
    # the tie score and the guard fails -- from the oracle over that shard's rows
    s_tie = oracle.c_search(stored, "bf16", qn[:1], 1)[0][0, 0]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if max(a, DUP_LO) < min(b, DUP_W[1]):
            s_sh, r_sh = oracle.c_search(stored[a:b], "bf16", qn[:1], KC + 1, row_offset=a)
            assert r_sh[0, KC] >= 0 and s_sh[0, KC] == s_tie, (a, b)
    # each planted row is its query's top-1 and lies in a shard of fewer than 64 rows
    for i, row in enumerate(planted_rows(cuts)):
        assert oracle.c_search(stored, "bf16", qn[6 + i:7 + i], 1)[1][0, 0] == row
    path = str(tmp_path / name)
    mp.start_processes(_ties_worker, args=(world, _free_port(), path, cuts, DUP_W[1], KS_W, B_W, world - 1, True),
                       nprocs=world, join=True, start_method="spawn")
    got = [np.load(f"{path}.{rank}.npz") for rank in range(world)]
    refs = {k: oracle.c_search(stored, "bf16", qn, k) for k in KS_W}
    for rank, g in enumerate(got):
        for k in KS_W:
            s_ref, r_ref = refs[k]
            np.testing.assert_array_equal(g[f"r{k}"], r_ref, err_msg=f"rank {rank} k={k}")
            np.testing.assert_array_equal(g[f"s{k}"], s_ref.astype(np.float32), err_msg=f"rank {rank} k={k}")
        np.testing.assert_array_equal(g["r_src"], refs[200][1], err_msg=f"rank {rank} src_rank batch")
        np.testing.assert_array_equal(g["s_src"], refs[200][0].astype(np.float32), err_msg=f"rank {rank} src_rank batch")
        assert list(g["r128"][0]) == [77] + list(range(DUP_LO, DUP_LO + 127))
        # routes: k = 10 pipelined (kc 32); 100 and 128 the scans at kc_for_k = 160 and 192; 200 exhaustive, twice
        assert list(g["scan_kc"]) == [32, 160, 192], (rank, g["scan_kc"])
        assert list(g["exact_m"]) == [200, 200] and int(g["exact"]) == 2 * B_W
        # the tie query and the near-tie query fail their guard at k = 10, 100 and 128: one collect each
        assert int(g["fallback"]) >= 6 and int(g["collect"]) == 3, (rank, int(g["fallback"]), int(g["collect"]))
        assert list(g["log"]) == list(got[0]["log"]), f"rank {rank} issued other collectives than rank 0"
    # ... and that sequence is the one the design states: per scan k one gather of the packed records and one of the
    # fallback's records (cap = fallback_cap(G) per failed query), per exhaustive batch one gather of the sorted
    # lists, the last one behind the broadcast from the last rank
    log = [tuple(x.split()) for x in got[0]["log"]]
    cap = fallback_cap(world)
    want = []
    for k, kc in ((10, 32), (100, 160), (128, 192)):
        want.append(("ncclAllGather", str(_record_len(B_W, kc) * 8)))
        nf = int(log[len(want)][1]) // 8 // (cap * 2 + 1)  # failed queries of this k (>= 2, the same on every rank)
        assert nf >= 2
        want.append(("ncclAllGather", str(_record_len(nf, cap) * 8)))
    want += [("ncclAllGather", str(B_W * 200 * 16)), ("ncclBroadcast", str(B_W * DIM * 4), str(world - 1)),
             ("ncclAllGather", str(B_W * 200 * 16))]
    assert log == want
    assert _record_len(B_W, 32) * 8 % 16 == 8
