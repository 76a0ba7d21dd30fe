"""GPU: the row-sharded search (hiprag.dist.ShardedSearch) on the kernels at 3 and 8 ranks sharing the GPU over gloo,
with the cuts of tests/sharded_cpu.py WIDE_CUTS -- a 20-row shard (fewer rows than kc = 32), a 10-row shard, an EMPTY
shard, and a block of 2,200 exact ties that covers two whole shards and crosses three boundaries -- and, before any
collective is involved, the per-shard pieces (hr_index_search_shard, its two-stream form, _collect, _exact) on
single-device indexes of 1 row, 20 rows, 20 removed rows and no rows at all.

What the pieces do on an empty shard is decided by the code, not by these runs (hr_index.hip, shard_chunk): with
no tile to visit `if (n_vis > 0)` skips SAMPLE and FILTER, `priv = a.private_bufs && n_vis > 0` makes k_select read
the shared counter k_prep_q zeroed, so it selects nothing and hands on `bound_approx = thr` = -inf (every group
maximum is still HR_KEY_NEG_INF, the floor -inf), and k_rescore writes (-inf, -1) records and
`bd = (ba == -inf) ? -inf`; exhaustive_topm has `if (n <= 0)`: m padding records.  Padding and a bound of -inf, on
the stream: what hr_group.hip writes for an empty shard by hand.  An empty rank therefore runs the same calls as
any other and issues every collective.  Bar everywhere: ids, score bits, -inf / -1 padding equal to the CPU oracle."""
import os
import socket

import numpy as np
import pytest

from sharded_cpu import B_W, DUP_W, KS_W, NT_W, WIDE_CUTS, planted_rows

pytestmark = pytest.mark.gpu

DIM, SEED, KC = 64, 5, 32
MASK_KEEP = 0.6


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------- B0: the per-shard pieces, one process
OFF = 720  # a non-zero row offset: the shard's rows are global rows OFF, OFF + 1, ...


def _records(t):
    """(scores f64, rows i64) of a device tensor of candidate records (..., 2)."""
    a = t.cpu().numpy()
    return a[..., 0], a[..., 1].view(np.int64)


def _sorted(s, r):
    """Each query's records in (score desc, row asc) order, padding last: a scan returns its candidates in the
    order of their approximate scores."""
    key_r = np.where(r >= 0, r, np.iinfo(np.int64).max)
    order = np.lexsort((key_r, -s), axis=-1)
    return np.take_along_axis(s, order, -1), np.take_along_axis(r, order, -1)


@pytest.mark.parametrize("n,removed", [(1, False), (20, False), (20, True), (0, False)])
def test_shard_pieces_on_tiny_and_empty_shards(n, removed):
    """hr_index_search_shard (one stream; scan + tail streams with a q_ready event), _collect and _exact on an
    index of n rows (all of them removed again if `removed`), with a row offset, with and without a device mask.
    Fewer live rows than kc: every live, allowed row comes back with its exact score, the rest is (-inf, -1), and
    the bound is -inf -- the shard hides nothing, so the guard of a merge over it cannot fail."""
    import torch

    import oracle
    from hiprag import _native
    from oracle import ref_numpy as R

    _native.load_library()
    Bq, k, cap, m = 5, 10, 64, 200
    raw = R.gen_rows(SEED, OFF, n, DIM)
    stored = R.process_rows(raw, "cosine", "bf16") if n else np.empty((0, DIM), np.uint16)
    idx = _native.NativeIndex(DIM, "bf16", "cosine", device=0)
    if n:
        idx.add(raw)
    if removed:
        idx.remove(np.arange(n))
    live = np.zeros(n, bool) if removed else np.ones(n, bool)
    assert idx.size() == (n, int(live.sum()))
    rng = np.random.default_rng(n + 1)
    q = rng.standard_normal((Bq, DIM)).astype(np.float32)
    if n:
        q[1] = raw[n // 2]
    qn = R.process_queries(q, "cosine")
    allowed = rng.random(n) < 0.5
    if n:
        allowed[0] = True
    qd = torch.from_numpy(q).cuda()
    # (an empty index still gets a real one-word bitmap: the pieces must not read past zero tiles)
    md = torch.from_numpy(np.concatenate([oracle.mask_from_bool(allowed), np.zeros(1, np.uint64)]).view(np.int64)).cuda()
    cur = torch.cuda.current_stream()
    tail = torch.cuda.Stream()
    for masked in (False, True):
        ok = live & allowed if masked else live
        mask_ref = oracle.mask_from_bool(ok) if n else None
        mp_ = md.data_ptr() if masked else 0

        def ref(depth):
            if n == 0:
                return np.full((Bq, depth), -np.inf), np.full((Bq, depth), -1, np.int64)
            return oracle.c_search(stored, "bf16", qn, depth, mask_ref, row_offset=OFF)

        s_ref, r_ref = ref(KC)
        assert (r_ref[:, -1] == -1).all()  # fewer rows than kc: every scan pads
        for two_streams in (False, True):
            cand = torch.full((Bq, KC, 2), 7.0, dtype=torch.float64, device="cuda")
            bound = torch.full((Bq,), 7.0, dtype=torch.float64, device="cuda")
            if two_streams:
                ready = torch.cuda.Event()
                ready.record(cur)
                idx.search_shard(qd.data_ptr(), Bq, k, KC, OFF, cand.data_ptr(), bound.data_ptr(), mask_ptr=mp_,
                                 stream=cur.cuda_stream, tail_stream=tail.cuda_stream, q_ready_event=ready.cuda_event)
                tail.synchronize()
            else:
                idx.search_shard(qd.data_ptr(), Bq, k, KC, OFF, cand.data_ptr(), bound.data_ptr(), mask_ptr=mp_,
                                 stream=cur.cuda_stream)
            torch.cuda.synchronize()
            what = f"n={n} removed={removed} masked={masked} two_streams={two_streams}"
            s, r = _sorted(*_records(cand))
            np.testing.assert_array_equal(r, r_ref, err_msg=what)
            np.testing.assert_array_equal(s, s_ref, err_msg=what)
            assert np.isneginf(bound.cpu().numpy()).all(), what
            # ... and the merge over this one record: the oracle's top-k, no guard failure
            so = torch.empty((Bq, k), dtype=torch.float32, device="cuda")
            ro = torch.empty((Bq, k), dtype=torch.int64, device="cuda")
            kth = torch.empty(Bq, dtype=torch.float64, device="cuda")
            fail = torch.full((Bq,), 7, dtype=torch.int32, device="cuda")
            _native.merge_candidates(0, cand.data_ptr(), bound.data_ptr(), 1, Bq, KC, k, so.data_ptr(), ro.data_ptr(),
                                     kth.data_ptr(), fail.data_ptr(), stream=cur.cuda_stream)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ro.cpu().numpy(), r_ref[:, :k], err_msg=what)
            np.testing.assert_array_equal(so.cpu().numpy(), s_ref[:, :k].astype(np.float32), err_msg=what)
            assert (fail.cpu().numpy() == 0).all(), what
        # collect: kth -inf takes every live, allowed row; +inf takes none; a real k-th score takes at least the rows
        # at or above it (the window is kth - E wide) and nothing that is not a row of the shard
        kth_h = np.array([-np.inf, np.inf, s_ref[2, min(4, n - 1)] if ok.sum() > 4 else -np.inf, -np.inf, np.inf])
        kd = torch.from_numpy(kth_h).cuda()
        cand = torch.full((Bq, cap, 2), 7.0, dtype=torch.float64, device="cuda")
        bound = torch.full((Bq,), 7.0, dtype=torch.float64, device="cuda")
        idx.search_shard_collect(qd.data_ptr(), Bq, kd.data_ptr(), cap, OFF, cand.data_ptr(), bound.data_ptr(),
                                 mask_ptr=mp_, stream=cur.cuda_stream)
        torch.cuda.synchronize()
        s, r = _sorted(*_records(cand))
        s_all, r_all = ref(cap)
        what = f"collect n={n} removed={removed} masked={masked}"
        assert np.isneginf(bound.cpu().numpy()).all(), what
        for b in range(Bq):
            if np.isneginf(kth_h[b]):
                np.testing.assert_array_equal(r[b], r_all[b], err_msg=what)
                np.testing.assert_array_equal(s[b], s_all[b], err_msg=what)
            elif np.isposinf(kth_h[b]):
                assert (r[b] == -1).all() and np.isneginf(s[b]).all(), what
            else:
                got = r[b] >= 0
                must = r_all[b][s_all[b] >= kth_h[b]]
                assert np.isin(must, r[b][got]).all(), what
                exact = dict(zip(r_all[b].tolist(), s_all[b].tolist()))  # (cap > n: every live, allowed row)
                assert len(set(r[b][got].tolist())) == got.sum(), what
                assert all(row in exact and exact[row] == sc for row, sc in zip(r[b][got].tolist(), s[b][got].tolist())), what
                assert np.isneginf(s[b][~got]).all(), what
        # exact: the sorted exact top-m
        rec = torch.full((Bq, m, 2), 7.0, dtype=torch.float64, device="cuda")
        idx.search_shard_exact(qd.data_ptr(), Bq, m, OFF, rec.data_ptr(), mask_ptr=mp_, stream=cur.cuda_stream)
        torch.cuda.synchronize()
        s, r = _records(rec)
        s_m, r_m = ref(m)
        np.testing.assert_array_equal(r, r_m, err_msg=f"exact n={n} removed={removed} masked={masked}")
        np.testing.assert_array_equal(s, s_m, err_msg=f"exact n={n} removed={removed} masked={masked}")
    idx.close()


# ---------------------------------------------------------------- B2: 3 and 8 ranks on the kernels
def _rows(lo, hi):
    """Raw rows [lo, hi) of the ties corpus: the counter-based rows with [DUP_W) replaced by copies of row 77."""
    from oracle import ref_numpy as R

    x = R.gen_rows(SEED, lo, hi - lo, DIM)
    a, b = max(lo, DUP_W[0]), min(hi, DUP_W[1])
    if a < b:
        x[a - lo:b - lo] = R.gen_rows(SEED, 77, 1, DIM)[0]
    return x


def _wide_queries(cuts):
    from oracle import ref_numpy as R

    q = np.random.default_rng(3).standard_normal((B_W, DIM)).astype(np.float32)
    dup = R.gen_rows(SEED, 77, 1, DIM)[0]
    q[0] = dup                  # 2,201 equal scores
    q[4] = dup + 0.02 * np.linalg.norm(dup) / np.sqrt(DIM) * q[4]  # near-ties
    for i, row in enumerate(planted_rows(cuts)):  # each tiny shard owns a top-1
        q[6 + i] = R.gen_rows(SEED, row, 1, DIM)[0]
    return q


def _allowed():
    return np.random.default_rng(11).random(NT_W) < MASK_KEEP


def _wide_worker(rank, world, port, path, cuts):
    from datetime import timedelta

    import torch
    import torch.distributed as dist

    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    import oracle
    from hiprag import _native
    from hiprag.dist import ShardedSearch

    torch.cuda.set_device(0)
    lo, hi = cuts[rank], cuts[rank + 1]
    idx = _native.NativeIndex(DIM, "bf16", "cosine", device=0)
    if hi > lo:
        idx.add(_rows(lo, hi))
    assert idx.size() == (hi - lo, hi - lo)
    ss = ShardedSearch(idx, lo, max_batch=B_W, device=torch.device("cuda", 0), max_k=16)
    assert ss.kc == KC and ss.G == world
    q = torch.from_numpy(_wide_queries(cuts)).cuda()
    # this shard's slice of the row mask (bit r = local row r); an empty shard passes a real, all-zero word
    words = np.concatenate([oracle.mask_from_bool(_allowed()[lo:hi]), np.zeros(1, np.uint64)])
    mask = torch.from_numpy(words.view(np.int64)).cuda()
    out = {}
    for k in KS_W:
        s, r = ss.search(q, k)
        out[f"s{k}"], out[f"r{k}"] = s.cpu().numpy(), r.cpu().numpy()
    s, r = ss.search(q, 10, mask_ptr=mask.data_ptr())
    out["s_mask"], out["r_mask"] = s.cpu().numpy(), r.cpu().numpy()
    # a batch only the last rank knows, pipelined: broadcast first (src_rank), then the scan
    s3 = torch.empty((B_W, 10), dtype=torch.float32, device="cuda")
    r3 = torch.empty((B_W, 10), dtype=torch.int64, device="cuda")
    ss.finalize(ss.submit(q if rank == world - 1 else torch.zeros_like(q), 10, s_out=s3, r_out=r3, src_rank=world - 1))
    torch.cuda.synchronize()
    out["s_src"], out["r_src"] = s3.cpu().numpy(), r3.cpu().numpy()
    ss.close()
    dist.barrier()
    dist.destroy_process_group()  # the last collective is behind this rank
    out["fallback"], out["exact"] = ss.fallback_queries, ss.exact_queries
    out["gathers"], out["broadcasts"] = ss.collective_calls["all_gather"], ss.collective_calls["broadcast"]
    np.savez(f"{path}.{rank}.npz", **out)


@pytest.mark.parametrize("name", ["w3_ties_cross_both", "w3_tiny_and_empty", "w8_tiny_empty_ties"])
def test_wide_worlds_on_one_gpu_match_oracle(tmp_path, name):
    """3 / 8 ranks, one spawn per cut list with every k, the 60 % mask and the src_rank batch inside it.  Every
    rank's ids and score bits equal the oracle over the whole corpus; the tie queries took the collect fallback on
    every rank; k = 200 took the exhaustive pass for the whole batch; every rank issued the same number of
    collectives (an empty rank included)."""
    import torch.multiprocessing as mp

    import oracle
    from oracle import ref_numpy as R

    cuts = WIDE_CUTS[name]
    world = len(cuts) - 1
    assert world <= 8  # never more than 8 workers beside this process on the GPU
    stored = R.process_rows(_rows(0, NT_W), "cosine", "bf16")
    qn = R.process_queries(_wide_queries(cuts), "cosine")
    allowed = _allowed()
    # every shard that holds copies holds more than kc of them -- allowed ones too -- so the tie query fails its
    # guard with and without the mask: from the oracle over that shard's rows
    for m in (None, allowed):
        s_tie = oracle.c_search(stored, "bf16", qn[:1], 1, None if m is None else oracle.mask_from_bool(m))[0][0, 0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if max(a, DUP_W[0]) < min(b, DUP_W[1]):
                s_sh, r_sh = oracle.c_search(stored[a:b], "bf16", qn[:1], KC + 1,
                                             None if m is None else oracle.mask_from_bool(m[a:b]))
                assert r_sh[0, KC] >= 0 and s_sh[0, KC] == s_tie, (a, b)
    for i, row in enumerate(planted_rows(cuts)):
        assert oracle.c_search(stored, "bf16", qn[6 + i:7 + i], 1)[1][0, 0] == row
    path = str(tmp_path / name)
    mp.start_processes(_wide_worker, args=(world, _free_port(), path, cuts), nprocs=world, join=True,
                       start_method="spawn")
    refs = {k: oracle.c_search(stored, "bf16", qn, k) for k in KS_W}
    ref_mask = oracle.c_search(stored, "bf16", qn, 10, oracle.mask_from_bool(allowed))
    got = [np.load(f"{path}.{rank}.npz") for rank in range(world)]
    for rank, g in enumerate(got):
        for k in KS_W:
            np.testing.assert_array_equal(g[f"r{k}"], refs[k][1], err_msg=f"rank {rank} k={k}")
            np.testing.assert_array_equal(g[f"s{k}"], refs[k][0].astype(np.float32), err_msg=f"rank {rank} k={k}")
        np.testing.assert_array_equal(g["r_mask"], ref_mask[1], err_msg=f"rank {rank} masked")
        np.testing.assert_array_equal(g["s_mask"], ref_mask[0].astype(np.float32), err_msg=f"rank {rank} masked")
        np.testing.assert_array_equal(g["r_src"], refs[10][1], err_msg=f"rank {rank} src_rank batch")
        np.testing.assert_array_equal(g["s_src"], refs[10][0].astype(np.float32), err_msg=f"rank {rank} src_rank batch")
        assert list(g["r128"][0]) == [77] + list(range(DUP_W[0], DUP_W[0] + 127))
        assert int(g["fallback"]) >= 1 and int(g["exact"]) == B_W, (rank, int(g["fallback"]), int(g["exact"]))
        assert int(g["fallback"]) == int(got[0]["fallback"])
        assert (int(g["gathers"]), int(g["broadcasts"])) == (int(got[0]["gathers"]), 1), rank
