"""Ticket schedules of hiprag.dist.ShardedSearch (shared by tests/test_sharded_tickets_cpu.py and
tests/test_gpu_sharded_tickets.py): batches of distinct sizes over a corpus with more exact ties than any scan keeps
candidates, the schedules as lists of operations, a driver that checks every finalize against the oracle's answer for
that batch's own queries, k and mask, and -- for the CPU file -- a one-process ShardedSearch whose shard hooks are the
oracle with the kernels' contracts (the stand-ins of CpuTies in tests/test_dist_cpu.py, restated over
merge_ref: that file's are closures of its spawned workers).

A schedule is a list of operations on 1-based batch numbers:
  ("S", i, k[, "mask"])  submit batch i with that k (and the 60 % row mask)      ("F", i)  finalize batch i's ticket
  ("FA",)  finalize_all()                                                        ("C",)   close()
"""
import numpy as np
import torch

import oracle
from hiprag import _native
from hiprag.dist import ShardedSearch
from merge_ref import ref_merge, ref_merge_sorted
from oracle import ref_numpy as R

KC = 32                      # the pipelined candidate count of max_k = 16
N_TIES = 100                 # > KC and > kc_for_k(50) = 96
MASK_KEEP = 0.6

# 3 and 8 ranks over uneven, tiny and empty shards (tests/test_dist_cpu.py on the oracle stand-ins,
# tests/test_gpu_dist_shards.py on the kernels): NT_W rows cut at WIDE_CUTS[name], rows [DUP_W[0], DUP_W[1]) copies
# of row 77, an odd batch (the packed record of B * kc 16-byte candidates + B 8-byte bounds is then 8 mod 16 bytes
# long), every route of k: the pipelined kc, the scans at kc_for_k(100) and kc_for_k(128), the exhaustive pass
NT_W, DUP_W, B_W, KS_W = 6000, (2000, 4200), 11, (10, 100, 128, 200)
WIDE_CUTS = {
    # a 20-row shard (< kc = 32), an empty shard, a 10-row shard; the tie block covers shards 4 and 5 whole and
    # crosses the boundaries at 2100, 3000 and 4100
    "w8_tiny_empty_ties": [0, 700, 720, 720, 2100, 3000, 4100, 5990, 6000],
    "w3_ties_cross_both": [0, 2100, 4100, 6000],   # 100 copies left and right of the middle shard's 2,000
    "w3_tiny_and_empty": [0, 25, 25, 6000],
}


def planted_rows(cuts):
    """The middle row of every shard with fewer than 64 rows: a query equal to it makes that shard's candidates
    part of the answer, so a gather that loses or misplaces a tiny shard's record cannot go unnoticed."""
    return tuple((a + b) // 2 for a, b in zip(cuts[:-1], cuts[1:]) if 0 < b - a < 64)


SCHEDULES = {
    "a_out_of_order": [("S", 1, 10), ("S", 2, 10), ("F", 1), ("F", 2), ("F", 2), ("F", 1)],
    "b_beyond_kc_50": [("S", 1, 10), ("S", 2, 50), ("F", 1), ("F", 2)],
    "c_beyond_kc_128": [("S", 1, 10), ("S", 2, 128), ("F", 1), ("F", 2)],
    "d_beyond_max_k_200": [("S", 1, 10), ("S", 2, 200), ("F", 1), ("F", 2)],
    "e_slot_reuse": [("S", 1, 10), ("S", 2, 10), ("S", 3, 10), ("F", 1), ("F", 2), ("F", 3)],
    "f_finalize_all": [("S", 1, 10), ("FA",), ("F", 1), ("F", 1)],
    "g_masked_implicit": [("S", 1, 10, "mask"), ("S", 2, 50), ("F", 1), ("F", 2)],
    "h_close": [("S", 1, 10), ("C",), ("F", 1)],
}
E_DEPTH1 = [("S", 1, 10), ("S", 2, 10), ("F", 1), ("F", 2)]  # schedule e at depth 1: S2 takes S1's slot


def scan_kc(k: int, dim: int = 0):
    """The candidate count of the scan that answers k (None: beyond HR_MAX_K, the exhaustive pass)."""
    if k <= KC:
        return KC
    return _native.kc_for_k(k, dim) if k <= _native.HR_MAX_K else None


class Case:
    """A corpus with N_TIES copies of one row and three query batches (B distinct, own queries, the tie query at a
    different position in each).  stored: the oracle's rows; q[i]: what submit gets; qn[i]: the oracle's processed
    queries; mask: the 60 % row mask (bool) and its bitmap."""

    def __init__(self, stored, dtype, q, qn, tie_pos, tie_rows, seed=11):
        self.stored, self.dtype, self.q, self.qn = stored, dtype, q, qn
        self.tie_pos, self.tie_rows = tie_pos, np.asarray(tie_rows)
        n = stored.shape[0]
        self.allowed = np.random.default_rng(seed).random(n) < MASK_KEEP
        # the masked tie query must still fail its guard: more allowed ties than the scan keeps
        assert int(self.allowed[self.tie_rows].sum()) > KC
        self.mask = oracle.mask_from_bool(self.allowed)
        self._refs = {}

    def ref(self, i: int, k: int, masked: bool):
        """(scores f32, rows) of batch i (1-based) from the oracle, computed once."""
        key = (i, k, masked)
        if key not in self._refs:
            s, r = oracle.c_search(self.stored, self.dtype, self.qn[i - 1], k, self.mask if masked else None)
            s, r = s.astype(np.float32), r
            s.setflags(write=False)
            r.setflags(write=False)
            self._refs[key] = (s, r)
        return self._refs[key]

    def guard_failures(self, i: int, k: int, masked: bool, dim: int = 0) -> int:
        """Queries of batch i an exact scan's guard cannot settle, from the guard's definition on the oracle's
        scores: the scan returned kc rows (its bound, the kc-th score, is finite) and the k-th score does not
        exceed it.  0 for a k answered by the exhaustive pass."""
        kc = scan_kc(k, dim)
        if kc is None:
            return 0
        s, r = oracle.c_search(self.stored, self.dtype, self.qn[i - 1], kc, self.mask if masked else None)
        return int(((r[:, -1] >= 0) & ~(s[:, k - 1] > s[:, -1])).sum())


def batches(tie, sizes, tie_pos, seed=17):
    """One (B, dim) float32 query batch per size: random queries with the tie row's direction taken out -- the
    copies score the same against ANY query, so a query that ranked the block among its top rows would fail its
    guard too; these rank it mid-corpus -- and the tie row itself at position tie_pos."""
    rng = np.random.default_rng(seed)
    t = (tie / np.linalg.norm(tie)).astype(np.float64)
    out = []
    for B, p in zip(sizes, tie_pos):
        x = rng.standard_normal((B, len(tie)))
        x = (x - np.outer(x @ t, t)).astype(np.float32)
        x[p] = tie
        out.append(x)
    return out


def cpu_case() -> Case:
    """3,000 synthetic bf16 cosine rows of dim 96, rows 1000..1099 copies of row 1000; B = 3, 5, 8."""
    n, dim = 3000, 96
    stored = oracle.c_build_synthetic(5, 0, n, dim, "bf16", "cosine", 1)
    stored[1000:1000 + N_TIES] = stored[1000]
    tie = R.dequantize(stored[1000:1001], "bf16")[0]
    tie_pos = (0, 2, 7)
    q = [R.process_queries(x, "cosine") for x in batches(tie, (3, 5, 8), tie_pos)]
    return Case(stored, "bf16", q, q, tie_pos, np.arange(1000, 1000 + N_TIES))


def check(s, r, s_ref, r_ref):
    """Ids and score bits, -inf / -1 padding."""
    np.testing.assert_array_equal(r, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s[valid], s_ref[valid])
    assert np.all(np.isneginf(s[~valid]))


def run_schedule(ss, case: Case, ops, own_out: bool, to_dev, mask_ptr: int):
    """Drive ops on ss.  own_out: the caller passes s_out / r_out (finalize must hand back those very tensors);
    else submit allocates them.  to_dev(ndarray) -> the tensor submit gets.  Every ("F", i) is checked against
    case.ref of batch i.  Returns {batch: (k, masked)} of what was submitted."""
    tickets, outs, sub = {}, {}, {}
    for op in ops:
        if op[0] == "S":
            i, k = op[1], op[2]
            masked = len(op) > 3
            q = to_dev(case.q[i - 1])
            B = q.shape[0]
            kw = {}
            if own_out:
                outs[i] = (torch.full((B, k), 7.0, dtype=torch.float32, device=q.device),
                           torch.full((B, k), -7, dtype=torch.int64, device=q.device))
                kw = dict(s_out=outs[i][0], r_out=outs[i][1])
            tickets[i] = ss.submit(q, k, mask_ptr=mask_ptr if masked else 0, **kw)
            sub[i] = (k, masked)
        elif op[0] == "F":
            i = op[1]
            s, r = ss.finalize(tickets[i])
            if own_out:
                assert s is outs[i][0] and r is outs[i][1], f"batch {i}: finalize returned other tensors"
            k, masked = sub[i]
            assert tuple(s.shape) == (case.q[i - 1].shape[0], k) == tuple(r.shape), f"batch {i}: another batch's shape"
            check(s.cpu().numpy(), r.cpu().numpy(), *case.ref(i, k, masked))
        elif op[0] == "FA":
            ss.finalize_all()
        elif op[0] == "C":
            ss.close()
        else:
            raise ValueError(op)
    assert len(set(map(id, tickets.values()))) == len(tickets), "two batches share a ticket"
    return sub


class CpuSharded(ShardedSearch):
    """One process, no process group (G = 1), on the CPU: the shard pieces are the oracle with the kernels'
    contracts -- the scan honours kc= and its bound is the last candidate's score (ties at the boundary fail the
    guard), a collect window larger than its buffer returns the shard's exact top rows (bound -inf), the exhaustive
    pass returns the sorted exact top-m, the merges are merge_ref's.  masks: {mask_ptr: bitmap}; seen records what
    every hook was given."""

    def __init__(self, case: Case, masks=None, **kw):
        self.case, self.masks = case, masks or {}
        self.seen = {"scan_kc": [], "scan_B": [], "collect": [], "exact_m": [], "merge": []}
        super().__init__(index=None, row_offset=0, device=torch.device("cpu"), max_k=16, **kw)

    def _search(self, qt, m, mask_ptr):
        return oracle.c_search(self.case.stored, self.case.dtype, qt.numpy(), m,
                               self.masks[mask_ptr] if mask_ptr else None, nthreads=1)

    @staticmethod
    def _put(cand, s, r):
        cand.view(torch.int64)[..., 1] = torch.from_numpy(r)
        cand[..., 0] = torch.from_numpy(s)

    def _stream(self):
        return 0

    def _shard_search(self, qt, k, cand, bound, mask_ptr, q_ready=None, kc=None):
        kc = kc or self.kc
        self.seen["scan_kc"].append(kc)
        self.seen["scan_B"].append(int(qt.shape[0]))
        s, r = self._search(qt, kc, mask_ptr)
        self._put(cand, s, r)
        bound[:] = torch.from_numpy(np.where(r[:, -1] >= 0, s[:, -1], -np.inf))

    def _shard_collect(self, qt, kth, cap, cand, bound, mask_ptr):
        self.seen["collect"].append((int(qt.shape[0]), mask_ptr))
        s, r = self._search(qt, cap, mask_ptr)
        keep = s >= kth.numpy()[:, None]
        keep |= keep[:, -1:]  # the window reaches past the buffer: the shard's exact top-cap instead
        self._put(cand, np.where(keep, s, -np.inf), np.where(keep, r, -1))
        bound[:] = -np.inf

    def _shard_exact(self, qt, m, cand, mask_ptr):
        self.seen["exact_m"].append(m)
        self._put(cand, *self._search(qt, m, mask_ptr))

    def _merge(self, cand_all, bound_all, G, Bq, kc, k, s_out, r_out, kth, fail):
        self.seen["merge"].append((Bq, kc, k))
        s, r, kt, f = ref_merge(cand_all.numpy().reshape(G, Bq, kc, 2), bound_all.numpy().reshape(G, Bq), k)
        for dst, src in ((s_out, s), (r_out, r), (kth, kt), (fail, f)):
            dst.copy_(torch.from_numpy(src))

    def _merge_sorted(self, cand_all, G, Bq, m, k, s_out, r_out):
        s, r = ref_merge_sorted(cand_all.contiguous().numpy().reshape(G, Bq, m, 2), k)
        s_out.copy_(torch.from_numpy(s))
        r_out.copy_(torch.from_numpy(r))
