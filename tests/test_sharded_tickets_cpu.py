"""CPU: the ticket protocol of hiprag.dist.ShardedSearch -- submit() returning a ticket, up to `depth` batches in flight,
finalize() / finalize_all() / close(), and a k above the pipelined kc answered synchronously -- driven the way
hiprag.rag.retriever._FusedRetrieve drives it: a ticket is held across later submits, and batches of different k (some
above kc = 32, one above HR_MAX_K) follow each other.  One process, no process group; the shard hooks are the oracle
with the kernels' contracts (tests/sharded_cpu.py), so only the host protocol is under test.

Every finalize is compared with oracle.c_search of that batch's own queries, k and mask: ids and score bits.  The
batches have B = 3, 5, 8 and their own queries, so another batch's answer has the wrong shape or the wrong ids; each
holds one query equal to a row the corpus has 100 copies of, whose guard fails at kc 32 and at kc_for_k(50) = 96 and
forces the collect fallback -- which must run once per batch, with the batch's own queries, k and mask.
"""
import importlib
import inspect
import pkgutil

import numpy as np
import pytest
import torch

import sharded_cpu as T
from hiprag import _native
from hiprag.dist import ShardedSearch


@pytest.fixture(scope="module")
def case():
    return T.cpu_case()


def _run(case, ops, own_out, depth=2):
    ptr = case.mask.ctypes.data
    ss = T.CpuSharded(case, masks={ptr: case.mask}, max_batch=8, depth=depth)
    assert ss.kc == T.KC and ss.G == 1 and not ss.collective and len(ss.slots) == depth
    sub = T.run_schedule(ss, case, ops, own_out, torch.from_numpy, ptr)
    ss.finalize_all()
    # the fallback ran exactly once for every query whose guard cannot hold, and for no other
    want = sum(case.guard_failures(i, k, masked) for i, (k, masked) in sub.items())
    assert ss.fallback_queries == want
    return ss, sub


def test_tie_queries_are_the_guard_failures(case):
    """What `guard_failures` counts is the tie query of each batch: one per batch at k = 10 (kc 32) and k = 50 (kc 96),
    masked or not, and none at k = 128 (kc 192 holds all 100 ties) or k = 200 (the exhaustive pass)."""
    assert T.scan_kc(10) == 32 and T.scan_kc(50) == 96 and T.scan_kc(128) == 192 and T.scan_kc(200) is None
    for i in (1, 2, 3):
        assert case.guard_failures(i, 10, False) == 1 and case.guard_failures(i, 10, True) == 1
        assert case.guard_failures(i, 50, False) == 1
        assert case.guard_failures(i, 128, False) == 0 and case.guard_failures(i, 200, False) == 0
        s, r = case.ref(i, 10, False)
        np.testing.assert_array_equal(r[case.tie_pos[i - 1]], case.tie_rows[:10])


@pytest.mark.parametrize("own_out", [True, False], ids=["caller_outputs", "returned_outputs"])
@pytest.mark.parametrize("name", sorted(T.SCHEDULES))
def test_schedule(case, name, own_out):
    ss, sub = _run(case, T.SCHEDULES[name], own_out)
    seen = ss.seen
    if name == "a_out_of_order":
        assert seen["scan_kc"] == [32, 32] and seen["scan_B"] == [3, 5]
        assert seen["collect"] == [(1, 0), (1, 0)] and ss.fallback_queries == 2
    elif name == "b_beyond_kc_50":
        # batch 1 is completed (its own fallback) before batch 2's synchronous scan at kc_for_k(50)
        assert seen["scan_kc"] == [32, 96] and seen["merge"][:2] == [(3, 32, 10), (1, 1024, 10)]
        assert ss.fallback_queries == 2 and ss.exact_queries == 0
    elif name == "c_beyond_kc_128":
        assert seen["scan_kc"] == [32, _native.kc_for_k(128)] and ss.fallback_queries == 1
    elif name == "d_beyond_max_k_200":
        assert seen["scan_kc"] == [32] and seen["exact_m"] == [200]
        assert ss.exact_queries == 5 and ss.fallback_queries == 1
    elif name == "e_slot_reuse":
        # S3 takes batch 1's slot: batch 1's fallback (one query of three) runs before batch 3's scan
        assert seen["scan_B"] == [3, 5, 8] and seen["merge"][:3] == [(3, 32, 10), (5, 32, 10), (1, 1024, 10)]
        assert ss.fallback_queries == 3
    elif name == "f_finalize_all":
        assert len(seen["collect"]) == 1 and ss.fallback_queries == 1
    elif name == "g_masked_implicit":
        # batch 1 was finalized by S2: its collect ran under ITS mask, batch 2's (unmasked) under none
        ptr = case.mask.ctypes.data
        assert seen["collect"] == [(1, ptr), (1, 0)] and seen["scan_kc"] == [32, 96]
    elif name == "h_close":
        assert len(seen["collect"]) == 1 and ss.fallback_queries == 1


@pytest.mark.parametrize("own_out", [True, False], ids=["caller_outputs", "returned_outputs"])
def test_schedule_e_depth_1(case, own_out):
    """One slot: S2 finalizes batch 1 to take its slot, and F1 afterwards is still batch 1's answer."""
    ss, _ = _run(case, T.E_DEPTH1, own_out, depth=1)
    assert ss.seen["merge"][:2] == [(3, 32, 10), (1, 1024, 10)] and ss.fallback_queries == 2


def test_finalize_refuses_what_is_not_its_ticket(case):
    a = T.CpuSharded(case, max_batch=8)
    b = T.CpuSharded(case, max_batch=8)
    q = torch.from_numpy(case.q[0])
    ta, tb, tb2 = a.submit(q, 10), b.submit(q, 10), b.submit(q, 50)
    for bad in (None, 0, a.slots[0], (ta.s_out, ta.r_out), tb, tb2):
        with pytest.raises(ValueError):
            a.finalize(bad)
    with pytest.raises(ValueError):
        b.finalize(ta)
    # the refusals finalized nothing (b's two: the k = 50 submit completed tb, then answered itself)
    assert a.fallback_queries == 0 and b.fallback_queries == 2 and ta.slot is not None
    s, r = a.finalize(ta)
    T.check(s.numpy(), r.numpy(), *case.ref(1, 10, False))
    s, r = b.finalize(tb2)
    T.check(s.numpy(), r.numpy(), *case.ref(1, 50, False))
    s, r = b.finalize(tb)
    T.check(s.numpy(), r.numpy(), *case.ref(1, 10, False))
    assert a.fallback_queries == 1 and b.fallback_queries == 2


def test_a_finalized_ticket_drops_its_queries(case):
    """The per-batch cost is the ticket: once finalized it holds the outputs only (no slot, no queries)."""
    ss = T.CpuSharded(case, max_batch=8)
    t = ss.submit(torch.from_numpy(case.q[1]), 10)
    assert t.slot is ss.slots[0] and t.q is not None
    ss.finalize(t)
    assert t.slot is None and t.q is None and ss.slots[0].ticket is None


# ---------------------------------------------------------------- the hooks' signatures
def _args(n):
    return tuple(object() for _ in range(n))


# hook -> the argument lists ShardedSearch passes it, one (args, kwargs) per form of call in hiprag/dist.py
# (submit and search: as ShardedSearch.search and hiprag.rag.retriever call them)
HOOK_CALLS = {
    "_stream": [((), {})],
    "_shard_search": [(_args(6), {}),                      # submit: q, k, cand, bound, mask_ptr, q_ready
                      (_args(5), {"kc": 96})],             # _submit_beyond_kc: q, k, cand, bound, mask_ptr, kc=
    "_shard_collect": [(_args(6), {})],                    # q, kth, cap, cand, bound, mask_ptr
    "_shard_exact": [(_args(4), {})],                      # q, m, cand, mask_ptr
    "_merge": [(_args(10), {})],                           # cand_all, bound_all, G, B, kc, k, s_out, r_out, kth, fail
    "_merge_sorted": [(_args(7), {})],                     # cand_all, G, B, m, k, s_out, r_out
    "_all_gather": [(_args(2), {})],                       # out, inp
    "_on_tail": [(_args(1), {})],                          # issue
    "_broadcast": [(_args(2), {})],                        # t, src
    "_exchange_and_merge": [(_args(7), {})],               # slot, rec, L, B, k, s_out, r_out
    "_failed_queries": [(_args(2), {})],                   # slot, B
    "_submit_beyond_kc": [(_args(6), {})],                 # q, k, s_out, r_out, mask_ptr, src_rank
    "_exact": [(_args(6), {})],                            # q, k, which, s_out, r_out, mask_ptr
    "_fallback": [(_args(7), {})],                         # q, k, failed, kth, s_out, r_out, mask_ptr
    "submit": [(_args(5), {"src_rank": None}), (_args(2), {}),
               (_args(2), {"s_out": 0, "r_out": 0, "mask_ptr": 0, "q_ready": None})],
    "finalize": [(_args(1), {})],
    "finalize_all": [((), {})],
    "search": [(_args(2), {}), (_args(2), {"s_out": 0, "r_out": 0, "mask_ptr": 0, "src_rank": None})],
    "close": [((), {})],
}


def _package_subclasses():
    import hiprag

    for m in pkgutil.walk_packages(hiprag.__path__, "hiprag."):
        if m.module_finder.find_spec(m.name).origin.endswith(".py"):  # (not the shared libraries beside them)
            importlib.import_module(m.name)
    out, todo = [], [ShardedSearch]
    while todo:
        for c in todo.pop().__subclasses__():
            todo.append(c)
            if c.__module__.split(".")[0] == "hiprag":
                out.append(c)
    return out


def test_the_table_is_the_base_class():
    """Every method a subclass could override is in the table, and the base class accepts every listed call."""
    methods = {n for n, v in vars(ShardedSearch).items() if inspect.isfunction(v) and n != "__init__"}
    assert methods == set(HOOK_CALLS)
    for name, calls in HOOK_CALLS.items():
        for args, kwargs in calls:
            inspect.signature(getattr(ShardedSearch, name)).bind(object(), *args, **kwargs)


def test_subclass_hooks_accept_the_base_class_calls():
    subs = _package_subclasses()
    assert "IvfShardedSearch" in {c.__name__ for c in subs}
    bad = []
    for cls in subs:
        for name, calls in HOOK_CALLS.items():
            if name not in vars(cls):
                continue
            for args, kwargs in calls:
                try:
                    inspect.signature(vars(cls)[name]).bind(object(), *args, **kwargs)
                except TypeError as e:
                    bad.append(f"{cls.__module__}.{cls.__name__}.{name}{inspect.signature(vars(cls)[name])}: {e}")
    assert not bad, "\n".join(bad)
