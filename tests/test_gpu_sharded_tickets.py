"""GPU: the ticket schedules of tests/test_sharded_tickets_cpu.py through the real kernels -- hiprag.dist.ShardedSearch
on one GPU with no process group, scan and tail streams on (depth 2), a ticket held across later submits, batches
of k = 10 followed by k = 50 / 128 (the synchronous scan above the pipelined kc) and k = 200 (every shard's exhaustive
pass) while a k = 10 batch is in flight.  Every finalize is compared with oracle.c_search of that batch's own queries,
k and mask: ids and score bits, -inf / -1 padding.

The corpus is the one of test_async_slots_out_of_order_and_fallback_before_mutation (tests/test_gpu_index.py): 6,000
rows, 100 of them copies of one row -- more ties than kc 32 or kc_for_k(50) = 96 keep, so each batch's tie query needs
the collect fallback.  The native guard_failures counter belongs to the single-index search (hr_index_search); on
this path the fallback is counted by ShardedSearch.fallback_queries, the exhaustive pass by stats()["exhaustive"].
"""
import numpy as np
import pytest

import oracle
import sharded_cpu as T
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

SIZES, TIE_POS = (7, 19, 33), (0, 5, 32)


def _case(native, dim, dtype):
    n = 6000
    raw = R.gen_rows(21, 0, n, dim)
    dups = np.sort(np.random.default_rng(5).choice(n, T.N_TIES, replace=False))
    raw[dups] = raw[dups[0]]
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.add(raw)
    q = T.batches(raw[dups[0]], SIZES, TIE_POS)
    case = T.Case(R.process_rows(raw, "cosine", dtype), dtype, q, [R.process_queries(x, "cosine") for x in q], TIE_POS,
                  dups)
    return idx, case


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


@pytest.fixture(scope="module")
def bf16(native):
    import torch

    idx, case = _case(native, 128, "bf16")
    mask_d = torch.from_numpy(case.mask.view(np.int64)).cuda()  # alive for the whole module
    yield idx, case, mask_d
    idx.close()


def _run(idx, case, mask_d, ops, own_out, dim, **kw):
    import torch

    from hiprag.dist import ShardedSearch

    ss = ShardedSearch(idx, 0, max_batch=64, max_k=16, device=torch.device("cuda", 0), **kw)
    assert ss.kc == T.KC and ss.G == 1 and (ss.tail is not None) == kw.get("overlap", True)
    st0 = idx.stats()
    try:
        sub = T.run_schedule(ss, case, ops, own_out, lambda a: torch.from_numpy(a).cuda(),
                             mask_d.data_ptr() if mask_d is not None else 0)
    finally:
        ss.close()
        torch.cuda.synchronize()
    st1 = idx.stats()
    # every tie query went through the collect fallback (the scans' guard may send others there too)
    want = sum(case.guard_failures(i, k, masked, dim) for i, (k, masked) in sub.items())
    print(f"fallback_queries {ss.fallback_queries} (tie queries {want}), exact_queries {ss.exact_queries}, "
          f"stats {st0} -> {st1}")
    assert ss.fallback_queries >= want
    return ss, sub, {key: st1[key] - st0[key] for key in st0}


def _path_asserts(name, ss, delta):
    if name in ("b_beyond_kc_50", "c_beyond_kc_128"):
        # batch 1's tie query took the collect fallback (batch 2's too at k = 50: 100 ties against kc 96)
        assert ss.fallback_queries >= 1
    if name == "b_beyond_kc_50":
        assert ss.fallback_queries >= 2
    if name == "d_beyond_max_k_200":
        assert ss.exact_queries == SIZES[1] and delta["exhaustive"] >= SIZES[1] and ss.fallback_queries >= 1


@pytest.mark.parametrize("own_out", [True, False], ids=["caller_outputs", "returned_outputs"])
@pytest.mark.parametrize("name", sorted(T.SCHEDULES))
def test_schedule(bf16, name, own_out):
    idx, case, mask_d = bf16
    ss, sub, delta = _run(idx, case, mask_d, T.SCHEDULES[name], own_out, 128, depth=2)
    _path_asserts(name, ss, delta)


@pytest.mark.parametrize("name", ["b_beyond_kc_50", "d_beyond_max_k_200", "e_slot_reuse"])
def test_schedule_without_the_tail_stream(bf16, name):
    idx, case, mask_d = bf16
    ss, sub, delta = _run(idx, case, mask_d, T.SCHEDULES[name], True, 128, depth=2, overlap=False)
    _path_asserts(name, ss, delta)


@pytest.mark.parametrize("own_out", [True, False], ids=["caller_outputs", "returned_outputs"])
def test_schedule_e_depth_1(bf16, own_out):
    idx, case, mask_d = bf16
    ss, _, _ = _run(idx, case, mask_d, T.E_DEPTH1, own_out, 128, depth=1)
    assert ss.fallback_queries >= 2


def test_schedule_b_f32_rows_dim_100(native):
    """f32 rows at dim 100 (padded to 128): both scans go through the 16-bit shadow, the one above kc while a shadow
    batch is in flight."""
    idx, case = _case(native, 100, "f32")
    try:
        ss, sub, delta = _run(idx, case, None, T.SCHEDULES["b_beyond_kc_50"], True, 100, depth=2)
        _path_asserts("b_beyond_kc_50", ss, delta)
    finally:
        idx.close()


def test_finalize_refuses_a_foreign_ticket(bf16):
    import torch

    from hiprag.dist import ShardedSearch

    idx, case, _ = bf16
    dev = torch.device("cuda", 0)
    a, b = (ShardedSearch(idx, 0, max_batch=64, max_k=16, device=dev) for _ in range(2))
    try:
        t = a.submit(torch.from_numpy(case.q[0]).cuda(), 10)
        for bad in (None, a.slots[0], t.result):
            with pytest.raises(ValueError):
                a.finalize(bad)
        with pytest.raises(ValueError):
            b.finalize(t)
        s, r = a.finalize(t)
        T.check(s.cpu().numpy(), r.cpu().numpy(), *case.ref(1, 10, False))
    finally:
        a.close()
        b.close()
