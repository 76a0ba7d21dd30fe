"""GPU: the shadow-8 FILTER's bias fold (hr_kernels.hpp: XFrag<F16, I8S>::get<false>, scan_body with BF) against the
restated bound (tests/shadow8_bias_ref.py) and the CPU oracle, the scan forced on with set_shadow8(2).

The MFMAs take the operand 1152 + s_d and the accumulators start at -C_q, so the partial sums carry 1152 times the
prefix sums of the query.  What can go wrong: a query whose elements do not cancel (all-positive, constant) against rows
at the ends of the int8 range, the start value of the wrong query in an accumulator register, a row of -C_q shared
between two batches in flight, the fallback body (1280 dims at 64 queries: no room in LDS) drifting from the fold's.
"""
import functools

import numpy as np
import pytest

import oracle
import shadow8_bias_ref as S
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

N_ROWS = 20_000
CUS16 = list(range(16))


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid].view(np.uint32), s_ref[valid].astype(np.float32).view(np.uint32))
    assert np.all(np.isneginf(s_gpu[~valid]))


# ---------------------------------------------------------------- bound per row
def _hostile_rows(n, dim):
    """Gaussian rows, and every fifth tile's first rows from the families at the ends of the int8 range: all elements
    equal (every int8 +127, or -127), alternating signs, an all-zero row."""
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    alt = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0).astype(np.float32)
    for t in range(0, n // 32, 5):
        rows[32 * t + 0] = 1.0
        rows[32 * t + 1] = -1.0
        rows[32 * t + 2] = alt
        rows[32 * t + 3] = 0.0
        rows[32 * t + 4] = np.abs(rows[32 * t + 4])
    return rows


def _hostile_queries(B, dim):
    rng = np.random.default_rng(1000 + dim)
    g = rng.standard_normal((B, dim))
    q = g.copy()
    fam = B // 8
    q[0 * fam:1 * fam] = np.abs(g[0 * fam:1 * fam])                      # all-positive
    q[1 * fam:2 * fam] = 1.0                                             # constant
    q[2 * fam:3 * fam] = 0.0
    q[2 * fam:3 * fam, 16:32] = np.abs(g[2 * fam:3 * fam, 16:32])        # one 16-block only
    q[3 * fam:4 * fam] = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0)    # alternating
    h = dim // 2
    q[4 * fam:5 * fam, :h] = np.abs(g[4 * fam:5 * fam, :h])              # exact zero sum
    q[4 * fam:5 * fam, h:2 * h] = -q[4 * fam:5 * fam, :h]
    q[4 * fam:5 * fam, 2 * h:] = 0.0
    q[5 * fam:6 * fam] = g[5 * fam:6 * fam] * 2.0 ** -(np.arange(dim) % 40)  # forty binades
    q[6 * fam:7 * fam] = -np.abs(g[6 * fam:7 * fam])                     # all-negative
    return q.astype(np.float32)                                          # the last eighth stays Gaussian


@pytest.mark.parametrize("B", [32, 64])
@pytest.mark.parametrize("dim", [64, 100, 128, 192, 768, 1024, 1280, 2048])
def test_every_row_within_the_returned_bound(native, dim, B):
    """debug_approx8 runs the scan's operand path (the fold, or at 1280 dims and 64 queries the subtracting fallback):
    |approx - exact| <= the returned E on every row, and the returned E is the restated one (old bound + bias term at
    the largest row scale; no term where the fallback runs) to 1e-9.  2048 dims plan 32-query groups and debug_approx8 stages the first group only, so
    its 64-query case checks the first 32 queries."""
    rows = _hostile_rows(N_ROWS, dim)
    q = _hostile_queries(B, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    idx.set_shadow8(2)
    approx, E = idx.debug_approx8(q)
    u = idx.shadow8_stats()["u_x8"]
    idx.close()
    xs = R.dequantize(R.process_rows(rows, "cosine", "bf16"), "bf16")
    qp = R.process_queries(q, "cosine")
    max_norm = float(np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1).max())) * (1.0 + 1e-12)
    e_ref, e_old, _ = S.guard_e8(qp, dim, max_norm, u, S.max_scale(xs), folded=S.fold_fits(dim, B))
    assert S.fold_fits(dim, B) == ((dim, B) != (1280, 64))
    nq = 32 if dim > 1280 else B
    exact = qp[:nq].astype(np.float64) @ xs.astype(np.float64).T
    slack = dim * 2.0 ** -52 * np.linalg.norm(qp[:nq].astype(np.float64), axis=1)[:, None] * \
        np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1))[None, :]
    err = (np.abs(approx[:nq].astype(np.float64) - exact) + slack).max(axis=1)
    print(f"BIAS8 dim {dim} B {B}: u_x8 {u:.3e}, max err/E {(err / E[:nq]).max():.3f}, "
          f"E/old E max {(e_ref / e_old).max():.4f} median {np.median(e_ref / e_old):.4f}")
    assert np.isfinite(approx[:nq]).all()
    assert np.all(err <= E[:nq]), (err, E)
    np.testing.assert_allclose(E, e_ref, rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------- searches
@functools.lru_cache(maxsize=2)
def _positive_corpus(n, dim):
    """All-positive rows (|Gaussian|), 64 all-positive queries planted on rows, the oracle's top 160 of each."""
    rng = np.random.default_rng(n + dim)
    rows = np.abs(rng.standard_normal((n, dim))).astype(np.float32)
    planted = rng.choice(n, 64, replace=False)
    q = (rows[planted] + 0.05 * np.abs(rng.standard_normal((64, dim)))).astype(np.float32)
    stored = R.process_rows(rows, "cosine", "bf16")
    qp = R.process_queries(q, "cosine")
    s_ref, r_ref = oracle.c_search(stored, "bf16", qp, 160)
    xs = R.dequantize(stored, "bf16")
    max_norm = float(np.sqrt((xs.astype(np.float64) ** 2).sum(axis=1).max())) * (1.0 + 1e-12)
    rows.setflags(write=False)
    return rows, q, qp, s_ref, r_ref, max_norm, S.max_scale(xs)


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("n,dim", [(40_000 + 13, 1024), (200_000 + 13, 64)])
def test_all_positive_searches_on_16_cus(native, n, dim, k):
    """16 CUs: every wave scans many tiles and refreshes in mid-scan.  Rows and score bits equal to the oracle's, one
    shadow-8 launch per batch, the replayed graph identical, and no guard failure among the queries whose reference
    gap s_k - s_kc8 exceeds 2 E (E from the restated bound, 0.1 % up as the steady-state file takes it)."""
    rows, q, qp, s_ref, r_ref, max_norm, max_scale = _positive_corpus(n, dim)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    idx.add(rows)
    idx.set_shadow8(2)
    idx.set_cu_mask(CUS16)
    try:
        l0, f0 = idx.shadow8_stats()["launches"], idx.stats()["guard_failures"]
        s, r = idx.search(q, k)
        st = idx.shadow8_stats()
        fails = idx.stats()["guard_failures"] - f0
        assert st["launches"] == l0 + 1
        _check(s, r, s_ref[:, :k], r_ref[:, :k])
        e = S.guard_e8(qp, dim, max_norm, st["u_x8"], max_scale, folded=S.fold_fits(dim, 64))[0] * (1.0 + 1e-3)
        kj = st["kc8"]
        assert k < kj <= 160
        qual = (r_ref[:, kj - 1] >= 0) & (s_ref[:, k - 1] - s_ref[:, kj - 1] > 2.0 * e)
        print(f"BIAS8 search {n}x{dim} k={k}: kc8 {kj}, {int(qual.sum())} of 64 qualify, {fails} guard failures")
        assert fails <= int((~qual).sum())
        s2, r2 = idx.search(q, k)  # the replayed graph
        assert idx.shadow8_stats()["launches"] == l0 + 2
        np.testing.assert_array_equal(r2, r)
        np.testing.assert_array_equal(s2.view(np.uint32), s.view(np.uint32))
    finally:
        idx.set_cu_mask(None)
        idx.close()


def test_pipelined_batches_do_not_share_the_bias_row(native):
    """Six batches back to back through ShardedSearch(depth=2), all-positive and Gaussian by turns: C_q of an
    all-positive query is ~30 000, of a Gaussian one a few hundred, so a row of -C_q read by the other batch in flight
    moves every score of that batch by far more than E."""
    import torch

    from hiprag.dist import ShardedSearch

    n, dim, B, k = 40_000 + 13, 1024, 64, 10
    rows, q_pos, _, s_pos, r_pos, _, _ = _positive_corpus(n, dim)
    rng = np.random.default_rng(5)
    q_gau = rng.standard_normal((B, dim)).astype(np.float32)
    s_gau, r_gau = oracle.c_search(R.process_rows(rows, "cosine", "bf16"), "bf16", R.process_queries(q_gau, "cosine"), k)
    idx = native.NativeIndex(dim, "bf16", "cosine", device=0)
    idx.add(rows)
    idx.set_shadow8(2)
    ss = ShardedSearch(idx, 0, max_batch=B, device=torch.device("cuda", 0), depth=2)
    try:
        qs = torch.from_numpy(np.stack([q_pos if i % 2 == 0 else q_gau for i in range(6)])).cuda()
        ready = torch.cuda.Event()
        ready.record()
        s = torch.empty((6, B, k), dtype=torch.float32, device="cuda")
        r = torch.empty((6, B, k), dtype=torch.int64, device="cuda")
        l0 = idx.shadow8_stats()["launches"]
        for i in range(6):
            ss.submit(qs[i], k, s_out=s[i], r_out=r[i], q_ready=ready)
        ss.finalize_all()
        torch.cuda.synchronize()
        assert idx.shadow8_stats()["launches"] == l0 + 6
        s, r = s.cpu().numpy(), r.cpu().numpy()
        for i in range(6):
            _check(s[i], r[i], (s_pos if i % 2 == 0 else s_gau)[:, :k], (r_pos if i % 2 == 0 else r_gau)[:, :k])
    finally:
        ss.close()
        idx.close()
