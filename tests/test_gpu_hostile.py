"""GPU: store, guard premise and search parity on corpora that are not isotropic Gaussians (tests/hostile_data.py).

The rest of the suite sweeps shapes, batch sizes, k, masks and FILTER forms over Gaussian rows.  Here the values vary:
a shared mean direction with outlier dimensions (every score in one band, many rows inside the guard window), one-sided
rows (no cancellation of accumulation errors), sparse rows (almost every score exactly 0: tie order decides), elements
over forty binades (f16 subnormals, row norms over 2^-10 .. 2^7) and a cluster of distinct near-duplicates whose exact
scores differ by less than the guard's additive constant.  tests/test_hostile_data_cpu.py pins those properties.

Bar, as everywhere: rows equal to the oracle's, score bits equal, -inf / -1 padding; |approx - exact| <= E for every
row.  The counters printed per case (main passes / guard failures / exhaustive passes) are observations,
asserted only where the input forces them: a query whose scores all tie (the all-zero query under cosine / ip) and the
near-duplicate cluster cannot be certified by any correct guard, so a fallback must have run."""
import functools

import numpy as np
import pytest

import hostile_data as H
import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

N = 20_011
DTYPES = ("bf16", "f16", "f32")
METRICS = ("cosine", "ip", "l2")


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


@functools.lru_cache(maxsize=2)
def _corpus(family, n, dim, metric, dtype):
    """(rows, member positions, centre); only the near-duplicate cluster depends on the dtype, only `wide` on the metric."""
    rows, pos, centre = H.corpus(family, 1, n, dim, metric, dtype)
    rows.setflags(write=False)
    return rows, pos, centre


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid], s_ref[valid].astype(np.float32))
    assert np.all(np.isneginf(s_gpu[~valid]))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- store
@pytest.mark.parametrize("dtype", DTYPES)
def test_store_quantiser_edges(native, dtype):
    """The quantisers' edge table (tests/test_oracle.py::test_quantizers_edge_values) and the f16 subnormal boundary
    (+-2^-14, +-2^-24, +-2^-25: the tie to zero, and the first value above it) through the device store, every value in
    every lane position: the stored bits are the oracle's.  (Raw ip rows; holds inf, so the index is never searched.)"""
    v = np.array([0.0, -0.0, 1e-40, -1e-40, 6e-8, 3e-8, 2.98e-8, 65504, 65519, 65520, 1e30, -1e30, np.inf, -np.inf,
                  1.0 + 2 ** -8, 1.0 + 3 * 2 ** -9, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25,
                  -2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23)], np.float32)
    rows = np.stack([np.roll(np.resize(v, 64), i) for i in range(len(v))])
    idx = native.NativeIndex(64, dtype, "ip")
    idx.add(rows)
    got = idx.get_rows(np.arange(len(rows)))
    ref = R.dequantize(R.quantize(rows, dtype), dtype)
    np.testing.assert_array_equal(_bits(got), _bits(ref))
    idx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_store_cosine_zero_rows_wide_and_scale(native, dtype):
    """Cosine store: the all-zero rows of the sparse family stay zero, the forty-binade rows are the oracle's bits
    (elements that normalise to f16 subnormals included), and rows multiplied by 2^(+-60) store the same bits as the
    rows themselves."""
    dim = 512
    sp = _corpus("sparse", N, dim, "cosine", dtype)[0]
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.add(sp)
    assert not _bits(idx.get_rows(H.sparse_zero_rows(N))).any()
    np.testing.assert_array_equal(_bits(idx.get_rows(np.arange(N))),
                                  _bits(R.dequantize(R.process_rows(sp, "cosine", dtype), dtype)))
    idx.close()
    wd = _corpus("wide", N, dim, "cosine", dtype)[0]
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.add(wd)
    np.testing.assert_array_equal(_bits(idx.get_rows(np.arange(N))),
                                  _bits(R.dequantize(R.process_rows(wd, "cosine", dtype), dtype)))
    idx.close()
    an = _corpus("anisotropic", N, dim, "cosine", dtype)[0]
    scale = np.where(np.arange(N) % 2 == 0, 2.0 ** 60, 2.0 ** -60).astype(np.float32)[:, None]
    ref = R.dequantize(R.process_rows(an, "cosine", dtype), dtype)
    for x in (an, an * scale):
        idx = native.NativeIndex(dim, dtype, "cosine")
        idx.add(x)
        np.testing.assert_array_equal(_bits(idx.get_rows(np.arange(N))), _bits(ref))
        idx.close()


# ---------------------------------------------------------------- guard premise
@pytest.mark.parametrize("dim,B", [(512, 48), (200, 7)])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", H.FAMILIES[:4])
def test_approx_error_within_guard_bound(native, family, dtype, metric, dim, B):
    """|approximate scan score - exact score| <= E_q on every row (the premise of the exactness guard, DESIGN.md
    "Exactness guard"), inner product and euclidean (scan score 2 q.x - |x|^2), on the four value families.
    The exact side is an fp64 matrix product; its own rounding (any summation order: at most dim 2^-52 |q||x|) is added
    to the error before the comparison, so the test asks no less than the canonical sum would."""
    rows = _corpus(family, N, dim, metric, dtype)[0]
    q, _ = H.queries(family, 2, rows, B, metric)
    idx = native.NativeIndex(dim, dtype, metric)
    idx.add(rows)
    approx, E = idx.debug_approx(q)
    idx.close()
    xs = R.dequantize(R.process_rows(rows, metric, dtype), dtype).astype(np.float64)
    qd = R.process_queries(q, metric).astype(np.float64)
    exact = qd @ xs.T
    xn = np.sqrt((xs * xs).sum(axis=1))
    slack = dim * 2.0 ** -52 * np.linalg.norm(qd, axis=1)[:, None] * xn[None, :]
    if metric == "l2":
        exact = 2.0 * exact - (xn * xn)[None, :]
        slack = 2.0 * slack + dim * 2.0 ** -52 * (xn * xn)[None, :]
    assert approx.shape == exact.shape and np.isfinite(approx).all()
    err = (np.abs(approx.astype(np.float64) - exact) + slack).max(axis=1)
    nz = np.abs(q).sum(axis=1) > 0  # (the all-zero query: err = 0, E = the additive constant alone)
    print(f"GUARD {family} {dtype} {metric} dim={dim}: max err = {err.max():.3e}, min E = {E[nz].min():.3e}, "
          f"max err/E = {(err / E).max():.3f}")
    assert np.all(err <= E), (err, E)


# ---------------------------------------------------------------- search parity through every FILTER form
def _f16_ok(family, dtype, metric):
    return dtype != "f16" or metric == "cosine" or family in ("anisotropic", "nonneg", "wide")


SEARCH_COMBOS = [(f, d, m) for f in H.FAMILIES for d in DTYPES for m in METRICS if _f16_ok(f, d, m)]
PLAN_512 = [(33, 10), (33, 40), (100, 10), (100, 40), (200, 10)]


def _parity(native, family, dtype, metric, dim, plan):
    """Every (B, k) of `plan` three ways -- unmasked, a 60 % random mask, a contiguous seventh of the rows removed --
    against one oracle search per way (a prefix of a batch is a batch of the same make, and the top-k is a prefix of
    the top-40).  Returns the counters' increase."""
    rows, pos, centre = _corpus(family, N, dim, metric, dtype)
    Bmax, kmax = max(b for b, _ in plan), max(k for _, k in plan)
    q, _ = H.queries(family, 3, rows, Bmax, metric, centre)
    stored = R.process_rows(rows, metric, dtype)
    qp = R.process_queries(q, metric)
    idx = native.NativeIndex(dim, dtype, metric)
    idx.add(rows)
    rng = np.random.default_rng(dim + len(family))
    allowed = rng.random(N) < 0.6
    live = np.ones(N, bool)
    live[H.remove_range(N)] = False
    start = idx.stats()
    for way in ("all", "mask", "removed"):
        if way == "removed":
            idx.remove(H.remove_range(N))
        eff = {"all": None, "mask": allowed, "removed": live}[way]
        mk = oracle.mask_from_bool(allowed) if way == "mask" else None
        s_ref, r_ref = oracle.c_search(stored, dtype, qp, kmax, None if eff is None else oracle.mask_from_bool(eff),
                                       metric=metric)
        lowest = np.arange(N) if eff is None else np.nonzero(eff)[0]
        for B, k in plan:
            n_parts = (native.kc_for_k(k, dim) + 31) // 32
            st0, w0, x0 = idx.stats(), idx.wide_launches(), idx.q256_launches()
            s, r = idx.search(q[:B], k, mk)
            _check(s, r, s_ref[:B, :k], r_ref[:B, :k])
            st1 = idx.stats()
            fell_back = st1["guard_failures"] > st0["guard_failures"] or st1["exhaustive"] > st0["exhaustive"]
            if way == "all":  # the form of FILTER the plan takes (tests/test_gpu_index.py::test_wide_filter_vs_oracle)
                if B <= 64:
                    assert idx.wide_launches() == w0 and idx.q256_launches() == x0
                elif B > 128 and n_parts == 1:
                    assert idx.q256_launches() == x0 + 1
                else:
                    assert idx.wide_launches() > w0 and idx.q256_launches() == x0
            if family == "neardup":
                # 200 distinct rows within 1e-9 of each other: no guard can certify k of them from <= 64 candidates
                assert st1["guard_failures"] > st0["guard_failures"], (way, B, k)
                assert np.isin(r[0], pos).all()
            elif metric != "l2":
                # the all-zero query: every score ties at 0, the answer is the lowest allowed rows, by a fallback
                np.testing.assert_array_equal(r[H.ZERO_AT], lowest[:k])
                assert not s[H.ZERO_AT].any()
                assert fell_back, (way, B, k)
    end = idx.stats()
    idx.close()
    return {key: end[key] - start[key] for key in end}


@pytest.mark.parametrize("family,dtype,metric", SEARCH_COMBOS, ids=lambda v: str(v))
def test_search_parity_dim512(native, family, dtype, metric):
    """33 queries (k_scan), 100 queries (the 128-query FILTER, one and two row parts) and 200 queries (the 256-query
    FILTER) at k = 10 / 40, each unmasked, masked and after a removal: ids and score bits equal to the oracle.
    (Under l2 the all-zero query scores 1 - |x|^2, an ordinary ranking by norm: checked against the oracle like any
    other query, with no counter condition.)"""
    d = _parity(native, family, dtype, metric, 512, PLAN_512)
    print(f"FALLBACK {family} {dtype} {metric} dim=512: main_passes / guard_failures / exhaustive = "
          f"{d['main_passes']} / {d['guard_failures']} / {d['exhaustive']}")


@pytest.mark.parametrize("family", H.FAMILIES)
def test_search_parity_dim256_q256(native, family):
    """200 queries at dim 256: the 32x32x16 form of the 256-query FILTER."""
    d = _parity(native, family, "bf16", "cosine", 256, [(200, 10)])
    print(f"FALLBACK {family} bf16 cosine dim=256: main_passes / guard_failures / exhaustive = "
          f"{d['main_passes']} / {d['guard_failures']} / {d['exhaustive']}")


# ---------------------------------------------------------------- sharded and persistent forms
def test_two_shards_and_merge_anisotropic(native):
    """Two row shards (search_shard) + the device merge on the anisotropic family, bf16: wherever the merged guard
    holds, ids and bits are the oracle's; the all-zero query (every score ties) must be flagged for the fallback, and the
    one-index synchronous search answers every query, flagged or not, as the oracle does."""
    torch = pytest.importorskip("torch")
    dim, B, k, kc, cut = 512, 24, 10, 32, 9_003
    rows = _corpus("anisotropic", N, dim, "cosine", "bf16")[0]
    q, _ = H.queries("anisotropic", 4, rows, B)
    s_ref, r_ref = oracle.c_search(R.process_rows(rows, "cosine", "bf16"), "bf16", R.process_queries(q, "cosine"), k)
    shards = [native.NativeIndex(dim, "bf16", "cosine") for _ in range(2)]
    shards[0].add(rows[:cut])
    shards[1].add(rows[cut:])
    qd = torch.from_numpy(q).cuda()
    st = torch.cuda.current_stream().cuda_stream
    cand = torch.empty((2, B, kc, 2), dtype=torch.float64, device="cuda")
    bounds = torch.empty((2, B), dtype=torch.float64, device="cuda")
    for g, (sh, off) in enumerate(zip(shards, [0, cut])):
        sh.search_shard(qd.data_ptr(), B, k, kc, off, cand[g].data_ptr(), bounds[g].data_ptr(), stream=st)
    sd = torch.empty((B, k), dtype=torch.float32, device="cuda")
    rd = torch.empty((B, k), dtype=torch.int64, device="cuda")
    kth = torch.empty(B, dtype=torch.float64, device="cuda")
    fail = torch.empty(B, dtype=torch.int32, device="cuda")
    native.merge_candidates(0, cand.data_ptr(), bounds.data_ptr(), 2, B, kc, k, sd.data_ptr(), rd.data_ptr(),
                            kth.data_ptr(), fail.data_ptr(), stream=st)
    torch.cuda.synchronize()
    ok = fail.cpu().numpy() == 0
    print(f"SHARDS anisotropic bf16: merged guard held for {int(ok.sum())} of {B} queries")
    assert not ok[H.ZERO_AT]
    assert ok.any()
    np.testing.assert_array_equal(rd.cpu().numpy()[ok], r_ref[ok])
    np.testing.assert_array_equal(sd.cpu().numpy()[ok], s_ref[ok].astype(np.float32))
    full = native.NativeIndex(dim, "bf16", "cosine")
    full.add(rows)
    _check(*full.search(q, k), s_ref, r_ref)
    for h in shards + [full]:
        h.close()


def test_persistent_filter_anisotropic(native):
    """The persistent FILTER (forced, mode 2) on the anisotropic family, bf16: three pipelined batches over its three
    workspaces, each with an all-zero query whose fallback runs beside the instance; every batch identical to the
    oracle.  (The persistent FILTER needs the early SAMPLE, which a shard gets from 16384 tiles on: this one case uses
    524,299 rows at dim 256 instead of the 20,011 of the rest.)"""
    torch = pytest.importorskip("torch")
    from hiprag.dist import ShardedSearch

    n, dim, B, k, nb = 524_299, 256, 64, 10, 3
    rng = np.random.default_rng(5)
    mu, hot = H.aniso_frame(dim)
    rows = rng.standard_normal((n, dim), dtype=np.float32) * np.float32(0.5 / np.sqrt(dim)) + mu.astype(np.float32)
    rows[:, hot] *= np.float32(20.0)
    q = np.stack([H.queries("anisotropic", 10 + i, rows, B)[0] for i in range(nb)])
    stored = oracle.c_quantize(oracle.c_normalize_rows(rows), "bf16")
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q.reshape(nb * B, dim), "cosine"), k)
    idx = native.NativeIndex(dim, "bf16", "cosine")
    try:
        idx.add(rows)
        idx.set_persist(2)
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(q).to(dev)
        ready = torch.cuda.Event()
        ready.record()
        ss = ShardedSearch(idx, 0, max_batch=B, device=dev, max_k=k)
        s = torch.empty((nb, B, k), dtype=torch.float32, device=dev)
        r = torch.empty((nb, B, k), dtype=torch.int64, device=dev)
        b0, g0 = idx.persist_stats()["batches"], idx.stats()
        for i in range(nb):
            ss.submit(qd[i], k, s_out=s[i], r_out=r[i], q_ready=ready)
        ss.finalize_all()
        torch.cuda.synchronize()
        st, g1 = idx.persist_stats(), idx.stats()
        assert st["error"] == 0 and st["batches"] - b0 == nb
        _check(s.cpu().numpy().reshape(nb * B, k), r.cpu().numpy().reshape(nb * B, k), s_ref, r_ref)
        np.testing.assert_array_equal(r.cpu().numpy()[:, H.ZERO_AT], np.tile(np.arange(k), (nb, 1)))
        assert g1["guard_failures"] > g0["guard_failures"] or g1["exhaustive"] > g0["exhaustive"]
    finally:
        idx.close()


# ---------------------------------------------------------------- IVF
def test_ivf_sparse_matches_oracle():
    """IVF-flat on the sparse family: the candidate top-k (k_topk_cand) faces records that are almost all exactly 0
    (and half of the rest negative, below them), so zeros decide the tail of a top-k by (score desc, id asc); the
    all-zero query ties every list and every row.  Probes, ids and scores identical to the oracle's IVF restatement;
    all lists probed == the flat search."""
    import torch

    from hiprag import _native
    from hiprag.ivf import IvfIndex

    dim, nlist, B, k, dtype = 512, 64, 16, 10, "bf16"
    x = _corpus("sparse", N, dim, "cosine", dtype)[0]
    xd = torch.from_numpy(x.copy()).cuda()
    ivf = IvfIndex(dim, nlist, dtype=dtype, metric="cosine")
    ivf.train(xd[:: max(1, N // (nlist * 40))], iters=8, seed=1)
    ivf.build(N, lambda i, j: xd[i:j], chunk=7000)
    q, _ = H.queries("sparse", 5, x, B)
    qp = R.process_queries(q, "cosine")
    stored = R.process_rows(x, "cosine", dtype)
    cent = ivf.centroids[:, :dim].cpu().numpy()
    row_list = ivf.lists_of_rows.cpu().numpy()
    qd = torch.from_numpy(q).cuda()
    for nprobe in (1, 5, nlist):
        cand = torch.empty((B, k, 2), dtype=torch.float64, device="cuda")
        bound = torch.empty(B, dtype=torch.float64, device="cuda")
        probes = torch.empty((B, nprobe, 2), dtype=torch.float64, device="cuda")
        ivf.search_candidates(qd, k, nprobe, cand, bound, probes=probes)
        torch.cuda.synchronize()
        s_ref, r_ref, p_ref = R.ivf_search(stored, dtype, qp, cent, row_list, nprobe, k)
        np.testing.assert_array_equal(probes.view(torch.int64)[..., 1].cpu().numpy(), p_ref)
        np.testing.assert_array_equal(cand.view(torch.int64)[..., 1].cpu().numpy(), r_ref)
        np.testing.assert_array_equal(cand[..., 0].cpu().numpy(), s_ref)
    assert (s_ref[H.ZERO_AT] == 0).all()
    s, r = ivf.search(qd, k, nlist)
    flat = _native.NativeIndex(dim, dtype, "cosine")
    flat.add(x)
    s_f, r_f = flat.search(q, k)
    np.testing.assert_array_equal(r.cpu().numpy(), r_f)
    np.testing.assert_array_equal(s.cpu().numpy(), s_f)
    flat.close()
