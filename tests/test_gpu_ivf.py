"""GPU parity of the IVF-flat candidate generation (hiprag.ivf, hr_ivf.hip; BASELINE config 5):
given the index's trained centroids and list assignment, the probed lists and the returned ids /
scores are identical to the oracle's IVF restatement (oracle/ref_numpy.ivf_search); with
nprobe = nlist the IVF search IS the exact search (identical to NativeIndex.search)."""
import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu


def _clustered(rng, n, dim, n_centers=40, spread=0.35):
    centers = rng.standard_normal((n_centers, dim)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    lab = rng.integers(0, n_centers, n)
    x = centers[lab] + spread * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    return x.astype(np.float32)


def _build(x, nlist, dtype, metric="cosine", chunk=1 << 18):
    import torch

    from hiprag.ivf import IvfIndex

    xd = torch.from_numpy(x).cuda()
    ivf = IvfIndex(x.shape[1], nlist, dtype=dtype, metric=metric)
    ivf.train(xd[:: max(1, len(x) // (nlist * 40))], iters=8, seed=1)
    ivf.build(len(x), lambda i, j: xd[i:j], chunk=chunk)
    return ivf


@pytest.mark.parametrize("dim,dtype,n,nlist,B,k", [(128, "bf16", 20000, 64, 32, 10), (96, "f16", 9000, 50, 17, 100),
                                                   (256, "f32", 6000, 24, 40, 32), (1024, "f16", 30000, 128, 64, 100),
                                                   (384, "bf16", 5000, 32, 20, 10), (768, "f16", 8000, 40, 33, 50),
                                                   (1100, "bf16", 3000, 16, 9, 10)])
def test_ivf_matches_oracle(dim, dtype, n, nlist, B, k):
    import torch

    rng = np.random.default_rng(dim + nlist)
    x = _clustered(rng, n, dim)
    ivf = _build(x, nlist, dtype, chunk=7000)  # several build chunks
    j = rng.choice(n, B // 2, replace=False)
    q = np.concatenate([x[j] + 0.02 * rng.standard_normal((len(j), dim)).astype(np.float32),
                        rng.standard_normal((B - len(j), dim)).astype(np.float32)]).astype(np.float32)
    stored = R.process_rows(x, "cosine", dtype)
    cent = ivf.centroids[:, :dim].cpu().numpy()
    row_list = ivf.lists_of_rows.cpu().numpy()
    for nprobe in (1, 5, nlist):
        qd = torch.from_numpy(q).cuda()
        cand = torch.empty((B, k, 2), dtype=torch.float64, device="cuda")
        bound = torch.empty(B, dtype=torch.float64, device="cuda")
        probes = torch.empty((B, nprobe, 2), dtype=torch.float64, device="cuda")
        ivf.search_candidates(qd, k, nprobe, cand, bound, probes=probes)
        torch.cuda.synchronize()
        s_ref, r_ref, p_ref = R.ivf_search(stored, dtype, R.process_queries(q, "cosine"), cent, row_list, nprobe, k)
        np.testing.assert_array_equal(probes.view(torch.int64)[..., 1].cpu().numpy(), p_ref)
        np.testing.assert_array_equal(cand.view(torch.int64)[..., 1].cpu().numpy(), r_ref)
        np.testing.assert_array_equal(cand[..., 0].cpu().numpy(), s_ref)
        assert torch.all(torch.isneginf(bound))
    # all lists probed: the IVF search is the exact search
    s, r = ivf.search(torch.from_numpy(q).cuda(), k, nlist)
    from hiprag import _native

    flat = _native.NativeIndex(dim, dtype, "cosine")
    flat.add(x)
    s_f, r_f = flat.search(q, k)
    np.testing.assert_array_equal(r.cpu().numpy(), r_f)
    np.testing.assert_array_equal(s.cpu().numpy(), s_f)


def test_ivf_ties_padding_dot_and_synthetic():
    """Duplicate rows tie-break by id, k beyond the visible rows pads with -1, dot metric, and the
    device synthetic build equals a host build of the same rows."""
    import torch

    from hiprag.ivf import IvfIndex

    rng = np.random.default_rng(7)
    dim, n, nlist = 64, 3000, 16
    x = _clustered(rng, n, dim, n_centers=8)
    dup = rng.choice(n, 50, replace=False)
    x[dup] = x[dup[0]]
    ivf = _build(x, nlist, "bf16", metric="ip")
    q = x[dup[:1]].copy()
    s_ref, r_ref, _ = R.ivf_search(R.process_rows(x, "ip", "bf16"), "bf16", q, ivf.centroids[:, :dim].cpu().numpy(),
                                   ivf.lists_of_rows.cpu().numpy(), 2, 700)
    s, r = ivf.search(torch.from_numpy(q).cuda(), 700, 2)
    np.testing.assert_array_equal(r.cpu().numpy(), r_ref)
    np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), s_ref.astype(np.float32).astype(np.float64))
    assert (r_ref[0] == -1).any()  # fewer visible rows than k
    # synthetic device build == host build of the same generator rows
    a = IvfIndex(dim, 8, dtype="f16")
    raw = R.gen_rows(3, 100, 4000, dim)
    a.train(torch.from_numpy(raw).cuda(), iters=4, seed=0)
    a.build_synthetic(3, 100, 4000)
    b = IvfIndex(dim, 8, dtype="f16")
    b.centroids = a.centroids.clone()
    rd = torch.from_numpy(raw).cuda()
    b.build(4000, lambda i, j: rd[i:j], id_offset=100)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.list_tiles, b.list_tiles)
    qq = torch.from_numpy(raw[:8] + 0.1).cuda()
    sa, ra = a.search(qq, 10, 3)
    sb, rb = b.search(qq, 10, 3)
    assert torch.equal(ra, rb) and torch.equal(sa, sb)
    assert int(ra.min()) >= 100


def test_ivf_sharded_search_tickets_and_k_limit():
    """hiprag.ivf.IvfShardedSearch on one GPU (no process group): search at k below and at the k it was built with,
    two batches in flight finalized out of order, a masked search, all identical to the oracle's IVF restatement over
    the index's own centroids and lists; nprobe = nlist is NativeIndex.search; a k above the built k is refused
    before any work, with the batch in flight left finalizable; no fallback ever runs (bounds are -inf)."""
    import torch

    from hiprag import _native
    from hiprag.ivf import IvfShardedSearch

    rng = np.random.default_rng(23)
    dim, n, nlist, K, nprobe = 64, 3000, 16, 40, 3
    x = _clustered(rng, n, dim, n_centers=12)
    ivf = _build(x, nlist, "bf16")
    stored = R.process_rows(x, "cosine", "bf16")
    cent = ivf.centroids[:, :dim].cpu().numpy()
    row_list = ivf.lists_of_rows.cpu().numpy()

    def queries(B):
        j = rng.choice(n, B // 2, replace=False)
        return np.concatenate([x[j] + 0.02 * rng.standard_normal((len(j), dim)).astype(np.float32),
                               rng.standard_normal((B - len(j), dim)).astype(np.float32)]).astype(np.float32)

    def same(got, q, k, npr=nprobe, lists=row_list):
        s, r = got
        s_ref, r_ref, _ = R.ivf_search(stored, "bf16", R.process_queries(q, "cosine"), cent, lists, npr, k)
        assert tuple(r.shape) == (len(q), k)
        np.testing.assert_array_equal(r.cpu().numpy(), r_ref)
        np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), s_ref.astype(np.float32).astype(np.float64))

    for bad in (0, 1025):
        with pytest.raises(ValueError, match="1024"):
            IvfShardedSearch(ivf, max_batch=32, k=bad, nprobe=nprobe)
    ss = IvfShardedSearch(ivf, max_batch=32, k=K, nprobe=nprobe)
    q9, q20 = queries(9), queries(20)
    d9, d20 = torch.from_numpy(q9).cuda(), torch.from_numpy(q20).cuda()
    for q, d in ((q9, d9), (q20, d20)):
        for k in (10, K):
            same(ss.search(d, k), q, k)
    # two batches in flight, finalized out of order (and once more: a ticket keeps its answer)
    ta, tb = ss.submit(d9, 10), ss.submit(d20, K)
    same(ss.finalize(tb), q20, K)
    same(ss.finalize(ta), q9, 10)
    same(ss.finalize(tb), q20, K)
    # k above the built k: refused before any work, what is in flight stays in flight
    t = ss.submit(d20, 10)
    for call in (ss.submit, ss.search):
        with pytest.raises(ValueError, match="41"):
            call(d9, K + 1)
    assert t.slot is not None and t.slot.ticket is t
    same(ss.finalize(t), q20, 10)
    # a masked search: the by-id row bitmap as the position mask hr_ivf_search reads (kept alive until finalize)
    allowed = rng.random(n) < 0.5
    words = oracle.mask_from_bool(allowed)
    md = torch.from_numpy(words.view(np.int64)).cuda()
    pm = torch.empty((ivf.n_positions + 31) // 32, dtype=torch.int32, device="cuda")
    _native.ivf_position_mask(ivf.ids.data_ptr(), ivf.n_positions, md.data_ptr(), len(words) * 64, pm.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    tm = ss.submit(d20, K, mask_ptr=pm.data_ptr())
    tu = ss.submit(d9, K)
    got = ss.finalize(tm)
    same(got, q20, K, lists=np.where(allowed, row_list, -1))
    assert allowed[got[1].cpu().numpy()[got[1].cpu().numpy() >= 0]].all()
    same(ss.finalize(tu), q9, K)
    assert ss.fallback_queries == 0 and ss.exact_queries == 0
    ss.close()
    # every list probed: the exact search
    full = IvfShardedSearch(ivf, max_batch=32, k=K, nprobe=nlist)
    s, r = full.search(d20, 10)
    flat = _native.NativeIndex(dim, "bf16", "cosine")
    flat.add(x)
    s_f, r_f = flat.search(q20, 10)
    np.testing.assert_array_equal(r.cpu().numpy(), r_f)
    np.testing.assert_array_equal(s.cpu().numpy(), s_f)
    assert full.fallback_queries == 0
    full.close()
    flat.close()
    ivf.close()
