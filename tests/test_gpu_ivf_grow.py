"""GPU: growable IVF lists (hiprag.ivf.IvfIndex.add / add_from / remove / compact / save / load over
hr_ivf_search_ext, hr_index_copy_rows, hr_ivf_position_mask).  Every comparison is exact: the results are the
oracle's IVF restatement (oracle/ref_numpy.ivf_search) over the rows stored so far, with the index's own
centroids and list assignment; removed rows have list -1 there, which makes them invisible."""
import numpy as np
import pytest

import oracle  # noqa: F401
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

NLIST = 16


def _clustered(rng, n, dim, n_centers=40, spread=0.35):
    centers = rng.standard_normal((n_centers, dim)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    lab = rng.integers(0, n_centers, n)
    x = centers[lab] + spread * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    return x.astype(np.float32)


def _tile_rot(t):
    return ((int(t) * 0x9E3779B1) & 0xFFFFFFFF) >> 27


def _queries(rng, x, B):
    j = rng.choice(len(x), B // 2, replace=False)
    return np.concatenate([x[j] + 0.02 * rng.standard_normal((len(j), x.shape[1])).astype(np.float32),
                           rng.standard_normal((B - len(j), x.shape[1])).astype(np.float32)]).astype(np.float32)


def _search(ivf, q, k, nprobe):
    import torch

    B = len(q)
    cand = torch.empty((B, k, 2), dtype=torch.float64, device="cuda")
    bound = torch.empty(B, dtype=torch.float64, device="cuda")
    probes = torch.empty((B, nprobe, 2), dtype=torch.float64, device="cuda")
    ivf.search_candidates(torch.from_numpy(q).cuda(), k, nprobe, cand, bound, probes=probes)
    torch.cuda.synchronize()
    assert torch.all(torch.isneginf(bound))
    return (cand[..., 0].cpu().numpy(), cand.view(torch.int64)[..., 1].cpu().numpy(),
            probes.view(torch.int64)[..., 1].cpu().numpy())


def _check_against_oracle(ivf, stored, dtype, q, n, nprobes=(1, 3, NLIST), ks=(10, 100)):
    """The index against the restatement over rows [0, n) (ids = row numbers), probes included."""
    cent = ivf.centroids[:, : ivf.dim].cpu().numpy()
    row_list = ivf.lists_of_rows.cpu().numpy()
    assert len(row_list) == n
    pq = R.process_queries(q, "cosine")
    out = {}
    for nprobe in nprobes:
        # one restatement per nprobe: its order is total, so the top-k of a smaller k is a prefix
        s_ref, r_ref, p_ref = R.ivf_search(stored[:n], dtype, pq, cent, row_list, nprobe, max(ks))
        for k in ks:
            s, r, p = _search(ivf, q, k, nprobe)
            np.testing.assert_array_equal(p, p_ref)
            np.testing.assert_array_equal(r, r_ref[:, :k])
            np.testing.assert_array_equal(s, s_ref[:, :k])
            out[nprobe, k] = (s, r)
    return out


# ---------------------------------------------------------------- hr_index_copy_rows
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("dim", [96, 128, 1100])
def test_copy_rows_keeps_the_stored_bits(dim, dtype):
    import torch

    from hiprag import _native

    rng = np.random.default_rng(dim)
    N = 1500
    x = _clustered(rng, N, dim)
    src = _native.NativeIndex(dim, dtype, "cosine")
    src.add(x)
    q = _queries(rng, x, 6)
    for n in (1, 33, 1000):
        rows = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
        pos = rng.choice(np.arange(64, 6000), n, replace=False).astype(np.int64)
        if n == 1:
            rows[0], pos[0] = 5, 32 * 7 + 5       # tile 0 (rotation 0) -> tile 7
        else:
            pos[0], pos[1] = 32 * 40 + 3, 32 * 40 + 17   # two rows in one destination tile
            pos[2:] = rng.choice(np.setdiff1d(np.arange(64, 6000), pos[:2]), n - 2, replace=False)
        assert any(_tile_rot(r // 32) != _tile_rot(p // 32) for r, p in zip(rows, pos))
        total = 6016
        dst = _native.NativeIndex(dim, dtype, "cosine", no_shadows=(n == 33))
        rd, pd = torch.from_numpy(rows).cuda(), torch.from_numpy(pos).cuda()
        dst.copy_rows_from(src, rd.data_ptr(), pd.data_ptr(), n, total)
        assert dst.size() == (total, n)
        np.testing.assert_array_equal(dst.get_rows(pos), src.get_rows(rows))
        # an exact search of the destination = one over the same rows of the source (a mask by row)
        bits = np.zeros((N + 63) // 64 * 64, bool)
        bits[rows] = True
        mask = np.packbits(bits, bitorder="little").view(np.uint64)
        k = min(10, n)
        s_d, r_d = dst.search(q, k)
        s_s, r_s = src.search(q, k, mask)
        np.testing.assert_array_equal(s_d, s_s)
        back = dict(zip(pos.tolist(), rows.tolist()))
        np.testing.assert_array_equal(np.vectorize(back.get)(r_d), r_s)
        # a second copy into the same destination: it grows as hr_index_add_device_at does
        if n == 33:
            more = np.array([total + 100], np.int64)
            md, sd = torch.from_numpy(more).cuda(), torch.from_numpy(rows[:1].copy()).cuda()
            dst.copy_rows_from(src, sd.data_ptr(), md.data_ptr(), 1, total + 128)
            assert dst.size() == (total + 128, n + 1)
            np.testing.assert_array_equal(dst.get_rows(more), src.get_rows(rows[:1]))
        dst.close()
    src.close()


def test_copy_rows_refuses_what_it_does_not_support():
    import torch

    from hiprag import _native

    a = _native.NativeIndex(64, "bf16", "cosine")
    a.add(np.ones((4, 64), np.float32))
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    for other in (_native.NativeIndex(64, "f16", "cosine"), _native.NativeIndex(64, "bf16", "ip"),
                  _native.NativeIndex(128, "bf16", "cosine")):
        with pytest.raises(NotImplementedError):
            other.copy_rows_from(a, one.data_ptr(), one.data_ptr(), 1, 32)
    e1, e2 = _native.NativeIndex(64, "bf16", "l2"), _native.NativeIndex(64, "bf16", "l2")
    e1.add(np.ones((4, 64), np.float32))
    with pytest.raises(NotImplementedError):
        e2.copy_rows_from(e1, one.data_ptr(), one.data_ptr(), 1, 32)
    with pytest.raises(NotImplementedError):
        a.copy_rows_from(a, one.data_ptr(), one.data_ptr(), 1, 32)


# ---------------------------------------------------------------- hr_ivf_position_mask
@pytest.mark.parametrize("n_positions", [1, 31, 32, 33, 95, 4096 + 7])
def test_position_mask(n_positions):
    import torch

    from hiprag import _native

    rng = np.random.default_rng(n_positions)
    n_mask_rows = 3 * 64
    ids = rng.integers(0, n_mask_rows + 100, n_positions).astype(np.int64)   # some at or beyond n_mask_rows
    ids[rng.random(n_positions) < 0.2] = -1                                   # pads
    ids[-1] = n_mask_rows                                                     # the first id beyond the bitmap
    if n_positions > 2:
        ids[0], ids[1] = n_mask_rows - 1, -1
    for fill in ("random", "zeros", "ones"):
        bits = {"random": rng.random(n_mask_rows) < 0.5, "zeros": np.zeros(n_mask_rows, bool),
                "ones": np.ones(n_mask_rows, bool)}[fill]
        words = np.packbits(bits, bitorder="little").view(np.uint64)
        exp_bits = np.zeros((n_positions + 31) // 32 * 32, bool)
        ok = (ids >= 0) & (ids < n_mask_rows)
        exp_bits[:n_positions][ok] = bits[ids[ok]]
        exp = np.packbits(exp_bits, bitorder="little").view(np.uint32)
        out = torch.full(((n_positions + 31) // 32 + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ids_d, words_d = torch.from_numpy(ids).cuda(), torch.from_numpy(words.view(np.int64)).cuda()
        _native.ivf_position_mask(ids_d.data_ptr(), n_positions, words_d.data_ptr(), n_mask_rows, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got[:-2], exp)
        assert (got[-2:] == 0x5A5A5A5A).all()     # nothing past ceil(n_positions / 32) words


# ---------------------------------------------------------------- growth
@pytest.mark.parametrize("dim,dtype,bulk", [(128, "bf16", True), (96, "f16", True), (1100, "f32", False)])
def test_incremental_adds_match_the_oracle(dim, dtype, bulk):
    import torch

    from hiprag import _native
    from hiprag.ivf import IvfIndex

    rng = np.random.default_rng(dim)
    n0, batches = 2000, [1, 31, 32, 33, 700, 64]
    x = _clustered(rng, n0 + sum(batches), dim)
    x[-64:] = x[n0 + 5]                     # the last batch: 64 duplicates of one stored vector (one list takes all)
    stored = R.process_rows(x, "cosine", dtype)       # once, for every prefix
    xd = torch.from_numpy(x).cuda()
    q = _queries(rng, x, 6)
    q[0] = x[-1]
    ivf = IvfIndex(dim, NLIST, dtype=dtype)
    ivf.train(xd[:n0:3], iters=8, seed=1)
    if bulk:
        ivf.build(n0, lambda i, j: xd[i:j])
        assert not ivf.extents and ivf.list_tiles is not None
    else:
        ivf.add(xd[:n0])
    flat = _native.NativeIndex(dim, dtype, "cosine")
    flat.add(x[:n0])
    n = n0
    for m in batches:
        lists = ivf.add(xd[n:n + m])          # ids default to the next row numbers
        flat.add(x[n:n + m])
        n += m
        assert ivf.extents and ivf.n == n and ivf.index.size()[1] == n
        if m == 64:
            assert len(set(lists.tolist())) == 1
        got = _check_against_oracle(ivf, stored, dtype, q, n)
        for k in (10, 100):                   # every list probed: the exact search over the same rows
            s_f, r_f = flat.search(q, k)
            np.testing.assert_array_equal(got[NLIST, k][1], r_f)
            np.testing.assert_array_equal(got[NLIST, k][0].astype(np.float32), s_f)
    assert ivf.n_ext > NLIST                  # the lists did grow by extents
    members = ivf.list_members()
    row_list = ivf.lists_of_rows.cpu().numpy()
    for l in range(NLIST):
        np.testing.assert_array_equal(np.sort(members[l]), np.nonzero(row_list == l)[0])
    with pytest.raises(ValueError):
        ivf.add(xd[:1], ids=[3])              # an id that is already stored
    ivf.close()


@pytest.fixture(scope="module")
def grown():
    """2000 bulk rows + 500 added, dim 128 bf16, with its reference rows (shared, read-only)."""
    import torch

    from hiprag.ivf import IvfIndex

    rng = np.random.default_rng(5)
    dim, dtype, n = 128, "bf16", 2500
    x = _clustered(rng, n, dim)
    xd = torch.from_numpy(x).cuda()

    def make():
        ivf = IvfIndex(dim, NLIST, dtype=dtype)
        ivf.train(xd[:2000:3], iters=8, seed=1)
        ivf.build(2000, lambda i, j: xd[i:j])
        ivf.add(xd[2000:2300])
        ivf.add(xd[2300:])
        return ivf

    return {"x": x, "stored": R.process_rows(x, "cosine", dtype), "q": _queries(rng, x, 6), "dtype": dtype, "n": n,
            "make": make}


def test_remove_and_compact(grown):
    ivf = grown["make"]()
    n, q = grown["n"], grown["q"]
    row_list = ivf.lists_of_rows.cpu().numpy().copy()
    big = int(np.argmax(np.bincount(row_list, minlength=NLIST) * (np.bincount(row_list, minlength=NLIST) < 250)))
    gone = np.nonzero(row_list == big)[0]                          # every row of one list ...
    rest = np.setdiff1d(np.arange(n), gone)
    rng = np.random.default_rng(9)
    gone = np.concatenate([gone, rng.choice(rest, 300 - len(gone), replace=False)])   # ... 300 ids in all
    assert len(gone) == 300 and ivf.remove(gone) == 300
    assert ivf.remove(gone[:10]) == 0 and ivf.remove([n + 5, 10 ** 9, -3]) == 0       # removed / unknown: no-op
    row_list[gone] = -1
    np.testing.assert_array_equal(ivf.lists_of_rows.cpu().numpy(), row_list)
    assert ivf.index.size()[1] == n - 300 and ivf.n_dead() == 300
    before = _check_against_oracle(ivf, grown["stored"], grown["dtype"], q, n)
    n_ext = ivf.n_ext
    ivf.compact()
    assert n_ext > NLIST and ivf.n_ext == NLIST and ivf.n_dead() == 0
    size = ivf.index.size()
    assert size[1] == n - 300 and size[0] == 32 * int(ivf.ntiles.sum())
    assert int((ivf.ids >= 0).sum()) == n - 300
    after = _check_against_oracle(ivf, grown["stored"], grown["dtype"], q, n)
    for key in before:
        np.testing.assert_array_equal(before[key][0], after[key][0])
        np.testing.assert_array_equal(before[key][1], after[key][1])
    # it still grows after the compaction, the removed list included
    import torch

    ivf.add(torch.from_numpy(grown["x"][gone[:40]]).cuda(), ids=gone[:40])
    row_list[gone[:40]] = ivf.lists_of_rows.cpu().numpy()[gone[:40]]
    assert (row_list[gone[:40]] >= 0).all()
    np.testing.assert_array_equal(ivf.lists_of_rows.cpu().numpy(), row_list)
    _check_against_oracle(ivf, grown["stored"], grown["dtype"], q, n, nprobes=(3,), ks=(100,))
    ivf.close()


def test_save_and_load(grown, tmp_path):
    import torch

    from hiprag.ivf import IvfIndex

    ivf = grown["make"]()
    ivf.remove(np.arange(100, 140))
    path = str(tmp_path / "lists.hri")
    ivf.save(path)
    back = IvfIndex.load(path)
    assert torch.equal(back.ids, ivf.ids) and back.n == ivf.n
    for name in ("ext_off", "ext", "list_ntiles", "lists_of_rows"):
        assert torch.equal(getattr(back, name), getattr(ivf, name)), name
    np.testing.assert_array_equal(back.pos_of_id, ivf.pos_of_id)
    for nprobe, k in ((1, 10), (3, 100), (NLIST, 10)):
        a, b = _search(ivf, grown["q"], k, nprobe), _search(back, grown["q"], k, nprobe)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    # the reloaded index goes on growing exactly as the original does
    xd = torch.from_numpy(grown["x"][100:140]).cuda()
    ivf.add(xd, ids=np.arange(100, 140))
    back.add(xd, ids=np.arange(100, 140))
    assert torch.equal(back.ids, ivf.ids) and torch.equal(back.ext, ivf.ext)
    # a bulk-built index saves too, without leaving its form
    bulk = IvfIndex(128, NLIST, dtype="bf16")
    bulk.centroids = ivf.centroids.clone()
    x2 = torch.from_numpy(grown["x"][:900]).cuda()
    bulk.build(900, lambda i, j: x2[i:j])
    bulk.save(str(tmp_path / "bulk.hri"))
    assert not bulk.extents
    again = IvfIndex.load(str(tmp_path / "bulk.hri"))
    assert torch.equal(again.ids, bulk.ids)
    for u, v in zip(_search(bulk, grown["q"], 10, 3), _search(again, grown["q"], 10, 3)):
        np.testing.assert_array_equal(u, v)
    for i in (ivf, back, bulk, again):
        i.close()


def test_bulk_built_index_is_unchanged(grown):
    """Never added to: contiguous lists through hr_ivf_search, the list_tiles and ids build() has always made."""
    import torch

    from hiprag.ivf import IvfIndex

    x = torch.from_numpy(grown["x"]).cuda()

    def make():
        ivf = IvfIndex(128, NLIST, dtype="bf16")
        ivf.train(x[::3], iters=8, seed=1)
        return ivf.build(len(x), lambda i, j: x[i:j], chunk=700)

    a, b = make(), make()
    assert not a.extents and a.ext is None and torch.equal(a.list_tiles, b.list_tiles) and torch.equal(a.ids, b.ids)
    row_list = a.lists_of_rows.cpu().numpy()
    counts = np.bincount(row_list, minlength=NLIST)
    lt = np.concatenate([[0], np.cumsum((counts + 31) // 32)])
    np.testing.assert_array_equal(a.list_tiles.cpu().numpy(), lt)
    ids = np.full(lt[-1] * 32, -1, np.int64)
    for l in range(NLIST):
        ids[lt[l] * 32: lt[l] * 32 + counts[l]] = np.nonzero(row_list == l)[0]      # row order inside a list
    np.testing.assert_array_equal(a.ids.cpu().numpy(), ids)
    assert a.max_list_tiles == int(((counts + 31) // 32).max())
    # the list-order rows keep no 8-bit shadow (they are never scanned by the exact search); a plain index does
    from hiprag import _native

    plain = _native.NativeIndex(128, "bf16", "cosine")
    plain.add(grown["x"][:64])
    assert plain.shadow8_stats()["built"] and not a.index.shadow8_stats()["built"]
    plain.close()
    _check_against_oracle(a, grown["stored"], "bf16", grown["q"], len(x), nprobes=(3,), ks=(10,))
    a.close()
    b.close()
