"""GPU: multi-device index handles (hr_group.hip) at 5 and 8 shards, on the shard edges tests/test_gpu_group.py's
9,000 to 70,000 rows over 2 to 4 shards never reach: shards of a few tiles (fewer live rows than kc: every shard pads
its candidates), shards that are still empty while a collection grows from nothing (n == 0), shards emptied by
deletes (n > 0, n_live == 0), exact ties on all 8 shards (the collect fallback at cap 1024: a merge of 8 x 1024 =
8192 records, the merge kernel's LDS maximum; collect windows beyond the cap: the per-shard exhaustive pass), and
save / load across 8 -> 1 -> 5 devices.  One process, the shards share the GPU (dev_ids repeated).
Bar: ids, then score bits, then -inf / -1 padding, identical to the CPU oracle over the whole corpus and to a
single-device index holding the same rows -- no tolerance -- through hr_index_search, hr_index_search_device and
the pipelined hr_index_search_submit / _finalize."""
import numpy as np
import pytest

import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

B = 33
KS = (1, 10, 100, 128)


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _devs(G):
    from hiprag import _native

    n = _native.device_count()
    return [i % n for i in range(G)]


def _check(s_gpu, r_gpu, s_ref, r_ref, what=""):
    np.testing.assert_array_equal(r_gpu, r_ref, err_msg=what)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid], s_ref[valid].astype(np.float32), err_msg=what)
    assert np.all(np.isneginf(s_gpu[~valid])), what


def _queries(raw, nq, rng):
    """Half planted next to stored rows, half random (as tests/test_gpu_group.py)."""
    n, dim = raw.shape
    j = rng.choice(n, min(n, nq // 2), replace=False)
    base = raw[j] / np.linalg.norm(raw[j], axis=1, keepdims=True)
    planted = base + 0.05 * rng.standard_normal((len(j), dim)).astype(np.float32) / np.sqrt(dim)
    return np.concatenate([planted, rng.standard_normal((nq - len(j), dim))]).astype(np.float32)


def _search(idx, how, q, k, allowed=None):
    """One search of idx through entry point `how`: "host" (hr_index_search), "device" (hr_index_search_device:
    queries, mask and outputs on the device) or "pipe" (hr_index_search_submit + _finalize; no mask)."""
    import torch

    if how == "host":
        return idx.search(q, k, None if allowed is None else oracle.mask_from_bool(allowed))
    qd = torch.from_numpy(q).cuda()
    s = torch.full((q.shape[0], k), 7.0, dtype=torch.float32, device="cuda")
    r = torch.full((q.shape[0], k), 7, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if how == "device":
        md = None if allowed is None else torch.from_numpy(oracle.mask_from_bool(allowed).view(np.int64)).cuda()
        idx.search_device(qd.data_ptr(), q.shape[0], k, s.data_ptr(), r.data_ptr(),
                          mask_ptr=0 if md is None else md.data_ptr(), stream=st)
    else:
        assert how == "pipe" and allowed is None
        t = idx.search_submit(qd.data_ptr(), q.shape[0], k, s.data_ptr(), r.data_ptr(), stream=st)
        assert t > 0
        idx.search_finalize(t)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def _hows(allowed):
    return ("host", "device") if allowed is not None else ("host", "device", "pipe")


def _small_corpus(native, G, dtype, metric, seed=13, dup_tiles=()):
    """A1's corpus: n = 3 * 32 * G + 17 rows of dim 128 (three tiles per shard and a partial one), added in ragged
    steps to a G-shard handle and a single-device index, then 5 % of the rows removed from both.  dup_tiles: tiles
    whose rows are all copies of the first of them."""
    dim, n = 128, 3 * 32 * G + 17
    raw = R.gen_rows(seed, 0, n, dim)
    # norms 0.5 .. 2: inside f16's range (the generator's elements are not), and ip / l2 rank unlike cosine
    scale = np.random.default_rng(seed).uniform(0.5, 2.0, n)
    raw = (raw / np.linalg.norm(raw, axis=1, keepdims=True) * scale[:, None]).astype(np.float32)
    for t in dup_tiles:
        raw[t * 32:(t + 1) * 32] = raw[dup_tiles[0] * 32]
    grp = native.NativeIndex(dim, dtype, metric, devices=_devs(G))
    one = native.NativeIndex(dim, dtype, metric)
    for lo, hi in [(0, 7), (7, 100), (100, 133), (133, n)]:
        assert grp.add(raw[lo:hi]) == lo
        one.add(raw[lo:hi])
    gone = np.random.default_rng(G).choice(n, n // 20, replace=False)
    grp.remove(gone)
    one.remove(gone)
    live = ~np.isin(np.arange(n), gone)
    assert grp.size() == one.size() == (n, int(live.sum()))
    return raw, grp, one, live


def _compare_all(grp, one, stored, dtype, metric, qn, q, live, masks, ks=KS, what=""):
    """Every k x mask x entry point of grp against the oracle over the whole corpus; the single-device index `one`
    (host search) must give the same bits too."""
    for k in ks:
        for name, m in masks.items():
            allowed = live if m is None else live & m
            s_ref, r_ref = oracle.c_search(stored, dtype, qn, k, oracle.mask_from_bool(allowed), metric=metric)
            assert np.isfinite(s_ref[r_ref >= 0]).all()
            if one is not None:
                _check(*_search(one, "host", q, k, m), s_ref, r_ref, f"{what} single k={k} mask={name}")
            for how in _hows(m):
                _check(*_search(grp, how, q, k, m), s_ref, r_ref, f"{what} G={len(grp.devices)} k={k} mask={name} {how}")


@pytest.mark.parametrize("G", [5, 8])
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f16", "ip"), ("f32", "l2")])
def test_few_tiles_per_shard(native, G, dtype, metric):
    """A1: about 91 live rows per shard.  At k = 100 (kc 160) and k = 128 (kc 192) every shard holds fewer live rows
    than kc and pads its candidates; the merge must drop the padding and the guard must not fail on a shard that
    returned all it has (bound -inf)."""
    raw, grp, one, live = _small_corpus(native, G, dtype, metric)
    n = len(raw)
    assert live.sum() / G < native.kc_for_k(100, 128) and native.kc_for_k(10, 128) < live.sum() / G - 32
    rng = np.random.default_rng(G * 7 + 1)
    q = _queries(raw, B, rng)
    two_tiles = np.zeros(n, bool)
    two_tiles[32:64] = two_tiles[(G + 2) * 32:(G + 3) * 32] = True  # tile 1 (shard 1) and tile G + 2 (shard 2)
    masks = {"none": None, "half": rng.random(n) < 0.5, "two_tiles": two_tiles}
    _compare_all(grp, one, R.process_rows(raw, metric, dtype), dtype, metric, R.process_queries(q, metric), q, live,
                 masks, what=f"{dtype}/{metric}")
    grp.close()
    one.close()


def test_growth_from_nothing_over_8_shards(native):
    """A2: a collection on 8 shards from its first row on.  Until it holds 225 rows some shard is empty (n == 0:
    shard_masks, group_search_impl and pipe_shard take their empty-shard branches; the exhaustive pass runs over
    shards with no rows).  After each add: k = 10, k = 100 (more than the rows present below 100:
    padding) and k = HR_MAX_K + 40 (the exhaustive pass), get_rows of every row, size()."""
    dim, G, dtype, metric = 64, 8, "bf16", "cosine"
    raw = R.gen_rows(29, 0, 257, dim)
    stored = R.process_rows(raw, metric, dtype)
    grp = native.NativeIndex(dim, dtype, metric, devices=_devs(G))
    one = native.NativeIndex(dim, dtype, metric)
    rng = np.random.default_rng(5)
    have = 0
    big = native.HR_MAX_K + 40
    for n in (1, 31, 32, 33, 255, 256, 257):
        assert grp.add(raw[have:n]) == have
        one.add(raw[have:n])
        have = n
        assert grp.size() == (n, n)
        q = _queries(raw[:n], 9, rng)
        qn = R.process_queries(q, metric)
        for k in (10, 100, big):
            s_ref, r_ref = oracle.c_search(stored[:n], dtype, qn, k, metric=metric)
            assert (r_ref[:, min(k, n):] == -1).all() and (r_ref[:, :min(k, n)] >= 0).all()
            _check(*_search(one, "host", q, k), s_ref, r_ref, f"n={n} single k={k}")
            _check(*_search(grp, "host", q, k), s_ref, r_ref, f"n={n} k={k} host")
            if k <= native.HR_MAX_K:
                _check(*_search(grp, "pipe", q, k), s_ref, r_ref, f"n={n} k={k} pipe")
                _check(*_search(grp, "device", q, k), s_ref, r_ref, f"n={n} k={k} device")
        every = grp.get_rows(np.arange(n))
        np.testing.assert_array_equal(every.view(np.uint32), R.dequantize(stored[:n], dtype).view(np.uint32))
        np.testing.assert_array_equal(every.view(np.uint32), one.get_rows(np.arange(n)).view(np.uint32))
    # the pipelined entry point serves the scan's k only: k above HR_MAX_K is refused, not answered wrongly
    with pytest.raises(ValueError):
        _search(grp, "pipe", q, big)
    grp.close()
    one.close()


def test_shards_emptied_by_deletes(native):
    """A3: every row of stripes 2 and 5 removed from the 8-shard corpus: those shards keep n > 0 with n_live == 0.
    Plus a mask that allows only removed rows (all padding) and one that allows shards 2 and 5 and one live row
    elsewhere (that row, then padding).  Two tiles of shard 0 and two of shard 1 hold copies of one row (more than
    kc = 32 live ones each), so the query equal to it fails its guard at k = 10 and group_fallback runs its collect
    pass over the two emptied shards as well."""
    G, dtype, metric = 8, "bf16", "cosine"
    raw, grp, one, live = _small_corpus(native, G, dtype, metric, dup_tiles=(8, 16, 9, 17))
    n = len(raw)
    assert min(live[8 * 32:9 * 32].sum() + live[16 * 32:17 * 32].sum(),
               live[9 * 32:10 * 32].sum() + live[17 * 32:18 * 32].sum()) > native.kc_for_k(10, 128)
    stripe = (np.arange(n) >> 5) % G
    dead = np.nonzero(live & ((stripe == 2) | (stripe == 5)))[0]
    grp.remove(dead)
    one.remove(dead)
    live = live & ~((stripe == 2) | (stripe == 5))
    assert grp.size() == (n, int(live.sum()))
    rng = np.random.default_rng(77)
    q = _queries(raw, B, rng)
    q[0] = raw[8 * 32]
    qn = R.process_queries(q, metric)
    stored = R.process_rows(raw, metric, dtype)
    for how in ("host", "device", "pipe"):
        before = grp.stats()["guard_failures"]
        _check(*_search(grp, how, q, 10), *oracle.c_search(stored, dtype, qn, 10, oracle.mask_from_bool(live)), how)
        assert grp.stats()["guard_failures"] > before, how
    only_removed = ~live
    lone = int(np.nonzero(live & (stripe == 6))[0][3])
    dead_shards_and_one = (stripe == 2) | (stripe == 5)
    dead_shards_and_one[lone] = True
    masks = {"none": None, "half": rng.random(n) < 0.5, "only_removed": only_removed,
             "dead_shards_and_one": dead_shards_and_one}
    _compare_all(grp, one, stored, dtype, metric, qn, q, live, masks, what="emptied")
    for how in ("host", "device"):
        s, r = _search(grp, how, q, 10, only_removed)
        assert (r == -1).all() and np.isneginf(s).all()
        s, r = _search(grp, how, q, 10, dead_shards_and_one)
        assert (r[:, 0] == lone).all() and (r[:, 1:] == -1).all()
    grp.close()
    one.close()


def _stripe_local(rows, G):
    """CPU restatement of the striping (stripe_row's inverse): global row -> (shard, local row)."""
    tile = rows >> 5
    return tile % G, ((tile // G) << 5) | (rows & 31)


def _stripe_global(local, G, s):
    """CPU restatement of stripe_row: shard s's local row -> global row."""
    return ((((local >> 5) * G) + s) << 5) | (local & 31)


@pytest.mark.parametrize("copies,overflow", [(2000, False), (9000, True)])
def test_ties_over_8_shards(native, copies, overflow):
    """A4: `copies` copies of one row spread over 12,000 rows on 8 shards.  2,000: every shard holds more than kc
    of them, every shard's guard fails, the collect fallback runs with cap 1024 and its merge takes 8 x 1024 = 8192
    records (k_merge's LDS maximum).  9,000: more than 1024 per shard, every collect window overflows into the
    per-shard exhaustive pass.  The answer to the tie query is the copies in ascending GLOBAL row order: that pins
    stripe_row over all 8 stripes (with `G - 1 - s` for `s` in it, shard 0's copies would come back as rows of
    stripe 7: _stripe_global(l, 8, 7 - s) != _stripe_global(l, 8, s) for every local row, so both the oracle
    comparison and the ascending-order assertion fail)."""
    dim, n, G, dtype, metric = 64, 12_000, 8, "bf16", "cosine"
    raw = R.gen_rows(37, 0, n, dim)
    dups = np.sort(np.random.default_rng(copies).choice(n, copies, replace=False))
    raw[dups] = raw[dups[0]]
    stored = R.process_rows(raw, metric, dtype)
    shard, local = _stripe_local(dups, G)
    per_shard = np.bincount(shard, minlength=G)
    cap = 1024  # fallback_cap(8)
    assert cap * G == 8192
    assert (per_shard > native.kc_for_k(100, dim)).all()
    assert (per_shard > cap).all() if overflow else (per_shard < cap // 2).all()
    np.testing.assert_array_equal(np.concatenate([_stripe_global(local[shard == s], G, s) for s in range(G)]),
                                  np.concatenate([dups[shard == s] for s in range(G)]))
    assert all((_stripe_global(local[shard == s], G, G - 1 - s) != dups[shard == s]).all() for s in range(G))
    q = np.concatenate([raw[dups[:1]], R.gen_rows(99, 0, 3, dim)]).astype(np.float32)
    qn = R.process_queries(q, metric)
    grp = native.NativeIndex(dim, dtype, metric, devices=_devs(G))
    grp.add(raw)
    for k in (10, 100):
        s_ref, r_ref = oracle.c_search(stored, dtype, qn, k, metric=metric)
        np.testing.assert_array_equal(r_ref[0], dups[:k])  # the oracle: the copies, ascending
        if overflow:
            # no HR_E_OVERFLOW expected: a shard whose window overflows returns its exact top-cap instead, and the
            # global top-k lies inside the union of the shards' top-cap lists (k <= cap) -- on the oracle
            union = []
            for s in range(G):
                rows_s = np.nonzero((np.arange(n) >> 5) % G == s)[0]
                union.append(rows_s[oracle.c_search(stored[rows_s], dtype, qn[:1], cap, metric=metric)[1][0]])
            assert np.isin(r_ref[0], np.concatenate(union)).all()
        for how in ("host", "pipe", "device"):
            before = grp.stats()
            s, r = _search(grp, how, q, k)
            _check(s, r, s_ref, r_ref, f"copies={copies} k={k} {how}")
            np.testing.assert_array_equal(r[0], dups[:k])
            after = grp.stats()
            assert after["guard_failures"] > before["guard_failures"], (how, k, before, after)
            if overflow:
                assert after["exhaustive"] >= before["exhaustive"] + G, (how, k, before, after)
    grp.close()


def test_save_load_8_to_1_to_5_devices(native, tmp_path):
    """A5: the 8-shard corpus (with its removed rows) saved, loaded into one device, saved again, loaded into 5
    shards: the same answers and the same rows throughout."""
    G, dtype, metric = 8, "bf16", "cosine"
    raw, grp, one, live = _small_corpus(native, G, dtype, metric)
    one.close()
    n = len(raw)
    rng = np.random.default_rng(3)
    q = _queries(raw, B, rng)
    qn = R.process_queries(q, metric)
    stored = R.process_rows(raw, metric, dtype)
    rows_ref = R.dequantize(stored, dtype).view(np.uint32)
    masks = {"none": None, "half": rng.random(n) < 0.5}
    p8, p1 = str(tmp_path / "g8.hri"), str(tmp_path / "one.hri")
    grp.save(p8)
    single = native.NativeIndex.load(p8)
    single.save(p1)
    g5 = native.NativeIndex.load(p1, devices=_devs(5))
    for name, idx in (("8", grp), ("8->1", single), ("8->1->5", g5)):
        assert idx.size() == (n, int(live.sum())), name
        np.testing.assert_array_equal(idx.get_rows(np.arange(n)).view(np.uint32), rows_ref, err_msg=name)
        if len(idx.devices) > 1:
            _compare_all(idx, None, stored, dtype, metric, qn, q, live, masks, ks=(10, 100), what=name)
        else:
            for k in (10, 100):
                for mname, m in masks.items():
                    ref = oracle.c_search(stored, dtype, qn, k, oracle.mask_from_bool(live if m is None else live & m),
                                          metric=metric)
                    _check(*_search(idx, "host", q, k, m), *ref, f"{name} k={k} mask={mname}")
    for idx in (grp, single, g5):
        idx.close()
