"""GPU: the shadow-8 scan (an int8 copy of a cosine corpus with one fp32 scale per row, streamed by the SAMPLE and the
64-query FILTER; hr_index_set_shadow8) against the CPU oracle.

Bar, as everywhere: rows equal to the oracle's, score bits equal, -inf / -1 padding -- with the scan forced on (mode 2)
and, on the same handle, off (mode 0); the launch counter shows which FILTER ran.  The guard's premise is checked on
every row: |shadow-8 approximate score - exact score| <= E_q with the reported u_x8, on Gaussian rows and on the
value families of tests/hostile_data.py that int8 treats worst (one-hot and all-zero rows, one huge element among tiny
ones, every row identical)."""
import functools

import numpy as np
import pytest

import hostile_data as H
import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "f16", "f32")


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _check(s_gpu, r_gpu, s_ref, r_ref):
    np.testing.assert_array_equal(r_gpu, r_ref)
    valid = r_ref >= 0
    np.testing.assert_array_equal(s_gpu[valid], s_ref[valid].astype(np.float32))
    assert np.all(np.isneginf(s_gpu[~valid]))


@functools.lru_cache(maxsize=8)
def _gauss(n, dim, B):
    """Gaussian rows (the suite's generator) and B queries: planted rows plus noise alternating with isotropic ones."""
    rows = R.gen_rows(3, 0, n, dim)
    rng = np.random.default_rng(n + dim)
    q = rng.standard_normal((B, dim)).astype(np.float32)  # odd positions stay isotropic, even ones are planted
    q[0::2] = rows[rng.integers(0, n, len(q[0::2]))] + q[0::2] * 2000
    rows.setflags(write=False)
    return rows, q


def _oracle(rows, dtype, q, k, allowed=None):
    stored = R.process_rows(rows, "cosine", dtype)
    mask = None if allowed is None else oracle.mask_from_bool(allowed)
    return oracle.c_search(stored, dtype, R.process_queries(q, "cosine"), k, mask)


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [64, 100, 1024])
@pytest.mark.parametrize("n", [4096 + 37, 33])
def test_shadow8_search_matches_oracle(native, n, dim, dtype):
    """A partial last tile and a two-tile corpus; D = 64 (one paired block), 100 (padded to 128), 1024; every stored
    dtype; B = 1 (one 32-query block) and 64; k = 1, 10 and 40 (kc8 = 160: five row parts, the plan's default for
    k = 40 has two).  Mode 2 and mode 0 on the same handle both equal the oracle, so they equal each other; the
    launch counter moves in mode 2 only."""
    rows, q = _gauss(n, dim, 64)
    kmax = 40
    s_ref, r_ref = _oracle(rows, dtype, q, kmax)
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.add(rows)
    assert idx.shadow8_stats()["built"]
    for B in (1, 64):
        for k in (1, 10, kmax):
            idx.set_shadow8(2)
            l0 = idx.shadow8_stats()["launches"]
            s2, r2 = idx.search(q[:B], k)
            st = idx.shadow8_stats()
            assert st["launches"] > l0, (B, k)
            assert st["kc8"] == (160 if k == kmax else 128)
            _check(s2, r2, s_ref[:B, :k], r_ref[:B, :k])
            idx.set_shadow8(0)
            s0, r0 = idx.search(q[:B], k)
            assert idx.shadow8_stats()["launches"] == st["launches"]
            _check(s0, r0, s_ref[:B, :k], r_ref[:B, :k])
            np.testing.assert_array_equal(r0, r2)
            np.testing.assert_array_equal(s0.view(np.uint32), s2.view(np.uint32))
    assert 0.0 < idx.shadow8_stats()["u_x8"] < 0.05  # Gaussian rows: ~ sqrt(D / 12) / 127 of the largest element
    idx.close()


def test_shadow8_default_mode_leaves_small_shards_alone(native):
    """Mode 1 (the default) scans the shadow only on shards beyond the dual-FILTER range: a small index never does."""
    rows, q = _gauss(4096 + 37, 64, 64)
    idx = native.NativeIndex(64, "bf16", "cosine")
    idx.add(rows)
    s, r = idx.search(q, 10)
    st = idx.shadow8_stats()
    assert st["launches"] == 0 and st["built"]
    assert st["u_x8"] == 0.0  # ... nor converts rows for a shadow no scan would read
    _check(s, r, *_oracle(rows, "bf16", q, 10))
    idx.set_shadow8(2)  # the stale rows are converted by the first search that scans them
    s, r = idx.search(q, 10)
    st = idx.shadow8_stats()
    assert st["launches"] > 0 and st["u_x8"] > 0.0
    _check(s, r, *_oracle(rows, "bf16", q, 10))
    idx.close()


# ---------------------------------------------------------------- guard premise
N_GUARD = 20_011


@functools.lru_cache(maxsize=4)
def _guard_corpus(name, dim):
    rng = np.random.default_rng(11)
    if name == "gauss":
        return np.array(R.gen_rows(5, 0, N_GUARD, dim))
    if name == "sparse":  # one-hot rows (every 50th), 1-8 nonzeros elsewhere, three all-zero rows
        return H.corpus("sparse", 1, N_GUARD, dim)[0]
    if name == "wide":  # elements over forty binades: after normalisation one or two huge elements among tiny ones
        return H.corpus("wide", 1, N_GUARD, dim)[0]
    if name == "identical":  # every row the same vector
        return np.repeat(H.anisotropic(rng, 1, dim), N_GUARD, axis=0)
    raise KeyError(name)


def _guard_queries(name, rows, B):
    if name == "gauss":
        rng = np.random.default_rng(12)
        q = rows[rng.integers(0, len(rows), B)] + rng.standard_normal((B, rows.shape[1])).astype(np.float32) * 2000
        q[1::2] = rng.standard_normal((len(q[1::2]), rows.shape[1]))
        return q.astype(np.float32)
    return H.queries("anisotropic" if name == "identical" else name, 2, rows, B)[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["gauss", "sparse", "wide", "identical"])
def test_shadow8_approx_error_within_guard_bound(native, name, dtype):
    """|shadow-8 approximate score - exact score| <= E_q on every row of a 20k-row corpus, E_q carrying the reported
    u_x8 (the premise of the exactness guard).  The exact side is an fp64 matrix product over the stored rows; its own
    rounding (at most dim 2^-52 |q||x|) is added to the error, so the test asks no less than the canonical sum would.
    Then the search itself, shadow-8 forced on: where int8 flushes a row's tiny elements u_x8 is large and the guard
    fails, and the answer must still be the oracle's (through the collect pass)."""
    dim, B, k = 256, 32, 10
    rows = _guard_corpus(name, dim)
    q = _guard_queries(name, rows, B)
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.add(rows)
    idx.set_shadow8(2)
    approx, E = idx.debug_approx8(q)
    u = idx.shadow8_stats()["u_x8"]
    xs = R.dequantize(R.process_rows(rows, "cosine", dtype), dtype).astype(np.float64)
    qd = R.process_queries(q, "cosine").astype(np.float64)
    exact = qd @ xs.T
    slack = dim * 2.0 ** -52 * np.linalg.norm(qd, axis=1)[:, None] * np.sqrt((xs * xs).sum(axis=1))[None, :]
    assert approx.shape == exact.shape and np.isfinite(approx).all()
    err = (np.abs(approx.astype(np.float64) - exact) + slack).max(axis=1)
    print(f"GUARD8 {name} {dtype}: u_x8 = {u:.3e}, max err = {err.max():.3e}, min E = {E.min():.3e}, "
          f"max err/E = {(err / E).max():.3f}")
    assert np.all(err <= E), (err, E)
    l0 = idx.shadow8_stats()["launches"]
    s, r = idx.search(q, k)
    assert idx.shadow8_stats()["launches"] > l0
    _check(s, r, *_oracle(rows, dtype, q, k))
    idx.close()


# ---------------------------------------------------------------- upkeep
def test_shadow8_follows_adds_removes_and_masks(native):
    """Search, add rows across a tile boundary, remove rows, search under a row bitmap: every search equals the
    oracle over the rows as they then are, with the shadow-8 FILTER serving each of them."""
    dim, dtype, k = 128, "bf16", 10
    rows, q = _gauss(1100, dim, 64)
    idx = native.NativeIndex(dim, dtype, "cosine")
    idx.set_shadow8(2)
    live = np.zeros(1100, bool)

    def search_and_check(allowed=None):
        l0 = idx.shadow8_stats()["launches"]
        n = idx.size()[0]
        eff = live[:n] if allowed is None else live[:n] & allowed[:n]
        s, r = idx.search(q, k, None if allowed is None else oracle.mask_from_bool(allowed[:n]))
        assert idx.shadow8_stats()["launches"] > l0
        _check(s, r, *_oracle(rows[:n], dtype, q, k, eff))

    idx.add(rows[:1000])
    live[:1000] = True
    search_and_check()
    idx.add(rows[1000:1050])  # rows 1000..1049: the rest of tile 31 and the start of tile 32
    live[1000:1050] = True
    search_and_check()
    gone = np.arange(990, 1030)
    idx.remove(gone)
    live[gone] = False
    search_and_check()
    idx.add(rows[1050:1100])
    live[1050:1100] = True
    search_and_check(np.random.default_rng(5).random(1100) < 0.5)
    idx.close()


def test_shadow8_allocation_failure_falls_back(native, monkeypatch):
    """No memory for the shadow (simulated by HIPRAG_SHADOW8_SIM_OOM=1, read when the rows grow): the add succeeds, the
    index keeps none and scans the 16-bit rows -- at create, and when an index that had one grows."""
    dim, dtype, k = 128, "f16", 10
    rows, q = _gauss(4096 + 37, dim, 64)
    ref = _oracle(rows, dtype, q, k)
    had = native.NativeIndex(dim, dtype, "cosine")
    had.set_shadow8(2)
    had.add(rows[:500])
    had.search(q, k)
    assert had.shadow8_stats()["built"] and had.shadow8_stats()["launches"] > 0
    monkeypatch.setenv("HIPRAG_SHADOW8_SIM_OOM", "1")
    fresh = native.NativeIndex(dim, dtype, "cosine")
    fresh.set_shadow8(2)
    fresh.add(rows)
    had.add(rows[500:])  # (grows past the first allocation)
    for idx in (fresh, had):
        l0 = idx.shadow8_stats()["launches"]
        assert not idx.shadow8_stats()["built"]
        s, r = idx.search(q, k)
        assert idx.shadow8_stats()["launches"] == l0
        _check(s, r, *ref)
        idx.close()


def test_shadow8_env_switch_off(native, monkeypatch):
    """HIPRAG_SHADOW8=0 at create: no shadow is kept, whatever the mode."""
    monkeypatch.setenv("HIPRAG_SHADOW8", "0")
    rows, q = _gauss(33, 64, 64)
    idx = native.NativeIndex(64, "bf16", "cosine")
    idx.set_shadow8(2)
    idx.add(rows)
    s, r = idx.search(q, 10)
    assert idx.shadow8_stats() == {"launches": 0, "kc8": 0, "built": False, "u_x8": 0.0}
    _check(s, r, *_oracle(rows, "bf16", q, 10))
    idx.close()
