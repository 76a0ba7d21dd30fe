"""GPU: the shadow-8 FILTER's refresh cadence (16 tiles, hr_index.hip refresh_every8) on a shard large enough that
every wave refreshes in mid-scan.

The other shadow-8 tests run corpora of a few thousand rows, where a wave scans one tile and no refresh after the
first ever happens.  Here 1.2M x 64 rows are 37,500 tiles over at most 2048 waves: 18 or more tiles per wave, so the
staggered 16-tile refresh fires in every wave, thresholds published by other waves are read back, and the candidate
regions must still hold what the looser cadence lets through -- rows and score bits equal to the oracle's, and no
query sent to the collect pass."""
import numpy as np
import pytest

import oracle
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

N, DIM, B = 1_200_000, 64, 64


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


@pytest.fixture(scope="module")
def corpus():
    stored = oracle.c_build_synthetic(1, 0, N, DIM, "bf16", "cosine")
    rng = np.random.default_rng(3)
    planted = np.concatenate([R.gen_rows(1, int(j), 1, DIM) for j in rng.choice(N, B, replace=False)])
    q = planted + rng.standard_normal((B, DIM)).astype(np.float32) * 20000  # near neighbours, not exact copies
    q[1::2] = rng.standard_normal((B // 2, DIM))                            # and isotropic queries
    q = q.astype(np.float32)
    s_ref, r_ref = oracle.c_search(stored, "bf16", R.process_queries(q, "cosine"), 40)  # once, shared by the cases
    return q, s_ref, r_ref


@pytest.mark.parametrize("k", [10, 40])
def test_shadow8_mid_scan_refreshes_keep_results_exact(native, corpus, k):
    q, s_ref, r_ref = corpus
    s_ref, r_ref = s_ref[:, :k], r_ref[:, :k]
    idx = native.NativeIndex(DIM, "bf16", "cosine")
    idx.add_synthetic(1, 0, N)
    idx.set_shadow8(2)
    f0 = idx.stats()["guard_failures"]
    s, r = idx.search(q, k)
    st = idx.shadow8_stats()
    assert st["launches"] > 0 and st["kc8"] == (160 if k == 40 else 128)
    np.testing.assert_array_equal(r, r_ref)
    np.testing.assert_array_equal(s, s_ref.astype(np.float32))
    assert idx.stats()["guard_failures"] == f0  # the cadence did not overflow a candidate region
    idx.close()
