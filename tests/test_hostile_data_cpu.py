"""CPU: the hostile corpora (tests/hostile_data.py) have the properties the GPU tests rely on.

tests/test_gpu_hostile.py compares the GPU search with the oracle on these families; it would pass just as well on
inputs that had quietly lost their edge (a sparse family that is not sparse, a near-duplicate cluster whose stored
rows collapsed into one, "wide" rows whose small elements no longer reach f16's subnormal range).  So each family's
stated property is asserted here, on the oracle alone, at the size the GPU tests use."""
import functools

import numpy as np
import pytest

import hostile_data as H
import oracle
from oracle import ref_numpy as R

N, DIM = 20_011, 512
DTYPES = ("bf16", "f16", "f32")
METRICS = ("cosine", "ip", "l2")


def _f16_ok(family, dtype, metric):
    """The (family, dtype, metric) combinations the GPU parity tests run: f16 rows with ip / l2 on the families whose
    raw values the issue lists for it."""
    return dtype != "f16" or metric == "cosine" or family in ("anisotropic", "nonneg", "wide")


COMBOS = [(f, d, m) for f in H.FAMILIES for d in DTYPES for m in METRICS if _f16_ok(f, d, m)]
# the guard-premise tests also run the sparse family on f16 rows with ip / l2 (values +-0.5, +-1, +-2 fit f16)
USED = COMBOS + [("sparse", "f16", "ip"), ("sparse", "f16", "l2")]


@functools.lru_cache(maxsize=2)
def _corpus(family, metric, dtype):
    rows, pos, centre = H.corpus(family, 0, N, DIM, metric, dtype)
    rows.setflags(write=False)
    return rows, pos, centre


def _setup(family, dtype, metric, B=32):
    rows, pos, centre = _corpus(family, metric if family == "wide" else "cosine", dtype if family == "neardup" else "")
    q, planted = H.queries(family, 0, rows, B, metric, centre)
    stored = oracle.c_quantize(oracle.c_normalize_rows(rows) if metric == "cosine" else rows, dtype)
    return rows, pos, centre, q, planted, stored, R.process_queries(q, metric)


@pytest.mark.parametrize("family,dtype,metric", USED, ids=lambda v: str(v))
def test_scores_finite_and_zero_query(family, dtype, metric):
    """Every oracle score is finite, the planted row of a planted query is its best row (cosine), and the all-zero
    query's answer is rows 0..k-1 with score 0 where every score ties (cosine and ip; its l2 score 1 - |x|^2 ranks the
    rows by norm instead)."""
    rows, pos, centre, q, planted, stored, qp = _setup(family, dtype, metric)
    assert np.isfinite(R.dequantize(stored, dtype)).all()
    s, r = oracle.c_search(stored, dtype, qp, 40, metric=metric)
    assert np.isfinite(s).all() and (r >= 0).all()
    if family != "neardup":
        assert not q[H.ZERO_AT].any()
        if metric != "l2":
            np.testing.assert_array_equal(r[H.ZERO_AT], np.arange(40))
            assert (s[H.ZERO_AT] == 0).all()
    if metric == "cosine" and family not in ("sparse", "neardup"):  # (sparse rows repeat: the lowest twin wins)
        pl = np.nonzero(planted >= 0)[0]
        pl = pl[pl != H.ZERO_AT]
        np.testing.assert_array_equal(r[pl, 0], planted[pl])


def test_anisotropic_scores_sit_in_a_band():
    rows, _, _, q, planted, stored, qp = _setup("anisotropic", "f32", "cosine")
    drawn = np.nonzero(planted < 0)[0]
    drawn = drawn[drawn != H.ZERO_AT]
    sc = R.dequantize(stored, "f32").astype(np.float64) @ qp[drawn].astype(np.float64).T
    lo, hi = np.percentile(sc, [1, 99])
    print(f"anisotropic: 1st..99th percentile of cosine scores {lo:.3f} .. {hi:.3f}")
    assert hi - lo < 0.6 and lo > 0.1  # one band, well away from 0 (isotropic Gaussians: +-0.1 around 0)
    s, _ = oracle.c_search(stored, "f32", qp[drawn], 40)
    print(f"anisotropic: median top-1 to top-40 gap {np.median(s[:, 0] - s[:, 39]):.4f}")
    assert np.median(s[:, 0] - s[:, 39]) < 0.1


def test_nonneg_is_one_sided():
    rows, _, _, q, _, stored, qp = _setup("nonneg", "bf16", "cosine")
    assert (rows >= 0).all() and (q >= 0).all()
    live = np.arange(len(q)) != H.ZERO_AT
    sc = R.dequantize(stored, "bf16").astype(np.float64) @ qp[live].astype(np.float64).T
    assert sc.min() > 0.4  # E|a||b| / E a^2 = 2/pi: no cancellation anywhere


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_scores_are_mostly_exact_zeros(dtype):
    rows, _, _, q, _, stored, qp = _setup("sparse", dtype, "cosine")
    nnz = (rows != 0).sum(axis=1)
    zr = H.sparse_zero_rows(N)
    assert (nnz[zr] == 0).all() and nnz.max() <= 8
    assert (np.delete(nnz, zr) >= 1).all()
    assert set(np.unique(np.abs(rows))) <= {0.0, 0.5, 1.0, 2.0}
    assert not R.dequantize(stored, dtype)[zr].any()  # normalisation leaves all-zero rows alone
    live = np.arange(len(q)) != H.ZERO_AT
    sc = R.exact_scores(stored[:4000], dtype, qp[live])
    frac = float((sc == 0).mean())
    print(f"sparse/{dtype}: {100 * frac:.1f} % of the scores are exactly 0")
    assert frac > 0.9
    onehot = rows[np.arange(0, N, 50)]  # identical one-hot rows: their order is the tie order
    assert len(np.unique(onehot, axis=0)) <= 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
def test_wide_elements_reach_below_f16_normals(dtype, metric):
    rows, _, _, _, _, stored, _ = _setup("wide", dtype, metric)
    x = np.abs(R.dequantize(stored, dtype))
    frac = float((x[x > 0] < H.F16_MIN_NORMAL).mean())
    print(f"wide/{dtype}/{metric}: {100 * frac:.0f} % of the nonzero stored elements lie below 2^-14")
    assert frac > 0.2
    if metric != "cosine":
        norms = np.linalg.norm(rows.astype(np.float64), axis=1)
        assert norms.min() < 2.0 ** -7 and norms.max() > 2.0 ** 5
        assert np.abs(rows).max() <= 2.0 ** 7  # inside f16's range


@pytest.mark.parametrize("family,dtype,metric", [c for c in COMBOS if c[0] == "neardup"], ids=lambda v: str(v))
def test_neardup_preconditions(family, dtype, metric):
    """The three preconditions of the near-duplicate cluster, per storage dtype, with the oracle: the stored rows stay
    distinct, the exact scores for the centre spread over less than guard_e's additive 1e-9, and the oracle's top-40
    lies inside the cluster."""
    rows, pos, centre, q, _, stored, qp = _setup(family, dtype, metric)
    np.testing.assert_array_equal(q[0], centre)
    members = stored[pos]
    distinct = len(np.unique(members.view(np.uint8).reshape(len(pos), -1), axis=0))
    sc = oracle.c_score_pairs(stored, dtype, qp[:1], np.zeros(len(pos), np.int32), pos, metric=metric)
    spread = float(sc.max() - sc.min())
    print(f"neardup/{dtype}/{metric}: {distinct} distinct stored rows, score spread {spread:.2e}")
    assert distinct >= 150
    assert spread < 1e-9
    s, r = oracle.c_search(stored, dtype, qp[:1], 40, metric=metric)
    assert np.isin(r[0], pos).all()
    bg = np.ones(N, bool)
    bg[pos] = False
    s_bg, _ = oracle.c_search(stored, dtype, qp[:1], 1, oracle.mask_from_bool(bg), metric=metric)
    assert s_bg[0, 0] < sc.min() - 0.1  # the background is nowhere near


@pytest.mark.parametrize("dtype", DTYPES)
def test_cosine_store_is_scale_invariant(dtype):
    """Multiplying row i by 2^(+-60) leaves the stored cosine row bit-identical: every step of the canonical
    normalisation commutes with an exact power of two."""
    rows = H.corpus("anisotropic", 0, N, DIM)[0]
    rows[5] = 0.0  # (a zero row stays zero at any scale)
    scale = np.where(np.arange(N) % 2 == 0, 2.0 ** 60, 2.0 ** -60).astype(np.float32)[:, None]
    scaled = rows * scale
    assert np.isfinite(scaled).all() and (np.abs(scaled[scaled != 0]) >= 2.0 ** -126).all()
    np.testing.assert_array_equal(R.process_rows(scaled, "cosine", dtype), R.process_rows(rows, "cosine", dtype))
    np.testing.assert_array_equal(oracle.c_quantize(oracle.c_normalize_rows(scaled), dtype),
                                  R.process_rows(rows, "cosine", dtype))
