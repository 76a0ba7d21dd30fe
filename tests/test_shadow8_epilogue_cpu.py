"""The arithmetic of the shadow-8 epilogue's folded scale and predicate (hr_kernels.hpp, scan_body: FOLD), pinned in
numpy: score = fma(acc, scale, addend) with addend -0.0 on an allowed lane and -inf on a forbidden one.

An fp32 FMA rounds the exact product plus the addend once.  The product of two fp32 values is exact in fp64 (24 + 24
significand bits, exponents far inside fp64's range), and adding a zero or an infinity to it in fp64 is exact too, so
float32(float64(a) * float64(b) + addend) is the FMA's result."""
import numpy as np

NEG_ZERO = np.float64(-0.0)
NEG_INF = np.float64(-np.inf)


def _fma(a, b, addend):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + addend).astype(np.float32)


def _mul(a, b):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return a * b


def _pairs():
    rng = np.random.default_rng(0)
    tiny = np.float32(1e-45)  # the smallest denormal
    edge = np.array([0.0, -0.0, 1.0, -1.0, tiny, -tiny, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1e-30, -1e-30,
                     1e-20, -3e-20, 3.0, -127.0, 16256.0, 3.4028235e38, -3.4028235e38, 1e30, -1e30, np.inf, -np.inf],
                    np.float32)
    ea, eb = [x.ravel() for x in np.meshgrid(edge, edge)]
    # accumulators as the scan has them (sums of products of int8 values and f16 queries) times row scales, and fp32
    # values over the whole exponent range, denormals and products that round to +-0 included
    acc = (rng.integers(-127, 128, 50_000) * rng.standard_normal(50_000) * 1024).astype(np.float32)
    rs = np.exp2(rng.uniform(-30, 0, 50_000)).astype(np.float32)
    wa = (rng.choice([-1.0, 1.0], 50_000) * np.exp2(rng.uniform(-149, 127, 50_000))).astype(np.float32)
    wb = (rng.choice([-1.0, 1.0], 50_000) * np.exp2(rng.uniform(-149, 127, 50_000))).astype(np.float32)
    return np.concatenate([ea, acc, wa]), np.concatenate([eb, rs, wb])


def _same_bits(x, y):
    nan = np.isnan(x) & np.isnan(y)
    return nan | (x.view(np.uint32) == y.view(np.uint32))


def test_minus_zero_addend_leaves_every_product_bit_as_it_is():
    a, b = _pairs()
    p = _mul(a, b)
    assert (p == 0).sum() > 100 and np.signbit(p[p == 0]).any()  # +-0 products and underflows are among the pairs
    assert (np.abs(p[np.isfinite(p) & (p != 0)]) < 1.2e-38).any()  # ... and denormal ones
    assert _same_bits(_fma(a, b, NEG_ZERO), p).all()


def test_plus_zero_addend_loses_the_sign_of_a_minus_zero_product():
    a, b = _pairs()
    exact = _mul(a.astype(np.float64), b.astype(np.float64))
    mz = (exact == 0) & np.signbit(exact)  # the exact product is -0: one factor a zero, the signs opposite
    assert mz.sum() >= 20
    got = _fma(a[mz], b[mz], np.float64(0.0))
    assert (got == 0).all() and not np.signbit(got).any()
    assert not _same_bits(got, _mul(a[mz], b[mz])).any()
    # a product that merely rounds to -0 keeps its sign either way (the sum is rounded once, from a nonzero value)
    uf = (exact != 0) & (_mul(a, b) == 0) & np.signbit(exact)
    assert uf.any() and np.signbit(_fma(a[uf], b[uf], np.float64(0.0))).all()


def test_minus_inf_addend_takes_every_finite_product_to_minus_inf():
    a, b = _pairs()
    fin = np.isfinite(a) & np.isfinite(b)  # (the exact product is finite then, even where fp32 would overflow)
    assert np.isinf(_mul(a[fin], b[fin])).any()
    assert np.isneginf(_fma(a[fin], b[fin], NEG_INF)).all()


def test_what_is_left_behaves_as_minus_inf_did():
    """A non-finite product (a padding row's scale, an overflowed accumulator) plus -inf is -inf or NaN: the group
    maximum (fmaxf: the other operand where one is NaN) ignores both, and both fail `v >= th` unless th is -inf --
    which is why the compare is masked by the allowed lanes."""
    a, b = _pairs()
    v = _fma(a, b, NEG_INF)
    assert (np.isneginf(v) | np.isnan(v)).all() and np.isnan(v).any()
    for g in (np.float32(-np.inf), np.float32(-3.5), np.float32(0.0)):
        assert (np.fmax(g, v) == g).all()
    with np.errstate(invalid="ignore"):
        assert not (v >= np.float32(-3.4028235e38)).any()
        assert (v >= np.float32(-np.inf)).sum() == np.isneginf(v).sum() > 0
