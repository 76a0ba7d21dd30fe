"""CPU: the bias fold of the shadow-8 scan (tests/shadow8_bias_ref.py) under a chained fp32 emulation.

The fold identity in exact arithmetic, and |folded fp32 chain - exact| <= the plain sum's accumulation term + the
per-query bias term, for every in-instruction order emulated, on the queries and rows that stress it: sums of the
query that do not cancel (all-positive, constant), that cancel exactly, that live in one instruction only, forty binades
of dynamic range, rows at the ends of the int8 range."""
from fractions import Fraction

import numpy as np
import pytest

import shadow8_bias_ref as S

DIMS = [64, 1024]


def _queries(dim):
    rng = np.random.default_rng(dim)
    g = rng.standard_normal(dim)
    fam = {
        "gaussian": g / np.linalg.norm(g),
        "all_positive": np.abs(g) / np.linalg.norm(g),
        "constant": np.full(dim, 1.0 / np.sqrt(dim)),
        "one_block": np.concatenate([np.zeros(16), np.abs(rng.standard_normal(16)), np.zeros(dim - 32)]),
        "alternating": np.where(np.arange(dim) % 2 == 0, 1.0, -1.0) / np.sqrt(dim),
        "zero_sum": np.concatenate([np.abs(g[:dim // 2]), -np.abs(g[:dim // 2])]) / np.linalg.norm(g),
        "forty_binades": g * 2.0 ** -(np.arange(dim) % 40),
    }
    fam["one_block"] /= np.linalg.norm(fam["one_block"])
    fam["forty_binades"] = fam["forty_binades"] / np.linalg.norm(fam["forty_binades"])
    names = list(fam)
    qh = np.stack([fam[n] for n in names]).astype(np.float16).astype(np.float64)  # (subnormals and zeros included)
    return names, qh


def _rows(dim):
    rng = np.random.default_rng(dim + 1)
    return np.stack([
        np.full(dim, 127.0),
        np.full(dim, -127.0),
        np.where(np.arange(dim) % 2 == 0, 127.0, -127.0),
        np.zeros(dim),
        np.clip(np.rint(rng.standard_normal(dim) * 40), -127, 127),
    ])


@pytest.mark.parametrize("dim", DIMS)
def test_fold_identity_exact(dim):
    """sum q^_d (1152 + s_d) - 1152 sum q^_d = sum q^_d s_d in rational arithmetic (f16 values are dyadic)."""
    names, qh = _queries(dim)
    s = _rows(dim)
    for b in range(len(qh)):
        qf = [Fraction(float(x)) for x in qh[b]]
        c = 1152 * sum(qf)
        assert Fraction(float(S.c_q(qh[b:b + 1])[0][0])) == c  # (fp64 holds it: a sum of dyadic f16 values)
        for r in range(len(s)):
            sf = [Fraction(int(x)) for x in s[r]]
            folded = sum(q * (1152 + x) for q, x in zip(qf, sf)) - c
            assert folded == sum(q * x for q, x in zip(qf, sf)), (names[b], r)


def test_operands_are_f16_exact():
    """1152 + s for s in -128 .. 127 is 1024 + byte, an integer of [1024, 1279]: exact in f16 (step 1 up to 2048)."""
    m = 1152.0 + np.arange(-128, 128)
    assert m.min() == 1024 and m.max() == S.OPERAND_MAX
    assert np.array_equal(m.astype(np.float16).astype(np.float64), m)


@pytest.mark.parametrize("order", ["forward", "reverse", "pairwise"])
@pytest.mark.parametrize("dim", DIMS)
def test_folded_chain_within_bound(dim, order):
    names, qh = _queries(dim)
    s = _rows(dim)
    _, start = S.c_q(qh)
    approx = S.chained_fp32(qh, S.OFFSET + s, start, order).astype(np.float64)
    exact = qh @ s.T
    plain = (dim + 64) * 2.0 ** -23 * np.linalg.norm(qh, axis=1)[:, None] * np.linalg.norm(s, axis=1)[None, :]
    term = S.bias_term(qh)[:, None]
    err = np.abs(approx - exact)
    for b, n in enumerate(names):
        print(f"BIAS {dim} {order} {n}: max err {err[b].max():.3e}, plain {plain[b].max():.3e}, term {term[b, 0]:.3e}")
    assert np.all(err <= plain + term), (err, plain + term)
