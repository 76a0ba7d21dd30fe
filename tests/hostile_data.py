"""Seeded corpora and query batches that are NOT isotropic Gaussians -- TEST INFRASTRUCTURE ONLY.

Every other GPU corpus of the suite is ``gen_rows`` / ``standard_normal``: row norms within a factor of 30, scores
spread evenly, dot products whose rounding errors cancel.  The five families here are the shapes real embedding
corpora take, each chosen for the part of the search it puts under load:

  anisotropic  a shared mean direction and four outlier dimensions: every cosine score sits in one narrow band, so
               many rows fall inside the guard window of the k-th score
  nonneg       one-sided (|N(0,1)|) rows and queries: every product is positive, accumulation errors cannot cancel
  sparse       1-8 nonzeros per row from {+-0.5, +-1, +-2}, three all-zero rows, repeated one-hot rows: almost every
               score is exactly 0 and the answer is decided by the (score desc, row asc) tie order
  wide         every element +-2^u, u uniform in [-40, 0]: after normalisation most elements lie below f16's smallest
               normal 2^-14 (the absolute term of the guard's storage error); for ip / l2 the row norms span 2^-10 .. 2^7
  neardup      200 rows equal to one unit vector except in 8 tiny elements that spell the member's index: distinct
               stored rows whose exact scores differ by less than the guard's additive constant (1e-9), so no correct
               guard can certify a top-k drawn from them

Corpus makers are pure numpy ``(rng, n, dim) -> float32 rows``; each family has a query maker.  Half of a batch is
planted (a corpus row plus a random vector 5 % of the row's largest magnitude long), half is drawn from the family
itself; batches of the first four families also hold ONE all-zero query (``ZERO_AT``).  Planted and drawn queries
alternate, so every prefix of a batch is a batch of the same make.
"""
from __future__ import annotations

import numpy as np

FAMILIES = ("anisotropic", "nonneg", "sparse", "wide", "neardup")
ZERO_AT = 1           # position of the all-zero query in a batch (families other than neardup)
NEARDUP_MEMBERS = 200
NEARDUP_CODED = 8     # elements that encode the member index (one bit each)
SPARSE_ZERO_ROWS = 3
F16_MIN_NORMAL = 2.0 ** -14


# ---------------------------------------------------------------- corpora
def aniso_frame(dim):
    """The family's unit mean direction and its four outlier dimensions (a function of dim alone, so corpus and
    queries share them)."""
    rng = np.random.default_rng([dim, 4242])
    mu = rng.standard_normal(dim)
    return mu / np.linalg.norm(mu), rng.choice(dim, 4, replace=False)


def anisotropic(rng, n, dim):
    mu, hot = aniso_frame(dim)
    x = mu[None, :] + 0.5 * rng.standard_normal((n, dim)) / np.sqrt(dim)
    x[:, hot] *= 20.0
    return x.astype(np.float32)


def nonneg(rng, n, dim):
    return np.abs(rng.standard_normal((n, dim))).astype(np.float32)


_SPARSE_VALUES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], np.float32)


def sparse(rng, n, dim, zero_rows=True):
    """1..8 nonzeros per row; every 50th row a one-hot +1 in one of 8 columns; rows [n // 2, n // 2 + 3) all-zero
    (a corpus; not the rows drawn as queries)."""
    x = np.zeros((n, dim), np.float32)
    nnz = rng.integers(1, 9, n)
    for j in range(8):
        rows = np.nonzero(nnz > j)[0]
        x[rows, rng.integers(0, dim, len(rows))] = _SPARSE_VALUES[rng.integers(0, len(_SPARSE_VALUES), len(rows))]
    hot = np.arange(0, n, 50)
    x[hot] = 0.0
    x[hot, rng.integers(0, 8, len(hot))] = 1.0
    if zero_rows:
        x[sparse_zero_rows(n)] = 0.0
    return x


def sparse_zero_rows(n):
    return np.arange(n // 2, n // 2 + SPARSE_ZERO_ROWS)


def wide(rng, n, dim, metric="cosine"):
    x = rng.choice(np.array([-1.0, 1.0]), (n, dim)) * np.exp2(rng.uniform(-40.0, 0.0, (n, dim)))
    if metric != "cosine":  # row norms over 2^-10 .. 2^7: still inside f16's range
        x *= np.exp2((np.arange(n) % 18 - 10).astype(np.float64))[:, None]
    return x.astype(np.float32)


def neardup_delta(dtype):
    """Magnitude of the coded elements.  bf16 / f32 keep 2^-20 (1 + bit 2^-7) apart (8 and 24 significand bits, the
    exponent range of fp32); f16 flushes such values to one subnormal, so its code sits just above the smallest
    normal, at 2^-13: the cluster's scores for the centre then spread over at most 7 bits x 2^-26 / 128 = 8.2e-10."""
    return 2.0 ** -13 if dtype == "f16" else 2.0 ** -20


def neardup(rng, n, dim, dtype="bf16"):
    """Returns (rows, member positions in member order, the centre).  Background: N(0, 1/dim) rows (norm ~ 1, score
    with the centre ~ N(0, 1/dim)); member m = the centre with coded element j multiplied by (1 + 2^-7) where bit j of
    m is set."""
    x = (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)
    delta = neardup_delta(dtype)
    c = rng.standard_normal(dim)
    coded = rng.choice(dim, NEARDUP_CODED, replace=False)
    c[coded] = 0.0
    c *= np.sqrt(1.0 - NEARDUP_CODED * delta * delta) / np.linalg.norm(c)
    c[coded] = delta
    centre = c.astype(np.float32)
    pos = rng.choice(n, NEARDUP_MEMBERS, replace=False)
    m = np.arange(NEARDUP_MEMBERS)
    members = np.repeat(centre[None, :], NEARDUP_MEMBERS, axis=0)
    bits = ((m[:, None] >> np.arange(NEARDUP_CODED)[None, :]) & 1).astype(np.float32)
    members[:, coded] = np.float32(delta) * (1.0 + bits * np.float32(2.0 ** -7))
    x[pos] = members
    return x, pos, centre


def corpus(family, seed, n, dim, metric="cosine", dtype="bf16"):
    """Rows of ``family`` (and for neardup the member positions and the centre, else None, None)."""
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    if family == "wide":
        return wide(rng, n, dim, metric), None, None
    if family == "neardup":
        return neardup(rng, n, dim, dtype)
    return {"anisotropic": anisotropic, "nonneg": nonneg, "sparse": sparse}[family](rng, n, dim), None, None


# ---------------------------------------------------------------- queries
def _planted(rng, rows, idx, noise):
    base = rows[idx].astype(np.float64)
    if noise:  # a random direction, as long as `noise` times the row's largest magnitude
        eps = rng.standard_normal(base.shape)
        eps /= np.linalg.norm(eps, axis=1, keepdims=True)
        base = base + noise * np.abs(base).max(axis=1, keepdims=True) * eps
    return base


def queries(family, seed, rows, B, metric="cosine", centre=None):
    """(B, dim) float32 queries for ``rows`` of ``family`` and the planted row of each query (-1: none).
    Even positions are planted, odd ones drawn from the family; position ZERO_AT is all-zero (not for neardup, whose
    position 0 is the cluster centre)."""
    rng = np.random.default_rng([FAMILIES.index(family), seed, 977])
    n, dim = rows.shape
    n_pl = (B + 1) // 2
    idx = rng.choice(n, n_pl, replace=False)
    if family == "sparse":
        idx = np.where(np.abs(rows[idx]).sum(axis=1) > 0, idx, 0)  # (never plant an all-zero row)
    pl = _planted(rng, rows, idx, 0.0 if family == "sparse" else 0.05)
    n_dr = B - n_pl
    if family == "anisotropic":
        dr = anisotropic(rng, max(n_dr, 1), dim)[:n_dr].astype(np.float64)
    elif family == "nonneg":
        pl = np.abs(pl)
        dr = np.abs(rng.standard_normal((n_dr, dim)))
    elif family == "sparse":
        dr = sparse(rng, max(n_dr, 1), dim, zero_rows=False)[:n_dr].astype(np.float64)
    elif family == "wide":
        dr = wide(rng, max(n_dr, 1), dim, metric)[:n_dr].astype(np.float64)
    else:
        dr = rng.standard_normal((n_dr, dim)) / np.sqrt(dim)
    q = np.empty((B, dim), np.float64)
    q[0::2] = pl
    q[1::2] = dr
    planted = np.full(B, -1, np.int64)
    planted[0::2] = idx
    if family == "neardup":
        q[0] = centre
        planted[0] = -1
    elif B > ZERO_AT:
        q[ZERO_AT] = 0.0
    return q.astype(np.float32), planted


def remove_range(n):
    """The contiguous seventh of the rows the parity tests delete."""
    return np.arange(n // 3, n // 3 + n // 7)
