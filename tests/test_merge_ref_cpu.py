"""CPU: the numpy references of tests/merge_ref.py against a brute force (a Python sort of tuples), and the crafted
cases of tests/test_gpu_merge_kernels.py against what they claim: every k_topk_cand case takes the path it is named
for, every k_merge case has the fail flag and k-th score written in its table."""
import struct
from collections import Counter

import numpy as np
import pytest

import merge_ref as M

NI = -np.inf
VALUES = [NI, -3.0, -0.0, 0.0, 0.25, 1.0, float(np.nextafter(1.0, 2.0)), 7.5]


def _brute(recs, k):
    """Top-k of (score, row) tuples, row < 0 absent, by a Python sort; padded with (-inf, -1); and the valid count."""
    valid = sorted((t for t in recs if t[1] >= 0), key=lambda t: (-t[0], t[1]))
    return (valid + [(NI, -1)] * k)[:k], len(valid)


def _random_records(rng, n):
    s = rng.choice(VALUES, n)
    r = rng.permutation(3 * n)[:n].astype(np.int64)
    absent = rng.random(n) < rng.choice([0.0, 0.2, 0.6, 1.0])
    r[absent] = -1 - rng.integers(0, 5, int(absent.sum()))
    s[absent & (rng.random(n) < 0.5)] = np.inf  # absent records that would win
    return s, r


def test_ref_merge_vs_brute_force():
    rng = np.random.default_rng(1)
    for _ in range(300):
        G, B, kc = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 9))
        k = int(rng.integers(1, kc + 1))
        s, r = _random_records(rng, G * B * kc)
        s, r = s.reshape(G, B, kc), r.reshape(G, B, kc)
        bounds = rng.choice(VALUES + [NI, NI, np.inf], (G, B))
        got_s, got_r, got_kth, got_fail = M.ref_merge(M.pack(s, r), bounds, k)
        assert got_s.dtype == np.float32 and got_r.dtype == np.int64 and got_fail.dtype == np.int32
        for q in range(B):
            top, n_valid = _brute([(float(s[g, q, c]), int(r[g, q, c])) for g in range(G) for c in range(kc)], k)
            assert [int(x) for x in got_r[q]] == [t[1] for t in top]
            assert [float(x) for x in got_s[q]] == [float(np.float32(t[0])) for t in top]  # as values: -0.0 == 0.0
            kth = top[k - 1][0] if n_valid >= k else NI
            assert float(got_kth[q]) == kth
            maxb = max(float(b) for b in bounds[:, q])
            assert int(got_fail[q]) == int(maxb > NI and (n_valid < k or not kth > maxb))


def test_ref_merge_sorted_vs_brute_force():
    rng = np.random.default_rng(2)
    for _ in range(300):
        G, B, m = int(rng.integers(1, 5)), int(rng.integers(1, 4)), int(rng.integers(1, 9))
        k = int(rng.integers(1, G * m + 4))
        s, r = _random_records(rng, G * B * m)
        s, r = s.reshape(G, B, m), r.reshape(G, B, m)
        got_s, got_r = M.ref_merge_sorted(M.pack(s, r), k)
        for q in range(B):
            top, _ = _brute([(float(s[g, q, c]), int(r[g, q, c])) for g in range(G) for c in range(m)], k)
            assert [int(x) for x in got_r[q]] == [t[1] for t in top]
            assert [float(x) for x in got_s[q]] == [float(np.float32(t[0])) for t in top]


def test_ref_topk_vs_brute_force():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n, m = int(rng.integers(0, 40)), int(rng.integers(1, 12))
        s, r = _random_records(rng, n)
        got_s, got_r = M.ref_topk(s, r, m)
        top, _ = _brute(list(zip(s.tolist(), r.tolist())), m)
        assert got_r.tolist() == [t[1] for t in top]
        assert got_s.tolist() == [t[0] for t in top]


def test_d2key_restates_the_kernels_key():
    def key(d):  # hr_common.hpp d2key on Python integers
        u = struct.unpack("<Q", struct.pack("<d", 0.0 if d == 0.0 else d))[0]
        return (~u & (2 ** 64 - 1)) if u >> 63 else u | 1 << 63

    rng = np.random.default_rng(4)
    x = np.concatenate([VALUES, [np.inf, 5e-324, -5e-324, 1e308, -1e308], rng.standard_normal(200)])
    keys = M.d2key(x)
    assert keys.dtype == np.uint64
    assert [int(v) for v in keys] == [key(float(d)) for d in x]
    assert key(-0.0) == key(0.0) and key(NI) > 0
    order = np.argsort(x, kind="stable")
    assert all(int(keys[a]) <= int(keys[b]) for a, b in zip(order[:-1], order[1:]))  # monotone
    assert all((int(keys[a]) == int(keys[b])) == (x[a] == x[b]) for a, b in zip(order[:-1], order[1:]))


def test_topk_path_small_restatement():
    """topk_path on segments small enough to classify by hand."""
    ids = np.arange(2000)
    assert M.topk_path(np.zeros(5), np.arange(5), 5) == "all"
    assert M.topk_path(np.zeros(6), np.array([0, 1, 2, 3, 4, -1]), 5) == "all"  # absents do not count
    assert M.topk_path(np.zeros(1024), np.arange(1024), 5) == "level1"  # 1024 tied records still fit
    assert M.topk_path(np.zeros(1025), np.arange(1025), 5) == "full+ids"
    assert M.topk_path(np.arange(2000.0), ids, 5) == "level1"  # integers: distinct upper key words
    close = 1.0 + np.arange(2000) * 2.0 ** -45  # one upper key word
    assert M.topk_path(close, ids, 5) == "full"
    assert M.topk_path(np.concatenate([close, [close[1995]]]), np.arange(2001), 6) == "full"  # 2 ties, both needed
    assert M.topk_path(np.concatenate([close, [close[1995]]]), np.arange(2001), 5) == "full+ids"  # 1 of 2


def test_topk_cases_take_the_paths_they_are_named_for():
    cases = M.topk_cases()
    hit = Counter()
    for c in cases:
        assert c["path"] in M.PATHS, c["name"]
        assert M.topk_path(c["scores"], c["ids"], c["m"]) == c["path"], c["name"]
        assert 1 <= c["m"] <= M.TOPK_MAX and len(c["scores"]) == len(c["ids"])
        valid = c["ids"][c["ids"] >= 0]
        assert len(np.unique(valid)) == len(valid), c["name"]  # ids are distinct
        assert not np.isnan(c["scores"]).any()
        hit[c["path"]] += 1
    assert all(hit[p] >= 2 for p in M.PATHS), hit
    assert {len(c["ids"]) for c in cases} >= set(M.TOPK_LENGTHS)
    assert sum(len(c["ids"]) for c in cases) < 250_000


@pytest.mark.parametrize("G,kc", [(3, 48), (5, 256)])
def test_merge_cases_match_their_table(G, kc):
    for k in (1, 10, kc):
        cases = M.merge_cases(G, kc, k)
        assert len({c["name"] for c in cases}) == len(cases)
        scores, rows, bounds = M.stack_merge_cases(cases)
        assert scores.shape == (G, len(cases), kc) and bounds.shape == (G, len(cases))
        s, r, kth, fail = M.ref_merge(M.pack(scores, rows), bounds, k)
        for q, c in enumerate(cases):
            tag = (c["name"], k)
            assert fail[q] == c["fail"], tag
            assert kth[q] == c["kth"], tag
            valid = rows[:, q][rows[:, q] >= 0]
            assert len(np.unique(valid)) == len(valid), tag  # rows are disjoint across ranks
            if c["rows_at"] == "ascending":
                assert (np.diff(r[q]) > 0).all() and (r[q] == np.sort(valid)[:k]).all(), tag
            else:
                for pos, row in c["rows_at"].items():
                    assert r[q, pos] == row, tag
        by = {c["name"]: q for q, c in enumerate(cases)}
        # the table holds both outcomes, and the cases that tell one rank's bound from the max over ranks
        assert 0 < sum(c["fail"] for c in cases) < len(cases)
        for name in ("last_rank_bound_only", "first_rank_bound_only"):
            b = bounds[:, by[name]]
            assert (b > kth[by[name]]).sum() == 1 and (b > NI).all()
        assert (scores[:, by["absent_inf_scattered"]][rows[:, by["absent_inf_scattered"]] < 0] == np.inf).all()
        for g in range(G):  # absents interleaved with the valid records of every list, not only at its tail
            absent = rows[g, by["absent_inf_scattered"]] < 0
            assert absent.any() and (~absent).any() and absent[:np.nonzero(~absent)[0][-1]].any()


def test_merge_sorted_cases_are_sorted_lists():
    for G in (1, 2, 3, 8):
        for m, k in ((64, 10), (64, 64), (64, 100), (64, 3 * 64 + 5)):
            scores, rows = M.merge_sorted_case(G, m, k)
            assert scores.shape == (G, 5, m)
            for g in range(G):
                for q in range(5):
                    s, r = scores[g, q], rows[g, q]
                    nv = int((r >= 0).sum())
                    assert (r[:nv] >= 0).all() and (r[nv:] < 0).all()  # padding at the tail only
                    srt_s, srt_r = M._sorted_valid(s, r)
                    assert (srt_r == r[:nv]).all() and (srt_s == s[:nv]).all()
            lens = (rows[:, 0] >= 0).sum(1)  # query 0: tails of different lengths, one list all padding
            assert lens[0] < m if G == 1 else len(set(lens.tolist())) >= min(G, 3) and (lens == 0).any()
            assert (rows[:, 1] >= 0).all() and len(np.unique(scores[:, 1])) == 1  # every record tied
            assert (rows[:, 4] < 0).all()
            assert (scores[:, 3][rows[:, 3] >= 0] == NI).any()
            for q in range(5):
                vq = rows[:, q][rows[:, q] >= 0]
                assert len(np.unique(vq)) == len(vq)
            # query 2: the records at positions k-1 and k of the union tie in score and sit in different lists
            s2, r2 = M.ref_merge_sorted(M.pack(scores, rows), min(k + 1, G * m))
            if G >= 2 and k < G * m:
                assert s2[2, k - 1] == s2[2, k]
                where = [int(np.nonzero(rows[:, 2] == r2[2, p])[0][0]) for p in (k - 1, k)]
                assert where[0] != where[1]
