"""GPU: interleaved host-form calls on ONE handle.  The host forms of the derived searches (MMR, collapsed, range, by
example, fused), search_masks and search stage their host arguments in one shared set of device buffers per handle
(HostStage, hr_internal.hpp), so what a call leaves behind -- a staged row mask, per-query bitmaps, mask_of, a larger
or smaller query batch -- must never reach the next call.  Handle A runs every host form in turn, masked calls before
unmasked ones, with batch sizes that grow and shrink (3, 70, 1: 70 is a second 64-query group), on 2,500 bf16 cosine
rows of 96 dims (79 tiles, 40 mask words, the last one partial); then 700 rows are added (50 mask words: the staged
masks must grow) and the sequence runs again with the batch sizes shifted.  Every call's outputs -- padding and
counts included -- must equal, bit for bit, the same call made as the first and only search on a fresh handle holding
the same rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N0, N1 = 96, 2500, 3200
BATCHES = [3, 70, 1]


@pytest.fixture(scope="module")
def native():
    from hiprag import _native

    _native.load_library()
    assert _native.device_count() >= 1, "no HIP device visible"
    return _native


def _bitmap(rng, n):
    """A row mask over n rows, about half of them allowed, no bit set at or beyond n."""
    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
    bits[:n] = rng.random(n) < 0.5
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def _calls(n, shift):
    """The sequence at n rows: (name, function of an index -> tuple of outputs), inputs fixed here."""
    rng = np.random.default_rng(77 + n)
    sizes = iter(BATCHES[(i + shift) % 3] for i in range(13))

    def queries():
        return rng.standard_normal((next(sizes), DIM)).astype(np.float32)

    def groups(Q):  # the members of Q queries: full groups of 16, then the rest (70: a group across the 64-query chunk)
        return [16] * (Q // 16) + ([Q % 16] if Q % 16 else [])

    m = [_bitmap(rng, n) for _ in range(3)]
    calls = []

    def add(name, fn):
        calls.append((name, fn))

    q = queries()
    add("mmr, mask", lambda ix, q=q: ix.search_mmr(q, 5, 0.5, mask=m[0]))
    q = queries()
    add("collapsed, no mask", lambda ix, q=q: ix.search_collapsed(q, 4))
    q = queries()
    add("range, mask", lambda ix, q=q: ix.search_range(q, 0.15, max_hits=16, mask=m[1]))
    q = queries()
    add("range, count only", lambda ix, q=q: ix.search_range(q, 0.15, max_hits=0))
    q = queries()
    ex = [[(7 * b) % n, (13 * b + 1) % n] for b in range(len(q))]
    add("examples, base vectors", lambda ix, q=q, ex=ex: ix.search_examples(ex, 5, q=q, mask=m[2]))
    q = queries()
    ex = [[(11 * b + 2) % n, (5 * b + 3) % n, n - 1 - b] for b in range(len(q))]
    add("examples, no base vectors", lambda ix, ex=ex: ix.search_examples(ex, 5))
    q = queries()
    add("fused, two bitmaps", lambda ix, q=q: ix.search_fused(q, groups(len(q)), 5, masks=np.stack(m[:2]),
                                                              mask_of=np.arange(len(q)) % 2))
    q = queries()
    add("fused, one bitmap", lambda ix, q=q: ix.search_fused(q, groups(len(q)), 5, masks=m[2][None, :],
                                                             mask_of=np.zeros(len(q), np.int32)))
    q = queries()
    add("fused, no bitmap", lambda ix, q=q: ix.search_fused(q, groups(len(q)), 5))
    q = queries()
    add("search_masks, D = 2", lambda ix, q=q: ix.search_masks(q, 6, np.stack(m[1:]), np.arange(len(q)) % 3 - 1))
    q = queries()
    add("search_masks, no bitmap", lambda ix, q=q: ix.search_masks(q, 6, None, np.full(len(q), -1, np.int32)))
    q = queries()
    add("search, mask", lambda ix, q=q: ix.search(q, 6, mask=m[0]))
    q = queries()
    add("search, no mask", lambda ix, q=q: ix.search(q, 6))
    return calls


def _bits(out):
    """The outputs of a call as byte strings (None stays None): equality is equality of every bit."""
    return [None if a is None else (a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes()) for a in out]


def test_interleaved_host_forms_match_fresh_handles(native):
    rows = np.random.default_rng(20240917).standard_normal((N1, DIM)).astype(np.float32)
    group_ids = (np.arange(N1) // 3).astype(np.int32)

    def fill(ix, lo, hi):
        ix.add(rows[lo:hi])
        ix.set_groups(lo, group_ids[lo:hi])

    a = native.NativeIndex(DIM, "bf16", "cosine")
    try:
        for n, lo, shift in ((N0, 0, 0), (N1, N0, 1)):
            fill(a, lo, n)
            assert a.size() == (n, n) and (n + 63) // 64 == (40 if n == N0 else 50) and N0 % 64 != 0
            for name, fn in _calls(n, shift):
                got = _bits(fn(a))
                fresh = native.NativeIndex(DIM, "bf16", "cosine")
                try:
                    fill(fresh, 0, n)
                    want = _bits(fn(fresh))
                finally:
                    fresh.close()
                assert len(got) == len(want)
                for i, (g, w) in enumerate(zip(got, want)):
                    same = g == w  # (kept out of the assert: no megabyte diffs in a failure report)
                    assert same, f"{name} at {n} rows: output {i} differs from a fresh handle's"
        # the masks above decide results (so a stale or a missing one would have shown): a masked search returns
        # allowed rows only, the same search without the mask returns rows the mask forbids
        rng = np.random.default_rng(5)
        q, m = rng.standard_normal((3, DIM)).astype(np.float32), _bitmap(rng, N1)
        allowed = np.unpackbits(m.view(np.uint8), bitorder="little").astype(bool)
        assert allowed[a.search(q, 6, mask=m)[1]].all()
        assert not allowed[a.search(q, 6)[1]].all()
    finally:
        a.close()
