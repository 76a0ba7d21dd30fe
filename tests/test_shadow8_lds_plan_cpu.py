"""CPU: the exactness argument of the shadow-8 FILTER's shared threshold refresh (scan_body: slice_apply), restated
in numpy over random monotone tables.

The table holds one key per (part, group) of a query, and keys only rise (atomicMax).  k_select takes
thr = max(min over the FINAL table, floor); the FILTER is exact iff no wave ever filters with a threshold above thr.
The new refresh builds a wave's threshold from (a) the min over a slice's snapshot of the table at some earlier
time, written to a row that (b) other waves read later, possibly stale or mixed from several times, and it
(c) publishes a wave's group maximum only where it beats the wave's own threshold.  Pinned here:
  1. whatever the order of slice refreshes and row reads, a threshold never exceeds max(min of the final table, floor);
  2. the publish rule withholds only values that could not lift the min over groups above the withholding wave's
     threshold -- so a table built under the rule gives every wave the thresholds the full table would, wherever those
     exceed what the wave already had."""
import numpy as np

NP_, G, Q, WAVES, NSL = 4, 32, 64, 8, 8
QS = Q // NSL  # queries per slice


def test_thresholds_from_slices_and_stale_rows_never_exceed_the_final_threshold():
    rng = np.random.default_rng(0)
    for trial in range(20):
        floor = rng.normal(-1.0, 1.0, Q).astype(np.float32)
        table = np.full((NP_, Q, G), -np.inf, np.float32)
        table[:] = rng.normal(-2.0, 1.0, table.shape)  # the SAMPLE pass's maxima
        if trial % 4 == 0:
            table[rng.integers(NP_), :, rng.integers(G)] = -np.inf  # a group nobody has published to yet
        row = np.full(Q, -np.inf, np.float32)
        th = np.tile(floor, (WAVES, 1))  # the first refresh takes the floor
        used = []  # (wave, thresholds it filtered with)
        r = np.arange(WAVES)
        for step in range(200):
            # the table only rises
            p, q, g = rng.integers(NP_), rng.integers(Q), rng.integers(G)
            table[p, q, g] = max(table[p, q, g], rng.normal(0.0, 1.5))
            w = rng.integers(WAVES)
            ev = rng.integers(3)
            if ev == 0:  # slice refresh: min over all parts and groups of a snapshot, written (not max'd) to the row
                s = r[w] % NSL
                r[w] += 1
                row[s * QS:(s + 1) * QS] = table[:, s * QS:(s + 1) * QS, :].min(axis=(0, 2))
            elif ev == 1:  # read of the row, any subset of its slots (a read torn across slots)
                m = rng.random(Q) < 0.7
                th[w, m] = np.maximum(th[w, m], row[m])
            else:
                used.append((w, th[w].copy()))
        final = np.maximum(table.min(axis=(0, 2)), floor)
        for w, t in used:
            assert np.all(t <= final), (trial, w)
        assert np.all(th <= final[None, :])


def test_publish_rule_withholds_nothing_a_threshold_could_use():
    rng = np.random.default_rng(1)
    for trial in range(20):
        # one query: each wave owns some rows of every group of one part and sees their scores tile by tile
        full = rng.normal(-2.0, 1.0, (NP_, G)).astype(np.float32)  # every maximum published (the old rule's upper end)
        ruled = full.copy()                                        # published under gmax > th
        floor = np.float32(rng.normal(-1.5, 0.5))
        th = np.full(WAVES, floor, np.float32)
        for step in range(300):
            w = rng.integers(WAVES)
            p = w % NP_
            gmax = rng.normal(-0.5, 1.5, G).astype(np.float32)  # the wave's group maxima since its last refresh
            before = th[w]
            full[p] = np.maximum(full[p], gmax)
            pub = gmax > before
            ruled[p, pub] = np.maximum(ruled[p, pub], gmax[pub])
            # the table stays a set of true scores: never above what publishing everything gives
            assert np.all(ruled <= full)
            # what the wave can learn: the min over the table, if above its threshold
            want = max(before, full.min())
            got = max(before, ruled.min())
            # a withheld value is <= th: it cannot lift the min over groups above th, so above th the two agree
            # for the wave's own contribution -- entries of ruled that lag full are all <= some wave's threshold
            lag = ruled < full
            assert np.all(full[lag] <= th.max()), trial
            assert got <= want
            if want > th.max():  # beyond every wave's threshold nothing was withheld
                assert got == want, (trial, step, got, want)
            th[w] = got
        assert max(ruled.min(), floor) <= max(full.min(), floor)
