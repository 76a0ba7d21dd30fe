"""OracleIndex with the boosted search of hiprag._native.NativeIndex (set_boost / search_boosted / boost_stats),
computed by tests/boost_ref.py -- CPU tests of the host logic of boosted searches only; injected explicitly
(``index_factory=``), as tests/fake_index.py.  The stage counters follow boost_ref.mechanism."""
import numpy as np

import boost_ref as BR
from fake_index import OracleIndex
from oracle import ref_numpy as R


class BoostOracleIndex(OracleIndex):
    MAX_COLS, MAX_WINDOW, MAX_K = 4, 8192, 128

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.cols = [np.zeros(0, np.float32) for _ in range(self.MAX_COLS)]
        self.set_calls: list = []    # per set_boost call: (col, row0, n)
        self.boost_calls: list = []  # per search_boosted call: (queries, k, alpha, betas, masked, probe, window)
        self.stages = {"window": 0, "all_rows": 0}

    def set_boost(self, col, row0, values):
        v = np.asarray(values, np.float32).reshape(-1)
        if not 0 <= col < self.MAX_COLS or not np.isfinite(v).all() or row0 < 0 or row0 + len(v) > len(self.rows):
            raise ValueError("bad boost column, values or rows")  # as hr_index_set_boost
        if len(self.cols[col]) < row0 + len(v):
            grown = np.zeros(row0 + len(v), np.float32)
            grown[: len(self.cols[col])] = self.cols[col]
            self.cols[col] = grown
        self.cols[col][row0:row0 + len(v)] = v
        self.set_calls.append((int(col), int(row0), len(v)))

    def search_boosted(self, q, k, alpha, betas, mask=None, probe=0, window=0):
        q = np.asarray(q, np.float32)
        if q.ndim == 1:
            q = q[None]
        betas = [float(b) for b in betas]
        ok = (1 <= k <= self.MAX_K and 2.0 ** -64 <= alpha <= 2.0 ** 64 and len(betas) <= self.MAX_COLS
              and all(abs(b) <= 2.0 ** 64 for b in betas) and (probe == 0 or k <= probe <= self.MAX_K)
              and (window == 0 or k <= window <= self.MAX_WINDOW))
        if not ok:
            raise ValueError("bad boosted-search arguments")  # as hr_index_search_boosted
        allowed = self.live.copy()
        if mask is not None:
            if len(np.asarray(mask).reshape(-1)) * 64 < len(self.rows):
                raise ValueError("row mask shorter than the index")
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        self.boost_calls.append((len(q), int(k), float(alpha), betas, mask is not None, int(probe), int(window)))
        qp = R.process_queries(q, self.metric)
        cols = self.cols[: len(betas)]
        if len(self.rows) and self.live.any():
            stage = BR.mechanism(self.rows, self.dtype, qp, k, alpha, betas, cols, allowed, self.metric, probe,
                                 window)["stage"]
            self.stages["window"] += int((stage == 1).sum())
            self.stages["all_rows"] += int((stage == 2).sum())
        else:
            self.stages["window"] += len(q)
        return BR.boost_ref(self.rows, self.dtype, qp, k, alpha, betas, cols, allowed, self.metric)

    def boost_stats(self):
        return dict(self.stages)
