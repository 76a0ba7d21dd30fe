"""OracleIndex with the range search of hiprag._native.NativeIndex (search_range), computed by tests/range_ref.py -- CPU
tests of the host logic of range searches only; injected explicitly (``index_factory=``), as tests/fake_index.py."""
import numpy as np

from fake_index import OracleIndex
from oracle import ref_numpy as R
from range_ref import range_ref, thresholds


class RangeOracleIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.range_calls: list = []  # per search_range call: (queries, thresholds, max_hits, masked)

    def search_range(self, q, min_score, max_hits=1024, mask=None):
        q = np.asarray(q, np.float32)
        if q.ndim == 1:
            q = q[None]
        t = thresholds(min_score, len(q))
        if not 0 <= max_hits <= 65536 or np.isnan(t).any():
            raise ValueError("bad max_hits or min_score")  # as hr_index_search_range
        allowed = self.live.copy()
        if mask is not None:
            if len(np.asarray(mask).reshape(-1)) * 64 < len(self.rows):
                raise ValueError("row mask shorter than the index")
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        self.range_calls.append((len(q), t.tolist(), int(max_hits), mask is not None))
        s, r, c = range_ref(self.rows, self.dtype, R.process_queries(q, self.metric), t, max_hits, allowed, self.metric)
        return (s, r, c) if max_hits else (None, None, c)
