"""OracleIndex with the fused multi-query search of hiprag._native.NativeIndex (search_fused), computed by
tests/fused_ref.py -- CPU tests of the host logic only; injected explicitly (``index_factory=``), as
tests/fake_index.py."""
import numpy as np

from fake_index import OracleIndex
from fused_ref import search_fused_ref


class FusedOracleIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.fused_calls: list = []  # per search_fused call: (groups, k, fetch_k, mode, rrf_k, weights, mask_of)

    def _bits(self, words):
        if len(np.asarray(words).reshape(-1)) * 64 < len(self.rows):
            raise ValueError("row mask shorter than the index")
        return np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little")[: len(self.rows)].astype(bool)

    def search_fused(self, q, groups, k, fetch_k=0, mode="rrf", rrf_k=60.0, weights=None, masks=None, mask_of=None):
        q = np.asarray(q, np.float32)
        groups = [int(m) for m in groups]
        if len(q) != sum(groups):
            raise ValueError("one query per member")
        allowed = self.live
        if mask_of is not None:
            mask_of = [int(d) for d in mask_of]
            m = np.zeros((0, 0), np.uint64) if masks is None else np.atleast_2d(np.asarray(masks, np.uint64))
            if len(mask_of) != len(q) or any(d < -1 or d >= len(m) for d in mask_of):
                raise ValueError("mask_of entry outside [-1, D)")
            allowed = [self.live if d < 0 else self.live & self._bits(m[d]) for d in mask_of]
        self.fused_calls.append((groups, int(k), int(fetch_k), mode, float(rrf_k),
                                 None if weights is None else [float(np.float32(w)) for w in weights], mask_of))
        return search_fused_ref(self.rows, self.dtype, q, groups, int(k), int(fetch_k), mode, float(rrf_k), weights,
                                allowed, self.metric)
