"""OracleIndex with the MMR search of hiprag._native.NativeIndex (search_mmr), computed by tests/mmr_ref.py -- CPU tests
of the host logic of MMR searches only; injected explicitly (``index_factory=``), as tests/fake_index.py."""
import numpy as np

from fake_index import AsyncOracleIndex, OracleIndex
from mmr_ref import mmr_ref
from oracle import ref_numpy as R


class MmrOracleIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.mmr_calls: list = []  # per search_mmr call: (queries, k, lam, fetch_k, masked)

    def search_mmr(self, q, k, lam, mask=None, fetch_k=0):
        q = np.asarray(q, np.float32)
        if q.ndim == 1:
            q = q[None]
        if not 1 <= k <= 128 or (fetch_k and not k <= fetch_k <= 128) or not 0.0 <= lam <= 1.0:
            raise ValueError("bad k, fetch_k or lambda")  # as hr_index_search_mmr
        allowed = self.live.copy()
        if mask is not None:
            if len(np.asarray(mask).reshape(-1)) * 64 < len(self.rows):
                raise ValueError("row mask shorter than the index")
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        self.mmr_calls.append((len(q), int(k), float(lam), int(fetch_k), mask is not None))
        return mmr_ref(self.rows, self.dtype, R.process_queries(q, self.metric), k, lam, fetch_k, allowed, self.metric)


class AsyncMmrOracleIndex(MmrOracleIndex, AsyncOracleIndex):
    """... with the asynchronous entry point plain batches take."""
