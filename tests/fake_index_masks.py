"""OracleIndex with the per-query-mask search of hiprag._native.NativeIndex (search_masks) -- CPU tests of the host
logic of mixed-filter batches only; injected explicitly (``index_factory=``), as tests/fake_index.py."""
import numpy as np

from fake_index import OracleIndex


class MaskOracleIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.mask_calls: list = []  # per search_masks call: (queries, distinct bitmaps referenced)

    def search_masks(self, q, k, masks, mask_of):
        q = np.asarray(q, np.float32)
        if q.ndim == 1:
            q = q[None]
        of = np.asarray(mask_of, np.int32).reshape(-1)
        masks = np.asarray(masks, np.uint64)
        if len(of) != len(q):
            raise ValueError("mask_of has the wrong length")
        if len(masks) and masks.shape[1] * 64 < len(self.rows):
            raise ValueError("row mask shorter than the index")  # as NativeIndex.search_masks
        if ((of < -1) | (of >= len(masks))).any():
            raise ValueError("mask_of entry outside [-1, D)")
        self.mask_calls.append((len(q), len({int(d) for d in of if d >= 0})))
        s = np.empty((len(q), k), np.float32)
        r = np.empty((len(q), k), np.int64)
        before = self.searches
        for i, d in enumerate(of):
            s[i], r[i] = (x[0] for x in self.search(q[i], k, None if d < 0 else masks[d]))
        self.searches = before + 1  # one launch
        return s, r


class GroupMaskOracleIndex(MaskOracleIndex):
    """A multi-device handle: search_masks is there and refuses, as the library does."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0, 0]

    def search_masks(self, q, k, masks, mask_of):
        raise NotImplementedError("per-query masks need a single-device handle")
