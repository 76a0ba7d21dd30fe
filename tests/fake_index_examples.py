"""OracleIndex with the search by example of hiprag._native.NativeIndex (build_queries / search_examples), computed by
tests/examples_ref.py -- CPU tests of the host logic only; injected explicitly (``index_factory=``), as
tests/fake_index.py."""
import numpy as np

from examples_ref import build_ref, default_weights, examples_ref
from fake_index import OracleIndex


class ExamplesOracleIndex(OracleIndex):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.devices = [0]
        self.example_calls: list = []  # per search_examples call: (examples, weights, k, has q, masked, keep)

    def _check(self, examples, weights, q):
        examples = [[int(r) for r in e] for e in examples]
        weights = default_weights(examples) if weights is None else [[np.float32(w) for w in ws] for ws in weights]
        for e, w in zip(examples, weights):  # as hr_index_search_examples
            if len(e) > 32 or (not e and q is None) or len(w) != len(e):
                raise ValueError("bad example list")
            if any(r < 0 or r >= len(self.rows) or not self.live[r] for r in e) or not np.isfinite(w).all():
                raise ValueError("bad example row or weight")
        return examples, weights

    def build_queries(self, examples, weights=None, q=None):
        examples, weights = self._check(examples, weights, q)
        return build_ref(self.rows, self.dtype, examples, weights, q)

    def search_examples(self, examples, k, weights=None, q=None, mask=None, keep=False):
        examples, weights = self._check(examples, weights, q)
        if k <= 0:
            raise ValueError("k must be positive")
        allowed = self.live.copy()
        if mask is not None:
            if len(np.asarray(mask).reshape(-1)) * 64 < len(self.rows):
                raise ValueError("row mask shorter than the index")
            bits = np.unpackbits(np.asarray(mask, np.uint64).view(np.uint8), bitorder="little")[: len(allowed)]
            allowed &= bits.astype(bool)
        self.example_calls.append((examples, weights, int(k), q is not None, mask is not None, bool(keep)))
        return examples_ref(self.rows, self.dtype, examples, k, weights, q, allowed, self.metric, keep)
