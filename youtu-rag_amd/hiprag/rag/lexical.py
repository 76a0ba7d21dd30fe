"""Keyword (BM25) search on the GPU: the analyzer and LexicalIndex over the native forward index (hr_lex).

The reference's HybridRetriever only delegates to the vector retriever and says what is missing
(utu/rag/knowledge_retrieval/base_retriever.py:123-139: "a full hybrid retrieval would include keyword-based
search (e.g., BM25) and combine scores").  This is that keyword search; HipVectorStore keeps one LexicalIndex beside
its dense index when ``index_params["lexical"]`` is set, row for row, and HybridRetriever fuses the two rankings.

Analyzer: the lower-cased text is split by ``[\\u4e00-\\u9fff]|[^\\W\\u4e00-\\u9fff]+|[^\\w\\s]`` (words, single
punctuation marks, every CJK ideograph a token of its own) and each token becomes the term id
``crc32(utf-8) % 2**22``.  Batches of ASCII texts go through the host text kernel (hr_hash_words: for ASCII the same
split and the same ids), everything else through ``re`` + ``zlib``.

Scoring (DESIGN.md "Keyword search"): BM25 with N, df and avgdl over the live rows, each term's contribution
computed in fp64 and rounded to 2**-32 fixed point, summed in 64-bit integers -- so a score does not depend on the
summation order and is bit-identical to the CPU restatement in tests/lex_ref.py.
"""
from __future__ import annotations

import re
import zlib

import numpy as np

from .. import _native

TERM_BITS = _native.HR_LEX_TERM_BITS
TERM_SPAN = 1 << TERM_BITS
MAX_QTERMS = _native.HR_LEX_MAX_QTERMS
MAX_K = _native.HR_LEX_MAX_K

_TOKEN = re.compile(r"[\u4e00-\u9fff]|[^\W\u4e00-\u9fff]+|[^\w\s]")


def analyze_py(text: str) -> list[int]:
    """Term ids of one text, in token order (the definition: re + zlib)."""
    return [zlib.crc32(t.encode("utf-8")) % TERM_SPAN for t in _TOKEN.findall(text.lower())]


def analyze_batch(texts, native: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """(term ids uint32, flat; offsets int64 (n + 1,)) of the texts.  An all-ASCII batch takes the host text kernel,
    anything else (or ``native=False``) the Python path: the same ids."""
    texts = list(texts)
    n = len(texts)
    off = np.zeros(n + 1, np.int64)
    if native and n and all(t.isascii() for t in texts):
        data = "".join(texts).encode("ascii")
        boff = np.zeros(n + 1, np.int64)
        np.cumsum(np.fromiter(map(len, texts), np.int64, n), out=boff[1:])
        ids, lengths = _native.hash_words(data, boff, 0, TERM_SPAN, -1, -1, -1)
        np.cumsum(lengths, out=off[1:])
        return ids.astype(np.uint32), off
    lists = [analyze_py(t) for t in texts]
    np.cumsum(np.fromiter(map(len, lists), np.int64, n), out=off[1:])
    ids = np.fromiter((i for t in lists for i in t), np.uint32, int(off[-1]))
    return ids, off


class LexicalIndex:
    """BM25 over texts on one GPU.  Rows are append positions (the store keeps them equal to the dense index's)."""

    def __init__(self, device: int = 0, k1: float = 1.2, b: float = 0.75, index_factory=None):
        self.device, self.k1, self.b = int(device), float(k1), float(b)
        self._factory = index_factory or (lambda: _native.NativeLexIndex(self.device))
        self._index = self._factory()

    def add_texts(self, texts) -> int:
        """Append one row per text; returns the first new row."""
        return self._index.add(analyze_batch(texts))

    def remove_rows(self, rows) -> None:
        self._index.remove(rows)

    def size(self) -> tuple[int, int]:
        return self._index.size()

    def search(self, queries, k: int, mask: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
        """(scores float64 (B, k), rows int64 (B, k)) of the query strings: score descending, then row ascending,
        -inf / -1 past the hits.  ``mask``: uint64 row bitmap (HipVectorStore.filter_bitmap)."""
        return self._index.search(analyze_batch(queries), int(k), mask, self.k1, self.b)

    def clear(self) -> None:
        self._index.close()
        self._index = self._factory()

    def close(self) -> None:
        self._index.close()
