"""CPU: the two argument helpers every host-form wrapper of NativeIndex goes through -- _queries (contiguous float32
(B, dim), width checked) and _mask_words (uint64 words, one bit per index row) -- with the messages the wrappers have
always raised.  No library is loaded and no device is touched: the object is made without __init__."""
import numpy as np
import pytest

from hiprag._native import NativeIndex


def bare_index(dim, n_rows):
    ix = NativeIndex.__new__(NativeIndex)
    ix.dim = dim
    ix._h = None  # (close() in __del__ then does nothing)
    ix.size = lambda: (n_rows, n_rows)
    return ix


def test_queries_and_mask_words_check_their_arguments():
    ix = bare_index(8, 130)  # 130 rows: 3 mask words
    one = ix._queries(np.arange(8, dtype=np.float64))  # a 1-D query is one query
    assert one.shape == (1, 8) and one.dtype == np.float32 and one.flags.c_contiguous
    assert np.array_equal(one[0], np.arange(8, dtype=np.float32))
    strided = np.ones((3, 16), np.float32)[:, ::2]
    got = ix._queries(strided)
    assert got.shape == (3, 8) and got.flags.c_contiguous
    with pytest.raises(ValueError) as e:
        ix._queries(np.zeros((2, 7), np.float32))
    assert str(e.value) == "query dim 7 != index dim 8"
    with pytest.raises(ValueError) as e:
        ix._queries(np.zeros(9, np.float32))
    assert str(e.value) == "query dim 9 != index dim 8"

    assert ix._mask_words(None) is None
    m = ix._mask_words(np.ones((1, 3), np.uint64))
    assert m.shape == (3,) and m.dtype == np.uint64
    with pytest.raises(ValueError) as e:
        ix._mask_words(np.ones(2, np.uint64))
    assert str(e.value) == "row mask has 2 words, the index 130 rows (needs 3)"
