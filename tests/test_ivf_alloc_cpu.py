"""CPU: the placement of incremental IVF adds (hiprag.ivf.plan_add), the store's index_type parsing
and the header's declarations of the growable-lists entry points.  No GPU call is made."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from hiprag.ivf import _extent_positions, plan_add
from hiprag.rag import HipVectorStore, VectorStoreConfig


class _Lists:
    """The host state IvfIndex keeps, driven through plan_add alone."""

    def __init__(self, nlist):
        z = lambda: np.zeros(nlist, np.int64)  # noqa: E731
        self.nlist, self.counts, self.caps, self.tails, self.ntiles, self.next_tile = nlist, z(), z(), z(), z(), 0
        self.ext = []                     # (list, first tile, tiles), creation order
        self.pos = {}                     # id -> position
        self.filled = [[] for _ in range(nlist)]   # per list: positions in fill order

    def add(self, lists, ids):
        before = (self.counts.copy(), self.caps.copy(), self.tails.copy(), self.ntiles.copy(), self.next_tile)
        out = plan_add(self.counts, self.caps, self.tails, self.ntiles, self.next_tile, lists)
        again = plan_add(*before, lists)
        for a, b in zip(out, again):      # deterministic, and the inputs were not touched
            np.testing.assert_array_equal(a, b)
        for a, b in zip(before[:4], (self.counts, self.caps, self.tails, self.ntiles)):
            np.testing.assert_array_equal(a, b)
        dest, new_ext, counts, caps, tails, ntiles, next_tile = out
        free_before = self.caps - self.counts
        add = np.bincount(lists, minlength=self.nlist)
        # one new extent at most per list, only for lists whose free slots do not suffice, in ascending
        # list order at the end of the index, tile for tile
        assert list(new_ext[:, 0]) == sorted(set(new_ext[:, 0].tolist()))
        t = self.next_tile
        for l, first, nt in new_ext.tolist():
            over = add[l] - free_before[l]
            assert over > 0 and first == t
            # growth rule: the tiles needed, at least 1/8 of the list's tiles so far, at least one tile
            assert nt == max(-(-over // 32), -(-self.ntiles[l] // 8), 1)
            assert nt * 8 >= self.ntiles[l] and nt * 32 >= over
            t += nt
        assert t == next_tile
        for l in range(self.nlist):
            if add[l] <= free_before[l]:
                assert l not in new_ext[:, 0]
        # free slots first, then the new extent; call order inside a list
        new_first = {l: f for l, f, _ in new_ext.tolist()}
        for l in range(self.nlist):
            d = dest[lists == l]
            nfree = min(len(d), int(free_before[l]))
            np.testing.assert_array_equal(d[:nfree], self.tails[l] + np.arange(nfree))
            if len(d) > nfree:
                np.testing.assert_array_equal(d[nfree:], new_first[l] * 32 + np.arange(len(d) - nfree))
            self.filled[l] += d.tolist()
        self.ext += new_ext.tolist()
        for i, p in zip(ids, dest.tolist()):
            assert i not in self.pos
            self.pos[i] = p
        self.counts, self.caps, self.tails, self.ntiles, self.next_tile = counts, caps, tails, ntiles, next_tile
        self.check()

    def check(self):
        # every id placed exactly once: positions are distinct
        assert len(set(self.pos.values())) == len(self.pos) == int(self.counts.sum())
        # extents are tile ranges (tile aligned by construction), disjoint, and tile the index without a gap
        spans = sorted((f, f + n) for _, f, n in self.ext)
        assert all(n >= 1 for _, _, n in self.ext)
        assert [s[0] for s in spans] == [0] + [s[1] for s in spans[:-1]] and (not spans or spans[-1][1] == self.next_tile)
        for l in range(self.nlist):
            mine = [(f, n) for ll, f, n in self.ext if ll == l]
            assert sum(n for _, n in mine) == self.ntiles[l] and self.caps[l] == 32 * self.ntiles[l]
            slots = _extent_positions([f for f, _ in mine], [n for _, n in mine])
            # a list's rows fill its extents front to back: the used slots are a prefix of its slots
            np.testing.assert_array_equal(slots[: self.counts[l]], self.filled[l])
            if self.counts[l] < self.caps[l]:
                assert self.tails[l] == slots[self.counts[l]]


@pytest.mark.parametrize("seed,nlist", [(0, 1), (1, 7), (2, 64)])
def test_random_add_sequences(seed, nlist):
    rng = np.random.default_rng(seed)
    st, nid = _Lists(nlist), 0
    for _ in range(60):
        m = int(rng.choice([0, 1, 2, 31, 32, 33, 100, 700]))
        p = rng.dirichlet(np.full(nlist, 0.3))
        lists = rng.choice(nlist, m, p=p).astype(np.int64)
        st.add(lists, range(nid, nid + m))
        nid += m
    assert len(st.pos) == nid
    # trickle adds do not fragment without bound: one-row adds to a list of T tiles open a new extent only every
    # max(1, T/8) tiles, so the extent count grows with the logarithm of the size
    state, n_ext = tuple(np.zeros(1, np.int64) for _ in range(4)) + (0,), 0
    for _ in range(32 * 200):
        out = plan_add(*state, np.zeros(1, np.int64))
        n_ext, state = n_ext + len(out[1]), out[2:]
    assert state[3][0] >= 200 and n_ext < 50


def test_first_row_of_an_empty_list_and_one_list_taking_everything():
    st = _Lists(5)
    st.add(np.array([3], np.int64), [0])
    assert st.ext == [[3, 0, 1]] and st.pos[0] == 0 and st.tails[3] == 1
    st.add(np.full(1000, 3, np.int64), range(1, 1001))         # one call, one list
    assert [e[0] for e in st.ext] == [3, 3] and st.ext[1][2] == -(-(1000 - 31) // 32)
    assert [st.pos[i] for i in range(1, 32)] == list(range(1, 32))   # the free slots of the first tile first
    st.add(np.array([0, 4, 0], np.int64), [2000, 2001, 2002])
    assert [e[0] for e in st.ext[2:]] == [0, 4] and st.pos[2002] == st.pos[2000] + 1
    with pytest.raises(ValueError):
        plan_add(st.counts, st.caps, st.tails, st.ntiles, st.next_tile, np.array([5], np.int64))


def _cfg(**kw):
    kw.setdefault("index_params", {"persist": False})
    return VectorStoreConfig(backend="hip", collection_name="c", persist_directory="unused", **kw)


def test_index_type_parsing():
    from hiprag.rag.ivf_store import IvfStoreIndex, wants_ivf

    for name in ("ivf_flat", "IVF_FLAT", "Ivf_Flat"):
        assert HipVectorStore(_cfg(index_type=name)).ivf is True
        assert HipVectorStore(_cfg(index_type=name, distance_metric="dot")).ivf is True
    for name in (None, "FLAT", "HNSW", "hnsw", "annoy", ""):
        assert HipVectorStore(_cfg(index_type=name)).ivf is False          # the exact store, no exception
        assert HipVectorStore(_cfg(index_type=name, distance_metric="euclidean")).ivf is False
        assert HipVectorStore(_cfg(index_type=name, index_params={"persist": False, "devices": [0, 1]})).ivf is False
    with pytest.raises(ValueError, match="euclidean"):
        HipVectorStore(_cfg(index_type="IVF_FLAT", distance_metric="euclidean"))
    with pytest.raises(ValueError, match="single-device"):
        HipVectorStore(_cfg(index_type="IVF_FLAT", index_params={"persist": False, "devices": [0, 1]}))
    assert wants_ivf("ivf_flat", "ip", [3]) and not wants_ivf("HNSW", "l2", [0, 1])
    # the IVF index is routed to the worker-thread batch path by what it does not have
    for name in ("search_device", "search_submit_host", "devices"):
        assert not hasattr(IvfStoreIndex, name)
    for name in ("add", "add_device", "remove", "search", "get_rows", "save", "load", "size", "reserve", "close"):
        assert callable(getattr(IvfStoreIndex, name))


def test_snapshot_cleanup_knows_the_side_file(tmp_path):
    from hiprag.rag import persist as P

    pt = P.Paths(str(tmp_path), "docs")
    names = [pt.gen(3, "hri"), pt.gen(3, "hri") + ".ivf.npz", pt.gen(3, "hri") + ".ivf.npz.tmp",
             os.path.join(str(tmp_path), "docs.gov.g3.hri.ivf.npz")]
    for n in names:
        open(n, "w").close()
    assert sorted(pt.all_files()) == sorted(names[:3])       # (a sibling collection's file is not ours)


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(REPO, "include", "hiprag.h")).read()
    for name in ("hr_ivf_search_ext", "hr_index_copy_rows", "hr_ivf_position_mask"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, re.M), name
    from hiprag import _native

    assert {"hr_ivf_search_ext", "hr_index_copy_rows", "hr_ivf_position_mask"} <= set(_native.EXPORTS)
