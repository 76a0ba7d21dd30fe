"""IVF-flat candidate generation on the HIP index (BASELINE.json configs[4]: "50M×1024 fp16 ANN
candidate-gen + cross-encoder rerank top-100").

The reference has no ANN index of its own: its production store is Chroma's HNSW
(chroma_store.py:41-59, approximate, third-party).  This is the MI355X replacement for that
approximate stage: an inverted-file index whose lists are stored in the same 32-row MFMA tile
layout as the exact index (one ``NativeIndex`` holds the rows in list order, every list starting
on a tile; pad rows are dead), searched by ``hr_ivf_search`` (youtu-rag_amd/csrc/hr_ivf.hip):

  * coarse stage: exact canonical fp64 scores of every centroid, top-``nprobe`` lists per query;
  * list stage: exact canonical fp64 scores of every row of the probed lists, top-k per query.

Results are therefore *exact within the probed lists* (bit-identical to the oracle's restatement,
tests/test_gpu_ivf.py); recall against the full exact search is the ANN trade-off, and
``nprobe = nlist`` is the exact search.  Each probed tile is read once per query, so a batch reads
about ``B * nprobe / nlist`` of the corpus instead of all of it.

Training (spherical k-means for cosine, max-inner-product k-means for dot) and list assignment
are build-time GEMMs and run through PyTorch (hipBLASLt); only the search is on the query path.
Growth: a bulk-built index keeps one contiguous tile range per list (``list_tiles``, ``hr_ivf_search``).  The
first incremental ``add`` switches it to *extents*: every list is a sequence of (first tile, tile count) ranges,
new ranges are allocated at the end of the index (``plan_add``), and the search goes through
``hr_ivf_search_ext``.  ``remove`` tombstones positions, ``compact`` rebuilds one extent per list without dead
rows, ``save`` / ``load`` persist rows and tables.  Results stay those of the oracle's restatement.

Multi-GPU: every rank holds its row shard's share of every list (shared centroids), returns its
exact top-k of its visible rows with bound -inf, and ``IvfShardedSearch`` merges them with the
same packed all-gather + merge as the exact search.
"""
from __future__ import annotations

import os

import numpy as np

from . import _native
from .dist import ShardedSearch


def _round64(d: int) -> int:
    return (d + 63) // 64 * 64


def plan_add(counts, caps, tails, ntiles, next_tile: int, new_lists, nlist: int | None = None):
    """Placement of one ``add`` call (pure, host, deterministic).

    State per list: ``counts`` slots used (live or tombstoned), ``caps`` slots allocated (32 per tile), ``tails``
    the position of the next free slot (meaningful where counts < caps: a list's free slots are the end of its
    last extent), ``ntiles`` tiles allocated; ``next_tile`` is the first unallocated tile of the index.
    ``new_lists[i]`` is the list of the call's i-th row.

    Within a list the rows keep the order of the call: they first fill the free slots, and what does not fit goes
    to ONE new extent of max(tiles needed, ceil(ntiles / 8), 1) tiles (so trickle adds do not fragment without
    bound); new extents are allocated at the end of the index in ascending list order.

    Returns (dest int64 (m,), new_ext int64 (j, 3) rows of (list, first tile, tiles), counts, caps, tails, ntiles,
    next_tile) -- the arrays are new, the inputs are left alone."""
    counts, caps, tails, ntiles = (np.asarray(a, np.int64) for a in (counts, caps, tails, ntiles))
    new_lists = np.asarray(new_lists, np.int64).reshape(-1)
    nl = len(counts) if nlist is None else int(nlist)
    m = len(new_lists)
    if m and (new_lists.min() < 0 or new_lists.max() >= nl):
        raise ValueError("list out of range")
    add = np.bincount(new_lists, minlength=nl).astype(np.int64)
    free = caps - counts
    over = np.maximum(add - free, 0)
    grow = np.where(over > 0, np.maximum(np.maximum((over + 31) // 32, (ntiles + 7) // 8), 1), 0)
    first = int(next_tile) + np.cumsum(grow) - grow          # (ascending list order)
    order = np.argsort(new_lists, kind="stable")
    start = np.cumsum(add) - add
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m, dtype=np.int64) - start[new_lists[order]]
    fits = rank < free[new_lists]
    dest = np.where(fits, tails[new_lists] + rank, first[new_lists] * 32 + rank - free[new_lists])
    grown = np.nonzero(grow)[0]
    new_ext = np.stack([grown, first[grown], grow[grown]], axis=1).astype(np.int64) if len(grown) else \
        np.zeros((0, 3), np.int64)
    tails2 = np.where(over > 0, first * 32 + over, tails + add)
    return dest, new_ext, counts + add, caps + 32 * grow, tails2, ntiles + grow, int(next_tile) + int(grow.sum())


def _extent_positions(first, nt):
    """Positions of the extents (first tile, tiles) in order, concatenated."""
    first, nt = np.asarray(first, np.int64), np.asarray(nt, np.int64)
    n = nt * 32
    total = int(n.sum())
    if total == 0:
        return np.zeros(0, np.int64)
    base = np.repeat(first * 32 - (np.cumsum(n) - n), n)
    return base + np.arange(total, dtype=np.int64)


class IvfIndex:
    """IVF-flat index of one shard on one GPU."""

    def __init__(self, dim: int, nlist: int, dtype: str = "f16", metric: str = "cosine", device: int = 0):
        import torch

        if metric not in ("cosine", "ip", "dot"):
            raise NotImplementedError("IVF lists support cosine and dot (inner product)")
        self.torch = torch
        self.dim, self.nlist, self.dtype = int(dim), int(nlist), dtype
        self.metric = "ip" if metric == "dot" else metric
        self.dev = torch.device("cuda", device)
        self.device = device
        self.dpad = _round64(self.dim)
        # list-order rows are never scanned by the exact search: no scan shadows
        self.index = _native.NativeIndex(self.dim, dtype, self.metric, device, no_shadows=True)
        self.centroids = None      # (nlist, dpad) fp32, processed (unit norm for cosine)
        self.list_tiles = None     # (nlist + 1,) int64 tile offsets
        self.ids = None            # (positions,) int64 original id per stored position, -1 for pads
        self.max_list_tiles = 0
        self.n = 0
        self.id_base = 0            # lists_of_rows / pos_of_id are indexed by id - id_base
        self.lists_of_rows = None   # (ids,) int64 device: list of the row with that id, -1 = none
        self.pos_of_id = None       # (ids,) int64 host: stored position of that id, -1 = none
        # extent form (after the first incremental add, compact() or load()); host tables are the truth, the
        # device copies (ext_off, ext, list_ntiles) are rebuilt after every change
        self.extents = False
        self.ext_list = self.ext_first = self.ext_nt = None   # host, creation order
        self.counts = self.caps = self.tails = self.ntiles = None
        self.next_tile = 0
        self.ext_off = self.ext = self.list_ntiles = None     # device
        self._ids_buf = None

    # ---------------------------------------------------------------- build
    def _process(self, x):
        torch = self.torch
        x = x.to(torch.float32)
        if self.metric == "cosine":
            x = torch.nn.functional.normalize(x, dim=1)
        return x

    def train(self, sample, iters: int = 10, seed: int = 0):
        """k-means on a (m, dim) fp32 device sample: spherical for cosine, max-inner-product with
        unit centroids for dot.  Empty lists keep their previous centroid."""
        torch = self.torch
        x = self._process(sample.to(self.dev))
        m = x.shape[0]
        if m < self.nlist:
            raise ValueError(f"training sample ({m}) smaller than nlist ({self.nlist})")
        g = torch.Generator(device=self.dev)
        g.manual_seed(int(seed))
        cent = x[torch.randperm(m, generator=g, device=self.dev)[: self.nlist]].clone()
        cent = torch.nn.functional.normalize(cent, dim=1)
        for _ in range(iters):
            assign = self._assign(x, cent)
            sums = torch.zeros_like(cent).index_add_(0, assign, x)
            cnt = torch.bincount(assign, minlength=self.nlist)
            upd = cnt > 0
            cent[upd] = torch.nn.functional.normalize(sums[upd], dim=1)
        c = torch.zeros((self.nlist, self.dpad), dtype=torch.float32, device=self.dev)
        c[:, : self.dim] = cent
        self.centroids = c.contiguous()
        return self

    def _assign(self, x, cent, chunk: int = 1 << 16):
        torch = self.torch
        out = torch.empty(x.shape[0], dtype=torch.int64, device=self.dev)
        for i in range(0, x.shape[0], chunk):
            out[i:i + chunk] = torch.argmax(x[i:i + chunk] @ cent.T, dim=1)
        return out

    def build(self, n: int, rows, id_offset: int = 0, chunk: int = 1 << 18):
        """Bulk build from ``rows(i0, i1) -> (i1 - i0, dim) fp32 device tensor`` (raw vectors; the
        store normalises for cosine).  Two passes: list assignment, then placement by list."""
        torch = self.torch
        if self.centroids is None:
            raise RuntimeError("train() the coarse quantizer first")
        if self.n or self.extents:
            raise RuntimeError("build() is the bulk path of an empty index; use add() to grow it")
        cent = self.centroids[:, : self.dim]
        lists = torch.empty(n, dtype=torch.int64, device=self.dev)
        for i in range(0, n, chunk):
            lists[i:i + chunk] = self._assign(self._process(rows(i, min(n, i + chunk))), cent)
        counts = torch.bincount(lists, minlength=self.nlist)
        tiles = (counts + 31) // 32
        list_tiles = torch.zeros(self.nlist + 1, dtype=torch.int64, device=self.dev)
        list_tiles[1:] = torch.cumsum(tiles, 0)
        order = torch.sort(lists, stable=True).indices          # rows grouped by list, row order inside
        first = torch.zeros(self.nlist, dtype=torch.int64, device=self.dev)
        first[1:] = torch.cumsum(counts, 0)[:-1]
        rank = torch.arange(n, dtype=torch.int64, device=self.dev) - first[lists[order]]
        dest = torch.empty(n, dtype=torch.int64, device=self.dev)
        dest[order] = list_tiles[lists[order]] * 32 + rank
        total = int(list_tiles[-1].item()) * 32
        self.index.reserve(total)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for i in range(0, n, chunk):
            j = min(n, i + chunk)
            x = rows(i, j).to(torch.float32).contiguous()
            d = dest[i:j].contiguous()
            self.index.add_device_at(x.data_ptr(), j - i, d.data_ptr(), total, stream=stream)
        ids = torch.full((max(total, 1),), -1, dtype=torch.int64, device=self.dev)
        ids[dest] = torch.arange(n, dtype=torch.int64, device=self.dev) + int(id_offset)
        self.ids, self.list_tiles = ids, list_tiles
        self.max_list_tiles = int(tiles.max().item()) if n else 0
        self.n = n
        self.lists_of_rows = lists  # row -> list (tests, the oracle restatement)
        self.id_base = int(id_offset)
        return self

    def build_synthetic(self, seed: int, row0: int, n: int, chunk: int = 1 << 18):
        """Build from the counter-based synthetic corpus rows [row0, row0 + n) (ids = global rows)."""
        torch = self.torch
        stream = lambda: torch.cuda.current_stream(self.dev).cuda_stream  # noqa: E731

        def rows(i0, i1):
            x = torch.empty((i1 - i0, self.dim), dtype=torch.float32, device=self.dev)
            _native.gen_rows_device(seed, row0 + i0, i1 - i0, self.dim, x.data_ptr(), stream())
            return x

        return self.build(n, rows, id_offset=row0, chunk=chunk)

    def list_members(self) -> list[np.ndarray]:
        """Original ids of every list (host; tests and diagnostics)."""
        ids = self.ids.cpu().numpy()
        if self.extents:
            order = np.argsort(self.ext_list, kind="stable")
            out = []
            for l in range(self.nlist):
                e = order[self.ext_list[order] == l]
                got = ids[_extent_positions(self.ext_first[e], self.ext_nt[e])]
                out.append(got[got >= 0])
            return out
        lt = self.list_tiles.cpu().numpy()
        return [ids[lt[l] * 32: lt[l + 1] * 32][ids[lt[l] * 32: lt[l + 1] * 32] >= 0] for l in range(self.nlist)]

    # ---------------------------------------------------------------- search
    def search_candidates(self, q, k: int, nprobe: int, cand, bound, probes=None, mask_ptr: int = 0, stream=None):
        """Exact top-k of the probed lists' rows for a (B, dim) fp32 device batch, as B*k candidate
        records (score, global id) + bounds (all -inf), on ``stream`` (default: current)."""
        torch = self.torch
        if self.ids is None:
            raise RuntimeError("build() the index first")
        st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        q = q.contiguous()
        if self.extents:
            self.index.ivf_search_ext(self.centroids.data_ptr(), self.nlist, self.ext_off.data_ptr(),
                                      self.ext.data_ptr() if self.ext.numel() else 0, self.list_ntiles.data_ptr(),
                                      self.max_list_tiles, self.ids.data_ptr(), q.data_ptr(), q.shape[0], nprobe, k,
                                      cand.data_ptr(), bound.data_ptr(), 0 if probes is None else probes.data_ptr(),
                                      mask_ptr, st)
            return
        self.index.ivf_search(self.centroids.data_ptr(), self.nlist, self.list_tiles.data_ptr(), self.max_list_tiles,
                              self.ids.data_ptr(), q.data_ptr(), q.shape[0], nprobe, k, cand.data_ptr(),
                              bound.data_ptr(), 0 if probes is None else probes.data_ptr(), mask_ptr, st)

    def search(self, q, k: int, nprobe: int):
        """(scores (B, k) fp32, ids (B, k) int64) device tensors; -inf / -1 padding."""
        torch = self.torch
        B = q.shape[0]
        cand = torch.empty((B, k, 2), dtype=torch.float64, device=self.dev)
        bound = torch.empty(B, dtype=torch.float64, device=self.dev)
        self.search_candidates(q, k, nprobe, cand, bound)
        s = cand[..., 0].to(torch.float32)
        r = cand.view(torch.int64)[..., 1].clone()
        return s, r

    # ---------------------------------------------------------------- growth
    @property
    def n_ext(self) -> int:
        return len(self.ext_list) if self.extents else self.nlist

    @property
    def n_positions(self) -> int:
        """Stored positions (32 per allocated tile)."""
        return int(self.ids.shape[0]) if self.ids is not None else 0

    def n_dead(self) -> int:
        """Used slots that hold a removed row (what compact() reclaims)."""
        used = int(self.counts.sum()) if self.extents else self.n
        return used - self.index.size()[1]

    def _grow_id_maps(self, n_ids: int):
        torch = self.torch
        have = 0 if self.pos_of_id is None else len(self.pos_of_id)
        if n_ids <= have:
            return
        pos = np.full(n_ids, -1, np.int64)
        lst = torch.full((n_ids,), -1, dtype=torch.int64, device=self.dev)
        if have:
            pos[:have] = self.pos_of_id
            lst[:have] = self.lists_of_rows
        self.pos_of_id, self.lists_of_rows = pos, lst

    def _to_extents(self):
        """Switch to the extent tables (idempotent): a bulk-built index becomes one extent per list."""
        if self.extents:
            return
        nl = self.nlist
        if self.ids is not None:  # bulk built
            lt = self.list_tiles.cpu().numpy().astype(np.int64)
            ids = self.ids.cpu().numpy()
            cnt = np.bincount(self.lists_of_rows.cpu().numpy(), minlength=nl).astype(np.int64) if self.n else \
                np.zeros(nl, np.int64)
            self.ext_list, self.ext_first, self.ext_nt = np.arange(nl, dtype=np.int64), lt[:-1].copy(), np.diff(lt)
            self.counts, self.ntiles = cnt, np.diff(lt)
            self.next_tile = int(lt[-1])
            pos = np.full(self.n, -1, np.int64)
            live = np.nonzero(ids[: self.next_tile * 32] >= 0)[0]
            pos[ids[live] - self.id_base] = live
            self.pos_of_id = pos
            self._ids_buf = self.ids[: self.next_tile * 32]
        else:
            self.ext_list = self.ext_first = self.ext_nt = np.zeros(0, np.int64)
            self.counts, self.ntiles = np.zeros(nl, np.int64), np.zeros(nl, np.int64)
            self.next_tile = 0
            self.pos_of_id = np.zeros(0, np.int64)
            self.lists_of_rows = self.torch.zeros(0, dtype=self.torch.int64, device=self.dev)
            self._ids_buf = self.torch.zeros(0, dtype=self.torch.int64, device=self.dev)
        self.caps = self.ntiles * 32
        self.tails = self.ext_first[:nl] * 32 + self.counts if len(self.ext_first) else np.zeros(nl, np.int64)
        self.extents = True
        self.list_tiles = None
        self._sync_tables()

    def _sync_tables(self):
        """Device copies of the extent tables (CSR by list, creation order inside a list) and the ids view."""
        torch = self.torch
        order = np.argsort(self.ext_list, kind="stable")
        off = np.zeros(self.nlist + 1, np.int64)
        off[1:] = np.cumsum(np.bincount(self.ext_list, minlength=self.nlist))
        ext = np.stack([self.ext_first[order], self.ext_nt[order]], axis=1) if len(order) else np.zeros((0, 2), np.int64)
        self.ext_off = torch.from_numpy(off).to(self.dev)
        self.ext = torch.from_numpy(np.ascontiguousarray(ext)).to(self.dev)
        self.list_ntiles = torch.from_numpy(self.ntiles.copy()).to(self.dev)
        self.max_list_tiles = int(self.ntiles.max()) if self.nlist else 0
        total = self.next_tile * 32
        if self._ids_buf.shape[0] < total:  # (amortised: the buffer grows by half)
            buf = torch.full((max(total, self._ids_buf.shape[0] * 3 // 2),), -1, dtype=torch.int64, device=self.dev)
            buf[: self._ids_buf.shape[0]] = self._ids_buf
            self._ids_buf = buf
        self.ids = self._ids_buf[: max(total, 1)] if self._ids_buf.shape[0] >= max(total, 1) else \
            torch.full((1,), -1, dtype=torch.int64, device=self.dev)

    def _place(self, lists: np.ndarray, ids: np.ndarray):
        """Plan the placement of rows with the given lists / ids and install the tables; returns (dest device
        tensor, positions after)."""
        torch = self.torch
        if self.next_tile * 32 + len(ids) + 32 * self.nlist > (1 << 31):
            raise ValueError("an IVF index holds at most 2^31 positions")
        rel = ids - self.id_base
        if len(rel) and rel.min() < 0:
            raise ValueError(f"ids below the index's id base {self.id_base}")
        if len(np.unique(rel)) != len(rel):
            raise ValueError("duplicate ids inside one add")
        self._grow_id_maps(int(rel.max()) + 1 if len(rel) else 0)
        if len(rel) and (self.pos_of_id[rel] >= 0).any():
            raise ValueError("an id of this add is already stored")
        dest, new_ext, self.counts, self.caps, self.tails, self.ntiles, self.next_tile = plan_add(
            self.counts, self.caps, self.tails, self.ntiles, self.next_tile, lists)
        if len(new_ext):
            self.ext_list = np.concatenate([self.ext_list, new_ext[:, 0]])
            self.ext_first = np.concatenate([self.ext_first, new_ext[:, 1]])
            self.ext_nt = np.concatenate([self.ext_nt, new_ext[:, 2]])
        self._sync_tables()
        self.pos_of_id[rel] = dest
        dest_d = torch.from_numpy(dest).to(self.dev)
        rel_d = torch.from_numpy(rel).to(self.dev)
        self.ids[dest_d] = torch.from_numpy(ids).to(self.dev)
        self.lists_of_rows[rel_d] = torch.from_numpy(np.asarray(lists, np.int64)).to(self.dev)
        self.n += len(ids)
        return dest_d, self.next_tile * 32

    def _ids_arg(self, ids, m: int) -> np.ndarray:
        if ids is None:
            have = 0 if self.pos_of_id is None else len(self.pos_of_id)
            return np.arange(have, have + m, dtype=np.int64) + self.id_base
        if hasattr(ids, "cpu"):
            ids = ids.cpu().numpy()
        ids = np.ascontiguousarray(np.asarray(ids, np.int64).reshape(-1))
        if len(ids) != m:
            raise ValueError("one id per row")
        return ids

    def add(self, rows, ids=None):
        """Add a (m, dim) fp32 device tensor of raw vectors with their ids (default: the next ids), after train(),
        with or without an earlier build().  Returns the lists the rows went to (host)."""
        torch = self.torch
        if self.centroids is None:
            raise RuntimeError("train() the coarse quantizer first")
        rows = rows.to(self.dev, torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be (m, {self.dim})")
        self._to_extents()
        ids = self._ids_arg(ids, rows.shape[0])
        if not len(ids):
            return np.zeros(0, np.int64)
        lists = self._assign(self._process(rows), self.centroids[:, : self.dim]).cpu().numpy()
        dest, total = self._place(lists, ids)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.index.add_device_at(rows.data_ptr(), rows.shape[0], dest.data_ptr(), total, stream=stream)
        return lists

    def add_from(self, src_index, src_rows, ids=None, lists=None, chunk: int = 1 << 16):
        """The same placement for rows already stored in ``src_index`` (a NativeIndex of the same dim, dtype and
        metric on this device): their stored bits are copied (hr_index_copy_rows), not normalised and rounded a
        second time.  ``ids`` default to the source row numbers; ``lists`` (optional) skips the assignment, which
        otherwise runs on the stored vectors."""
        torch = self.torch
        if self.centroids is None:
            raise RuntimeError("train() the coarse quantizer first")
        src_rows = np.ascontiguousarray(np.asarray(src_rows, np.int64).reshape(-1))
        ids = src_rows.copy() if ids is None else self._ids_arg(ids, len(src_rows))
        self._to_extents()
        if not len(src_rows):
            return np.zeros(0, np.int64)
        if lists is None:
            cent = self.centroids[:, : self.dim]
            parts = []
            for i in range(0, len(src_rows), chunk):
                x = torch.from_numpy(src_index.get_rows(src_rows[i:i + chunk])).to(self.dev)
                parts.append(self._assign(self._process(x), cent).cpu().numpy())
            lists = np.concatenate(parts)
        lists = np.ascontiguousarray(np.asarray(lists, np.int64).reshape(-1))
        dest, total = self._place(lists, ids)
        src_d = torch.from_numpy(src_rows).to(self.dev)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        self.index.copy_rows_from(src_index, src_d.data_ptr(), dest.data_ptr(), len(src_rows), total, stream=stream)
        return lists

    def remove(self, ids):
        """Tombstone the rows with these ids (unknown or already removed ids: no-op).  Returns the number removed."""
        torch = self.torch
        if hasattr(ids, "cpu"):
            ids = ids.cpu().numpy()
        rel = np.unique(np.asarray(ids, np.int64).reshape(-1)) - self.id_base
        if self.ids is None or not len(rel):
            return 0
        self._to_extents()
        rel = rel[(rel >= 0) & (rel < len(self.pos_of_id))]
        rel = rel[self.pos_of_id[rel] >= 0]
        if not len(rel):
            return 0
        pos = self.pos_of_id[rel]
        self.index.remove(pos)
        self.pos_of_id[rel] = -1
        self.ids[torch.from_numpy(pos).to(self.dev)] = -1
        self.lists_of_rows[torch.from_numpy(rel).to(self.dev)] = -1
        self.n -= len(rel)
        return len(rel)

    def compact(self):
        """Rebuild into a fresh list-order index: one extent per list, no dead rows (stored bits copied)."""
        torch = self.torch
        self._to_extents()
        order = np.argsort(self.ext_list, kind="stable")
        pos = _extent_positions(self.ext_first[order], self.ext_nt[order])   # list by list, fill order inside
        lst = np.repeat(self.ext_list[order], self.ext_nt[order] * 32)
        ids = self.ids.cpu().numpy() if len(pos) else np.zeros(0, np.int64)
        keep = ids[pos] >= 0 if len(pos) else np.zeros(0, bool)
        pos, lst = pos[keep], lst[keep]
        nl = self.nlist
        cnt = np.bincount(lst, minlength=nl).astype(np.int64)
        nt = (cnt + 31) // 32
        first = np.cumsum(nt) - nt
        start = np.cumsum(cnt) - cnt
        dest = first[lst] * 32 + np.arange(len(pos), dtype=np.int64) - start[lst]
        total = int(nt.sum()) * 32
        fresh = _native.NativeIndex(self.dim, self.dtype, self.metric, self.device, no_shadows=True)
        new_ids = torch.full((max(total, 1),), -1, dtype=torch.int64, device=self.dev)
        if len(pos):
            src_d, dst_d = torch.from_numpy(pos).to(self.dev), torch.from_numpy(dest).to(self.dev)
            fresh.reserve(total)
            fresh.copy_rows_from(self.index, src_d.data_ptr(), dst_d.data_ptr(), len(pos), total,
                                 stream=torch.cuda.current_stream(self.dev).cuda_stream)
            new_ids[dst_d] = self.ids[src_d]
            self.pos_of_id[ids[pos] - self.id_base] = dest
        self.index.close()
        self.index = fresh
        self.ext_list, self.ext_first, self.ext_nt = np.arange(nl, dtype=np.int64), first, nt
        self.counts, self.ntiles, self.caps = cnt, nt.copy(), nt * 32
        self.tails = first * 32 + cnt
        self.next_tile = int(nt.sum())
        self._ids_buf = new_ids
        self._sync_tables()
        return self

    # ---------------------------------------------------------------- persistence
    def save(self, path: str):
        """The list-order rows to ``path`` (hr_index_save) and the tables to ``path + ".npz"`` (no pickle)."""
        if self.centroids is None or self.ids is None:
            raise RuntimeError("nothing to save: train() and add rows first")
        if self.extents:
            el, ef, en = self.ext_list, self.ext_first, self.ext_nt
            counts, tails, next_tile = self.counts, self.tails, self.next_tile
            pos_of_id = self.pos_of_id
        else:  # (a bulk-built index stays in its form; the file holds the equivalent extents)
            lt = self.list_tiles.cpu().numpy().astype(np.int64)
            el, ef, en = np.arange(self.nlist, dtype=np.int64), lt[:-1], np.diff(lt)
            counts = np.bincount(self.lists_of_rows.cpu().numpy(), minlength=self.nlist).astype(np.int64)
            tails, next_tile = ef * 32 + counts, int(lt[-1])
            ids = self.ids.cpu().numpy()
            pos_of_id = np.full(self.n, -1, np.int64)
            live = np.nonzero(ids[: next_tile * 32] >= 0)[0]
            pos_of_id[ids[live] - self.id_base] = live
        self.index.save(path)
        with open(path + ".npz.tmp", "wb") as f:
            np.savez(f, centroids=self.centroids.cpu().numpy(), ext_list=el, ext_first=ef, ext_nt=en, counts=counts,
                     tails=tails, ids=self.ids.cpu().numpy()[: next_tile * 32],
                     lists_of_rows=self.lists_of_rows.cpu().numpy(), pos_of_id=pos_of_id,
                     meta=np.array([self.dim, self.nlist, next_tile, self.id_base, self.n], np.int64),
                     store_dtype=np.array(self.dtype), metric=np.array(self.metric))
        os.replace(path + ".npz.tmp", path + ".npz")

    @classmethod
    def load(cls, path: str, device: int = 0) -> "IvfIndex":
        import torch

        z = np.load(path + ".npz", allow_pickle=False)
        dim, nlist, next_tile, id_base, n = (int(v) for v in z["meta"])
        self = cls.__new__(cls)
        self.torch = torch
        self.dim, self.nlist, self.dtype, self.metric = dim, nlist, str(z["store_dtype"]), str(z["metric"])
        self.dev, self.device, self.dpad = torch.device("cuda", device), device, _round64(dim)
        self.index = _native.NativeIndex.load(path, device=device, dim=dim, dtype=self.dtype, metric=self.metric,
                                              no_shadows=True)
        self.centroids = torch.from_numpy(z["centroids"]).to(self.dev).contiguous()
        self.list_tiles, self.n, self.id_base = None, n, id_base
        self.ext_list, self.ext_first, self.ext_nt = (z[k].astype(np.int64) for k in ("ext_list", "ext_first", "ext_nt"))
        self.counts, self.tails = z["counts"].astype(np.int64), z["tails"].astype(np.int64)
        self.ntiles = np.bincount(self.ext_list, weights=self.ext_nt, minlength=nlist).astype(np.int64)
        self.caps, self.next_tile = self.ntiles * 32, next_tile
        self.pos_of_id = z["pos_of_id"].astype(np.int64)
        self.lists_of_rows = torch.from_numpy(z["lists_of_rows"].astype(np.int64)).to(self.dev)
        self._ids_buf = torch.from_numpy(z["ids"].astype(np.int64)).to(self.dev)
        self.ids = None
        self.extents = True
        self.ext_off = self.ext = self.list_ntiles = None
        self.max_list_tiles = 0
        self._sync_tables()
        return self

    def close(self):
        self.index.close()


class IvfShardedSearch(ShardedSearch):
    """Row-sharded IVF over the ranks (shared centroids): each rank's exact top-k of its visible
    rows, one packed all-gather, the exact merge.  Bounds are -inf, so no fallback ever runs.

    ``k`` is the largest k a search may ask for (every rank returns its top-``k``): the candidates are exact only
    over the probed lists, so there is no flat-scan answer for a larger k to fall back to, and submit / search
    refuse it.  ``k`` itself is bounded by what hr_ivf_search returns per query (IVF_MAX_K) and by the merge
    kernel's LDS (ranks * k <= MERGE_MAX_CANDIDATES)."""

    IVF_MAX_K = 1024               # hr_ivf_search: 1 <= k <= 1024
    MERGE_MAX_CANDIDATES = 8192    # k_merge sorts G * kc records in LDS (launch_merge: 16 B each, 160 KiB)

    def __init__(self, ivf: IvfIndex, max_batch: int, k: int, nprobe: int, group=None, depth: int = 2):
        import torch.distributed as dist

        k = int(k)
        G = dist.get_world_size(group) if dist.is_initialized() else 1
        limit = min(self.IVF_MAX_K, self.MERGE_MAX_CANDIDATES // G)
        if not 1 <= k <= limit:
            raise ValueError(f"k = {k}: an IVF sharded search over {G} rank(s) serves 1 <= k <= {limit} (hr_ivf_search "
                             f"returns at most {self.IVF_MAX_K} rows per query, the merge holds at most "
                             f"{self.MERGE_MAX_CANDIDATES} candidates = ranks * k)")
        super().__init__(ivf.index, 0, max_batch, kc=k, group=group, device=ivf.dev, depth=depth, overlap=False)
        self.ivf, self.nprobe = ivf, int(nprobe)

    def _check_k(self, k):
        if int(k) > self.kc:  # (before any work: what is in flight stays in flight)
            raise ValueError(f"k = {int(k)} above the k = {self.kc} this IVF searcher was built with (the probed lists' "
                             "candidates have no exact answer beyond it)")

    def submit(self, q, k: int, *args, **kwargs):
        self._check_k(k)
        return super().submit(q, k, *args, **kwargs)

    def search(self, q, k: int, *args, **kwargs):
        self._check_k(k)
        return super().search(q, k, *args, **kwargs)

    def _shard_search(self, q, k, cand, bound, mask_ptr, q_ready=None, kc=None):
        # (q_ready: no early SAMPLE here, the queries are ready in stream order; kc: never set, k <= self.kc)
        self.ivf.search_candidates(q, self.kc, self.nprobe, cand, bound, mask_ptr=mask_ptr, stream=self._stream())
