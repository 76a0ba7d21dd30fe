"""HipVectorStore: the reference's BaseVectorStore served by the MI355X index.

Drop-in for ChromaVectorStore (utu/rag/storage/implementations/chroma_store.py,
the production store) with the exact-search semantics of FAISSVectorStore
(faiss_store.py):
  * add_chunks (chroma :64-88): metadata stored as {document_id, chunk_index,
    **non-None chunk.metadata}; ids already present are skipped with a warning,
    ids repeated inside one call raise ValueError (Chroma DuplicateIDError);
  * search (chroma :90-148): exact top-k on the GPU; cosine/"dot" similarity =
    inner product (faiss :179-180; chroma's 1 - distance :135 for those spaces),
    "euclidean" similarity = 1 - squared L2 distance (chroma's "l2" space, :48-53);
    ``filters`` are compiled to a row bitmap (plain dict or Chroma where-clause,
    filters.py: cached per predicate) and applied inside the scan, i.e. exact top-k
    among matching rows;
  * delete / delete_by_document_id / delete_by_metadata (chroma :150-222):
    row tombstones in the index + removal from the host tables;
  * get_by_id (chroma :224-247); count / clear / delete_collection.

Concurrency (SURVEY §7 hard part 5).  The reference calls Chroma synchronously inside
``async def`` (chroma_store.py:118) and its callers issue one query per
``VectorRetriever.retrieve`` (base_retriever.py:58-63).  Here ``search`` hands the query
to a micro-batcher: every ``search`` awaiting at the same time (same filter) becomes ONE
GPU launch, run in a worker thread (``asyncio.to_thread``; ctypes drops the GIL), so the
event loop keeps running and concurrent retrievers share one corpus pass.  Requests that
arrive while a launch is in flight form the next batch (no timer: the batch size follows
the load).  Results are identical to sequential calls (top-k of a smaller k is the prefix of
the larger k's, order score desc / row asc).

Embeddings: the index keeps the normalised vectors in ``dtype``: fp32 by default, what the
reference stores (faiss_store.py:98; Chroma float32), so rankings and scores are the reference's.
``dtype: bf16`` (opt-in) halves the bytes per row and doubles the scan rate; search is then exact
over the stored bf16 values, whose ranking departs from the fp32 answer where two rows' scores lie
within the bf16 rounding of their dot products: recall@10 against the exact fp32 top-10 measured
0.99 at 1M-10M rows (bench.py --full ``recall_at_10_vs_fp32``, tests/test_gpu_scale.py).  Chroma returns the raw fp32
embedding it stored (chroma_store.py:233-244): ``keep_embeddings: true`` keeps a host fp32
copy for ``get_by_id`` / ``include_embeddings``; without it they return the stored
(normalised, quantised) row.

Persistence: generation snapshots + an append-only journal (persist.py); ``add_chunks`` and
``delete*`` write O(chunk) bytes.  ``index_params.devices`` (list of GPU ids) shards the rows
of one collection over several GPUs inside one handle (hr_index_create with n_dev > 1).

Keyword search (opt-in, ``index_params.lexical: true``; single device): a BM25 forward index (lexical.py) holds the
chunk contents row for row beside the dense index -- every add, delete and clear goes to both, a load rebuilds it
from the stored contents (no file of its own) -- and ``keyword_search`` / ``keyword_search_batch`` answer through the
same tables and the same ``filters`` bitmaps as ``search_batch``.  HybridRetriever fuses the two rankings.

Collapsed search (``search(..., collapse=True)`` / ``search_batch(..., collapse=True)``; single device): one hit per
group -- the best chunk of each of the ``top_k`` best groups, exactly (hr_index_search_collapsed).  The
group of a row is its ``document_id`` (``index_params.collapse_field``, the default) or the value of the metadata key
that field names; a row without that key groups by its document_id, as kb_file_search's
``metadata.get("source", document_id)`` does (kb_search_toolkit.py:547).  The value -> id dictionary (keyed on
(type, value): 1, 1.0 and True stay apart) and a host int32 column are built at the first collapsed search and
extended by every add; nothing of them is persisted.

MMR search (``search(..., mmr_lambda=0.5)`` / ``search_batch(..., mmr_lambda=0.5)``, optional ``fetch_k``; single
device): ``top_k`` hits that are relevant but do not repeat each other, chosen on the GPU by maximal marginal relevance
from the exact top-``fetch_k`` (hr_index_search_mmr).  The hits come in selection order with their
plain-search scores, so the scores are not monotone.  Concurrent MMR queries of one (lambda, fetch_k, filter) share a
launch whatever their ``top_k``.  Not combined with ``collapse``.

Range search (``search_range_batch(qs, min_score, max_hits)`` / ``count_above_batch`` / ``await search_range``; single
device): every chunk scoring at least ``min_score`` -- one threshold or one per query -- and the exact number of them,
not the best k of a guessed ``top_k`` (hr_index_search_range).  Each query gets a ``RangeHits(hits,
total)``: the first ``max_hits`` hits, best first, and the count whatever ``max_hits`` is (``truncated``: the list was
cut).  Range calls do not go through the micro-batcher; the single-query form runs in a worker thread.

Search by example (``search_similar_batch(positive_ids, negative_ids, top_k)`` / ``await search_similar(chunk_ids)``):
"more like these chunks" -- the query is built from the STORED vectors of the named chunks, ``pos_weight / |P|`` each
for the positives and ``-neg_weight / |N|`` for the negatives on top of an optional query embedding, on the GPU, and
the named chunks never appear in their own answer (hr_index_search_examples).  An index without a native
``search_examples`` (several devices, IVF_FLAT) gets the same arithmetic composed on the host from ``get_rows`` and
``search``.  Calls do not go through the micro-batcher; the single-query form runs in a worker thread.

Fused multi-query search (``search_fused_batch(query_groups, top_k, fusion="rrf" | "max")`` / ``await
search_fused(query_embeddings)``): several query embeddings per question -- rewrites, a HyDE answer, sub-questions, each
with its own where-clause if need be -- searched exactly in one scan and fused per question on the GPU, by reciprocal
rank (``sum of weight / (rrf_k + rank)``) or by the best score (hr_index_search_fused).  Each group gets
a ``FusedHits(hits, members)``: the (Chunk, fused score) pairs and per hit the bitmask of the group's queries that
found it.  An index without a native ``search_fused`` (several devices, IVF_FLAT) gets the same arithmetic composed on
the host from ``search``.  Calls do not go through the micro-batcher; the single-group form runs in a worker thread.

Boosted search (``index_params.boost_fields``: up to four numeric metadata keys; ``search_boosted_batch(qs, top_k,
boost_weights={field: weight}, sim_weight=1.0)`` / ``await search_boosted``; single device): the ``top_k`` chunks by
``sim_weight * similarity + sum of weight * field`` over the whole collection, exactly -- importance, recency or
popularity blended into the ranking, not a re-ranking of a guessed similarity window (hr_index_search_boosted;
DESIGN.md 4m).  The fields' values live in boost columns on the index, built lazily from the metadata tables (missing,
non-numeric and non-finite values are 0.0) and never persisted.  Each query gets a ``BoostedHits(hits, blended)``: the
(Chunk, similarity) pairs in blended order and the blended values.  Calls do not go through the micro-batcher; the
single-query form runs in a worker thread.

``index_type: "IVF_FLAT"`` (any letter case; single device, cosine / dot): the index is an ``IvfStoreIndex``
(ivf_store.py) -- the same exact index plus an IVF replica that answers searches once ``ivf_train_rows`` live rows
are stored (``index_params``: nlist, nprobe, ivf_train_rows = 64 nlist, ivf_seed).  It comes in through the
``index_factory`` / ``index_loader`` seam; the tables, journal and snapshots are those of the exact store, plus one
``.hri.ivf.npz`` per generation.  Any other ``index_type`` (None, "FLAT", "HNSW", ...) is the exact store.
"""
from __future__ import annotations

import asyncio
import contextlib
import json
import logging
import math
import os
import threading
from array import array
from collections import deque
from typing import Any, NamedTuple

import numpy as np

from .. import _native
from . import filters as F
from . import persist as P
from .base import BaseVectorStore, Chunk
from .lexical import MAX_K as _LEX_MAX_K, LexicalIndex
from .config import VectorStoreConfig
from .ivf_store import IvfStoreIndex, wants_ivf

_F32_MAX = float(np.finfo(np.float32).max)  # boost values beyond it are no float32: they count as 0.0

try:  # the per-hit result assembly in C (csrc/host/hostfast.c, built by csrc/Makefile); host-side only, same output
    from . import _hostfast
except ImportError:  # pragma: no cover - a source tree without the build: the Python loop below
    _hostfast = None


def _assemble_py(C, rec_l, meta_l, score_l, per_q, embs, untrack=False):
    """The per-query (Chunk, score) lists of a batch's gathered hits; _hostfast.assemble is the same in C
    (`untrack` only applies there)."""
    out, i = [], 0
    for cnt in per_q:  # one pass: each query's hits straight into its list
        res = []
        for j in range(i, i + cnt):
            r = rec_l[j]
            if r is None:
                continue
            m = meta_l[j]
            res.append((C(r[0], m.get("document_id", ""), r[2], m.get("chunk_index", 0), dict(m),
                          None if embs is None else embs[j]), score_l[j]))
        out.append(res)
        i += cnt
    return out


def _assemble_results_py(C, R, rec_l, meta_l, score_l, per_q, embs, ks, ths, untrack=False):
    """The per-query RetrievalResult lists of a batch's gathered hits for calls with top_k ks[q] and similarity
    threshold ths[q] (VectorRetriever._to_results over _assemble_py's pairs cut to top_k); _hostfast.assemble_results
    is the same in C (`untrack` only applies there)."""
    out, i = [], 0
    for q, cnt in enumerate(per_q):
        res, pos, kq, th = [], 0, ks[q], ths[q]
        for j in range(i, i + cnt):
            r = rec_l[j]
            if r is None or pos >= kq:
                continue
            pos += 1
            if th > 0.0 and not score_l[j] >= th:
                continue
            m = meta_l[j]
            res.append(R(C(r[0], m.get("document_id", ""), r[2], m.get("chunk_index", 0), dict(m),
                           None if embs is None else embs[j]), score_l[j], pos))
        out.append(res)
        i += cnt
    return out


logger = logging.getLogger(__name__)

_METRIC = {"cosine": "cosine", "dot": "ip", "euclidean": "l2"}


def build_queries_host(idx, examples, weights, q=None) -> np.ndarray:
    """hr_index_build_queries restated over ``idx.get_rows``: per query ``q[b]`` (or 0) plus, in list order,
    ``float64(fp32 weight) * float64(stored row)``, accumulated in float64 and cast to fp32 once."""
    flat = [int(r) for e in examples for r in e]
    x = np.asarray(idx.get_rows(flat), np.float32).astype(np.float64) if flat else None
    dim = x.shape[1] if flat else np.asarray(q).shape[-1]
    acc = np.zeros((len(examples), dim), np.float64)
    if q is not None:
        acc += np.asarray(q, np.float32).reshape(len(examples), dim)
    pos = 0
    for b, (e, w) in enumerate(zip(examples, weights)):
        for j in range(len(e)):
            acc[b] = acc[b] + np.float64(np.float32(w[j])) * x[pos]
            pos += 1
    with np.errstate(over="ignore"):
        return acc.astype(np.float32)


def search_examples_host(idx, examples, k: int, weights, q=None, mask=None, keep: bool = False):
    """NativeIndex.search_examples for an index without one, with the same bits wherever ``idx.search`` is exact:
    build_queries_host, ONE ``idx.search`` for k + (the longest example list) rows, every query's own examples dropped
    from its list, the first k kept, -inf / -1 after them."""
    examples = [[int(r) for r in e] for e in examples]
    built = build_queries_host(idx, examples, weights, q)
    depth = 0 if keep else max((len(e) for e in examples), default=0)
    s, r = idx.search(built, int(k) + depth, mask)
    out_s, out_r = _padded(len(examples), int(k))
    for b, e in enumerate(examples):
        stay = r[b] >= 0
        if not keep:
            stay &= ~np.isin(r[b], e)
        sel = np.nonzero(stay)[0][: int(k)]
        out_s[b, : len(sel)], out_r[b, : len(sel)] = s[b][sel], r[b][sel]
    return out_s, out_r


def fuse_lists_host(scores, rows, groups, k: int, mode: str = "rrf", rrf_k: float = 60.0, weights=None):
    """hr_fuse_lists restated in Python float (IEEE double) arithmetic: ``rows`` / ``scores`` are Q ranked lists of P
    slots (row -1 = padding), ``groups`` the member count of every group.  "rrf": per distinct row 0.0, then per member
    in member order ``fused = fused + float(fp32 weight) / (rrf_k + float(rank))``, ranks from 1; "max": the largest
    fp32 score, NaN as -inf.  Ordered by fused descending, then row ascending; returns (fused float64 (G, k), rows
    int64 (G, k), members uint32 (G, k)) with -inf / -1 / 0 after the distinct rows."""
    rows, scores = np.asarray(rows, np.int64), np.asarray(scores, np.float32)
    G, P = len(groups), rows.shape[1]
    out_f = np.full((G, int(k)), -np.inf, np.float64)
    out_r = np.full((G, int(k)), -1, np.int64)
    out_m = np.zeros((G, int(k)), np.uint32)
    rk, q0 = float(rrf_k), 0
    for g, m in enumerate(groups):
        acc: dict = {}  # row -> [fused, member bits]
        for j in range(int(m)):
            w = 1.0 if weights is None else float(np.float32(weights[q0 + j]))
            r_l, s_l = rows[q0 + j].tolist(), scores[q0 + j].tolist()
            for p in range(P):
                r = r_l[p]
                if r < 0:
                    continue
                if mode == "rrf":
                    cur = acc.setdefault(r, [0.0, 0])
                    cur[0] = cur[0] + w / (rk + float(p + 1))
                else:
                    cur = acc.setdefault(r, [-np.inf, 0])
                    sc = s_l[p]
                    if sc == sc and sc > cur[0]:  # (NaN counts as -inf)
                        cur[0] = sc
                cur[1] |= 1 << j
        for t, (r, (f, bits)) in enumerate(sorted(acc.items(), key=lambda kv: (-kv[1][0], kv[0]))[: int(k)]):
            out_f[g, t], out_r[g, t], out_m[g, t] = f, r, bits
        q0 += int(m)
    return out_f, out_r, out_m


class FusedHits(NamedTuple):
    """One group's answer to a fused search: its (Chunk, fused score) pairs, best first, and per hit the bitmask of
    the group's members that found it (bit j: the j-th query of the group holds the chunk in its list)."""
    hits: list
    members: list


class RangeHits(NamedTuple):
    """One query's answer to a range search: the first ``max_hits`` hits, best first, and the exact number of rows
    at or above the threshold."""
    hits: list
    total: int

    @property
    def truncated(self) -> bool:
        """More rows reached the threshold than ``hits`` holds."""
        return self.total > len(self.hits)


class BoostedHits(NamedTuple):
    """One query's answer to a boosted search: its (Chunk, similarity) pairs ordered by the blended value, best first,
    and per hit that blended value (``sim_weight * similarity + sum of boost_weights[f] * f``, float64)."""
    hits: list
    blended: list


class _ObjColumn:
    """A growable per-row column of Python objects in a numpy object array.  Used instead of a list for
    the 10M-entry host tables: an object ndarray is not tracked by Python's cycle collector, a list is,
    and every full collection walked the lists' 10M entries (~0.1 s each; p99 search latency under
    load 600 ms without it, 6-70 ms with it -- tools/bench_async.py).  Holds only acyclic values."""

    __slots__ = ("a", "n")

    def __init__(self, values=()):
        values = list(values)
        self.a = np.empty(max(1024, len(values)), object)
        for i, v in enumerate(values):  # element-wise: tuples must stay objects, not become array rows
            self.a[i] = v
        self.n = len(values)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.a[i]

    def __setitem__(self, i, v):
        self.a[i] = v

    def __iter__(self):
        return iter(self.a[: self.n])

    def append(self, v):
        if self.n == len(self.a):
            grown = np.empty(2 * len(self.a), object)
            grown[: self.n] = self.a
            self.a = grown
        self.a[self.n] = v
        self.n += 1


class _Prep(NamedTuple):
    """One batch of a top-k search as _prep_search checked it: (B, dim) fp32 queries, top_k, the batch's one
    where-clause or a list with one (or None) per query, and its mode: plain, one hit per group (collapse), or
    maximal marginal relevance (mmr: the checked (lambda, pool size) of _mmr_mode)."""
    q: np.ndarray
    top_k: int
    filters: Any
    collapse: bool = False
    mmr: tuple | None = None


class _Pending(NamedTuple):
    """One queued query of the micro-batcher; queries of one mode -- the (collapse, mmr) of _Prep -- and one key
    (_filter_key(filters)) share a launch."""
    q: np.ndarray
    top_k: int
    filters: Any
    key: str
    fut: asyncio.Future
    mode: tuple


_PLAIN = (False, None)  # the mode of a plain query


class _SearchBatcher:
    """Coalesces concurrent ``search`` calls into batched launches (one per filter group; with
    ``index_params.mixed_filters`` one launch takes plain queries of any filters, each with its own row mask).

    Up to ``depth`` launches are in flight, and the Chunk objects of a finished batch are assembled on the
    event-loop thread while the next launch runs.  An unfiltered batch on a single-device index is launched
    from the event loop itself through the library's asynchronous entry point
    (hr_index_search_submit_host: the call only enqueues the GPU work and returns); its completion arrives
    as a count on an eventfd the loop watches (written by a host function behind the batch's results), so
    no Python thread takes part -- no GIL hand-off between a worker and the loop per launch.  Filtered
    batches, multi-device handles, and launches that find the handle or the store busy run the blocking
    search in a worker thread (``asyncio.to_thread``; ctypes drops the GIL), and so do collapsed and MMR batches."""

    def __init__(self, store: "HipVectorStore", max_batch: int, depth: int = 2):
        self.store, self.max_batch, self.depth = store, max(1, int(max_batch)), max(1, int(depth))
        self.pending: list = []
        self.running = False
        self.launches = 0         # diagnostics
        self.native_launches = 0  # ... of which through the asynchronous native entry point
        self.efd = -1             # eventfd of native completions (one count per finished batch)
        self._native: deque = deque()  # completion futures of native launches, in submission order
        self._loop = None         # the loop the eventfd reader is registered with
        self._drain_loop = None   # the loop the running drain belongs to
        self._inflight: dict = {}  # the running drain's launches: awaitable -> (batch, prep, native info or None)

    def submit(self, q: np.ndarray, top_k: int, filters, collapse: bool = False, mmr: tuple | None = None
               ) -> asyncio.Future:
        """Queue one query; the future resolves to its (Chunk, score) list.  A plain call, not a coroutine: the
        caller's own coroutine awaits the future, so a query in flight holds one coroutine frame fewer for the
        cycle collector to walk and promote (the store's event loop is collector-bound under load)."""
        dim = self.store.dim
        if dim is not None and q.shape[0] != dim:  # checked before queueing: a bad query fails alone
            raise ValueError(f"query dim {q.shape[0]} != collection dim {dim}")
        loop = asyncio.get_running_loop()
        if self._drain_loop is not None and self._drain_loop is not loop and self._drain_loop.is_closed():
            self._recover_from_closed_loop(loop)
        fut = loop.create_future()
        # the mode is part of the group key: collapsed and plain queries never share a launch, and MMR queries
        # (mmr = (lambda, pool size), _mmr_mode) share one with MMR queries of the same lambda, pool size and filter
        # only -- of any top_k: a k'-pick answer is the prefix of the k-pick one, so the launch runs at the batch's
        # largest top_k and _drain cuts each query's list to its own
        mode = _PLAIN if mmr is None and not collapse else (bool(collapse), mmr)
        self.pending.append(_Pending(q, int(top_k), filters, _filter_key(filters), fut, mode))
        if not self.running:
            self.running, self._drain_loop = True, loop
            # start draining on the next loop iteration: every task that is ready now enqueues first
            loop.call_soon(lambda: loop.create_task(self._drain()))
        return fut

    def _recover_from_closed_loop(self, loop):
        """The loop that ran the last drain has closed -- possibly under it (asyncio.run ending with searches queued
        or in flight: the drain never ran, or was cancelled with native launches outstanding): finish those
        native launches here (blocking collects: their slots free, results dropped -- nobody waits for them), drop
        their completion counts from the eventfd, forget the dead loop's queries and start afresh on `loop`."""
        for _batch, _prep, info in list(self._inflight.values()):
            if info is not None:
                with contextlib.suppress(Exception):
                    self.store._collect_native(info, blocking=True)
        self._inflight = {}
        if self.efd >= 0:
            with contextlib.suppress(BlockingIOError, OSError):
                os.eventfd_read(self.efd)  # (the collects waited for every notify of those launches)
        self._native.clear()
        self._loop = None  # its reader went with the closed loop; native_fd registers one with `loop`
        self.pending = [e for e in self.pending if e.fut.get_loop() is loop]
        self.running, self._drain_loop = False, None

    def _take(self):
        first = self.pending[0]
        # mixed_filters: a launch of plain queries fills across filter keys (the batch then carries one filter per
        # query, HipVectorStore._run_mixed); collapsed and MMR queries keep one launch per filter group and never share
        # a launch with plain ones or with each other.  The rule is unconditional: the per-query-mask call beat one launch per filter at
        # every point of the sweep (2 to 64 filters, 0.1 % to 30 % of the rows each, 1M and 10M rows: CHANGELOG.md);
        # a launch whose queries share one filter takes the single-mask search (_prep_search)
        mixed = self.store.mixed_filters and first.mode == _PLAIN
        batch, rest = [], []
        for e in self.pending:
            same = e.mode == _PLAIN if mixed else e.key == first.key and e.mode == first.mode
            (batch if same and len(batch) < self.max_batch else rest).append(e)
        self.pending = rest
        return batch

    @staticmethod
    def _batch_filters(batch):
        """The filters of a batch: the one where-clause its queries share, else one per query."""
        if all(e.key == batch[0].key for e in batch):
            return batch[0].filters
        return [e.filters for e in batch]

    @staticmethod
    def _fail(batch, exc):
        for e in batch:
            if not e.fut.done():
                e.fut.set_exception(exc)

    # -- native completions
    def native_fd(self, loop) -> int:
        """The eventfd native launches signal, its reader registered with `loop` (-1: unavailable)."""
        if self.efd < 0:
            if not hasattr(os, "eventfd"):
                return -1
            self.efd = os.eventfd(0, os.EFD_NONBLOCK | os.EFD_CLOEXEC)
        if self._loop is not loop:
            loop.add_reader(self.efd, self._on_completions)
            self._loop = loop
        return self.efd

    def _on_completions(self):
        try:
            n = os.eventfd_read(self.efd)
        except BlockingIOError:
            return
        for _ in range(n):  # batches finish in submission order (one stream)
            if not self._native:
                break
            fut = self._native.popleft()
            if not fut.done():
                fut.set_result(None)

    def _release_loop(self):
        if self._loop is not None and not self._native:
            with contextlib.suppress(Exception):
                self._loop.remove_reader(self.efd)
            self._loop = None

    def close(self):
        self._release_loop()
        if self.efd >= 0 and not self._native:
            os.close(self.efd)
            self.efd = -1

    def _launch(self, loop, prep):
        """Start one batch: (awaitable, info).  info is None for a worker-thread launch (the awaitable's
        result is the search), else the native launch to collect once the awaitable resolves."""
        info = self.store._submit_native(prep, self, loop)
        if info is not None:
            fut = loop.create_future()
            self._native.append(fut)
            self.native_launches += 1
            return fut, info
        return asyncio.ensure_future(asyncio.to_thread(self.store._run_search, prep)), None

    async def _drain(self):
        loop = asyncio.get_running_loop()
        inflight: dict = {}  # awaitable -> (batch, prep, native launch info or None)
        self._inflight = inflight  # (seen by _recover_from_closed_loop if this loop closes under the drain)
        batch: list = []
        try:
            while self.pending or inflight:
                while self.pending and len(inflight) < self.depth:
                    batch = self._take()
                    try:
                        qs = np.stack([e.q for e in batch])
                        k = max(e.top_k for e in batch)
                        self.launches += 1
                        prep = self.store._prep_search(qs, k, self._batch_filters(batch), *batch[0].mode)
                        aw, info = self._launch(loop, prep)
                    except Exception as exc:  # noqa: BLE001 -- this batch's waiters see the failure
                        self._fail(batch, exc)
                        continue
                    inflight[aw] = (batch, prep, info)
                batch = []
                if not inflight:
                    continue
                done, _ = await asyncio.wait(list(inflight), return_when=asyncio.FIRST_COMPLETED)
                for aw in done:
                    batch, prep, info = inflight.pop(aw)
                    try:
                        if info is None:
                            ran = aw.result()
                        else:
                            ran = self.store._collect_native(info, blocking=False)
                            if ran is None:  # the store is busy (a mutation holds its lock): collect in a worker
                                t = asyncio.ensure_future(asyncio.to_thread(self.store._collect_native, info, True))
                                inflight[t] = (batch, prep, None)
                                batch = []
                                continue
                        res = self.store._assemble(prep, ran)
                    except Exception as exc:  # noqa: BLE001 -- every waiter sees the failure
                        self._fail(batch, exc)
                        continue
                    for e, r in zip(batch, res):
                        if not e.fut.done():
                            e.fut.set_result(r if len(r) <= e.top_k else r[: e.top_k])
                batch = []
        except BaseException as exc:  # never leave a waiter hanging: fail what this drain holds
            err = exc if isinstance(exc, Exception) else RuntimeError(f"search batcher stopped: {exc!r}")
            self._fail(batch, err)
            for b, _, _ in inflight.values():
                self._fail(b, err)
            raise
        finally:
            self.running = False
            self._release_loop()


def _filter_key(filters) -> str:
    if not filters:
        return ""
    return json.dumps(filters, sort_keys=True, default=repr)


def _as_queries(q, dim: int | None) -> np.ndarray:
    """One query embedding or a batch of them as (B, dim) fp32 (dim None: any width)."""
    q = np.asarray(q, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    if dim is not None and q.shape[1] != dim:
        raise ValueError(f"query dim {q.shape[1]} != collection dim {dim}")
    return q


def _per_query_filters(filters, n: int):
    """``filters`` as the searches run it: one where-clause (or None) for the whole batch as it is; a list / tuple with
    one per query checked against the n queries -- the one clause where all agree (the single-mask search), else the
    list."""
    if isinstance(filters, (list, tuple)):
        filters = list(filters)
        if len(filters) != n:
            raise ValueError(f"{len(filters)} filters for {n} queries")
        if len({_filter_key(f) for f in filters}) == 1:
            filters = filters[0] or None
    return filters


def _padded(n: int, width: int):
    """(scores, rows) of n queries with no hits yet: -inf fp32 / -1 int64."""
    return np.full((n, width), -np.inf, np.float32), np.full((n, width), -1, np.int64)


class HipVectorStore(BaseVectorStore):
    def __init__(self, config: VectorStoreConfig, *, index_factory=None, index_loader=None, lexical_factory=None):
        self.config = config
        params = dict(config.index_params or {})
        self.lexical = bool(params.get("lexical", False))
        self.dtype = params.get("dtype", "f32")  # the reference's store dtype; bf16 is an opt-in
        devs = params.get("devices")
        self.devices = [int(d) for d in devs] if devs else [int(params.get("device", 0))]
        self.device = self.devices[0]
        if self.lexical and len(self.devices) > 1:
            raise ValueError("index_params.lexical needs a single-device store (the lexical index is not sharded)")
        self._lex_factory = lexical_factory or (lambda: LexicalIndex(
            self.device, float(params.get("bm25_k1", 1.2)), float(params.get("bm25_b", 0.75))))
        self.capacity = int(params.get("capacity", 0))
        # collapsed search: what a row groups by -- its document_id, or this metadata key (document_id where absent)
        self.collapse_field = str(params.get("collapse_field", "document_id"))
        # boosted search: the metadata keys (at most 4) whose numeric values are the index's boost columns, in order
        self.boost_fields = [str(f) for f in params.get("boost_fields") or []]
        if len(self.boost_fields) > _native.HR_BOOST_MAX_COLS or len(set(self.boost_fields)) != len(self.boost_fields):
            raise ValueError(f"index_params.boost_fields takes at most {_native.HR_BOOST_MAX_COLS} distinct keys")
        self.include_embeddings = bool(params.get("include_embeddings", False))
        self.keep_embeddings = bool(params.get("keep_embeddings", False))
        # returned Chunks with atomic-valued metadata left off the cycle collector (faster under heavy load; a cycle
        # a caller later builds through such a Chunk is then never collected).  Off: ordinary tracked objects.
        self.untracked_results = bool(params.get("untracked_results", False))
        self.persist = bool(params.get("persist", True))
        self.fsync = bool(params.get("fsync", True))
        self.journal_fraction = float(params.get("journal_fraction", 0.25))
        self.metric = _METRIC[config.distance_metric]
        if self.dtype not in _native.DTYPES:
            raise ValueError(f"unknown index dtype {self.dtype!r}")
        # index_type "IVF_FLAT": the exact index plus an IVF replica, through the same factory / loader seam
        self.ivf = wants_ivf(config.index_type, self.metric, self.devices)
        if self.ivf:
            ivf_kw = dict(device=self.device, nlist=int(params.get("nlist", 1024)), nprobe=int(params.get("nprobe", 16)),
                          train_rows=params.get("ivf_train_rows"), seed=int(params.get("ivf_seed", 0)))
            default_factory = lambda dim: IvfStoreIndex(dim, self.dtype, self.metric, **ivf_kw)  # noqa: E731
            default_loader = lambda path, dim, dtype, metric: IvfStoreIndex.load(  # noqa: E731
                path, dim, dtype, metric, **ivf_kw)
        else:
            default_factory = lambda dim: _native.NativeIndex(dim, self.dtype, self.metric,  # noqa: E731
                                                              devices=self.devices)
            default_loader = lambda path, dim, dtype, metric: _native.NativeIndex.load(  # noqa: E731
                path, devices=self.devices, dim=dim, dtype=dtype, metric=metric)
        self._factory = index_factory or default_factory
        self._loader = index_loader or default_loader
        self._batcher = _SearchBatcher(self, int(params.get("max_batch", 64)), int(params.get("search_depth", 2)))
        # unfiltered batches launched from the event loop through the asynchronous native entry point
        self.native_async = bool(params.get("native_async", True))
        # mixed-filter batches: the micro-batcher fills a launch across filter keys and the index answers it with
        # per-query row masks in one exact scan (NativeIndex.search_masks); off: one launch per filter group
        self.mixed_filters = bool(params.get("mixed_filters", False))
        self.mixed_launches = 0   # diagnostics: batches answered by one per-query-mask call
        self.grouped_launches = 0  # ... per-filter launches of list-form batches the index could not take at once
        self._lock = threading.RLock()
        self._paths = P.Paths(config.persist_directory, config.collection_name)
        self._gen = 0
        self._journal: P.Journal | None = None
        self._snapshot_bytes = 0
        self._reset_tables()
        if self.persist:
            self._load_if_present()

    def _reset_tables(self):
        # bumped on every reset (clear / delete_collection): a search that ran against the previous
        # tables must not resolve its rows through the new ones
        self._epoch = getattr(self, "_epoch", 0) + 1
        self._index = None
        if getattr(self, "_lex", None) is not None:
            self._lex.close()
        self._lex = None  # the lexical index (index_params.lexical), created with the first rows
        self.dim: int | None = None
        # host tables, one entry per index row (None = deleted): a tuple of atoms (id, document_id, content,
        # chunk_index) and the stored metadata dict.  Kept apart on purpose: a tuple of atoms and a dict of
        # atoms are untracked by Python's cycle collector, a record dict holding a dict is not -- at 10M
        # rows every full collection then walked 20M+ objects (seconds-long pauses under load)
        self._records = _ObjColumn()  # per row: (id, document_id, content, chunk_index) or None
        self._metas = _ObjColumn()    # per row: the stored metadata dict or None
        self._id_to_row: dict[str, int] = {}
        self._doc_rows: dict[str, array] = {}  # document -> its rows (array('q'): not GC-tracked either)
        self._cols = F.MetadataColumns()
        self._live = np.zeros(0, bool)
        self._raw = None  # keep_embeddings: (capacity, dim) fp32 host copy
        self._defer, self._dirty = 0, False
        # collapsed search, built at the first one (_ensure_groups): (type, value) -> group id, the host column of
        # group ids (one int32 per row, -1 for a dead row) and how many of its rows the index holds already
        self._group_ids: dict | None = None
        self._group_col = np.zeros(0, np.int32)
        self._group_rows = self._group_sent = 0
        # boosted search, built at the first one (_ensure_boosts): the host columns (one float32 row of this array per
        # boost field, 0.0 for a dead row or a value that is no finite number) and how many rows the index holds
        self._boost_cols: np.ndarray | None = None
        self._boost_rows = self._boost_sent = 0

    # ---------------------------------------------------------------- persistence
    def _load_if_present(self):
        pt = self._paths
        if os.path.exists(pt.manifest):
            with open(pt.manifest) as f:
                man = json.load(f)
            g = int(man["gen"])
            idx_path, rows_path, emb_path = pt.gen(g, "hri"), pt.gen(g, "rows.jsonl"), pt.gen(g, "emb.npy")
            self._gen = g
        else:
            idx_path, rows_path = pt.legacy  # round-1 layout
            emb_path, man = None, None
            if not (os.path.exists(idx_path) and os.path.exists(rows_path)):
                return
        header, records = P.read_rows(rows_path)
        self.dim = int(header["dim"])
        self.dtype, self.metric = header["dtype"], header["metric"]  # the files' own, not the config's
        self._index = self._loader(idx_path, self.dim, self.dtype, self.metric)
        n_idx = self._index.size()[0]
        n_hdr = int(header.get("n_rows", len(records)))
        if not (n_idx == n_hdr == len(records)) or (man is not None and int(man["n_rows"]) != n_idx):
            self._index.close()
            self._index = None
            raise RuntimeError(f"collection files disagree on the row count (index {n_idx}, rows header {n_hdr}, "
                               f"records {len(records)}); refusing to load {rows_path}")
        raw = None
        if self.keep_embeddings and emb_path and os.path.exists(emb_path):
            raw = np.load(emb_path, allow_pickle=False)
        self._install(records, raw)
        self._snapshot_bytes = os.path.getsize(idx_path)
        if man is not None:  # replay the journal of this generation
            n_ops = 0
            for op, a, b in P.Journal.replay(pt.gen(self._gen, "journal")):
                if op == "add":
                    first = self._index.add(b)
                    if first != len(self._records):
                        raise RuntimeError("journal replay: row numbering diverged")
                    self._append_tables(a, b)
                else:
                    self._remove_tables(a.tolist(), journal=False)
                n_ops += 1
            if n_ops:
                logger.info("replayed %d journal entries", n_ops)
        logger.info("loaded %d chunks from %s", len(self._id_to_row), idx_path)

    @staticmethod
    def _split_record(rec: dict | None):
        if rec is None:
            return None, None
        return (rec["id"], rec["document_id"], rec["content"], rec.get("chunk_index", 0)), rec.get("metadata", {})

    def record(self, row: int) -> dict | None:
        """The stored record of a row as the persisted dict (None if deleted)."""
        t = self._records[row]
        if t is None:
            return None
        return {"id": t[0], "document_id": t[1], "content": t[2], "chunk_index": t[3], "metadata": self._metas[row]}

    def _install(self, records: list, raw):
        split = [self._split_record(rec) for rec in records]
        self._records = _ObjColumn(t for t, _ in split)
        self._metas = _ObjColumn(m for _, m in split)
        del split
        self._live = np.array([r is not None for r in records], bool)
        for row, rec in enumerate(self._records):
            if rec is not None:
                self._id_to_row[rec[0]] = row
                self._doc_rows.setdefault(rec[1], array("q")).append(row)
        self._cols.append([m or {} for m in self._metas])
        self._lex_append(0, [None if t is None else t[2] for t in self._records])
        if self.keep_embeddings:
            self._raw = np.zeros((max(len(records), 1024), self.dim), np.float32)
            if raw is not None and len(raw) == len(records):
                self._raw[: len(records)] = raw

    @contextlib.contextmanager
    def deferred_save(self):
        """Write one snapshot at the end of a block of adds/deletes (bulk ingest) instead of
        journaling each call."""
        self._defer += 1
        try:
            yield self
        finally:
            self._defer -= 1
            if self._defer == 0 and self._dirty:
                self.flush()

    def flush(self):
        """Write a new snapshot generation now (folds the journal in)."""
        with self._lock:
            self._dirty = False
            if not self.persist or self._index is None:
                return
            pt = self._paths
            os.makedirs(self.config.persist_directory, exist_ok=True)
            g = self._gen + 1
            n = len(self._records)
            self._index.save(pt.gen(g, "hri"))
            P.write_rows(pt.gen(g, "rows.jsonl"), {"format": P.FORMAT, "gen": g, "n_rows": n, "dim": self.dim,
                                                  "dtype": self.dtype, "metric": self.metric},
                         (self.record(r) for r in range(n)))
            if self.keep_embeddings:
                P.fsync_write(pt.gen(g, "emb.npy"), writer=lambda f: np.save(f, self._raw[:n], allow_pickle=False))
            P.fsync_write(pt.manifest, json.dumps({"format": P.FORMAT, "gen": g, "n_rows": n, "dim": self.dim,
                                                   "dtype": self.dtype, "metric": self.metric}).encode())
            old = self._gen
            if self._journal is not None:
                self._journal.close()
                self._journal = None
            self._gen = g
            self._snapshot_bytes = os.path.getsize(pt.gen(g, "hri"))
            for f in P.Paths(self.config.persist_directory, self.config.collection_name).all_files():
                if f.startswith(pt.base + f".g{old}.") or f in pt.legacy:
                    with contextlib.suppress(OSError):
                        os.remove(f)

    def rebuild_ivf(self) -> None:
        """Retrain the IVF replica of an ``index_type: "IVF_FLAT"`` store on the rows stored now and replace it
        (nothing retrains by itself as a collection drifts)."""
        with self._lock:
            if self._index is None or not hasattr(self._index, "rebuild_ivf"):
                raise ValueError('rebuild_ivf needs a store with index_type "IVF_FLAT" that holds rows')
            self._index.rebuild_ivf(np.nonzero(self._live[: len(self._records)])[0])

    def _log(self, op: str, rows=None, records=None, vectors=None):
        """Persist one mutation: journal it, or mark the deferred block dirty."""
        if not self.persist or self._index is None:
            return
        if self._defer or self._gen == 0:  # (no snapshot yet: the first write is a snapshot)
            self._dirty = True
            if not self._defer:
                self.flush()
            return
        if self._journal is None:
            self._journal = P.Journal(self._paths.gen(self._gen, "journal"), fsync=self.fsync)
        if op == "add":
            self._journal.append_add(records, vectors)
        else:
            self._journal.append_delete(rows)
        if self._journal.size > max(64 << 20, self.journal_fraction * self._snapshot_bytes):
            self.flush()

    # ---------------------------------------------------------------- writes
    def _fresh(self, chunks: list[Chunk]) -> list[int]:
        """Indices of chunks whose id is not stored yet (chroma skips existing ids, chroma_store.py:64-88)."""
        ids = [c.id for c in chunks]
        if len(set(ids)) != len(ids):
            raise ValueError("duplicate chunk ids inside one add_chunks call")
        keep = [i for i, c in enumerate(chunks) if c.id not in self._id_to_row]
        if len(keep) < len(chunks):
            logger.warning("skipping %d chunk(s) whose id already exists", len(chunks) - len(keep))
        return keep

    def _ensure_index(self, dim: int):
        if self._index is None:
            self.dim = int(dim)
            self._index = self._factory(self.dim)
            if self.capacity:
                self._index.reserve(self.capacity)
        elif dim != self.dim:
            raise ValueError(f"embedding dim {dim} != collection dim {self.dim}")

    @staticmethod
    def _record(c: Chunk) -> dict:
        meta = {"document_id": c.document_id, "chunk_index": c.chunk_index,
                **{k: v for k, v in (c.metadata or {}).items() if v is not None}}
        return {"id": c.id, "document_id": c.document_id, "content": c.content, "chunk_index": c.chunk_index,
                "metadata": meta}

    def _append_tables(self, records: list[dict], vectors: np.ndarray | None):
        first = len(self._records)
        for i, rec in enumerate(records):
            t, m = self._split_record(rec)
            self._records.append(t)
            self._metas.append(m)
            if rec is not None:
                self._id_to_row[rec["id"]] = first + i
                self._doc_rows.setdefault(rec["document_id"], array("q")).append(first + i)
        self._cols.append([(rec or {}).get("metadata", {}) for rec in records])
        self._lex_append(first, [None if rec is None else rec["content"] for rec in records])
        if self._group_ids is not None:
            self._extend_groups(len(self._records))
        if self._boost_cols is not None:
            self._extend_boosts(len(self._records))
        n = len(self._records)
        if len(self._live) < n:
            live = np.zeros(max(n, 2 * len(self._live), 1024), bool)
            live[: len(self._live)] = self._live
            self._live = live
        self._live[first:n] = [rec is not None for rec in records]
        if self.keep_embeddings:
            if self._raw is None or len(self._raw) < n:
                raw = np.zeros((max(n, 2 * (0 if self._raw is None else len(self._raw)), 1024), self.dim), np.float32)
                if self._raw is not None:
                    raw[: len(self._raw)] = self._raw
                self._raw = raw
            if vectors is not None:
                self._raw[first:n] = vectors

    def _extend_groups(self, n: int):
        """Group ids of rows [_group_rows, n) into the host column (store lock held)."""
        first = self._group_rows
        if n <= first:
            return
        if len(self._group_col) < n:
            col = np.full(max(n, 2 * len(self._group_col), 1024), -1, np.int32)
            col[:first] = self._group_col[:first]
            self._group_col = col
        ids, field, by_doc = self._group_ids, self.collapse_field, self.collapse_field == "document_id"
        for row in range(first, n):
            rec = self._records[row]
            if rec is None:
                self._group_col[row] = -1
                continue
            v = rec[1] if by_doc else (self._metas[row] or {}).get(field, rec[1])
            try:
                key = (type(v), v)
                g = ids.get(key)
            except TypeError:  # an unhashable value (a list): by its text
                key = (type(v), repr(v))
                g = ids.get(key)
            if g is None:
                g = ids[key] = len(ids)
            self._group_col[row] = g
        self._group_rows = n

    def _ensure_groups(self):
        """The group column current on the host and on the device (store lock held, an index present): built from the
        host tables at the first collapsed search -- after a reload too, nothing of it is persisted -- then extended by
        _append_tables; the rows the index has not seen yet go up here."""
        n = len(self._records)
        if self._group_ids is None:
            self._group_ids, self._group_rows, self._group_sent = {}, 0, 0
        self._extend_groups(n)
        if self._group_sent < n:
            self._index.set_groups(self._group_sent, self._group_col[self._group_sent:n])
            self._group_sent = n

    def _extend_boosts(self, n: int):
        """Boost values of rows [_boost_rows, n) into the host columns (store lock held): bool / int / float metadata
        values as float32; a missing, non-numeric or non-finite one (also one beyond float32) is 0.0."""
        first = self._boost_rows
        if n <= first:
            return
        if self._boost_cols.shape[1] < n:
            cols = np.zeros((len(self.boost_fields), max(n, 2 * self._boost_cols.shape[1], 1024)), np.float32)
            cols[:, :first] = self._boost_cols[:, :first]
            self._boost_cols = cols
        for row in range(first, n):
            meta = self._metas[row] if self._records[row] is not None else None
            for c, field in enumerate(self.boost_fields):
                v = (meta or {}).get(field)
                x = 0.0
                if isinstance(v, (bool, int, float)):
                    try:
                        x = float(v)
                    except OverflowError:
                        x = 0.0
                    if not math.isfinite(x) or abs(x) > _F32_MAX:
                        x = 0.0
                self._boost_cols[c, row] = x
        self._boost_rows = n

    def _ensure_boosts(self):
        """The boost columns current on the host and on the device (store lock held, an index present): built from the
        metadata tables at the first boosted search -- after a reload too, nothing of them is persisted -- then
        extended by _append_tables; the rows the index has not seen yet go up here."""
        n = len(self._records)
        if self._boost_cols is None:
            self._boost_cols = np.zeros((len(self.boost_fields), 0), np.float32)
            self._boost_rows = self._boost_sent = 0
        self._extend_boosts(n)
        if self._boost_sent < n:
            for c in range(len(self.boost_fields)):
                self._index.set_boost(c, self._boost_sent, self._boost_cols[c, self._boost_sent:n])
            self._boost_sent = n

    def _lex_append(self, first: int, contents: list):
        """The same rows into the lexical index (None: a dead row -- it takes its row number and no terms)."""
        if not self.lexical or not contents:
            return
        if self._lex is None:
            self._lex = self._lex_factory()
        got = self._lex.add_texts([c or "" for c in contents])
        if got != first:
            raise RuntimeError(f"lexical index row {got} != host table row {first}")
        dead = [first + i for i, c in enumerate(contents) if c is None]
        if dead:
            self._lex.remove_rows(dead)

    def _register(self, fresh: list[Chunk], first: int, vectors: np.ndarray | None):
        records = [self._record(c) for c in fresh]
        if first != len(self._records):
            raise RuntimeError(f"index row {first} != host table size {len(self._records)}")
        self._append_tables(records, vectors)
        self._log("add", records=records, vectors=vectors)
        logger.info("added %d chunks to %s", len(fresh), self.config.collection_name)

    # The async mutators and get_by_id take the store lock in a worker thread: a search launch holds it
    # for a whole GPU pass, and the event loop (where the batcher assembles results) must never wait on it.
    async def add_chunks(self, chunks: list[Chunk]) -> None:
        if not chunks:
            return
        await asyncio.to_thread(self.add_chunks_sync, chunks)

    def add_chunks_sync(self, chunks: list[Chunk]) -> None:
        if not chunks:
            return
        with self._lock:
            fresh = [chunks[i] for i in self._fresh(chunks)]
            if not fresh:
                return
            if any(c.embedding is None for c in fresh):
                raise ValueError("every chunk needs an embedding")
            emb = np.asarray([c.embedding for c in fresh], dtype=np.float32)
            if emb.ndim != 2:
                raise ValueError("embeddings must all have the same dimension")
            self._ensure_index(emb.shape[1])
            self._register(fresh, self._index.add(emb), emb)

    def add_chunks_device(self, chunks: list[Chunk], embeddings, stream: int | None = None) -> int:
        """add_chunks for embeddings that are already on the GPU (the in-process embedder's output):
        `embeddings` is a (len(chunks), dim) float32 device tensor; the vectors never visit the host
        on the index path (replaces embed_texts -> add_chunks, processors.py:413-418; a host copy is
        made only for the journal / keep_embeddings).  Returns the number added."""
        import torch

        if not chunks:
            return 0
        if embeddings.dim() != 2 or embeddings.shape[0] != len(chunks) or not embeddings.is_cuda:
            raise ValueError("embeddings must be a (len(chunks), dim) device tensor")
        with self._lock:
            keep = self._fresh(chunks)
            if not keep:
                return 0
            dev = embeddings.device
            # the given stream orders everything here: gathers / casts run on it too
            ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)) if stream is not None \
                else contextlib.nullcontext()
            with ctx:
                emb = embeddings if len(keep) == len(chunks) else embeddings[torch.as_tensor(keep, device=dev)]
                emb = emb.to(torch.float32).contiguous()
                self._ensure_index(emb.shape[1])
                stream = torch.cuda.current_stream(dev).cuda_stream
                first = self._index.add_device(emb.data_ptr(), emb.shape[0], stream)
            need_host = self.keep_embeddings or (self.persist and not self._defer and self._gen > 0)
            self._register([chunks[i] for i in keep], first, emb.cpu().numpy() if need_host else None)
            return len(keep)

    def _remove_tables(self, rows: list[int], journal: bool = True) -> int:
        rows = [int(r) for r in rows if 0 <= r < len(self._records) and self._records[r] is not None]
        if not rows:
            return 0
        self._index.remove(np.asarray(rows, np.int64))
        if self._lex is not None:
            self._lex.remove_rows(rows)
        for r in rows:
            rec = self._records[r]
            self._id_to_row.pop(rec[0], None)
            doc = self._doc_rows.get(rec[1])
            if doc is not None:
                doc.remove(r)
                if not doc:
                    del self._doc_rows[rec[1]]
            self._records[r] = None
            self._metas[r] = None
            self._live[r] = False
        if journal:
            self._log("del", rows=rows)
        return len(rows)

    def _delete_sync(self, chunk_ids: list[str]) -> None:
        with self._lock:
            if self._index is not None:
                self._remove_tables([self._id_to_row[c] for c in chunk_ids if c in self._id_to_row])

    async def delete(self, chunk_ids: list[str]) -> None:
        if not chunk_ids or self._index is None:
            return
        await asyncio.to_thread(self._delete_sync, chunk_ids)

    def _delete_document_sync(self, document_id: str) -> int:
        with self._lock:
            if self._index is None:
                return 0
            return self._remove_tables(list(self._doc_rows.get(document_id, ())))

    async def delete_by_document_id(self, document_id: str) -> int:
        if self._index is None or document_id not in self._doc_rows:  # (a new document: no thread hop)
            return 0
        n = await asyncio.to_thread(self._delete_document_sync, document_id)
        logger.info("deleted %d chunks for document_id %s", n, document_id)
        return n

    def _delete_by_metadata_sync(self, metadata_filter: dict[str, Any]) -> int:
        with self._lock:
            if self._index is None:
                return 0
            n = len(self._records)
            hit = F.evaluate(metadata_filter, self._cols) & self._live[:n]
            return self._remove_tables(np.nonzero(hit)[0].tolist())

    async def delete_by_metadata(self, metadata_filter: dict[str, Any]) -> int:
        if self._index is None or not metadata_filter:
            return 0
        return await asyncio.to_thread(self._delete_by_metadata_sync, metadata_filter)

    def _clear_sync(self):
        with self._lock:
            if self._journal is not None:
                self._journal.close()
            if self._index is not None:
                self._index.close()
            self._reset_tables()
            self._gen, self._journal = 0, None
            for p in self._paths.all_files():
                with contextlib.suppress(OSError):
                    os.remove(p)

    async def clear(self) -> None:
        await asyncio.to_thread(self._clear_sync)

    def delete_collection(self) -> None:
        """Drop the collection and its files (chroma_store.py:331, synchronous there too)."""
        self._clear_sync()

    def close(self) -> None:
        """Fold the journal into a snapshot and release the device index."""
        self._batcher.close()
        with self._lock:
            if self._journal is not None and self._journal.size:
                self.flush()
            if self._journal is not None:
                self._journal.close()
                self._journal = None
            if self._index is not None:
                self._index.close()
                self._index = None
            if self._lex is not None:
                self._lex.close()
                self._lex = None

    # ---------------------------------------------------------------- reads
    def _chunk(self, row: int, embedding=None, tables=None) -> Chunk:
        recs, metas = tables or (self._records, self._metas)
        rec = recs[row]
        meta = metas[row]
        # a fresh metadata dict per result, as Chroma returns (callers may mutate it)
        return Chunk(rec[0], meta.get("document_id", ""), rec[2], meta.get("chunk_index", 0), dict(meta),
                     embedding)

    def filter_bitmap(self, filters: dict[str, Any] | None):
        """uint64 row bitmap of a where-clause (None = no filter)."""
        if not filters:
            return None
        return F.evaluate_words(filters, self._cols)

    def _embeddings(self, rows: list[int]):
        if self.keep_embeddings and self._raw is not None:
            return self._raw[np.asarray(rows, np.int64)]
        return self._index.get_rows(rows)

    def search_batch(self, query_embeddings, top_k: int = 5,
                     filters: dict[str, Any] | list[dict[str, Any] | None] | None = None, *,
                     collapse: bool = False, mmr_lambda: float | None = None,
                     fetch_k: int | None = None) -> list[list[tuple[Chunk, float]]]:
        """Batched search: one GPU launch for all queries (BatchedVectorRetriever, the micro-batcher).
        ``filters``: one where-clause for every query, or a list with one where-clause or None per query (a length
        other than the number of queries raises ValueError) -- answered by one per-query-mask scan where the index
        has one (a single-device exact index), else by one launch per distinct filter; the results are the same.
        ``collapse=True``: one hit per group (collapse_field), the best chunk of each of the top_k best groups.
        ``mmr_lambda`` in [0, 1]: a diversified list (maximal marginal relevance) -- top_k greedy picks
        of the largest mmr_lambda * score - (1 - mmr_lambda) * (similarity to the hits picked so far) from the exact
        top-``fetch_k`` (default min(HR_MAX_K, max(32, 4 top_k))).  The hits come in selection order, each with its
        plain-search score: the scores are not monotone down the list.  Not combined with ``collapse``; ``fetch_k``
        without ``mmr_lambda`` means nothing."""
        mmr = self._mmr_mode(top_k, mmr_lambda, fetch_k, collapse)
        prep = self._prep_search(query_embeddings, top_k, filters, collapse, mmr)
        return self._assemble(prep, self._run_search(prep))

    @staticmethod
    def _mmr_mode(top_k: int, mmr_lambda, fetch_k, collapse: bool):
        """None for a search without ``mmr_lambda``, else its checked (lambda, pool size): every limit of
        hr_index_search_mmr is checked here, before a query is queued, so a bad one fails alone."""
        if mmr_lambda is None:
            return None
        if collapse:
            raise ValueError("mmr_lambda and collapse=True do not combine")
        lam, k, top = float(mmr_lambda), int(top_k), _native.HR_MAX_K
        if not 0.0 <= lam <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"mmr_lambda must be in [0, 1] (got {mmr_lambda})")
        if k > top:
            raise ValueError(f"an MMR search returns at most {top} hits (top_k = {top_k})")
        pool = min(top, max(32, 4 * k)) if fetch_k is None else int(fetch_k)
        if pool < max(k, 1) or pool > top:
            raise ValueError(f"fetch_k must be in [top_k, {top}] (got {fetch_k}, top_k = {top_k})")
        return lam, pool

    @staticmethod
    def _check_collapsed_k(top_k):
        if int(top_k) > _native.HR_MAX_K:
            raise ValueError(f"a collapsed search returns at most {_native.HR_MAX_K} groups (top_k = {top_k})")

    @staticmethod
    def _single_device(idx) -> bool:
        """The handle keeps its rows on one GPU (an index that does not say so does)."""
        return len(getattr(idx, "devices", (0,))) == 1

    def _tables(self):
        """The host tables a search resolves its rows through, and the epoch they belong to."""
        return (self._records, self._metas, self._epoch)

    def keyword_search_batch(self, queries: list[str], top_k: int = 5, filters: dict[str, Any] | None = None
                             ) -> list[list[tuple[Chunk, float]]]:
        """BM25 keyword search of the chunk contents (``index_params.lexical``): per query its (Chunk, score) list,
        score descending then row ascending, among the rows ``filters`` allows that hold at least one of the query's
        terms.  One forward-index scan on the GPU for the whole batch; same tables, lock and filter bitmaps as
        search_batch."""
        if not self.lexical:
            raise ValueError("keyword search needs index_params.lexical = true")
        queries = list(queries)
        with self._lock:
            tables = self._tables()
            n_live = self.count_sync()
            if self._lex is None or n_live == 0 or int(top_k) <= 0 or not queries:
                return [[] for _ in queries]
            k = min(int(top_k), n_live)
            if k > _LEX_MAX_K:
                raise ValueError(f"keyword search returns at most {_LEX_MAX_K} hits per query")
            raw = self._lex.search(queries, k, self.filter_bitmap(filters))
        return self._assemble((queries, int(top_k), filters), (raw, tables))

    def keyword_search(self, query: str, top_k: int = 5, filters: dict[str, Any] | None = None
                       ) -> list[tuple[Chunk, float]]:
        return self.keyword_search_batch([query], top_k, filters)[0]

    # search_batch in three steps, so the micro-batcher can run only the middle one in a worker thread
    # (it holds the GIL for little but the ctypes call; a worker doing the Python parts was starved by
    # a busy event loop) and assemble on the event-loop thread while the next launch runs
    def _prep_search(self, query_embeddings, top_k: int, filters, collapse: bool = False, mmr: tuple | None = None
                     ) -> _Prep:
        """The checked batch of a top-k search; mmr: the (lambda, pool size) of _mmr_mode."""
        q = _as_queries(query_embeddings, self.dim)
        return _Prep(q, int(top_k), _per_query_filters(filters, q.shape[0]), bool(collapse), mmr)

    def _run_mmr(self, q, top_k: int, filters, n_live: int, mmr: tuple):
        """The native MMR search (store lock held, rows present); mmr: the (lambda, pool size) of _mmr_mode."""
        idx = self._index
        if not self._single_device(idx):
            raise ValueError("an MMR search needs a single-device store")
        if not hasattr(idx, "search_mmr"):
            raise NotImplementedError(f"{type(idx).__name__} has no MMR search")
        return idx.search_mmr(q, min(top_k, n_live), mmr[0], self.filter_bitmap(filters), mmr[1])

    def _run_collapsed(self, q, top_k: int, filters, n_live: int):
        """The collapsed native search (store lock held, rows present)."""
        self._check_collapsed_k(top_k)
        idx = self._index
        if not self._single_device(idx):
            raise ValueError("a collapsed search needs a single-device store")
        if not hasattr(idx, "search_collapsed") or not hasattr(idx, "set_groups"):
            raise NotImplementedError(f"{type(idx).__name__} has no collapsed search")
        self._ensure_groups()  # under the same lock hold as the search
        return idx.search_collapsed(q, min(top_k, n_live), self.filter_bitmap(filters))

    def _distinct_filters(self, filters: list):
        """(clause_of, bitmaps) of a per-query filter list: each query's where-clause as its number among the distinct
        ones, in first-use order, and the distinct clauses' row bitmaps through the filter cache (None = no filter)."""
        order: dict[str, int] = {}
        clauses, clause_of = [], np.empty(len(filters), np.int32)
        for i, f in enumerate(filters):
            key = _filter_key(f)
            if key not in order:
                order[key] = len(clauses)
                clauses.append(f or None)
            clause_of[i] = order[key]
        return clause_of, [self.filter_bitmap(f) for f in clauses]

    @staticmethod
    def _stack_bitmaps(clause_of, bitmaps: list):
        """(masks, mask_of) for search_masks: the bitmaps that exist stacked into one (D, words) uint64 array and, per
        query, its row of that array (-1 for a query without a filter)."""
        slot, rows = np.full(len(bitmaps), -1, np.int32), []
        for c, bm in enumerate(bitmaps):
            if bm is not None:
                slot[c] = len(rows)
                rows.append(np.ascontiguousarray(bm, np.uint64).reshape(-1))
        stacked = np.zeros((len(rows), max((len(r) for r in rows), default=0)), np.uint64)
        for j, r in enumerate(rows):
            stacked[j, : len(r)] = r
        return stacked, slot[clause_of]

    def _takes_masks(self, idx) -> bool:
        """The index answers per-query masks in one call: a single-device exact index with search_masks."""
        return hasattr(idx, "search_masks") and not self.ivf and self._single_device(idx)

    def _per_clause(self, distinct, width: int, call):
        """A per-query filter list on a call that takes one row mask: ``call(sel, bitmap) -> (scores, rows)`` once per
        distinct where-clause (`distinct`: the list's _distinct_filters), for the queries `sel` that carry it -- so
        ``filters[sel[0]]`` is the clause -- scattered back in query order into (B, width) arrays padded with -inf /
        -1.  An answer narrower than `width` fills its first columns; one without lists (None, None) fills none."""
        clause_of, bitmaps = distinct
        scores, rows = _padded(len(clause_of), width)
        for c, bitmap in enumerate(bitmaps):
            sel = np.nonzero(clause_of == c)[0]
            s, r = call(sel, bitmap)
            self.grouped_launches += 1
            if s is not None:
                scores[sel, : s.shape[1]], rows[sel, : r.shape[1]] = s, r
        return scores, rows

    def _run_mixed(self, q, top_k: int, filters: list, n_live: int, collapse: bool = False, mmr: tuple | None = None):
        """A batch with one where-clause (or None) per query (store lock held, rows present).  Distinct predicates
        resolve to bitmaps through the filter cache; a single-device exact index answers the batch with ONE
        per-query-mask call (NativeIndex.search_masks).  Multi-device handles, IVF_FLAT stores and collapsed batches
        keep one launch per distinct filter, scattered back in query order -- the same results -- and so do MMR
        batches."""
        idx = self._index
        k = min(top_k, n_live)
        distinct = self._distinct_filters(filters)
        if not collapse and mmr is None and self._takes_masks(idx):
            try:
                out = idx.search_masks(q, k, *self._stack_bitmaps(*distinct))
                self.mixed_launches += 1
                return out
            except NotImplementedError:
                pass  # (a handle that cannot take per-query masks: group below)
        if collapse:
            self._check_collapsed_k(top_k)

        def call(sel, bitmap):
            if collapse:
                return self._run_collapsed(q[sel], top_k, filters[sel[0]], n_live)
            if mmr is not None:
                return self._run_mmr(q[sel], top_k, filters[sel[0]], n_live, mmr)
            return idx.search(q[sel], k, bitmap)

        return self._per_clause(distinct, k, call)

    def _run_search(self, prep: _Prep):
        """The native search, under the store lock.  Everything that depends on the collection's
        current state -- the live row count, the filter bitmap (sized to the index's rows NOW, not when
        the query was queued: rows added in between would otherwise make the bitmap too short), the
        tables the rows resolve through -- is taken here, under the same lock as the search."""
        q, top_k, filters = prep.q, prep.top_k, prep.filters
        with self._lock:  # ordered against mutations
            tables = self._tables()
            n_live = self.count_sync()
            if self._index is None or n_live == 0 or top_k <= 0:
                return None, tables
            if isinstance(filters, list):
                return self._run_mixed(q, top_k, filters, n_live, prep.collapse, prep.mmr), tables
            if prep.mmr is not None:
                return self._run_mmr(q, top_k, filters, n_live, prep.mmr), tables
            if prep.collapse:
                return self._run_collapsed(q, top_k, filters, n_live), tables
            # top_k beyond the live rows returns them all (Chroma/FAISS); beyond HR_MAX_K the native
            # search takes its exhaustive exact path (same results, one corpus pass per query)
            return self._index.search(q, min(top_k, n_live), self.filter_bitmap(filters)), tables

    def search_device_sync(self, q, top_k: int):
        """(raw, tables) of an unfiltered search of the queries in `q`, a (B, dim) float32 torch tensor that may live
        on the GPU (the in-process embedder's output): the native search reads it in place and only the B * k results
        come back to the host -- no query vectors through host memory (the fused retrieve, retriever.py).  Pass the
        result with the _prep_search of the same queries to _assemble.  An index without a device entry point (tests)
        gets a host copy."""
        return self._search_device(q, top_k, None)

    def search_masks_device_sync(self, q, top_k: int, filters: list):
        """search_device_sync for queries that carry one where-clause (or None) each: (raw, tables) of ONE
        per-query-mask search of the device queries in `q` (the fused retrieve on a mixed_filters store).  The bitmaps
        go up once per call; an index without the device entry point, a multi-device handle or k beyond HR_MAX_K gets
        a host copy of the queries through _run_mixed."""
        return self._search_device(q, top_k, filters)

    def _search_device(self, q, top_k: int, filters: list | None):
        """The two device-query searches: `filters` None = unfiltered, else one where-clause (or None) per query."""
        import torch

        if q.dim() != 2 or (self.dim is not None and q.shape[1] != self.dim):
            raise ValueError(f"queries must be (B, {self.dim})")
        if filters is not None and len(filters) != q.shape[0]:
            raise ValueError(f"{len(filters)} filters for {q.shape[0]} queries")
        with self._lock:  # ordered against mutations, as _run_search
            tables = self._tables()
            n_live = self.count_sync()
            idx = self._index
            if idx is None or n_live == 0 or top_k <= 0:
                return None, tables
            k = min(int(top_k), n_live)
            if filters is None:
                on_device = hasattr(idx, "search_device") and self._single_device(idx)
            else:
                on_device = hasattr(idx, "search_masks_device") and self._takes_masks(idx)
            if not q.is_cuda or k > _native.HR_MAX_K or not on_device:
                q = q.detach().cpu().numpy()
                if filters is None:
                    return idx.search(q, k, None), tables
                return self._run_mixed(q, int(top_k), list(filters), n_live), tables
            q = q.to(torch.float32).contiguous()
            B = q.shape[0]
            s_out, r_out, fetch = self._device_out(q, B, k)
            st = torch.cuda.current_stream(q.device)
            if filters is None:
                idx.search_device(q.data_ptr(), B, k, s_out.data_ptr(), r_out.data_ptr(), stream=st.cuda_stream)
                return fetch(), tables
            masks, mask_of = self._stack_bitmaps(*self._distinct_filters(list(filters)))
            m_dev = torch.from_numpy(masks.view(np.int64)).to(q.device) if masks.size else None
            of_dev = torch.from_numpy(np.ascontiguousarray(mask_of, np.int32)).to(q.device)
            idx.search_masks_device(q.data_ptr(), B, k, s_out.data_ptr(), r_out.data_ptr(),
                                    m_dev.data_ptr() if m_dev is not None else 0, masks.shape[0], masks.shape[1],
                                    of_dev.data_ptr(), stream=st.cuda_stream)
            self.mixed_launches += 1
            return fetch(), tables  # (m_dev, of_dev alive until the results are back)

    @staticmethod
    def _device_out(q, B: int, k: int):
        """One device buffer for a (B, k) answer -- the fp32 scores, then the int64 rows 8-byte aligned -- as (scores
        view, rows view, fetch): ``fetch()`` brings the buffer back in one copy (after the search, on the same stream)
        and returns the host (scores, rows)."""
        import torch

        ns = (B * k + 1) // 2 * 2
        out = torch.empty((ns + 2 * B * k,), dtype=torch.float32, device=q.device)

        def fetch():
            host = out.cpu().numpy()
            return host[:B * k].reshape(B, k).copy(), host[ns:].view(np.int64).reshape(B, k).copy()

        return out[:B * k], out[ns:].view(torch.int64), fetch

    def _submit_native(self, prep, batcher: _SearchBatcher, loop):
        """Launch an unfiltered batch through the asynchronous native entry point from the event loop
        (None: this batch takes the worker-thread path -- a filter, no async-capable index, k beyond
        HR_MAX_K, an empty collection, or the store / handle busy: nothing here ever waits)."""
        if prep.collapse or prep.mmr is not None:  # the worker-thread route, as filtered batches
            return None
        q, top_k, filters = prep.q, prep.top_k, prep.filters
        idx = self._index
        if (filters or idx is None or not self.native_async or top_k <= 0 or top_k > _native.HR_MAX_K
                or not hasattr(idx, "search_submit_host") or not self._single_device(idx)):
            return None
        if not self._lock.acquire(blocking=False):  # a mutation (in a worker thread) holds the store
            return None
        try:
            n_live = self.count_sync()
            if n_live == 0 or self._index is not idx:
                return None
            fd = batcher.native_fd(loop)
            if fd < 0:
                return None
            k = min(top_k, n_live)
            try:
                ticket = idx.search_submit_host(q, k, fd)
            except (NotImplementedError, _native.BusyError):
                return None
            return idx, ticket, q.shape[0], k, self._tables()
        finally:
            self._lock.release()

    def _collect_native(self, info, blocking: bool):
        """(raw, tables) of a finished native launch, as _run_search returns them; None when not blocking
        and the store lock is held, the handle is busy or the batch needs its exact fallback (the caller then
        collects in a worker thread)."""
        idx, ticket, B, k, tables = info
        if not self._lock.acquire(blocking=blocking):
            return None
        try:
            if idx is not self._index or tables[2] != self._epoch:  # cleared / closed since: rows are gone
                return None, tables
            if not blocking and hasattr(idx, "search_poll"):
                # a batch whose collect would run the exact fallback (a synchronous corpus pass) or a handle held
                # by another call: collect in a worker thread, never on the event loop
                try:
                    if idx.search_poll(ticket) != 1:
                        return None
                except _native.BusyError:
                    return None
            return idx.search_collect(ticket, B, k), tables
        finally:
            self._lock.release()

    def _gather(self, ran, extra=None, embeddings: bool = True):
        """The host lists of a finished batch's hits -- (rec_l, meta_l, score_l, per_q, embs) -- or None when the store
        was cleared since the search ran (its rows are gone).  The hits' host records are gathered for the whole batch
        at once (object-array fancy indexing instead of a Python lookup per row and field).  `extra`: one more (B, k)
        array of the search, returned as a sixth list of the same hits; `embeddings` False: embs None whatever
        include_embeddings says."""
        raw, (recs, metas, epoch) = ran
        if raw is None or epoch != self._epoch:
            return None
        scores, rows = raw
        # the tables the search ran against (append-only; a row deleted since then reads None, dropped)
        # rows the index returned but the tables do not hold yet (an add racing a native launch) are
        # treated like rows added after the search
        valid = (rows >= 0) & (rows < min(len(recs), len(metas)))
        hit_rows = rows[valid]
        rec_l = recs.a[hit_rows].tolist()
        meta_l = metas.a[hit_rows].tolist()
        score_l = scores[valid].tolist()
        per_q = valid.sum(axis=1).tolist()
        embs = None
        if embeddings and self.include_embeddings and len(hit_rows):
            keep = [i for i, r in enumerate(rec_l) if r is not None]
            with self._lock:
                if epoch != self._epoch:
                    return None
                e = self._embeddings(hit_rows[keep].tolist())
            embs = [None] * len(rec_l)
            for j, i in enumerate(keep):
                embs[i] = e[j].tolist()
        if extra is not None:
            return rec_l, meta_l, score_l, per_q, embs, extra[valid].tolist()
        return rec_l, meta_l, score_l, per_q, embs

    def _assemble(self, prep, ran) -> list[list[tuple[Chunk, float]]]:
        """(Chunk, score) lists of a finished batch.  Runs on the event loop while the next launch is in
        flight, so it is the host's per-hit cost under load: each hit is a slotted Chunk (two tracked objects per hit
        with its tuple) with a fresh metadata dict, as Chroma returns."""
        g = self._gather(ran)
        if g is None:
            return [[] for _ in range(len(prep[0]))]
        return (_hostfast.assemble if _hostfast is not None else _assemble_py)(Chunk, *g, self.untracked_results)

    def _assemble_results(self, ran, ks: list[int], ths: list[float], result_cls) -> list[list]:
        """A finished batch as the retriever's per-call results (result_cls(chunk, score, rank): top_k ks[q], threshold
        ths[q], ranks before the threshold -- base_retriever.py:66-80 without a reranker), built in one pass without
        the (Chunk, score) pairs: one tracked object fewer per hit for the cycle collector, and no Chunk for a hit past
        its call's top_k."""
        g = self._gather(ran)
        if g is None:
            return [[] for _ in ks]
        fn = _hostfast.assemble_results if _hostfast is not None else _assemble_results_py
        return fn(Chunk, result_cls, *g, [int(k) for k in ks], [float(t) for t in ths], self.untracked_results)

    async def search(self, query_embedding: list[float], top_k: int = 5, filters: dict[str, Any] | None = None, *,
                     collapse: bool = False, mmr_lambda: float | None = None,
                     fetch_k: int | None = None) -> list[tuple[Chunk, float]]:
        """One query through the micro-batcher; ``collapse``, ``mmr_lambda`` and ``fetch_k`` as search_batch."""
        mmr = self._mmr_mode(top_k, mmr_lambda, fetch_k, collapse)  # checked before queueing: a bad query fails alone
        if int(top_k) <= 0:
            return []
        q = np.asarray(query_embedding, dtype=np.float32).reshape(-1)
        if collapse:
            self._check_collapsed_k(top_k)  # checked before queueing: a bad query fails alone
        return await self._batcher.submit(q, top_k, filters, collapse, mmr)

    # -- range search (hr_index_search_range): every chunk scoring at least min_score, and how many
    def _prep_range(self, query_embeddings, min_score, max_hits: int, filters):
        """(q, thresholds, max_hits, filters) of a range search, every limit checked: a bad request fails here,
        before any native call."""
        q = _as_queries(query_embeddings, self.dim)
        max_hits = int(max_hits)
        if max_hits < 0 or max_hits > _native.HR_RANGE_MAX_HITS:
            raise ValueError(f"max_hits must be in [0, {_native.HR_RANGE_MAX_HITS}] (got {max_hits})")
        t = np.asarray(min_score, np.float32).reshape(-1)
        if len(t) not in (1, q.shape[0]):
            raise ValueError(f"{len(t)} thresholds for {q.shape[0]} queries")
        t = np.ascontiguousarray(np.broadcast_to(t, (q.shape[0],)))
        if np.isnan(t).any():
            raise ValueError("min_score must not be NaN")
        filters = _per_query_filters(filters, q.shape[0])
        if not self._single_device(self._index):
            raise ValueError("a range search needs a single-device store")
        return q, t, max_hits, filters

    def _run_range(self, prep):
        """The native range search under the store lock, as _run_search: ((scores, rows) or None, counts, tables).  A
        per-query filter list runs one call per distinct where-clause, scattered back in query order."""
        q, t, max_hits, filters = prep
        B = q.shape[0]
        with self._lock:  # ordered against mutations
            tables = self._tables()
            idx = self._index
            counts = np.zeros(B, np.int64)
            if idx is None or self.count_sync() == 0:
                return None, counts, tables
            if not self._single_device(idx):
                raise ValueError("a range search needs a single-device store")
            if not hasattr(idx, "search_range"):
                raise NotImplementedError(f"{type(idx).__name__} has no range search")
            if not isinstance(filters, list):
                s, r, counts = idx.search_range(q, t, max_hits, self.filter_bitmap(filters))
                return (None if s is None else (s, r)), np.asarray(counts, np.int64), tables

            def call(sel, bitmap):  # (a count-only call, max_hits 0, has no lists: s, r None)
                s, r, counts[sel] = idx.search_range(q[sel], t[sel], max_hits, bitmap)
                return s, r

            raw = self._per_clause(self._distinct_filters(filters), max_hits, call)
            return (raw if max_hits else None), counts, tables

    def search_range_batch(self, query_embeddings, min_score, max_hits: int = 1024, filters=None) -> list[RangeHits]:
        """Every stored chunk whose score is at least ``min_score`` (a scalar or one value per query), exactly: per
        query a RangeHits of the first ``max_hits`` hits, best first, and the exact total -- ``truncated`` tells
        whether the list was cut.  ``filters``: one where-clause, or a list with one (or None) per query."""
        prep = self._prep_range(query_embeddings, min_score, max_hits, filters)
        return self._range_hits(prep, self._run_range(prep))

    def _range_hits(self, prep, ran) -> list[RangeHits]:
        raw, counts, tables = ran  # (raw None -- count-only, nothing stored -- assembles to empty lists)
        return [RangeHits(hits, int(c)) for hits, c in zip(self._assemble(prep, (raw, tables)), counts)]

    def count_above_batch(self, query_embeddings, min_score, filters=None) -> list[int]:
        """How many stored chunks score at least ``min_score``, per query: the count-only range search."""
        prep = self._prep_range(query_embeddings, min_score, 0, filters)
        return [int(c) for c in self._run_range(prep)[1]]

    async def search_range(self, query_embedding: list[float], min_score: float, max_hits: int = 1024,
                           filters: dict[str, Any] | None = None) -> RangeHits:
        """One query's range search, off the event loop (a range call is a corpus pass of its own, not a
        micro-batched top-k)."""
        q = np.asarray(query_embedding, dtype=np.float32).reshape(1, -1)
        prep = self._prep_range(q, min_score, max_hits, filters)  # checked here: a bad request fails alone
        return self._range_hits(prep, await asyncio.to_thread(self._run_range, prep))[0]

    # -- boosted search (hr_index_search_boosted): similarity blended with per-row metadata boosts
    def _prep_boosted(self, query_embeddings, top_k: int, boost_weights, sim_weight, filters, probe, window):
        """(q, k, alpha, betas, filters, probe, window) of a boosted search, every limit checked: a bad request fails
        here, before any native call.  betas: one weight per configured boost field, 0.0 for a field not named."""
        q = _as_queries(query_embeddings, self.dim)
        k = int(top_k)
        if k < 1 or k > _native.HR_MAX_K:
            raise ValueError(f"top_k must be in [1, {_native.HR_MAX_K}] (got {k})")
        alpha = float(sim_weight)
        if not (2.0 ** -64 <= alpha <= 2.0 ** 64):
            raise ValueError(f"sim_weight must be in [2**-64, 2**64] (got {sim_weight})")
        if not isinstance(boost_weights, dict):
            raise ValueError("boost_weights must be a dict of boost field -> weight")
        betas = [0.0] * len(self.boost_fields)
        for name, w in boost_weights.items():
            if name not in self.boost_fields:
                raise ValueError(f"{name!r} is not a configured boost field (index_params.boost_fields = "
                                 f"{self.boost_fields})")
            w = float(w)
            if not abs(w) <= 2.0 ** 64:
                raise ValueError(f"boost weight of {name!r} must be finite and at most 2**64 in size (got {w})")
            betas[self.boost_fields.index(name)] = w
        probe = 0 if probe is None else int(probe)
        if probe != 0 and not k <= probe <= _native.HR_MAX_K:
            raise ValueError(f"probe must be in [top_k, {_native.HR_MAX_K}] (got {probe})")
        window = 0 if window is None else int(window)
        if window != 0 and not k <= window <= _native.HR_BOOST_MAX_WINDOW:
            raise ValueError(f"window must be in [top_k, {_native.HR_BOOST_MAX_WINDOW}] (got {window})")
        filters = _per_query_filters(filters, q.shape[0])
        if not self._single_device(self._index):
            raise ValueError("a boosted search needs a single-device store")
        return q, k, alpha, betas, filters, probe, window

    def _run_boosted(self, prep):
        """The native boosted search under the store lock, as _run_range: ((scores, rows) or None, blended, tables).
        The boost columns are brought up to date under the same lock hold.  A per-query filter list runs one call per
        distinct where-clause, scattered back in query order."""
        q, k, alpha, betas, filters, probe, window = prep
        with self._lock:  # ordered against mutations
            tables = self._tables()
            idx = self._index
            if idx is None or self.count_sync() == 0:
                return None, None, tables
            if not self._single_device(idx):
                raise ValueError("a boosted search needs a single-device store")
            if not hasattr(idx, "search_boosted") or not hasattr(idx, "set_boost"):
                raise NotImplementedError(f"{type(idx).__name__} has no boosted search")
            self._ensure_boosts()
            if not isinstance(filters, list):
                v, s, r = idx.search_boosted(q, k, alpha, betas, self.filter_bitmap(filters), probe, window)
                return (s, r), np.asarray(v, np.float64), tables
            blended = np.full((q.shape[0], k), -np.inf, np.float64)

            def call(sel, bitmap):
                blended[sel], s, r = idx.search_boosted(q[sel], k, alpha, betas, bitmap, probe, window)
                return s, r

            return self._per_clause(self._distinct_filters(filters), k, call), blended, tables

    def _boosted_hits(self, prep, ran) -> list[BoostedHits]:
        raw, blended, tables = ran
        g = None if raw is None else self._gather((raw, tables), extra=blended)
        if g is None:
            return [BoostedHits([], []) for _ in range(len(prep[0]))]
        rec_l, meta_l, score_l, per_q, embs, bl_l = g
        out, i = [], 0
        for hits, cnt in zip(_assemble_py(Chunk, rec_l, meta_l, score_l, per_q, embs), per_q):
            # (a hit deleted since the search ran is dropped, and its blended value with it)
            out.append(BoostedHits(hits, [v for r, v in zip(rec_l[i:i + cnt], bl_l[i:i + cnt]) if r is not None]))
            i += cnt
        return out

    def search_boosted_batch(self, query_embeddings, top_k: int = 5, *, boost_weights: dict, sim_weight: float = 1.0,
                             filters=None, probe: int | None = None, window: int | None = None) -> list[BoostedHits]:
        """The ``top_k`` chunks by ``sim_weight * similarity + sum of boost_weights[f] * metadata[f]`` over the WHOLE
        collection, exactly -- not a re-ranking of a guessed similarity window (hr_index_search_boosted).  The fields
        are those of ``index_params.boost_fields`` (numeric metadata; missing, non-numeric or non-finite values count
        as 0.0); a negative weight is a penalty.  Per query a BoostedHits: the (Chunk, similarity) pairs in blended
        order, and the blended values.  ``filters``: one where-clause, or a list with one (or None) per query;
        ``probe`` / ``window``: the native call's pilot depth and stage-1 window (None: its defaults)."""
        prep = self._prep_boosted(query_embeddings, top_k, boost_weights, sim_weight, filters, probe, window)
        return self._boosted_hits(prep, self._run_boosted(prep))

    async def search_boosted(self, query_embedding: list[float], top_k: int = 5, *, boost_weights: dict,
                             sim_weight: float = 1.0, filters: dict[str, Any] | None = None,
                             probe: int | None = None, window: int | None = None) -> BoostedHits:
        """One query's boosted search, off the event loop (a boosted call is two corpus passes of its own, not a
        micro-batched top-k)."""
        q = np.asarray(query_embedding, dtype=np.float32).reshape(1, -1)
        prep = self._prep_boosted(q, top_k, boost_weights, sim_weight, filters, probe, window)  # a bad request fails alone
        return self._boosted_hits(prep, await asyncio.to_thread(self._run_boosted, prep))[0]

    # -- search by example (hr_index_search_examples): "more like these chunks"
    def _prep_similar(self, positive_ids, negative_ids, top_k: int, filters, query_embeddings, pos_weight, neg_weight):
        """(example rows, fp32 weights, base queries or None, top_k, filters) of a search by example, every limit
        checked and every id resolved: a bad request fails here, before any native call."""
        def ids_of(entry):
            if entry is None:
                return []
            return [entry] if isinstance(entry, str) else list(entry)

        pos = [ids_of(p) for p in positive_ids]
        B = len(pos)
        neg = [[] for _ in range(B)] if negative_ids is None else [ids_of(n) for n in negative_ids]
        if len(neg) != B:
            raise ValueError(f"{len(neg)} negative lists for {B} queries")
        pw, nw = float(pos_weight), float(neg_weight)
        if not (np.isfinite(pw) and np.isfinite(nw)):
            raise ValueError("pos_weight and neg_weight must be finite")
        q = None
        if query_embeddings is not None:
            q = _as_queries(query_embeddings, None)
            if q.shape[0] != B:
                raise ValueError(f"{q.shape[0]} query embeddings for {B} queries")
            q = _as_queries(q, self.dim)  # (the dim after the count, as the checks always ran)
        filters = _per_query_filters(filters, B)
        examples, weights = [], []
        with self._lock:
            for P_, N_ in zip(pos, neg):
                if len(P_) + len(N_) > _native.HR_EX_MAX:
                    raise ValueError(f"a query takes at most {_native.HR_EX_MAX} example chunks "
                                     f"(got {len(P_) + len(N_)})")
                if not P_ and not N_ and q is None:
                    raise ValueError("a query without example chunks needs a query embedding")
                rows = []
                for cid in P_ + N_:
                    row = self._id_to_row.get(cid)
                    if row is None:
                        raise ValueError(f"unknown chunk id {cid!r}")
                    rows.append(int(row))
                examples.append(rows)
                w = [np.float64(pw) / len(P_) for _ in P_] + [-np.float64(nw) / len(N_) for _ in N_]
                weights.append([np.float32(v) for v in w])
        return examples, weights, q, int(top_k), filters

    def _run_similar(self, prep):
        """The search by example under the store lock, as _run_search: ((scores, rows) or None, tables).  Natively
        where the index can, else composed on the host; a per-query filter list runs one call per distinct clause."""
        examples, weights, q, top_k, filters = prep
        B = len(examples)
        with self._lock:  # ordered against mutations
            tables = self._tables()
            idx, n_live = self._index, self.count_sync()
            if idx is None or n_live == 0 or top_k <= 0 or B == 0:
                return None, tables
            k = min(top_k, n_live)
            native = hasattr(idx, "search_examples") and self._single_device(idx)

            def call(sel, bitmap):
                ex, w = [examples[i] for i in sel], [weights[i] for i in sel]
                qs = None if q is None else q[sel]
                if native:
                    return idx.search_examples(ex, k, w, qs, bitmap)
                return search_examples_host(idx, ex, k, w, qs, bitmap)

            if not isinstance(filters, list):
                return call(np.arange(B), self.filter_bitmap(filters)), tables
            return self._per_clause(self._distinct_filters(filters), k, call), tables

    def search_similar_batch(self, positive_ids, negative_ids=None, top_k: int = 5, filters=None,
                             query_embeddings=None, pos_weight: float = 1.0, neg_weight: float = 1.0
                             ) -> list[list[tuple[Chunk, float]]]:
        """"More like these chunks", one query per entry of ``positive_ids`` (a chunk id or a list of them; matching
        entries of ``negative_ids``: chunks to steer away from; ``query_embeddings``: optional base vectors, one per
        query).  The query is ``base + pos_weight * mean(stored positives) - neg_weight * mean(stored negatives)``
        (weights ``pos_weight / |P|`` and ``-neg_weight / |N|``, float64 then fp32), searched exactly; the named chunks
        are never among their own hits.  ``filters``: one where-clause, or a list with one (or None) per query.  An
        unknown chunk id raises ValueError naming it; a query takes at most 32 example chunks."""
        prep = self._prep_similar(positive_ids, negative_ids, top_k, filters, query_embeddings, pos_weight, neg_weight)
        return self._assemble(prep, self._run_similar(prep))

    async def search_similar(self, chunk_ids, top_k: int = 5, filters: dict[str, Any] | None = None, *,
                             negative_ids=None, query_embedding=None) -> list[tuple[Chunk, float]]:
        """One search by example -- ``chunk_ids``: a chunk id or a list of them -- off the event loop."""
        ids = [chunk_ids] if isinstance(chunk_ids, str) else list(chunk_ids)
        neg = negative_ids
        if neg is not None:
            neg = [[neg] if isinstance(neg, str) else list(neg)]
        qe = None if query_embedding is None else np.asarray(query_embedding, np.float32).reshape(1, -1)
        prep = self._prep_similar([ids], neg, top_k, filters, qe, 1.0, 1.0)  # checked here: a bad request fails alone
        return self._assemble(prep, await asyncio.to_thread(self._run_similar, prep))[0]

    # -- fused multi-query search (hr_index_search_fused): groups of queries, one fused list per group
    def _prep_fused(self, query_groups, top_k: int, fusion: str, rrf_k, fetch_k, weights, filters):
        """(q, member counts, top_k, pool depth, mode, rrf_k, flat fp32 weights or None, filters) of a fused search,
        every limit of hr_index_search_fused checked: a bad request fails here, before any native call."""
        if fusion not in _native.FUSE_MODES:
            raise ValueError(f"fusion must be 'rrf' or 'max' (got {fusion!r})")
        groups = [_as_queries(g, None) for g in query_groups]  # (the dim below, with the fused search's own text)
        counts = [int(g.shape[0]) for g in groups]
        if any(m < 1 or m > _native.HR_FUSE_MAX_MEMBERS or g.ndim != 2 for m, g in zip(counts, groups)):
            raise ValueError(f"a group takes 1 to {_native.HR_FUSE_MAX_MEMBERS} query embeddings")
        dim = self.dim if self.dim is not None else (groups[0].shape[1] if groups else 0)
        if any(g.shape[1] != dim for g in groups):
            raise ValueError(f"query dim != collection dim {dim}")
        q = np.concatenate(groups) if groups else np.zeros((0, dim or 1), np.float32)
        k, top = int(top_k), _native.HR_MAX_K
        if k > top:
            raise ValueError(f"a fused search returns at most {top} hits (top_k = {top_k})")
        rk = float(rrf_k)
        if not (np.isfinite(rk) and rk >= 0.0):
            raise ValueError(f"rrf_k must be finite and not negative (got {rrf_k})")
        pool = (max(k, 1) if fusion == "max" else min(top, max(4 * k, 50))) if fetch_k is None else int(fetch_k)
        if pool < max(k, 1) or pool > top:
            raise ValueError(f"fetch_k must be in [top_k, {top}] (got {fetch_k}, top_k = {top_k})")
        w = None
        if weights is not None:
            if fusion == "max":
                raise ValueError("max fusion takes no weights")
            weights = [list(np.atleast_1d(np.asarray(ws, np.float64))) for ws in weights]
            if [len(ws) for ws in weights] != counts:
                raise ValueError("weights must have the shape of query_groups")
            w = np.asarray([v for ws in weights for v in ws], np.float64).astype(np.float32)
            if not np.isfinite(w).all():
                raise ValueError("weights must be finite")
        filters = _per_query_filters(filters, len(q))  # (a list: one where-clause or None per member, flattened)
        if isinstance(filters, list) and not self.mixed_filters:
            raise ValueError("one filter per member needs index_params.mixed_filters = true")
        return q, counts, k, pool, fusion, rk, w, filters

    def _run_fused(self, prep):
        """The fused search under the store lock, as _run_search: ((fused, rows, members) or None, tables).  Natively
        where the index can (a single-device exact index), else composed on the host from its plain search -- one per
        distinct filter -- and fuse_lists_host: the same results."""
        q, counts, k, pool, mode, rk, w, filters = prep
        with self._lock:  # ordered against mutations
            tables = self._tables()
            idx, n_live = self._index, self.count_sync()
            if idx is None or n_live == 0 or k <= 0 or not counts:
                return None, tables
            distinct = self._distinct_filters(filters) if isinstance(filters, list) else None
            if hasattr(idx, "search_fused") and not self.ivf and self._single_device(idx):
                if distinct is not None:
                    masks, mask_of = self._stack_bitmaps(*distinct)
                    self.mixed_launches += 1
                else:
                    bm = self.filter_bitmap(filters)
                    masks, mask_of = (None, None) if bm is None else (bm, np.zeros(len(q), np.int32))
                return idx.search_fused(q, counts, k, pool, mode, rk, w, masks, mask_of), tables
            depth = min(pool, n_live)  # (an index's plain search may refuse more rows than it has)
            if distinct is not None:
                scores, rows = self._per_clause(distinct, pool, lambda sel, bitmap: idx.search(q[sel], depth, bitmap))
            else:
                scores, rows = _padded(len(q), pool)
                scores[:, :depth], rows[:, :depth] = idx.search(q, depth, self.filter_bitmap(filters))
            return fuse_lists_host(scores, rows, counts, k, mode, rk, w), tables

    def _assemble_fused(self, n_groups: int, ran) -> list[FusedHits]:
        """A finished fused batch as FusedHits: _assemble's (Chunk, score) pairs, never with embeddings, and the
        member bits of the hits that are still stored."""
        raw, tables = ran
        g = None if raw is None else self._gather((raw[:2], tables), extra=raw[2], embeddings=False)
        if g is None:
            return [FusedHits([], []) for _ in range(n_groups)]
        rec_l, meta_l, score_l, per_g, _, mem_l = g
        out, i = [], 0
        for hits, cnt in zip(_assemble_py(Chunk, rec_l, meta_l, score_l, per_g, None), per_g):
            # (a hit deleted since the search ran is dropped, and its member bits with it)
            out.append(FusedHits(hits, [m for r, m in zip(rec_l[i:i + cnt], mem_l[i:i + cnt]) if r is not None]))
            i += cnt
        return out

    def search_fused_batch(self, query_groups, top_k: int = 5, *, fusion: str = "rrf", rrf_k: float = 60,
                           fetch_k: int | None = None, weights=None, filters=None) -> list[FusedHits]:
        """Several queries per question, one fused list per question: ``query_groups`` is a list of groups, each 1 to
        16 query embeddings (rewrites, HyDE answers, sub-questions of one question).  Every member is searched exactly
        for ``fetch_k`` chunks -- all members of all groups in one scan -- and each group's lists are fused on the GPU.
        ``fusion="rrf"``: reciprocal rank, ``sum of weight / (rrf_k + rank)`` over the members holding the chunk, in
        float64 in member order (``weights``: the shape of ``query_groups``, default 1; ``fetch_k`` default
        ``min(128, max(4 top_k, 50))``; the score is a function of the rank window, not a similarity).
        ``fusion="max"``: the largest similarity any member gives the chunk (what merging searches by score does;
        ``fetch_k`` default ``top_k``; no weights).  Ordered by fused score descending, then row ascending.
        ``filters``: one where-clause for everything, or a list with one (or None) per member in flattened order (needs
        ``index_params.mixed_filters``).  Per group a FusedHits: the (Chunk, fused score) pairs and, per hit, the
        bitmask of the members that found it.  An index without the native call (IVF_FLAT, multi-device) is composed on
        the host from its plain search, with the same results wherever that search is exact."""
        prep = self._prep_fused(query_groups, top_k, fusion, rrf_k, fetch_k, weights, filters)
        return self._assemble_fused(len(prep[1]), self._run_fused(prep))

    async def search_fused(self, query_embeddings, top_k: int = 5, filters=None, *, fusion: str = "rrf",
                           rrf_k: float = 60, fetch_k: int | None = None, weights=None) -> FusedHits:
        """One group -- the query embeddings of one question -- off the event loop; keywords as search_fused_batch
        (``weights``: one per embedding; ``filters``: one where-clause or one per embedding)."""
        prep = self._prep_fused([query_embeddings], top_k, fusion, rrf_k, fetch_k,
                                None if weights is None else [weights], filters)  # a bad request fails alone
        return self._assemble_fused(1, await asyncio.to_thread(self._run_fused, prep))[0]

    def get_by_id_sync(self, chunk_id: str) -> Chunk | None:
        with self._lock:
            row = self._id_to_row.get(chunk_id)
            if row is None:
                return None
            return self._chunk(row, self._embeddings([row])[0].tolist())

    async def get_by_id(self, chunk_id: str) -> Chunk | None:
        return await asyncio.to_thread(self.get_by_id_sync, chunk_id)

    def row_of(self, chunk_id: str) -> int | None:
        """The index row of a stored chunk (None: not stored) -- the tie-break order of fused rankings."""
        return self._id_to_row.get(chunk_id)

    def count_sync(self) -> int:
        return len(self._id_to_row)

    async def count(self) -> int:
        return self.count_sync()


class VectorStoreFactory:
    """``VectorStoreFactory.create(config)`` like storage/base_storage.py:15-43.

    "hip" selects the MI355X index; "chroma" configs (the reference default) are
    served by the same index, which reproduces Chroma's add/query/where semantics
    with exact search (a persisted Chroma directory is not read)."""

    @staticmethod
    def create(config: VectorStoreConfig, **kwargs) -> BaseVectorStore:
        backend = config.backend.lower()
        if backend in ("hip", "chroma"):
            return HipVectorStore(config=config, **kwargs)
        raise ValueError(f"Unsupported vector store backend: {backend}")

    @staticmethod
    def list_backends() -> list[str]:
        return ["hip", "chroma"]
