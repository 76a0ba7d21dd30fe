"""Retrievers over any BaseVectorStore / BaseEmbedder pair.

VectorRetriever keeps the reference's semantics exactly
(utu/rag/knowledge_retrieval/base_retriever.py:14-99):
  * ``top_k`` falls back to config.top_k (:53); ``filters`` / ``similarity_threshold``
    come from kwargs (:54-55);
  * the store is asked for ``2*top_k`` when a reranker is set, else ``top_k`` (:61-63),
    with the keyword call ``query_embedding=``;
  * ranks are the 1-based positions BEFORE threshold filtering (:72), and a
    threshold <= 0 disables filtering (:71);
  * optional rerank, then ``[:top_k]`` (:75-80).
``collapse=True`` in the kwargs (no counterpart in the reference) asks the store for one hit per group -- the best chunk
of each of the best documents (HipVectorStore, ``collapse_field``); threshold, ranks and the ``2*top_k`` fetch under a
reranker apply to the collapsed list as to the plain one.
``mmr_lambda=`` (with an optional ``fetch_k=``) in the kwargs asks the store for a diversified list instead (maximal
marginal relevance, HipVectorStore.search_batch): the hits arrive in selection order with their plain-search scores, and
threshold, ranks and the ``2*top_k`` fetch under a reranker apply to that list in the same way.
BatchedVectorRetriever overrides batch_retrieve (the reference's loop at :95-98)
with one query-embedding batch and one GPU search launch for the whole batch,
producing the same per-query results.
"""
from __future__ import annotations

import asyncio
import logging
import os
import threading
import time
import weakref

from .base import BaseEmbedder, BaseReranker, BaseRetriever, BaseVectorStore, RetrievalResult
from .config import RetrieverConfig

logger = logging.getLogger(__name__)


class _Cohort:
    """One event loop's waiting retrieve calls and whether its drain is running."""

    __slots__ = ("pending", "running", "__weakref__")

    def __init__(self):
        self.pending: list = []
        self.running = False


class _FusedRetrieve:
    """Concurrent ``retrieve`` calls (base_retriever.py:53-63: embed_query, then store.search) as cohorts of up to
    ``max_batch`` queries, each cohort ONE embedder forward whose (B, dim) output stays on the GPU and goes straight
    into ONE store search -- no per-query vector lists through the host, no second batching stage.

    One worker thread pipelines the cohorts: it enqueues cohort i+1's forward and its search (the pipelined shard
    search of hiprag.dist.ShardedSearch on the store's index: scan + tail streams, guard flags copied asynchronously)
    BEFORE it waits for cohort i's results, so the GPU always has the next cohort queued behind the current one while
    the host tokenises, finalizes and hands results back.  The store's lock is held from a cohort's submit to its
    finalize (a mutation must not move rows under a search in flight).  The Chunk objects are built on the caller's
    loop.  Results are those of the two-step path for the same vectors (the same exact search).  Each event loop has
    its own queue and drain (futures are resolved on their own loop only)."""

    def __init__(self, retriever: "VectorRetriever", max_batch: int):
        import queue

        self.r, self.max_batch = retriever, max(1, int(max_batch))
        self._queues: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
        self._qlock = threading.Lock()
        self._work: "queue.Queue" = queue.Queue()  # cohorts from every loop, to the worker
        self._thread = None
        self._tlock = threading.Lock()
        self._searcher = None  # (index, ShardedSearch) of the store's current index
        self._k = 0  # the current cohort's largest top_k (worker thread)
        self.cohorts = 0  # diagnostics: cohorts run / queries through them / cohorts overlapped with the next
        self.queries = 0
        self.pipelined = 0
        # diagnostics (worker thread, seconds): forward tokenise + launch, search submit, finalize (the device wait
        # included), and cohorts finalized with no next cohort queued behind them (pipeline bubbles)
        self.timing = {"encode": 0.0, "submit": 0.0, "finalize": 0.0, "bubbles": 0}

    def submit(self, query: str, top_k: int, threshold: float, filters=None) -> asyncio.Future:
        """Queue one call; `filters` (a mixed_filters store only): the call's where-clause -- the cohort's search then
        runs as one per-query-mask call through the synchronous device path."""
        loop = asyncio.get_running_loop()
        fut = loop.create_future()
        with self._qlock:
            c = self._queues.get(loop)
            if c is None:
                c = self._queues[loop] = _Cohort()
        c.pending.append((query, int(top_k), float(threshold), fut, filters or None))
        if not c.running:
            c.running = True
            loop.call_soon(self._form, c, loop)
        return fut

    def _form(self, c: _Cohort, loop):
        """On the loop, one iteration after the first call: hand the waiting calls to the worker in cohorts."""
        c.running = False
        while c.pending:
            batch, c.pending = c.pending[: self.max_batch], c.pending[self.max_batch:]
            batch = [e for e in batch if not e[3].done()]
            if batch:
                self._work.put((loop, batch))  # (before the check: a worker that is just leaving sees it)
                self._ensure_worker()

    def _ensure_worker(self):
        with self._tlock:
            if self._thread is None or not self._thread.is_alive():
                self._thread = threading.Thread(target=self._worker, name="hiprag-retrieve", daemon=True)
                self._thread.start()

    # ---- worker thread
    def _search(self, q, filters=None):
        """Launch the cohort's search (store lock held by the caller).  Returns a finisher -> (raw, tables).
        `filters`: one where-clause or None per query when some call of the cohort carries one."""
        store = self.r.vector_store
        if filters is not None:  # per-query masks: the synchronous device path (never the pipelined submit)
            ran = store.search_masks_device_sync(q, self._k, filters)
            return lambda: ran
        tables = store._tables()
        idx, n_live = store._index, store.count_sync()
        B, k = q.shape[0], self._k
        if idx is None or n_live == 0 or k <= 0:
            return lambda: (None, tables)
        k = min(k, n_live)
        ss = self._sharded(idx, B) if q.is_cuda else None
        if ss is None:  # (CPU tests, multi-device handles, k beyond the pipelined path: the synchronous search)
            ran = store.search_device_sync(q, k)
            return lambda: ran
        # (k above the searcher's kc: submit completes the cohort in flight -- its ticket keeps its answer -- and
        # answers this one synchronously)
        ticket = ss.submit(q, k)

        def finish():
            s_out, r_out = ss.finalize(ticket)
            return (s_out.cpu().numpy(), r_out.cpu().numpy()), tables
        return finish

    def _sharded(self, idx, B):
        from .. import _native

        store = self.r.vector_store
        if not hasattr(idx, "search_shard") or not store._single_device(idx) or self._k > _native.HR_MAX_K:
            return None
        if self._searcher is None or self._searcher[0] is not idx or self._searcher[1].max_batch < B:
            import torch

            from ..dist import ShardedSearch

            self._drop_searcher()
            dev = torch.device("cuda", idx.device)
            self._searcher = (idx, ShardedSearch(idx, 0, max_batch=max(B, self.max_batch), device=dev, max_k=16))
        return self._searcher[1]

    def _deliver(self, loop, batch, ran, exc=None):
        """Back on the caller's loop: Chunks from the finished search, each call's top_k and threshold."""
        if exc is None:
            try:
                res = self.r.vector_store._assemble_results(ran, [e[1] for e in batch], [e[2] for e in batch],
                                                            RetrievalResult)
            except Exception as e:  # noqa: BLE001
                exc = e
        for i, (_, kq, th, f, _flt) in enumerate(batch):
            if f.done():
                continue
            if exc is not None:
                f.set_exception(exc)
            else:
                f.set_result(res[i])

    def _post(self, loop, batch, ran, exc=None):
        if loop.is_closed():
            return  # (the caller's loop ended: nobody waits for these)
        try:
            loop.call_soon_threadsafe(self._deliver, loop, batch, ran, exc)
        except RuntimeError:  # closed between the check and the call
            pass

    def _worker(self):
        import queue

        store = self.r.vector_store
        inflight = None  # (loop, batch, finisher) of the cohort whose search is on the GPU
        locked = False
        while True:
            try:
                item = self._work.get(timeout=0.5) if inflight is None else self._work.get_nowait()
            except queue.Empty:
                item = None
            if item is None and inflight is None:
                with self._tlock:  # (under the lock _ensure_worker takes: a cohort put now starts a new worker)
                    if self._work.empty():
                        self._thread = None
                        return  # idle: the thread ends
                continue
            nxt = None
            tm = self.timing
            if item is not None:
                loop, batch = item
                try:
                    self._k = max(e[1] for e in batch)
                    t0 = time.perf_counter()
                    q = self.r.embedder.encode_queries([e[0] for e in batch])  # (device, enqueued)
                    t1 = time.perf_counter()
                    if not locked:
                        store._lock.acquire()
                        locked = True
                    flt = [e[4] for e in batch]
                    nxt = (loop, batch, self._search(q, flt if any(flt) else None))
                    tm["encode"] += t1 - t0
                    tm["submit"] += time.perf_counter() - t1
                except Exception as e:  # noqa: BLE001 -- this cohort's callers see the failure
                    self._post(loop, batch, None, e)
            if inflight is not None:
                loop0, batch0, finish = inflight
                if nxt is None:
                    tm["bubbles"] += 1
                t0 = time.perf_counter()
                try:
                    ran = finish()
                    self._post(loop0, batch0, ran)
                except Exception as e:  # noqa: BLE001
                    self._post(loop0, batch0, None, e)
                tm["finalize"] += time.perf_counter() - t0
                self.cohorts += 1
                self.queries += len(batch0)
                if nxt is not None:
                    self.pipelined += 1
            inflight = nxt
            if inflight is None and locked:
                store._lock.release()
                locked = False

    def _drop_searcher(self):
        """Release the pipelined searcher of a previous index (nothing is in flight: the worker finalizes every
        cohort before it takes the next index); a store that closed its index already released what it held."""
        if self._searcher is None:
            return
        idx, ss = self._searcher
        self._searcher = None
        if getattr(idx, "_h", None):
            ss.close()

    def close(self):
        t = self._thread
        if t is not None:
            t.join(timeout=10)
        self._drop_searcher()


class VectorRetriever(BaseRetriever):
    def __init__(self, vector_store: BaseVectorStore, embedder: BaseEmbedder, config: RetrieverConfig | None = None,
                 reranker: BaseReranker | None = None):
        self.vector_store = vector_store
        self.embedder = embedder
        self.config = config or RetrieverConfig()
        self.reranker = reranker
        if self.config.enable_reranking and self.reranker is None:
            # the reference builds RerankerFactory.create(backend="auto", model=config.reranker_model)
            # (base_retriever.py:36-40), an HTTP client; the MI355X replacement is the in-process
            # cross-encoder (local checkpoint if reranker_model is a path, else the seeded preset)
            from .rerankers import RerankerFactory

            self.reranker = RerankerFactory.create(backend="rocm", model_name_or_path=self.config.reranker_model)
        # the fused path (one forward + one device-query search per cohort of concurrent calls) where both halves are
        # hiprag's: the in-process embedder and the HIP store; anything else keeps the reference's two awaits
        self._fused = _FusedRetrieve(self, getattr(embedder, "batch_size", 64)) if self._fusable() else None

    def _fusable(self) -> bool:
        if os.environ.get("HIPRAG_FUSED_RETRIEVE", "1") == "0":  # (A/B switch: the reference's two awaits)
            return False
        return (self.reranker is None and callable(getattr(self.vector_store, "search_device_sync", None))
                and callable(getattr(self.vector_store, "_assemble_results", None))
                and callable(getattr(self.embedder, "encode_queries", None))
                and hasattr(self.embedder, "_fwd_lock") and getattr(self.embedder, "fused_retrieve", True))

    def _to_results(self, hits, threshold: float) -> list[RetrievalResult]:
        out = []
        for pos, (chunk, score) in enumerate(hits):
            if threshold <= 0.0 or score >= threshold:
                out.append(RetrievalResult(chunk=chunk, score=score, rank=pos + 1))
        return out

    async def _finish(self, query: str, results: list[RetrievalResult], top_k: int) -> list[RetrievalResult]:
        if self.reranker and results:
            results = await self.reranker.rerank(query=query, results=results, top_k=top_k)
        return results[:top_k]

    @staticmethod
    def _mode_kwargs(kwargs) -> dict:
        """The store keywords of a collapsed or MMR call (empty: the reference's call, for any store)."""
        extra = {"collapse": True} if kwargs.get("collapse", False) else {}
        if kwargs.get("mmr_lambda") is not None:
            extra["mmr_lambda"] = kwargs["mmr_lambda"]
            if kwargs.get("fetch_k") is not None:
                extra["fetch_k"] = kwargs["fetch_k"]
        return extra

    async def retrieve(self, query: str, top_k: int | None = None, **kwargs) -> list[RetrievalResult]:
        top_k = top_k or self.config.top_k
        threshold = kwargs.get("similarity_threshold", self.config.similarity_threshold)
        extra = self._mode_kwargs(kwargs)
        collapse = bool(extra)  # collapsed and MMR calls bypass the fused cohort path
        filters = kwargs.get("filters")
        # filtered calls stay in the cohort on a mixed_filters store (one forward, one per-query-mask search)
        mixed = bool(filters) and isinstance(filters, dict) and getattr(self.vector_store, "mixed_filters", False) \
            and callable(getattr(self.vector_store, "search_masks_device_sync", None))
        if self._fused is not None and (not filters or mixed) and self.reranker is None and not collapse:
            if mixed:
                return await self._fused.submit(query, top_k, threshold, filters)
            return await self._fused.submit(query, top_k, threshold)
        qv = await self.embedder.embed_query(query)
        hits = await self.vector_store.search(query_embedding=qv, top_k=top_k * 2 if self.reranker else top_k,
                                              filters=kwargs.get("filters"), **extra)
        return await self._finish(query, self._to_results(hits, threshold), top_k)

    async def retrieve_above(self, query: str, threshold: float | None = None, limit: int = 1024,
                             filters: dict | None = None) -> list[RetrievalResult]:
        """Every chunk scoring at least ``threshold``, best first, at most ``limit`` of them: the store's range
        search, so nothing relevant hides below a guessed top_k.  ``None`` means ``config.similarity_threshold`` and
        the value is used as given -- here 0.0 is a threshold like any other, unlike retrieve(), where <= 0 disables
        the cut.  Ranks are 1-based; the optional reranker and the final cut apply as in retrieve()."""
        search_range = getattr(self.vector_store, "search_range", None)
        if search_range is None:
            raise NotImplementedError(f"{type(self.vector_store).__name__} has no range search")
        t = self.config.similarity_threshold if threshold is None else threshold
        qv = await self.embedder.embed_query(query)
        found = await search_range(query_embedding=qv, min_score=float(t), max_hits=int(limit), filters=filters)
        results = [RetrievalResult(chunk=chunk, score=score, rank=pos + 1)
                   for pos, (chunk, score) in enumerate(found.hits)]
        return await self._finish(query, results, int(limit))

    async def retrieve_boosted(self, query: str, top_k: int | None = None, *, boost_weights: dict,
                               sim_weight: float = 1.0, filters: dict | None = None,
                               similarity_threshold: float | None = None) -> list[RetrievalResult]:
        """The ``top_k`` chunks by ``sim_weight * similarity + sum of boost_weights[f] * metadata[f]`` over the whole
        collection -- the store's boosted search (``index_params.boost_fields``), not a re-ranking of a guessed
        similarity window.  ``score`` is the blended value; ``similarity_threshold`` (default
        ``config.similarity_threshold``, <= 0 disables it as in retrieve()) cuts by the SIMILARITY of a hit, so it
        keeps its meaning whatever the weights.  Ranks are 1-based, before the cut; the optional reranker and the
        final cut apply as in retrieve().

        The reference's memory ranking (memory_toolkit.py:919), ``0.5 * similarity + 0.3 * importance_score + 0.2 *
        recency`` with ``recency = 2 ** (-(now - created_at) / 24h)``, needs no column rewrite as time passes: store
        ``importance_score`` and the static ``recency_base = 2 ** ((created_at - epoch) / 24h)`` as boost fields; the
        query-time factor ``2 ** (-(now - epoch) / 24h)`` folds into that column's weight:
        ``boost_weights={"importance_score": 0.3, "recency_base": 0.2 * 2 ** (-(now - epoch) / 24h)}, sim_weight=0.5``
        (choose ``epoch`` near the newest memories so that ``recency_base`` stays inside float32)."""
        search_boosted = getattr(self.vector_store, "search_boosted", None)
        if search_boosted is None:
            raise NotImplementedError(f"{type(self.vector_store).__name__} has no boosted search")
        top_k = top_k or self.config.top_k
        threshold = self.config.similarity_threshold if similarity_threshold is None else similarity_threshold
        qv = await self.embedder.embed_query(query)
        found = await search_boosted(query_embedding=qv, top_k=top_k * 2 if self.reranker else top_k,
                                     boost_weights=boost_weights, sim_weight=sim_weight, filters=filters)
        results = [RetrievalResult(chunk=chunk, score=float(v), rank=pos + 1)
                   for pos, ((chunk, sim), v) in enumerate(zip(found.hits, found.blended))
                   if not (threshold > 0 and sim < threshold)]
        return await self._finish(query, results, top_k)

    async def retrieve_similar(self, chunk_id_or_ids, top_k: int | None = None, filters: dict | None = None,
                               negative_ids=None, query: str | None = None) -> list[RetrievalResult]:
        """"More like this chunk": the store's search by example over the stored vectors of ``chunk_id_or_ids`` (one
        id or a list), steered away from ``negative_ids``; ``query`` is embedded and used as the base vector
        (relevance feedback on top of the question).  The named chunks are never returned.  Ranks (1-based, before the
        threshold), ``config.similarity_threshold`` and the final cut as in retrieve(); the reranker needs a text to
        rank against, so it applies only with ``query``."""
        search_similar = getattr(self.vector_store, "search_similar", None)
        if search_similar is None:
            raise NotImplementedError(f"{type(self.vector_store).__name__} has no search by example")
        top_k = top_k or self.config.top_k
        rerank = self.reranker is not None and query is not None
        qv = await self.embedder.embed_query(query) if query is not None else None
        hits = await search_similar(chunk_id_or_ids, top_k=top_k * 2 if rerank else top_k, filters=filters,
                                    negative_ids=negative_ids, query_embedding=qv)
        results = self._to_results(hits, self.config.similarity_threshold)
        return await self._finish(query, results, top_k) if rerank else results[:top_k]

    async def retrieve_fused(self, queries: list[str], top_k: int | None = None, *, fusion: str = "rrf",
                             filters=None, rrf_k: float = 60, fetch_k: int | None = None, weights=None,
                             similarity_threshold: float | None = None) -> list[RetrievalResult]:
        """Several phrasings of ONE question -- rewrites, a HyDE answer, sub-questions -- answered as one list: one
        ``embed_queries`` call over all of them and one fused search of the store (``search_fused``): every phrasing
        searched exactly, the lists fused on the GPU.  ``fusion="rrf"``: reciprocal rank, ``sum of weight / (rrf_k +
        rank)``; ``fusion="max"``: the best similarity any phrasing gives the chunk.  ``filters``: one where-clause, or
        one per phrasing.  ``score`` is the fused score and ``rank`` counts from 1 (before the threshold).
        ``similarity_threshold`` (default ``config.similarity_threshold``) applies to "max" scores only: an RRF score
        is a sum of reciprocal ranks, not a similarity, and is never cut by it.  The optional reranker ranks against
        the first phrasing; then ``[:top_k]``, as in retrieve()."""
        search_fused = getattr(self.vector_store, "search_fused", None)
        if search_fused is None:
            raise NotImplementedError(f"{type(self.vector_store).__name__} has no fused search")
        queries = list(queries)
        if not queries:
            return []
        top_k = top_k or self.config.top_k
        threshold = self.config.similarity_threshold if similarity_threshold is None else similarity_threshold
        embed_many = getattr(self.embedder, "embed_queries", None)
        qvs = await embed_many(queries) if embed_many else [await self.embedder.embed_query(q) for q in queries]
        depth = top_k * 2 if self.reranker else top_k
        if fetch_k is not None and fetch_k >= top_k:  # (the reranker's margin never asks for more than the pools hold)
            depth = min(depth, int(fetch_k))
        found = await search_fused(qvs, top_k=depth, filters=filters, fusion=fusion, rrf_k=rrf_k, fetch_k=fetch_k,
                                   weights=weights)
        results = self._to_results(found.hits, threshold if fusion == "max" else 0.0)
        return await self._finish(queries[0], results, top_k)

    async def batch_retrieve(self, queries: list[str], top_k: int | None = None, **kwargs
                             ) -> list[list[RetrievalResult]]:
        return [await self.retrieve(query=q, top_k=top_k, **kwargs) for q in queries]


class BatchedVectorRetriever(VectorRetriever):
    """Same results as VectorRetriever, but batch_retrieve embeds all queries at once
    (``embed_queries`` when the embedder has it) and runs one batched search."""

    async def batch_retrieve(self, queries: list[str], top_k: int | None = None, **kwargs
                             ) -> list[list[RetrievalResult]]:
        if not queries:
            return []
        search_batch = getattr(self.vector_store, "search_batch", None)
        if search_batch is None:
            return await super().batch_retrieve(queries, top_k=top_k, **kwargs)
        top_k = top_k or self.config.top_k
        threshold = kwargs.get("similarity_threshold", self.config.similarity_threshold)
        embed_many = getattr(self.embedder, "embed_queries", None)
        qvs = await embed_many(queries) if embed_many else [await self.embedder.embed_query(q) for q in queries]
        extra = self._mode_kwargs(kwargs)
        hits = search_batch(qvs, top_k * 2 if self.reranker else top_k, kwargs.get("filters"), **extra)
        results = [self._to_results(h, threshold) for h in hits]
        rerank_batch = getattr(self.reranker, "rerank_batch", None)
        if rerank_batch is not None:  # one set of cross-encoder batches for every query's pairs
            idx = [i for i, r in enumerate(results) if r]
            try:
                for i, r in zip(idx, rerank_batch([queries[i] for i in idx], [results[i] for i in idx], top_k)):
                    results[i] = r
                return [r[:top_k] for r in results]
            except Exception as e:  # per-query path keeps the reference's failure semantics
                logger.error(f"batched reranking failed ({e}); reranking query by query")
        return [await self._finish(q, r, top_k) for q, r in zip(queries, results)]


def rrf_fuse(dense: list, lexical: list, rrf_k: float = 60.0) -> list[tuple]:
    """Reciprocal-rank fusion of two rankings given as (key, rank, payload) lists (ranks from 1): per key
    ``sum over the lists holding it of 1 / (rrf_k + rank)``, the dense term added first; returns (key, fused score,
    payload) by fused score descending, then key ascending (the payload of the first list that holds the key)."""
    fused: dict = {}
    for hits in (dense, lexical):
        for key, rank, payload in hits:
            term = 1.0 / (rrf_k + rank)
            if key in fused:
                fused[key][0] += term
            else:
                fused[key] = [term, payload]
    return [(key, v[0], v[1]) for key, v in sorted(fused.items(), key=lambda kv: (-kv[1][0], kv[0]))]


class HybridRetriever(BaseRetriever):
    """Dense + keyword retrieval fused by reciprocal rank (the reference's HybridRetriever delegates to the vector
    retriever and leaves the rest as a TODO, base_retriever.py:102-154: "a full hybrid retrieval would include
    keyword-based search (e.g., BM25) and combine scores").

    Over a store with a lexical index (HipVectorStore with ``index_params.lexical``: it has ``keyword_search_batch``)
    every query runs the dense search and the BM25 keyword search at depth ``fetch_k`` (default
    ``min(128, max(4 * top_k, 50))``) and the two rankings are fused: ``fused(chunk) = sum of 1 / (rrf_k + rank)`` over
    the lists that hold it (ranks from 1, the dense term added first), ordered by fused score descending, then chunk
    row ascending.  ``similarity_threshold`` drops dense hits as in VectorRetriever (ranks taken before it); keyword
    hits are not thresholded.  Then the optional reranker and ``[:top_k]``.  Over any other store: the delegation."""

    def __init__(self, vector_store: BaseVectorStore, embedder: BaseEmbedder, config: RetrieverConfig | None = None,
                 reranker: BaseReranker | None = None, *, fusion: str = "rrf", rrf_k: float = 60,
                 fetch_k: int | None = None):
        if fusion != "rrf":
            raise ValueError(f"unsupported fusion {fusion!r} (only 'rrf')")
        self.vector_retriever = BatchedVectorRetriever(vector_store=vector_store, embedder=embedder, config=config,
                                                       reranker=reranker)
        self.vector_store, self.embedder = vector_store, embedder
        self.config = config or RetrieverConfig()
        self.fusion, self.rrf_k, self.fetch_k = fusion, float(rrf_k), fetch_k

    @property
    def reranker(self):
        return self.vector_retriever.reranker

    def _keyword_search(self):
        fn = getattr(self.vector_store, "keyword_search_batch", None)
        return fn if callable(fn) and getattr(self.vector_store, "lexical", True) else None

    def _row_of(self, chunk) -> tuple:
        """The fusion key of a chunk: its row in the store (unknown stores: the order of its id)."""
        row_of = getattr(self.vector_store, "row_of", None)
        row = row_of(chunk.id) if row_of is not None else None
        return (0, row, "") if row is not None else (1, 0, chunk.id)

    async def retrieve(self, query: str, top_k: int | None = None, **kwargs) -> list[RetrievalResult]:
        if self._keyword_search() is None:
            return await self.vector_retriever.retrieve(query=query, top_k=top_k, **kwargs)
        return (await self.batch_retrieve([query], top_k=top_k, **kwargs))[0]

    async def batch_retrieve(self, queries: list[str], top_k: int | None = None, **kwargs
                             ) -> list[list[RetrievalResult]]:
        keyword_search = self._keyword_search()
        if keyword_search is None:
            return await self.vector_retriever.batch_retrieve(queries=queries, top_k=top_k, **kwargs)
        if kwargs.get("collapse", False):
            raise ValueError("HybridRetriever does not fuse collapsed lists: collapse=True needs a store without an "
                             "active keyword search, or VectorRetriever")
        if kwargs.get("mmr_lambda") is not None:
            raise ValueError("HybridRetriever does not fuse MMR lists: mmr_lambda needs a store without an active "
                             "keyword search, or VectorRetriever")
        if not queries:
            return []
        top_k = top_k or self.config.top_k
        threshold = kwargs.get("similarity_threshold", self.config.similarity_threshold)
        filters = kwargs.get("filters")
        fetch_k = self.fetch_k or min(128, max(4 * top_k, 50))
        vr = self.vector_retriever
        embed_many = getattr(self.embedder, "embed_queries", None)
        qvs = await embed_many(queries) if embed_many else [await self.embedder.embed_query(q) for q in queries]
        search_batch = getattr(self.vector_store, "search_batch", None)
        if search_batch is not None:
            dense = search_batch(qvs, fetch_k, filters)
        else:
            dense = [await self.vector_store.search(query_embedding=qv, top_k=fetch_k, filters=filters) for qv in qvs]
        lexical = keyword_search(queries, fetch_k, filters)
        out = []
        for q, d_hits, l_hits in zip(queries, dense, lexical):
            d = [(self._row_of(r.chunk), r.rank, r.chunk) for r in vr._to_results(d_hits, threshold)]
            lx = [(self._row_of(c), pos + 1, c) for pos, (c, _) in enumerate(l_hits)]
            fused = rrf_fuse(d, lx, self.rrf_k)
            results = [RetrievalResult(chunk=c, score=s, rank=i + 1) for i, (_, s, c) in enumerate(fused)]
            out.append(await vr._finish(q, results, top_k))
        return out
