/*
 * hiprag.h -- C ABI of libhiprag.so, the MI355X-native vector index behind
 * youtu-rag's KB-search plugin interfaces.
 *
 * Every entry point replaces one numeric call of the reference's vector store
 * (paths relative to the youtu-rag tree; the store is a BaseVectorStore,
 * utu/rag/base.py:187-232):
 *
 *   hr_index_create    ChromaVectorStore.__init__ / FAISSVectorStore.__init__
 *                        (chroma_store.py:25-62 get_or_create_collection with hnsw:space;
 *                         faiss_store.py:31-58 IndexFlatIP/IndexFlatL2 choice :102-105)
 *   hr_index_add       add_chunks -> collection.add / normalize_L2 + index.add
 *                        (chroma_store.py:64-88, faiss_store.py:89-127)
 *   hr_index_remove    delete / delete_by_document_id (row tombstones)
 *                        (chroma_store.py:150-183, faiss_store.py:201-254)
 *   hr_index_search    search -> collection.query(n_results=top_k, where=...)
 *                        (chroma_store.py:90-148; exact semantics of faiss_store.py:129-199)
 *   hr_index_search_device  the same on device-resident queries/results (batched
 *                        VectorRetriever.batch_retrieve, base_retriever.py:82-99)
 *   hr_index_size      count (chroma_store.py:249-255, faiss_store.py:283-289)
 *   hr_index_get_rows  get_by_id's stored embedding (chroma_store.py:224-247)
 *   hr_index_save/load PersistentClient dir / faiss write_index+pickle
 *                        (chroma_store.py:41-44, faiss_store.py:61-87)
 *   hr_index_search_shard / hr_index_search_shard_collect / hr_merge_candidates
 *                      row-sharded multi-GPU search (no reference counterpart: the
 *                      reference is single-process)
 *   hr_pool_normalize  the embedding server's masked mean-pool + F.normalize
 *                        (docs/content/docs/en/youtu-embedding/deploying-locally.mdx:75-79, :98-115)
 *
 * Conventions: every int-returning call returns 0 on success or a negative
 * HR_E_* code; hr_last_error() then holds a thread-local message.  Handles are
 * opaque; calls on one handle are serialised by an internal mutex.  Host
 * pointers are caller-owned; "_device"/"_shard"/merge calls take device pointers
 * and run on the given hipStream_t (NULL = the null stream, which is also
 * PyTorch's default stream); host-pointer calls use the handle's own stream and
 * return after synchronising it.  Scores follow the
 * reference's similarity convention (cosine/dot: inner product; euclidean: 1 - |q - x|^2).  Result order:
 * score descending, then row ascending; unfilled slots hold score -inf, row -1.
 * Diagnostic / measurement entry points (kernel counters, scan timing, stamps) are in include/hiprag_diag.h.
 */
#ifndef HIPRAG_H
#define HIPRAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hr_index hr_index;

enum { HR_F32 = 0, HR_BF16 = 1, HR_F16 = 2 };         /* storage dtype */
/* distance metric (chroma_store.py:48-53): cosine (rows + queries L2-normalised, score = inner
 * product), ip ("dot": raw inner product), l2 ("euclidean": score = 1 - squared distance, Chroma's
 * similarity = 1 - distance, :135) */
enum { HR_COSINE = 0, HR_IP = 1, HR_L2 = 2 };
enum {
    HR_OK = 0,
    HR_E_INVALID = -1,   /* bad argument -> Python ValueError */
    HR_E_HIP = -2,       /* HIP runtime error -> RuntimeError */
    HR_E_UNSUPPORTED = -3,
    HR_E_OVERFLOW = -4,  /* candidate buffer overflow in the exact fallback */
    HR_E_IO = -5,
    HR_E_BUSY = -6       /* hr_index_search_submit_host: another call holds the handle (never waits) */
};

#define HR_MAX_K 128           /* largest top-k (kb_file_search recall 15 x 3, rerank top-100) */
#define HR_MAX_KC 256          /* largest per-shard candidate count kc (k = HR_MAX_K with its margin) */

/* n_dev > 1: one handle over n_dev devices (dev_ids, repeats allowed), rows striped by 32-row tile.  The handle's
 * merge takes n_dev * kc candidates per query and holds 8192 at the most, so n_dev * hr_kc_for_k_dim(HR_MAX_K, dim)
 * <= 8192 is required -- up to 42 devices below 2048 dims, 32 from there on; more is HR_E_INVALID here (and in
 * hr_index_load), checked with the other arguments before any device call, not a failure of the first large-k search. */
int hr_index_create(int dim, int dtype, int metric, int n_dev, const int* dev_ids, hr_index** out);
/* hr_index_create / hr_index_load with creation flags (single-device handles only; 0 = the plain call).
 * HR_CREATE_NO_SHADOWS: the index keeps neither the 16-bit shadow of fp32 rows nor the 8-bit shadow of a cosine
 * corpus -- for an index that never runs a main scan pass, such as the list-order rows behind hr_ivf_search,
 * whose shadows would only cost memory (+50 % of a 16-bit corpus). */
enum { HR_CREATE_NO_SHADOWS = 1 };
int hr_index_create_ex(int dim, int dtype, int metric, int n_dev, const int* dev_ids, int flags, hr_index** out);
int hr_index_load_ex(const char* path, int n_dev, const int* dev_ids, int flags, hr_index** out);
int hr_index_reserve(hr_index* h, int64_t capacity_rows);
int hr_index_add(hr_index* h, const float* rows, int64_t n, int64_t* first_row_out);
int hr_index_add_synthetic(hr_index* h, uint64_t seed, int64_t global_row0, int64_t n, int64_t* first_row_out);
/* Same as hr_index_add for n fp32 rows already in device memory (e.g. the in-process embedder's
 * hr_pool_normalize output): ordered after the work queued on `stream`, no host round trip of the
 * vectors; returns once the rows are stored (rows_dev may then be reused).
 * Replaces embed_texts -> add_chunks in BaseProcessor._chunk_and_store (processors.py:413-418). */
int hr_index_add_device(hr_index* h, const float* rows_dev, int64_t n, int64_t* first_row_out, void* stream);
/* Store n fp32 device rows at explicit positions dest_dev[i] (< n_rows_after, previously unused),
 * e.g. rows placed by list for an IVF index; the index then holds n_rows_after rows, positions
 * never written stay dead.  Ordered after the work queued on `stream`; returns once stored. */
int hr_index_add_device_at(hr_index* h, const float* rows_dev, int64_t n, const int64_t* dest_dev,
                           int64_t n_rows_after, void* stream);
/* Copy the STORED bits of n rows of src (row numbers src_rows_dev[i]) to the previously unused positions
 * dst_pos_dev[i] (< n_rows_after) of dst, tile layout to tile layout (the slot swizzle is honoured on both sides);
 * the positions become live, dst takes src's max norm and then holds n_rows_after rows, as after
 * hr_index_add_device_at.  Re-adding a stored cosine row through hr_index_add_device_at would normalise it a second
 * time and could change its bits; this keeps them, so IVF lists hold exactly what the exact index holds.  Pairs
 * with an index out of range on either side are skipped.  Two different single-device handles on one device with
 * the same dim, dtype and metric, cosine or dot; anything else: HR_E_UNSUPPORTED.  Ordered after the work queued
 * on `stream`; returns once copied. */
int hr_index_copy_rows(hr_index* dst, hr_index* src, const int64_t* src_rows_dev, const int64_t* dst_pos_dev,
                       int64_t n, int64_t n_rows_after, void* stream);
/* The synthetic corpus generator (the one hr_index_add_synthetic and the oracle use) writing n fp32
 * rows of dimension dim, row-major, to device memory on `stream`. */
int hr_gen_rows_device(uint64_t seed, int64_t row0, int64_t n, int dim, float* out_dev, void* stream);
int hr_index_remove(hr_index* h, const int64_t* rows, int64_t n);
/* Host queries and outputs.  1 <= k <= HR_MAX_K: the scan path.  k > HR_MAX_K (Chroma's n_results
 * has no cap, chroma_store.py:118-120): an exhaustive exact pass per query (same scores and order,
 * one corpus pass + one n-row sort per query).  Slots past the live (allowed) rows: -inf / -1. */
int hr_index_search(hr_index* h, const float* q, int B, int k, const uint64_t* row_mask, float* scores_out,
                    int64_t* rows_out);
int hr_index_search_device(hr_index* h, const float* q_dev, int B, int k, const uint64_t* row_mask_dev,
                           float* scores_out_dev, int64_t* rows_out_dev, void* stream);
/* Mixed-filter batches: every query carries its own row mask and the batch still shares one exact scan per 64
 * queries (each agent searches its own files: kb_file_search builds a where-clause per call, kb_search_toolkit.py;
 * one hr_index_search per distinct filter is one launch, and with dense filters one corpus read, per filter).
 * masks: D row bitmaps of the same format as row_mask, mask_stride 64-bit words apart (mask_stride * 64 >= the
 * index's row count, else HR_E_INVALID); mask_of[i]: the bitmap of query i, or -1 = no mask (outside [-1, D):
 * HR_E_INVALID).  Query i gets exactly what hr_index_search(h, q_i, 1, k, masks + mask_of[i] * mask_stride, ...)
 * gives: the same rows, order (canonical fp64 score desc, row asc) and fp32 score bits, -inf / -1 past the live,
 * allowed rows.  D = 0 or every entry -1 is the unmasked search.  Any k (k > HR_MAX_K: the exhaustive pass per
 * query with that query's bitmap).  Per chunk of 64 queries (32 above 1280 dims) the scans visit the tiles SOME
 * query allows (the union of the referenced bitmaps; a dense union or a query without a mask keeps the full scan)
 * and apply a per-query predicate in the SAMPLE and the FILTER; queries whose exactness guard fails go through the
 * single-mask collect fallback, once per distinct bitmap among them.  A multi-device handle: HR_E_UNSUPPORTED (run
 * one hr_index_search per distinct mask).  The device form takes every pointer in device memory (mask_of
 * included), is ordered after the work queued on `stream` and returns with it idle. */
int hr_index_search_masks(hr_index* h, const float* q, int B, int k, const uint64_t* masks, int D, int64_t mask_stride,
                          const int32_t* mask_of, float* scores_out, int64_t* rows_out);
int hr_index_search_masks_device(hr_index* h, const float* q_dev, int B, int k, const uint64_t* masks_dev, int D,
                                 int64_t mask_stride, const int32_t* mask_of_dev, float* scores_out_dev,
                                 int64_t* rows_out_dev, void* stream);
/* Pipelined form of hr_index_search_device (no mask, k <= HR_MAX_K): enqueue a batch and return a
 * ticket; hr_index_search_finalize(ticket) waits for that batch's exactness-guard flags, runs the exact
 * fallback for queries that need it and returns once scores_out/rows_out hold the final results.  A
 * multi-device handle keeps two batches in flight, every shard submitted by a host thread of its own
 * (so host time per batch does not grow with the number of devices); submitting a third finalizes the
 * oldest.  q_dev and the outputs must stay valid until the batch is finalized; other calls on the handle
 * finalize every batch in flight first.  A single-device handle completes the batch inside submit
 * (ticket 0).  Replaces VectorRetriever.batch_retrieve's sequential search loop (base_retriever.py:82-99)
 * for a store spanning the node's GPUs (one cached store per collection, base_toolkit.py:79-91). */
int hr_index_search_submit(hr_index* h, const float* q_dev, int B, int k, float* scores_out_dev, int64_t* rows_out_dev,
                           void* stream, int64_t* ticket_out);
int hr_index_search_finalize(hr_index* h, int64_t ticket);
/* Asynchronous search of host queries on a single-device handle (the drop-in store's micro-batcher on
 * an asyncio event loop; VectorRetriever.retrieve's store.search, base_retriever.py:58-63): copies the B
 * queries to pinned staging, enqueues the whole pass (query copy, prep, SAMPLE, FILTER, select, rescore,
 * merge, results + guard flags back to pinned memory) and returns a ticket without waiting.  When the
 * batch's results are in host memory a host function writes an 8-byte 1 to notify_fd (an eventfd the
 * caller polls; -1: none).  hr_index_search_collect(ticket) then copies the scores / rows out (after
 * running the exact fallback for queries that need it, synchronously).  At most two batches are in
 * flight, collected in any order (a third submit returns HR_E_BUSY until one is collected); adds, removes
 * and reserve wait for batches in flight first and run their exact fallbacks against the rows the batches
 * were submitted against; submit never blocks on the handle: while another call holds it, it returns
 * HR_E_BUSY at once.  No row mask; 1 <= k <= HR_MAX_K; an empty index or a multi-device handle
 * returns HR_E_UNSUPPORTED (use hr_index_search). */
int hr_index_search_submit_host(hr_index* h, const float* q, int B, int k, int notify_fd, int64_t* ticket_out);
int hr_index_search_collect(hr_index* h, int64_t ticket, float* scores_out, int64_t* rows_out);
/* State of a submitted batch without waiting: *state_out = 0 still running, 1 results ready, 2 ready but some
 * queries need the exact fallback (collect then runs a corpus pass: call it off the event loop).  HR_E_BUSY
 * while another call holds the handle. */
int hr_index_search_poll(hr_index* h, int64_t ticket, int* state_out);
/* Collapsed search: the exact top-k DISTINCT groups of every query, each represented by its best row (Milvus'
 * group-by search, Elasticsearch's collapse; replaces kb_file_search's over-fetch + host de-duplication by
 * metadata.get("source", document_id), kb_search_toolkit.py:539-568, which cannot know whether another file sits
 * just below its fetch window).
 * The group column: one int32 id per row, -1 = no group.  hr_index_set_groups writes ids of rows [row0, row0 + n)
 * from host memory; ids below -1 and rows at or beyond the index's row count: HR_E_INVALID.  The column is a device
 * array owned by the handle, allocated by the first call (an index that never collapses pays nothing), grown by
 * doubling with its contents kept, new entries -1; rows added later are -1 until set.  The library keeps
 * largest id + 1 as the group count.  hr_index_save does not write the column: the caller derives it again.
 * Semantics: let A be the live rows the mask allows with id >= 0, ordered as every search orders (canonical fp64
 * score desc, row asc); walk A and keep a row only when its group has not been seen.  The first k kept rows are
 * the result, scores cast to fp32 as hr_index_search does, slots after the last kept row -inf / -1.  With every
 * row in a group of its own the result is hr_index_search's, bit for bit; with one group it is one row.
 * Two stages: the exact search for `probe` rows (0 = the default: HR_MAX_K, 32 for k = 1; else k <= probe <=
 * HR_MAX_K) collapsed on the device; a query whose probe came back full with fewer than k groups goes through an
 * all-rows pass -- canonical score of every live, allowed row, atomic max per group, the exact record selector --
 * one query at a time in a workspace of 12 bytes per index row + 32 bytes per group, with no n-row sort.
 * 1 <= k <= HR_MAX_K, any B, every dtype and metric; a multi-device handle: HR_E_UNSUPPORTED; no group column:
 * HR_E_INVALID.  The device form is ordered after the work queued on `stream` and returns with it idle. */
int hr_index_set_groups(hr_index* h, int64_t row0, int64_t n, const int32_t* groups /* host */);
int hr_index_search_collapsed(hr_index* h, const float* q, int B, int k, int probe, const uint64_t* row_mask,
                              float* scores_out, int64_t* rows_out);
int hr_index_search_collapsed_device(hr_index* h, const float* q_dev, int B, int k, int probe,
                                     const uint64_t* row_mask_dev, float* scores_out_dev, int64_t* rows_out_dev,
                                     void* stream);
/* MMR search: k rows per query chosen by maximal marginal relevance -- relevant rows that do not repeat each other
 * (LangChain's max_marginal_relevance_search) -- on the device, bit for bit restatable (tests/mmr_ref.py).
 * Pool: the exact top-P of hr_index_search(h, q, B, P, row_mask), P = fetch_k, in its order (canonical score desc,
 * row asc; live, allowed rows only; slots with row -1 are padding and never candidates).  rel[j] = the fp32 score of
 * pool position j, widened to double.
 * Similarity: sim(s, j) = the canonical fp64 score, under the index's metric, of stored row j against a QUERY whose
 * components are stored row s widened to fp32 (lane-strided fp64 accumulation over the padded dim, the butterfly
 * sum, and for l2 1 - ((|s|^2 - 2 s.j) + |j|^2)), read from the stored rows.  The selected row always takes the
 * query role: for l2 on fp32 rows sim(s, j) and sim(j, s) can differ in the last bit.
 * Greedy selection: step 0 takes position 0.  maxsim[j] = the fp64 max of sim(s, j) over the rows s selected so
 * far.  Every further step takes the unselected candidate with the largest
 *     v[j] = lambda * rel[j] - (1 - lambda) * maxsim[j]
 * -- two products and a subtraction, each rounded once, no fused multiply-add, 1 - lambda computed once; a NaN v[j]
 * counts as -inf; ties go to the lowest pool position.  It stops after min(k, candidates in the pool) picks.
 * Output: the rows in SELECTION order, each with its fp32 relevance rel (what hr_index_search returns for it, so a
 * score threshold keeps its meaning); the scores are therefore NOT monotone down the list.  Remaining slots
 * -inf / -1.  lambda = 1 is hr_index_search's top-k; for a fixed fetch_k and lambda the k'-pick answer is the
 * first k' entries of the k-pick answer.  The pool is exact and the answer a function of it: no fallback stage.
 * Limits: 1 <= k <= fetch_k <= HR_MAX_K; fetch_k = 0: the default min(HR_MAX_K, max(32, 4 k)); lambda outside
 * [0, 1] or NaN: HR_E_INVALID; a multi-device handle: HR_E_UNSUPPORTED; an empty index returns padding.  The
 * device form is ordered after the work queued on `stream` and returns with it idle. */
int hr_index_search_mmr(hr_index* h, const float* q, int B, int k, int fetch_k, double lambda,
                        const uint64_t* row_mask, float* scores_out, int64_t* rows_out);
int hr_index_search_mmr_device(hr_index* h, const float* q_dev, int B, int k, int fetch_k, double lambda,
                               const uint64_t* row_mask_dev, float* scores_out_dev, int64_t* rows_out_dev,
                               void* stream);
/* Range search: every row scoring at least a threshold, with the exact count (FAISS range_search, Milvus / Qdrant
 * score-threshold search; the reference's similarity_threshold cuts only what a guessed top_k already fetched,
 * retriever.py:273-276).
 * Hits: row r is a hit of query b iff it is live, the mask allows it and (float)s >= min_score[b], s the canonical
 * fp64 score under the index's metric (cosine / ip: inner product; l2: 1 - |q - x|^2) and the cast the one
 * hr_index_search returns -- the comparison is made on the fp32 number callers see and threshold on.  A row whose
 * score is NaN is never a hit.  min_score[b] NaN: HR_E_INVALID; -inf makes every live, allowed row a hit; +inf is
 * legal.
 * counts_out[b] is the exact number of hits, also when it exceeds max_hits.  scores_out / rows_out hold the first
 * min(count, max_hits) hits in the order every search uses (canonical fp64 score desc, row asc), scores cast to
 * fp32, remaining slots -inf / -1: without NaN scores, hr_index_search(q_b, k = live rows) cut where its fp32 score
 * drops below the threshold, bit for bit.
 * Two stages: one collect pass of the corpus against a per-query floor derived from the threshold and the exactness
 * guard's error bound, into a region of max(1024, 2 max_hits) records per query, rescored exactly, counted and
 * ordered on the device; a query whose region overflowed goes through an all-rows pass -- canonical score of every
 * live, allowed row, the hits compacted and only the hits sorted -- one query at a time in a workspace of 12 bytes
 * per index row (+ 28 per hit).
 * Limits: 0 <= max_hits <= HR_RANGE_MAX_HITS; max_hits = 0 is a count-only call (scores_out / rows_out may be
 * NULL); any B >= 1, every dtype and metric; an empty index returns counts 0 and padding; the mask follows the
 * rules of hr_index_search; a multi-device handle: HR_E_UNSUPPORTED.  The device form (every pointer in device
 * memory) is ordered after the work queued on `stream` and returns with it idle. */
#define HR_RANGE_MAX_HITS 65536
int hr_index_search_range(hr_index* h, const float* q, int B, const float* min_score /* B */, int max_hits,
                          const uint64_t* row_mask, float* scores_out /* B*max_hits */,
                          int64_t* rows_out /* B*max_hits */, int64_t* counts_out /* B */);
int hr_index_search_range_device(hr_index* h, const float* q_dev, int B, const float* min_score_dev, int max_hits,
                                 const uint64_t* row_mask_dev, float* scores_out_dev, int64_t* rows_out_dev,
                                 int64_t* counts_out_dev, void* stream);
/* Boosted search: the exact top-k of similarity blended with per-row boosts, over the whole collection
 * (Elasticsearch function_score / rank_feature, Qdrant's score-boosting formula, Vespa rank profiles, Milvus boost
 * rankers; the reference's memory search re-ranks a guessed top_k window on the host with 0.5 similarity + 0.3
 * importance + 0.2 recency, memory_toolkit.py:865-924; tests/boost_ref.py restates all of it).
 * Boost columns: up to HR_BOOST_MAX_COLS columns of one fp32 per row.  hr_index_set_boost writes values[0, n) (HOST)
 * to rows [row0, row0 + n) of column col.  values must be finite: a NaN or infinite value, col outside
 * [0, HR_BOOST_MAX_COLS) or rows at or beyond the index's row count: HR_E_INVALID, all checked on the host before any
 * device call.  A column is a device array owned by the handle: its first set allocates it (an index that never
 * boosts pays nothing), it grows by doubling and keeps its contents, new entries are 0.0f; rows added later read 0.0
 * until set, a column never set reads 0.0 everywhere; a range may be set again at any time.  hr_index_save does not
 * write the columns (the caller derives them again, as the group column); hr_index_destroy frees them.
 * Search, per query: over the live rows the mask allows, s(r) the canonical fp64 score under the index's metric (the
 * bits the range search compares), the blended value in fp64
 *     v(r) = (...((alpha * s(r)) + beta[0] * (double)b_0(r)) + beta[1] * (double)b_1(r)) ...)
 * -- every product and every addition rounded once, in column order, no fused multiply-add.  The result is the first
 * k rows by (v desc, row asc; -0.0 and 0.0 are equal and written as 0.0): blended_out holds v, scores_out (float)s(r)
 * -- the number hr_index_search returns for that row, so similarity thresholds keep their meaning -- rows_out the
 * row; slots past the live, allowed rows hold -inf / -inf / -1.  A row whose v is NaN is never returned.  On corpora
 * without NaN scores, alpha = 1 with every beta zero, every referenced column all zero, or n_cols = 0 is
 * hr_index_search in rows, order and fp32 score bits.  beta is always a HOST array.
 * Mechanism (part of the contract: the stage that answers a query follows from it).
 *   1 pilot   the exact search for P = probe rows; tau = the k-th largest true v among the pool's rows (rescored in
 *             fp64; rows with a NaN v do not count), -inf when the pool holds fewer than k of them.
 *   2 floor   bext_c = the largest value of column c over ALL rows [0, n) when beta[c] >= 0, the smallest when
 *             beta[c] < 0 (dead, masked and never-set rows included; a device reduction cached on the handle until
 *             the column is written or the index grows).  Vmax(x) = the blend with s := x and every b_c := bext_c.
 *             Rounded products and sums are monotone in each operand, so v(r) <= Vmax(s(r)) and Vmax is
 *             non-decreasing.  t0 = the smallest fp32 value with Vmax((double)t0) >= tau, by bisection over the
 *             ordered fp32 bit patterns on the device; t = nextafterf(t0, -inf).  Every row with v(r) >= tau then
 *             has (float)s(r) >= t; no slack constant.
 *   3 window  (stage 1) the range search at min_score = t with max_hits = window.  A query whose exact hit count is
 *             <= window has every candidate in hand: the window's rows are rescored (v), sorted by (v desc, row asc)
 *             in LDS and the first k written.
 *   4 all     (stage 2) a query whose count exceeds window, one at a time: the canonical score of every live,
 *             allowed row, turned into v in place, the rows with v >= tau selected, a stable descending radix sort of
 *             those rows only, the first k taken.  No n-row sort.
 * Limits, all checked on the host before any launch (and before the handle is looked at): 1 <= k <= HR_MAX_K; alpha
 * finite and in [2^-64, 2^64]; |beta[c]| <= 2^64, negative values are legal (a penalty); 0 <= n_cols <=
 * HR_BOOST_MAX_COLS; probe = 0: the default min(HR_MAX_K, max(32, 4 k)), else k <= probe <= HR_MAX_K; window = 0: the
 * default 4096, else k <= window <= HR_BOOST_MAX_WINDOW.  Any B >= 1, every dtype and metric; an empty index returns
 * padding; a multi-device handle: HR_E_UNSUPPORTED; the mask follows the rules of hr_index_search.  The device form
 * (q, mask and outputs in device memory) is ordered after the work queued on `stream` and returns with it idle. */
#define HR_BOOST_MAX_COLS 4
#define HR_BOOST_MAX_WINDOW 8192
int hr_index_set_boost(hr_index* h, int col, int64_t row0, int64_t n, const float* values /* host */);
int hr_index_search_boosted(hr_index* h, const float* q, int B, int k, double alpha,
                            const double* beta /* n_cols, host */, int n_cols, int probe, int window,
                            const uint64_t* row_mask, double* blended_out /* B*k */, float* scores_out /* B*k */,
                            int64_t* rows_out /* B*k */);
int hr_index_search_boosted_device(hr_index* h, const float* q_dev, int B, int k, double alpha,
                                   const double* beta /* n_cols, host */, int n_cols, int probe, int window,
                                   const uint64_t* row_mask_dev, double* blended_out_dev, float* scores_out_dev,
                                   int64_t* rows_out_dev, void* stream);
/* Search by example: queries built on the device from stored rows ("more like this chunk": Qdrant's recommend,
 * Weaviate's nearObject, Pinecone's query by id; tests/examples_ref.py restates it bit for bit).
 * A batch of B queries.  Query b has an optional fp32 base vector q[b] (q = NULL: none) and m_b = ex_off[b + 1] -
 * ex_off[b] examples: the stored rows ex_rows[e] with the fp32 weights ex_weights[e], e in [ex_off[b], ex_off[b + 1]);
 * a negative weight is a negative example.  ex_off holds B + 1 non-decreasing offsets; the three lists are always
 * HOST arrays (they are ids, not vectors), also in the device forms.
 * Built query, per component d < dim, in fp64: acc = (double)q[b][d], or 0.0 without q; then for e in list order
 * acc = acc + (double)w_e * (double)x_e[d], x_e[d] the stored element of row ex_rows[e] widened to fp32 (the bits
 * hr_index_get_rows returns); built[b][d] = (float)acc, round to nearest even.  The product of two fp32 values is
 * exact in fp64, so one rounding per example and one cast: a fused multiply-add gives the same bits.
 * hr_index_build_queries writes the B built queries row-major (B * dim floats); its device form reads q_dev and writes
 * q_out_dev in device memory, and its output may feed any *_device search (range, MMR, collapsed, masks).
 * hr_index_search_examples: the answer of query b is what hr_index_search(h, built[b], 1, k, row_mask) gives with the
 * rows of b's example list removed from the candidates -- the same processing of the query (cosine: normalised by
 * the canonical query prep), the same order (canonical fp64 score desc, row asc), the same fp32 score bits; slots past
 * the remaining live, allowed rows hold -inf / -1.  Positive and negative examples are both excluded; a row listed
 * twice adds its weights and is excluded once; a row the mask forbids is still a legal example.  flags = HR_EX_KEEP
 * switches the exclusion off: the answer is then hr_index_search of the built queries, bit for bit.
 * Mechanism: one search of the batch for K' = k + M rows, M = the largest m_b (0 with HR_EX_KEEP), then the examples
 * dropped from every list on the device.  The top-K' of the allowed rows minus at most m_b of them contains the
 * top-k of the remainder, so the result is exact and there is no fallback stage of its own; K' > HR_MAX_K takes the
 * exhaustive exact pass of hr_index_search.
 * Limits: 0 <= m_b <= HR_EX_MAX; m_b = 0 without q, an example row outside [0, n) or removed, a NaN or infinite
 * weight: HR_E_INVALID, all checked on the host before any kernel is launched.  A built query that comes out all
 * zero (weights that cancel) is legal: it scores 0 everywhere and the order is row ascending.  k >= 1, any B >= 1,
 * every dtype and metric; an empty index returns padding; a multi-device handle: HR_E_UNSUPPORTED.  The device
 * forms are ordered after the work queued on `stream` and return with it idle. */
#define HR_EX_MAX 32           /* examples of one query */
enum { HR_EX_KEEP = 1 };       /* hr_index_search_examples flags: the examples stay candidates */
int hr_index_build_queries(hr_index* h, const int64_t* ex_rows, const float* ex_weights, const int64_t* ex_off, int B,
                           const float* q /* B*dim or NULL */, float* q_out /* B*dim */);
int hr_index_build_queries_device(hr_index* h, const int64_t* ex_rows, const float* ex_weights, const int64_t* ex_off,
                                  int B, const float* q_dev, float* q_out_dev, void* stream);
int hr_index_search_examples(hr_index* h, const float* q, const int64_t* ex_rows, const float* ex_weights,
                             const int64_t* ex_off, int B, int k, int flags, const uint64_t* row_mask,
                             float* scores_out, int64_t* rows_out);
int hr_index_search_examples_device(hr_index* h, const float* q_dev, const int64_t* ex_rows, const float* ex_weights,
                                    const int64_t* ex_off, int B, int k, int flags, const uint64_t* row_mask_dev,
                                    float* scores_out_dev, int64_t* rows_out_dev, void* stream);
/* Fused multi-query search: several ranked lists per question -- rewritten queries, HyDE, sub-questions, widened
 * filter scopes -- fused on the device by reciprocal rank or by the largest score (Elasticsearch's rrf retriever,
 * Qdrant's query with fusion: rrf, LangChain's MultiQueryRetriever / EnsembleRetriever; the reference's agent merges
 * its searches by max score on the host, meta_retrieval_toolkit.py:619-627; tests/fused_ref.py restates all of it).
 * hr_fuse_lists -- the fusion alone, on lists that already lie in device memory.
 * Input: Q = grp_off[G] ranked lists of P slots each, in the format every search writes: slot p of list i holds
 * rows[i * P + p] and scores[i * P + p]; a row of -1 (any negative row) is padding and never an entry; the rows of one
 * list are distinct.  Group g owns the lists [grp_off[g], grp_off[g + 1]): its members, m_g of them.  grp_off (G + 1
 * offsets, grp_off[0] = 0) and weights (Q values, or NULL) are always HOST arrays, like ex_off above.
 * Semantics, per group, over the distinct rows r that appear in any of its members:
 *   HR_FUSE_RRF  fused(r) starts at 0.0 in fp64; then, for the members i in member order that hold r, at 1-based
 *                position p_i: fused = fused + (double)w_i / (rrf_k + (double)p_i), w_i = weights[i], 1.0f when
 *                weights is NULL.  One division and one addition per term, each rounded once, no reassociation (a
 *                fused multiply-add cannot arise).  With two members and NULL weights this is the retriever's
 *                rrf_fuse bit for bit, order included.
 *   HR_FUSE_MAX  fused(r) is the largest fp32 score among the members holding r, widened to double; a NaN score
 *                counts as -inf; weights must be NULL (else HR_E_INVALID).
 *   order        fused descending, then row ascending (-0.0 and 0.0 are equal): the project's order everywhere.  The
 *                first min(k, distinct rows) are written; the remaining slots hold -inf / -1 / 0.
 *   members_out  (may be NULL) bit j is set iff member grp_off[g] + j holds the row: which rewrite found the chunk.
 * Limits: 1 <= m_g <= HR_FUSE_MAX_MEMBERS (an empty group: HR_E_INVALID); 1 <= k <= P <= HR_MAX_K; G >= 1; rrf_k
 * finite and >= 0; weights finite (zero and negative ones are legal); mode one of the two values -- all checked on
 * the host before any launch.  One workgroup per group sorts the group's <= 2048 entries in LDS; no floating-point
 * atomics, nothing that depends on scheduling.  Ordered after the work queued on `stream` of `device`; returns with
 * it idle.
 * hr_index_search_fused -- the members searched and fused in one call.  q: Q query vectors; member i's pool is exactly
 * what hr_index_search_masks(h, q_i, 1, fetch_k, masks, D, mask_stride, mask_of + i, ...) returns for it (D = 0:
 * hr_index_search, and mask_of may be NULL): the same rows, order and fp32 score bits.  All Q members go through the
 * scan as one batch (the single-mask search when every member names the same bitmap: identical by contract), the
 * pools are fused by hr_fuse_lists with P = fetch_k and never leave the device.
 * fetch_k = 0 is the default: min(HR_MAX_K, max(4 k, 50)) for RRF (the HybridRetriever's depth), k for MAX; else
 * k <= fetch_k <= HR_MAX_K; 1 <= k <= HR_MAX_K.
 * RRF is a function of the rank window (Elasticsearch's rank_window_size): a deeper fetch_k can change the answer.
 * MAX with fetch_k >= k returns the corpus-wide k largest values of max_i score_i(r): a row outside every pool scores
 * no more than each pool's last entry; only the choice among rows with EQUAL fp32 fused score at the cut is
 * pool-defined.  With one member, RRF (any positive weight) returns that member's top-k rows in order.  The pools are
 * exact and the answer a function of them: no fallback stage of its own.
 * An empty index returns padding; a multi-device handle: HR_E_UNSUPPORTED; the mask rules are those of
 * hr_index_search_masks.  The device form takes every vector, mask (mask_of included) and output pointer in device
 * memory, is ordered after the work queued on `stream` and returns with it idle. */
#define HR_FUSE_MAX_MEMBERS 16 /* lists of one group */
enum { HR_FUSE_RRF = 0, HR_FUSE_MAX = 1 };
int hr_fuse_lists(int device, const int64_t* rows_dev /* Q*P */, const float* scores_dev /* Q*P */, int P,
                  const int64_t* grp_off /* G+1, HOST */, const float* weights /* Q or NULL, HOST */, int G, int k,
                  int mode, double rrf_k, double* fused_out_dev /* G*k */, int64_t* rows_out_dev /* G*k */,
                  uint32_t* members_out_dev /* G*k, nullable */, void* stream);
int hr_index_search_fused(hr_index* h, const float* q /* Q*dim */, const int64_t* grp_off, const float* weights, int G,
                          int k, int fetch_k, int mode, double rrf_k, const uint64_t* masks, int D,
                          int64_t mask_stride, const int32_t* mask_of /* Q */, double* fused_out, int64_t* rows_out,
                          uint32_t* members_out);
int hr_index_search_fused_device(hr_index* h, const float* q_dev, const int64_t* grp_off, const float* weights, int G,
                                 int k, int fetch_k, int mode, double rrf_k, const uint64_t* masks_dev, int D,
                                 int64_t mask_stride, const int32_t* mask_of_dev, double* fused_out_dev,
                                 int64_t* rows_out_dev, uint32_t* members_out_dev, void* stream);
int hr_index_size(hr_index* h, int64_t* n_out, int64_t* n_live_out);
/* Shape of a handle (e.g. one returned by hr_index_load): dim, storage dtype, metric, devices. */
int hr_index_info(hr_index* h, int* dim_out, int* dtype_out, int* metric_out, int* n_dev_out);
int hr_index_get_rows(hr_index* h, const int64_t* rows, int64_t n, float* out);
int hr_index_save(hr_index* h, const char* path);
int hr_index_load(const char* path, int n_dev, const int* dev_ids, hr_index** out);
void hr_index_destroy(hr_index* h);

/* Row-sharded search pieces (one process per GPU; RCCL moves the candidates).
 * Candidate record = {double exact_score; int64 global_row} (16 bytes).
 * kc = candidates per query kept by a shard (k <= kc <= HR_MAX_KC); the scan keeps
 * ceil(kc/32) row parts of group maxima.  hr_kc_for_k gives the kc the single-GPU search
 * uses below 2048 dims: k + max(16, k/2) rounded up to a multiple of 32, at most HR_MAX_KC (margin
 * for the guard; 32 for k <= 16).  hr_kc_for_k_dim(k, dim) is the kc for a given dim (the margin
 * grows to max(20, k) from 2048 dims on); hr_kc_for_k(k) = hr_kc_for_k_dim(k, 0). */
int hr_kc_for_k(int k);
int hr_kc_for_k_dim(int k, int dim);
int hr_index_search_shard(hr_index* h, const float* q_dev, int B, int k, int kc, const uint64_t* row_mask_dev,
                          int64_t row_offset, void* cand_out_dev /* B*kc records */,
                          double* bound_out_dev /* B */, void* stream);
/* Pipelined form of hr_index_search_shard: the scan (query prep, SAMPLE, FILTER) runs on
 * scan_stream over all but a few CUs, select + exact rescoring on tail_stream, which waits for
 * the scan by event; the outputs are ready in tail_stream order.  Consecutive calls alternate
 * between two workspaces, so batch i's tail (and whatever the caller queues after it on
 * tail_stream: the all-gather, the merge) overlaps batch i+1's scan.  Everything the caller
 * enqueued on scan_stream before the call is ordered before the tail-stream work (the tail waits
 * for this batch's scan), so outputs written on scan_stream earlier need no extra sync.  Same
 * results as hr_index_search_shard. */
int hr_index_search_shard_async(hr_index* h, const float* q_dev, int B, int k, int kc, const uint64_t* row_mask_dev,
                                int64_t row_offset, void* cand_out_dev, double* bound_out_dev, void* scan_stream,
                                void* tail_stream);
/* Same, with the event (hipEvent_t, nullable) after which the caller's queries q_dev are ready.
 * With it, a large shard's query prep and SAMPLE pass run early, on the index's own stream over
 * the CUs the previous batch's FILTER scan leaves free, instead of between the two FILTER scans
 * on scan_stream (results identical; only the order of work changes).  Without it: as above. */
int hr_index_search_shard_async_ev(hr_index* h, const float* q_dev, int B, int k, int kc,
                                   const uint64_t* row_mask_dev, int64_t row_offset, void* cand_out_dev,
                                   double* bound_out_dev, void* scan_stream, void* tail_stream,
                                   void* q_ready_event);
int hr_index_search_shard_collect(hr_index* h, const float* q_dev, int B, const double* kth_dev /* B */,
                                  int cap, const uint64_t* row_mask_dev, int64_t row_offset,
                                  void* cand_out_dev /* B*cap records */, double* bound_out_dev, void* stream);
int hr_merge_candidates(int device, const void* cand_dev /* G*B*kc records */, const double* bounds_dev /* G*B */,
                        int G, int B, int kc, int k, float* scores_out_dev, int64_t* rows_out_dev,
                        double* kth_out_dev, int32_t* fail_out_dev, void* stream);
/* The same with explicit per-rank strides (bytes) between the ranks' candidate blocks and bound
 * blocks, so one all-gather can move each rank's packed record [B*kc candidates][B bounds]
 * (cand_rank_stride = bound_rank_stride = B*kc*16 + B*8). */
int hr_merge_candidates_strided(int device, const void* cand_dev, const double* bounds_dev, int64_t cand_rank_stride,
                                int64_t bound_rank_stride, int G, int B, int kc, int k, float* scores_out_dev,
                                int64_t* rows_out_dev, double* kth_out_dev, int32_t* fail_out_dev, void* stream);

/* Exact top-m of every query over the whole shard (the exhaustive pass: canonical fp64 score of every live, allowed
 * row + a stable sort), as B*m candidate records {score, local row + row_offset} on the device in (score desc, row
 * asc) order, (-inf, -1) padding past the shard's rows.  The row-sharded search's path for k above the scan's kc and
 * for collect windows larger than their buffer -- the single index's hr_index_search k > HR_MAX_K pass, per shard
 * (Chroma's n_results has no cap, chroma_store.py:118-120; FAISS returns the exact top-k on ties,
 * faiss_store.py:148-176).  One corpus pass and one n-row sort per query; synchronises `stream`. */
int hr_index_search_shard_exact(hr_index* h, const float* q_dev, int B, int m, const uint64_t* row_mask_dev,
                                int64_t row_offset, void* cand_out_dev, void* stream);
/* Merge of G ranks' sorted exact lists (hr_index_search_shard_exact records, m per query; rank g's block at
 * cand_dev + g * cand_rank_stride bytes, 0 = dense B*m*16) into the top-k (score desc, row asc; -inf / -1 padding).
 * Any G * m (hr_merge_candidates is bounded by its LDS to G * kc <= 8192); ranks' rows must be disjoint. */
int hr_merge_sorted(int device, const void* cand_dev, int64_t cand_rank_stride, int G, int B, int m, int k,
                    float* scores_out_dev, int64_t* rows_out_dev, void* stream);

/* IVF-flat lists search (BASELINE config 5 candidate generation): h holds
 * the rows in list order (list l = tiles [list_tiles_dev[l], list_tiles_dev[l+1]) of 32 rows, pad
 * rows dead), ids_dev the original id of every position (-1 for pads), centroids_dev the nlist
 * processed fp32 centroids (row stride = dim rounded up to 64, zero padded).  Per query: exact top-
 * nprobe lists by canonical fp64 score (ties: lower list first), then the exact top-k of the rows of
 * those lists by canonical score (ties: lower id first), as B*k candidate records (global ids,
 * (-inf, -1) padding) and bound = -inf (nothing unreturned can matter: the same merge as the exact
 * search combines shards).  max_list_tiles: tiles of the largest list (sizes the unit buffer).
 * probes_out_dev (nullable): the B*nprobe probed lists as records {score, list}.  Cosine / dot. */
int hr_ivf_search(hr_index* h, const float* centroids_dev, int nlist, const int64_t* list_tiles_dev,
                  int64_t max_list_tiles, const int64_t* ids_dev, const float* q_dev, int B, int nprobe, int k,
                  const uint64_t* row_mask_dev, void* cand_out_dev, double* bound_out_dev, void* probes_out_dev,
                  void* stream);
/* hr_ivf_search over growable lists: list l is the sequence of extents ext_dev[e] = {first tile, tile count}
 * (int64 pairs), e in [ext_off_dev[l], ext_off_dev[l+1]), list_ntiles_dev[l] tiles in all; max_list_tiles is the
 * largest of those totals.  A list without extents and an extent without tiles are legal.  Same stages and the
 * same results as hr_ivf_search (only the unit list is built from the extent table); the order of a list's
 * extents cannot change them, the final selection orders by (score desc, id asc).  The caller keeps the three
 * tables consistent and every extent inside the index; a tile beyond the index's rows is never read. */
int hr_ivf_search_ext(hr_index* h, const float* centroids_dev, int nlist, const int64_t* ext_off_dev,
                      const int64_t* ext_dev, const int64_t* list_ntiles_dev, int64_t max_list_tiles,
                      const int64_t* ids_dev, const float* q_dev, int B, int nprobe, int k,
                      const uint64_t* row_mask_dev, void* cand_out_dev, double* bound_out_dev, void* probes_out_dev,
                      void* stream);
/* The position-order row mask hr_ivf_search takes (one uint32 word per 32-row tile), from a bitmap by id
 * (row_mask_dev: uint64 words, n_mask_rows bits): bit p % 32 of out_dev[p / 32] is set iff 0 <= ids_dev[p] <
 * n_mask_rows and the bitmap has bit ids_dev[p].  Writes ceil(n_positions / 32) words; any n_positions. */
int hr_ivf_position_mask(const int64_t* ids_dev, int64_t n_positions, const uint64_t* row_mask_dev,
                         int64_t n_mask_rows, uint32_t* out_dev, void* stream);

/* Exact top-m of B segments of {double score; int64 id} records, order (score desc, id asc), records
 * with id < 0 absent; segment b = [seg_off_records_dev[b], seg_off_records_dev[b+1]) if given, else
 * [b*seg_stride, (b+1)*seg_stride).  Out: B*m records, (-inf, -1) padding; m <= 1024.  The
 * reranker's per-query selection (replaces the reranking service's sort + top_n, openai_reranker.py
 * :92-110 / the /rerank response order). */
int hr_topk_records(const void* in_dev, const int64_t* seg_off_records_dev, int64_t seg_stride, int B, int m,
                    void* out_dev, void* stream);

/* K7: masked mean-pool of the first-dim hidden states with the first n_instr
 * tokens of every sequence masked out, then L2-normalise (fp32 out, B×H). */
int hr_pool_normalize(const void* hidden_dev, int dtype, const int32_t* mask_dev, int B, int T, int H, int n_instr,
                      float* out_dev, void* stream);
/* K7 over packed (unpadded) hidden states: sequence b is rows [cu[b], cu[b+1]) of an N x H matrix (real
 * tokens only, cu: B+1 int32 offsets on the device); same mask rule (first n_instr tokens out), same
 * sums as hr_pool_normalize on the right-padded batch.  The in-process embedder's unpadded forward. */
int hr_pool_normalize_packed(const void* hidden_dev, int dtype, const int32_t* cu_dev, int B, int H, int n_instr,
                             float* out_dev, void* stream);
/* Host (no GPU): the offline tokenizer's word split + crc32 word hash over n_texts ASCII texts (bytes
 * [offsets[i], offsets[i+1]) of `text`): lower-cased \w+ | [^\w\s] tokens -> first_id + crc32 % span,
 * at most `cap` per text (cap < 0: all), wrapped in cls_id ... sep_id when both are >= 0.  ids_out
 * (capacity ids_cap) receives the texts' ids back to back, lengths_out[i] each text's count.
 * HR_E_INVALID for a non-ASCII byte or a full ids_out.  (hiprag.rag.rocm_embedder.HashWordTokenizer) */
int hr_hash_words(const char* text, const int64_t* offsets, int64_t n_texts, int64_t first_id, int64_t span, int64_t cap,
                  int64_t cls_id, int64_t sep_id, int64_t* ids_out, int64_t ids_cap, int64_t* lengths_out);
/* K8: out = LayerNorm(x + r) * gamma + beta over rows x H (H <= 4096), dtype of x, r, gamma, beta and
 * out (HR_F32 / HR_BF16 / HR_F16); the encoder layers' residual add + LayerNorm fused
 * (BertSelfOutput / BertOutput, modeling_bert.py; XLM-R the same).  Ordered on `stream`. */
int hr_add_layernorm(const void* x_dev, const void* r_dev, const void* gamma_dev, const void* beta_dev, void* out_dev,
                     int64_t rows, int H, float eps, int dtype, void* stream);

/* The query embedder's short-sequence attention (hr_attn.hip): for each sequence b (tokens [cu[b], cu[b+1]) of the
 * packed batch, cu: B+1 int32 on the device) and head h, softmax(scale * Q K^T) V over the sequence's own tokens, from
 * the fused QKV projection qkv_dev [N][3][nH][d] (row stride 3 nH d) into out_dev [N][nH][d]: Q K^T and P V on MFMA
 * with fp32 accumulation, the softmax in fp32, P rounded to the input type for the P V product (as the flash
 * kernel), the output rounded once.  BertSelfAttention (modeling_bert.py) on the real tokens, as
 * scaled_dot_product_attention per sequence.  HR_E_UNSUPPORTED outside its scope (d != 64, max_len > 64, fp32,
 * rows not 16-byte aligned): the caller's flash varlen kernel serves those.
 * PRECONDITION: max_len >= cu[b+1] - cu[b] for every b, and cu is non-decreasing.  max_len is the only thing that
 * decides whether the kernel applies; the kernel reads the lengths on the device and never compares them with it, so
 * with an understated max_len the rows of a sequence longer than 64 tokens are undefined (its first 64 rows are
 * computed from tiles indexed past their 64 keys, the rest are never written) and no error is reported.  Empty
 * sequences (cu[b+1] == cu[b]) are allowed and write nothing; only the N = cu[B] rows of out_dev are written. */
int hr_attn_varlen(const void* qkv_dev, int dtype, const int32_t* cu_dev, int B, int nH, int d, int max_len,
                   float scale, void* out_dev, void* stream);
/* In place: x = 0.5 x (1 + erf(x / sqrt 2)) (BertIntermediate's "gelu", torch.nn.functional.gelu with
 * approximate='none'; fp32 per element, rounded once), n elements of bf16 / f16. */
int hr_gelu_erf(void* x_dev, int dtype, int64_t n, void* stream);

/* The persistent FILTER (pipelined shard batches of <= 64 queries, k <= 16, no mask, early SAMPLE: the per-GPU
 * step of a row-sharded node).  One long-lived launch streams the corpus batch after batch -- no per-batch launch
 * ramp and tail; replaces the per-batch FILTER launch behind hr_index_search_shard_async_ev (same results).
 * set_persist: 0 off, 1 shards of 4.2M-5.1M rows (default: where it measured faster than per-batch launches),
 * 2 every shard size.  persist_close: no further batch
 * for now (the running instance exits once through its batches instead of after its 300 us idle timeout).  (Its
 * counters and stamps: hr_index_persist_stats / _trace, include/hiprag_diag.h.) */
int hr_index_set_persist(hr_index* h, int mode);
int hr_index_persist_close(hr_index* h);
/* The 8-bit shadow of a cosine corpus (any stored dtype): an int8 copy of the rows with one fp32 scale per row, kept
 * beside them (+50 % of a 16-bit corpus' memory; built lazily after row writes, never written to files;
 * HIPRAG_SHADOW8=0 at create, or a failed allocation, keeps none; HIPRAG_SHADOW8_SIM_OOM=1 makes that allocation
 * fail whenever the rows grow -- for tests of the fallback).  The SAMPLE and the 64-query FILTER of a main pass
 * stream it instead of the 16-bit rows; candidates are rescored from the stored rows and the exactness guard carries
 * the shadow's measured error, so results are unchanged.  set_shadow8: 0 off, 1 (default) shards beyond 5.1M rows --
 * where it measured faster, 2 wherever the path is built (one query group, k up to 32, a single-device index). */
int hr_index_set_shadow8(hr_index* h, int mode);
/* CU partitioning (no reference counterpart: the reference's embedder and store are separate services, here the
 * query embedder's forward and the scan share one GPU -- base_retriever.py:57-63 embed_query -> search).
 * set_cu_mask: this index's internal streams run on the CUs of `mask` only (bit i of word j = CU 32 j + i;
 * n_words = 0: all CUs) and its launch grids are sized for that many CUs; blocks while asynchronous batches are
 * in flight (HR_E_BUSY).  stream_create_cu_mask: a stream restricted the same way (the caller's scan / tail /
 * embedder streams), released with hr_stream_destroy. */
int hr_index_set_cu_mask(hr_index* h, const uint32_t* mask, int n_words);
int hr_stream_create_cu_mask(int device, const uint32_t* mask, int n_words, void** stream_out);
/* Waits for the work queued on the stream, then destroys it.  Nothing may use the stream afterwards -- including a
 * framework that remembers it: PyTorch's pinned-host allocator records every stream a non_blocking copy to or from a
 * pinned tensor ran on, and touches those streams again when that tensor is freed, so such tensors must be freed
 * before the stream is destroyed (hiprag's own code copies through hr_memcpy_async instead). */
int hr_stream_destroy(void* stream);
/* Asynchronous copy of `bytes` bytes on `stream` (direction from the pointers: unified addressing). */
int hr_memcpy_async(void* dst, const void* src, int64_t bytes, void* stream);
int hr_device_count(int* n_out);
/* Cumulative counters since creation (the store's metrics) -- out[0] main scan passes, out[1] queries that
 * failed the exactness guard (collect fallback), out[2] queries answered by the exhaustive pass. */
int hr_index_stats(hr_index* h, int64_t out[3]);
/* The 256-query FILTER (hr_q256.hip: 129-256-query batches, bf16 / f16 / fp32 rows, D = 256..1024, k <= 16, no
 * tile list -- one corpus pass for four 64-query groups, VectorRetriever.batch_retrieve / the store's micro-batches of
 * up to 256 single-query calls, base_retriever.py:96-98, chroma_store.py:118-120).  set_q256(h, 0) sends those
 * batches to two 128-query FILTER launches instead (A/B; hr_index_q256_launches in include/hiprag_diag.h counts
 * its launches). */
int hr_index_set_q256(hr_index* h, int on);

/* Keyword (BM25) search: the lexical index behind HybridRetriever (the reference's HybridRetriever only delegates
 * to the vector retriever and names the debt, base_retriever.py:123-139: "a full hybrid retrieval would include
 * keyword-based search (e.g., BM25) and combine scores").  A forward index -- per row its distinct 22-bit term ids
 * ascending, packed `term << 10 | tf` (tf = min(count, 1023)), and dl = min(token count, 65535) -- in CSR arrays on
 * ONE device, scanned once per query batch.  Scores are the BM25 sum in 64-bit fixed point (2^-32 units, every
 * term contribution computed in fp64 without contraction and rounded half-to-even), so they do not depend on the
 * summation order and equal a CPU restatement bit for bit (DESIGN.md "Keyword search").  Statistics (N, df, avgdl)
 * are over live rows; a row mask does not change them.  Row numbers are append positions, as hr_index's. */
typedef struct hr_lex hr_lex;
#define HR_LEX_TERM_BITS 22    /* term id = crc32(token) % 2^22 */
#define HR_LEX_MAX_QTERMS 64   /* distinct terms of one query (the smallest ids are kept) */
#define HR_LEX_MAX_K 1024      /* largest top-k (hr_topk_records' limit) */
/* Host only (no GPU): pack the raw token ids (each < 2^22) of n texts -- text i = tokens[offsets[i] ..
 * offsets[i+1]) -- into entries_out (capacity entries_cap; the token count always suffices), row_off_out[n + 1]
 * (CSR offsets from 0) and dl_out[n]. */
int hr_lex_pack(const uint32_t* tokens, const int64_t* offsets, int64_t n, uint32_t* entries_out, int64_t entries_cap,
                int64_t* row_off_out, uint16_t* dl_out);
int hr_lex_create(int device, hr_lex** out);
void hr_lex_destroy(hr_lex* h);
/* Append n rows (hr_lex_pack of the tokens); the device arrays grow by doubling. */
int hr_lex_add(hr_lex* h, const uint32_t* tokens, const int64_t* offsets, int64_t n, int64_t* first_row_out);
/* Tombstone rows and take them out of N, df and sum_dl; removing a dead row is a no-op. */
int hr_lex_remove(hr_lex* h, const int64_t* rows, int64_t n);
int hr_lex_size(hr_lex* h, int64_t* n_out, int64_t* n_live_out);
/* The global statistics: N (live rows) and the sum of dl over them; df of n_terms given term ids. */
int hr_lex_stats(hr_lex* h, int64_t* n_live_out, int64_t* sum_dl_out);
int hr_lex_df(hr_lex* h, const uint32_t* terms, int64_t n_terms, int32_t* df_out);
/* Top-k of B queries -- query i = term ids q_terms[q_off[i] .. q_off[i+1]) (de-duplicated, capped at
 * HR_LEX_MAX_QTERMS, terms no live row holds ignored) -- among the live rows the mask allows (row_mask: host
 * bitmap as hr_index_search's, nullable) that hold at least one of its terms.  1 <= k <= HR_LEX_MAX_K, any B.
 * Out: B*k fp64 scores and rows, (score desc, row asc), -inf / -1 past the hits. */
int hr_lex_search(hr_lex* h, const uint32_t* q_terms, const int64_t* q_off, int B, int k, double k1, double b,
                  const uint64_t* row_mask, double* scores_out, int64_t* rows_out);

const char* hr_last_error(void);
int hr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HIPRAG_H */
