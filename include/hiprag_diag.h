/*
 * hiprag_diag.h -- diagnostic and measurement entry points of libhiprag.so (tests, tools/ and bench.py use them to
 * check which kernel served a batch and to time its passes).  They have no counterpart in the reference and are not
 * part of the drop-in boundary (include/hiprag.h); same conventions: 0 or a negative HR_E_* code.
 */
#ifndef HIPRAG_DIAG_H
#define HIPRAG_DIAG_H

#include "hiprag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics: tiles each wave of the most recent k_scan FILTER launch scanned ([query group][wave], blocking;
 * up to cap counts, the number in n_out).  Every unit is scanned exactly once per group, so the counts sum to
 * groups x units -- the invariant of the round-robin dealing, its rotation and the dynamic tail. */
int hr_index_wave_tiles(hr_index* h, uint32_t* out, int cap, int* n_out);

/* The persistent FILTER (hr_index_set_persist): out[0] = batches served, out[1] = error word (a bounded wait gave up;
 * 0 = none), out[2] = instances that ran.  persist_trace: per epoch of the last n (oldest first), 5 device stamps in
 * us relative to the first one's post -- post, first / last workgroup start, first / last workgroup arrival
 * (blocking). */
int hr_index_persist_stats(hr_index* h, int64_t out[3]);
int hr_index_persist_trace(hr_index* h, int n, double* out, int* n_out);

/* Scan timing is off by default (each recorded event leaves a ~6 us bubble on the stream);
 * set_scan_timing(h, N) records HIP events around every N-th main pass (0 = off). */
int hr_index_set_scan_timing(hr_index* h, int every);
/* Timing of the main-pass scans (ms, HIP events recorded on the search stream).
 * take_scan_times harvests, in launch order, every (SAMPLE, FILTER) pair launched since the
 * previous harvest (blocking on the pending events; up to cap entries; count in n_out);
 * last_scan_ms harvests everything and reports the most recent pair.  A batch of the persistent FILTER reports
 * as its FILTER time the period between its last workgroup arrival and the previous batch's (device clock). */
int hr_index_take_scan_times(hr_index* h, float* sample_ms, float* filter_ms, int cap, int* n_out);
int hr_index_last_scan_ms(hr_index* h, float* sample_ms, float* filter_ms);

/* Diagnostics: approximate MFMA scores of every row (B <= 64; approx_out B×n) and the
 * per-query error bound E_q that the exactness guard uses (e_out, B). */
int hr_index_debug_approx(hr_index* h, const float* q, int B, float* approx_out, double* e_out);
/* The same for the shadow-8 scan (hr_index_set_shadow8): its approximate scores (f16 queries, int8 rows, row scale)
 * and its E_q, which carries u_x8.  HR_E_UNSUPPORTED when the index keeps no 8-bit shadow. */
int hr_index_debug_approx8(hr_index* h, const float* q, int B, float* approx_out, double* e_out);
/* Diagnostics of the shadow-8 scan: out[0] = shadow-8 FILTER launches issued so far (graph replays not counted),
 * out[1] = candidate depth kc8 the most recent one planned (selected and rescored per query before the trim to the
 * caller's kc), out[2] = 1 if the index keeps an 8-bit shadow; *u_x8 (nullable) = the guard's storage term, the
 * largest |x - scale * int8| over the stored rows relative to the largest row norm. */
int hr_index_shadow8_stats(hr_index* h, int64_t out[3], double* u_x8);
/* Diagnostics: candidates appended by the most recent FILTER scan (sum, max per query). */
int hr_index_last_candidates(hr_index* h, int64_t* total, int64_t* max_per_query);

/* Diagnostics: hr_index_search calls answered by replaying a captured HIP graph (an unmasked,
 * untimed search with k <= HR_MAX_K, from the second call of a (B, k) shape on; HIPRAG_SYNC_GRAPH=0
 * turns the graphs off).  The results are those of the normal path: the graph is that path, captured. */
int hr_index_graph_replays(hr_index* h, int64_t* out);
/* Diagnostics: 128-query FILTER launches issued so far (65..256-query chunks at D = 256..1024; graph replays
 * not counted) -- tests use it to check which FILTER served a batch. */
int hr_index_wide_launches(hr_index* h, int64_t* out);
/* Diagnostics: 256-query FILTER launches issued so far (graph replays not counted). */
int hr_index_q256_launches(hr_index* h, int64_t* out);
/* Diagnostics: FILTER launches that ran with per-query row masks (hr_index_search_masks: one per chunk of up to 64
 * queries that took the main pass; the single-mask fallbacks of queries whose guard failed are not counted). */
int hr_index_qmask_launches(hr_index* h, int64_t* out);
/* set_qmask_timing(h, 1) records HIP events around the mask prep of every chunk of hr_index_search_masks (and waits
 * for them: measurement only); qmask_last_ms then reports, summed over the most recent call's chunks, out[0] = the
 * union of the bitmaps + the tile-list build (its count read back included), out[1] = the allow-table build (ms). */
int hr_index_set_qmask_timing(hr_index* h, int on);
int hr_index_qmask_last_ms(hr_index* h, double out[2]);

/* Diagnostics of the collapsed search (hr_index_search_collapsed): cumulative queries answered from the probe
 * (out[0]) and by the all-rows pass (out[1]).  set_collapse_timing(h, 1) records HIP events around the stages of
 * every collapsed call; collapse_last_ms then reports the most recent call's probe search, prefix kernel and
 * all-rows stage (ms; the last one covers all its incomplete queries, host waits between them included). */
int hr_index_collapse_stats(hr_index* h, int64_t out[2]);
int hr_index_set_collapse_timing(hr_index* h, int on);
int hr_index_collapse_last_ms(hr_index* h, double out[3]);

/* Diagnostics of the MMR search (hr_index_search_mmr): set_mmr_timing(h, 1) records HIP events around the two stages
 * of every MMR call; mmr_last_ms then reports the most recent call's probe search (out[0]) and selection kernel
 * (out[1]), in ms.  Off by default. */
int hr_index_set_mmr_timing(hr_index* h, int on);
int hr_index_mmr_last_ms(hr_index* h, double out[2]);

/* Diagnostics of the range search (hr_index_search_range), cumulative: queries answered by stage 1, the window scan
 * (out[0]), queries answered by stage 2, the all-rows pass (out[1]), and window-scan launches (out[2]).  A range
 * call moves none of hr_index_stats' counters: those count the top-k search's guard failures and exhaustive passes. */
int hr_index_range_stats(hr_index* h, int64_t out[3]);
/* Tiles each wave of the most recent window scan (the last chunk's collect pass) scanned, as hr_index_wave_tiles
 * reports a FILTER's ([query group][wave], blocking; up to cap counts, the number in n_out). */
int hr_index_range_wave_tiles(hr_index* h, uint32_t* out, int cap, int* n_out);

/* Diagnostics of the boosted search (hr_index_search_boosted), cumulative: queries answered by stage 1, the window
 * (out[0]), and by stage 2, the all-rows pass (out[1]); the queries of a call on an empty index count under out[0].
 * The window is a range search: a boosted call also moves hr_index_range_stats' counters. */
int hr_index_boost_stats(hr_index* h, int64_t out[2]);

/* Diagnostics of the pipelined search: out[0] = caller host time per submit (us), out[1] = host time
 * per batch of the busiest shard thread (us), out[2] = batches submitted. */
int hr_index_host_us(hr_index* h, double* out);

/* Diagnostics: device time of the most recent hr_lex_search by HIP events, summed over its sub-batches --
 * out[0] = the forward-index scan (k_lex_score and the segment padding), out[1] = the top-k selection (ms),
 * out[2] = sub-batches.  Zeros when the call launched nothing (no query had a known term). */
int hr_lex_last_ms(hr_lex* h, double* out);

#ifdef __cplusplus
}
#endif
#endif /* HIPRAG_DIAG_H */
