// hr_internal.hpp -- host-side internals shared by the libhiprag.so translation units
// (hr_index.hip: index handles and the exact search; hr_ivf.hip: the IVF lists search; the derived searches
// hr_collapse / hr_mmr / hr_range / hr_examples / hr_fuse / hr_boost .hip).  Shared here: the error macro, DevBuf and up256,
// the index handle with its ONE host-form staging area (HostStage) and inner-search pool (pool_s / pool_r), the
// staging helpers every host form is written in (stage_queries, stage_mask, stage_masks, stage_out /
// stage_download), TileListScope, and the fp32 / int64 padding launcher (pad_results, hr_exhaustive.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <atomic>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hiprag.h"
#include "../../include/hiprag_diag.h"
#include "hr_common.hpp"

using namespace hr;

// ---------------------------------------------------------------- errors
int set_err(int code, const std::string& msg);  // thread-local message for hr_last_error (hr_index.hip)
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(HR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ---------------------------------------------------------------- device buffers
// bumped whenever a work buffer is (re)allocated or freed: a captured HIP graph holds raw buffer
// addresses, so a graph captured before the bump is stale (see SyncGraph)
inline std::atomic<uint64_t> g_buf_gen{0};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        g_buf_gen.fetch_add(1);
        hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            g_buf_gen.fetch_add(1);
        }
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const {
        return (T*)p;
    }
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Staging of the host forms (host queries / masks in, host results out): ONE set per handle.  Every host form runs
// under h->mu and none calls another, so no two are live at once.  Nothing an *_impl ensures lives here: a pointer
// taken from these buffers stays valid for the whole call.
struct HostStage {
    DevBuf q,   // the queries (hr_index_search's graph path captures its address: see SyncGraph)
        aux,    // a second per-query input (range search: the thresholds)
        mask,   // one row mask, or D bitmaps words64 apart
        of,     // mask_of of the D bitmaps
        out;    // one result block of 256-byte aligned segments (stage_out); hr_index.hip's row staging
};

namespace hr {  // hr_exhaustive.hip
// n slots of -inf / -1 (k_pad_results), at most 2^30 per launch
int pad_results(float* s_out, int64_t* r_out, int64_t n, hipStream_t st);
// the exhaustive pass's first half on its own (k_exact_all): keys[r] = d2key(canonical fp64 score of row r), 0 for
// a deleted or masked-out row, vals[r] = r, for r in [0, n); the collapsed search's stage 2 reduces them by group
int exact_all_keys(const uint8_t* rows, int dtype, int S, int dpad, const float* qv, int metric, double qn2,
                   const uint32_t* live, const uint32_t* mask, int64_t n, uint64_t* keys, uint32_t* vals,
                   hipStream_t st);
size_t exhaustive_scratch_bytes(int64_t n);
int exhaustive_topm(const uint8_t* rows, int dtype, int S, int dpad, const float* qv, int metric, double qn2,
                    const uint32_t* live,
                    const uint32_t* mask, int64_t n, int64_t row_offset, int m, Cand* out, void* scratch,
                    size_t scratch_bytes, hipStream_t st, int sG = 1, int ss = 0);
// G ranks' sorted exact top-m lists (rank stride cstride bytes) -> the top-k (score desc, row asc; -inf / -1 padding)
int launch_merge_sorted(const Cand* cand, int64_t cstride, int G, int B, int m, int k, float* s_out, int64_t* r_out,
                        hipStream_t st);
size_t tile_list_scratch_bytes(int64_t n_tiles);
int build_tile_list(const uint32_t* live, const uint32_t* mask, int64_t n_tiles, uint32_t* list, uint32_t* count,
                    void* scratch, size_t scratch_bytes, hipStream_t st);
// hr_qmask.hip: per-query row masks (hr_index_search_masks).  QMaskRefs: the distinct bitmaps a chunk of <= 64
// queries references; launch_qmask_union ORs them into one u32 word per tile; launch_qallow_build writes the
// lane-order allow words ([tile][64], what the QM scans read through ScanArgs::mask) of the n_units visited tiles for the chunk's B <= QB * 32
// queries (mask_of: B device entries in [-1, D), -1 = no mask)
struct QMaskRefs {
    int32_t d[64];
};
int launch_qmask_union(const uint64_t* masks, int64_t stride, const QMaskRefs& refs, int nref, int64_t n_tiles,
                       uint32_t* out, hipStream_t st);
int launch_qallow_build(const uint64_t* masks, int64_t stride, const int32_t* mask_of, int B, int QB, const uint32_t* live,
                        const uint32_t* tile_list, int64_t n_units, uint32_t* qallow, hipStream_t st);
// hr_wide.hip: the 128-query FILTER (one workgroup per CU, 4 waves; pbuf / pcnt regions [2 groups][4 * cus][64])
struct ScanArgs;
bool wide_filter_ok(int dtype, int S);
int launch_filter_wide(int mt, int dtype, int S, int cus, const ScanArgs& a, hipStream_t st);
// row parts of the eight-wave form (kc > 32): 32 groups per part, one 16 KiB key table each in LDS beside the two
// streamed window buffers (2 x 32 KiB, or 2 x 16 KiB for fp32 rows): at most 5 (bf16 / f16) or 7 (fp32) parts,
// kc <= 160 / 224
constexpr int wide_max_parts(int dtype) { return dtype == F32 ? 7 : 5; }
// hr_q256.hip: the 256-query FILTER (four 64-query groups in one pass; bf16 / f16 rows, D = 256..1024, one row
// part); candidate regions [4 groups][4 * cus waves][64][kCapW] as k_scan's
bool q256_filter_ok(int dtype, int S);
int launch_filter_q256(int mt, int dtype, int S, int cus, const ScanArgs& a, hipStream_t st);
// hr_persist.hip: the persistent FILTER (plans with 64-query tiles: P = 16 for 16-bit rows, 4 for fp32 rows)
struct PersistCtl;
struct PersistLaunch;
int launch_persist(int mt, int dtype, int P, int cus, const PersistLaunch& pa, int lds, hipStream_t st);
int launch_persist_post(PersistCtl* c, uint32_t e, hipStream_t st);
int launch_persist_close(PersistCtl* c, hipStream_t st);
int launch_persist_wait(PersistCtl* c, uint32_t e, uint32_t nwg, uint32_t* host_err, hipStream_t st);
}  // namespace hr

static constexpr int kCap = 8192;       // candidate buffer per query (shared-buffer / collect mode)
static constexpr int kCapW = 32;        // private candidate slots per (wave, query) (FILTER mode)
static constexpr int kScanThreads = 512;

// Per-batch search workspace.  Two sets ping-pong between consecutive pipelined batches
// (hr_index_search_shard_async: batch i's select/rescore on the tail stream overlaps batch
// i+1's scan on the scan stream); a third serves the synchronous and collect paths.
struct Scratch {
    DevBuf q32, qfrag, qerr, mkeys, floor_q, cnt, buf, sel_rows, sel_cnt, bound_approx, overflow, pbuf, pcnt, dyn_q,
        tl, tl_tmp,  // device-mask tile list (+ its count after the list) and its rocPRIM scratch
        wtiles,      // diagnostics: tiles each wave of the most recent FILTER launch scanned (ScanArgs::wave_tiles)
        cand8,       // shadow-8 scan: the exact candidates of its deeper kc, before the trim to the caller's kc
        qunion,      // per-query masks: OR of the chunk's bitmaps, one word per tile (the tile list's mask)
        qallow,      // per-query masks: lane-order allow words, [tile][64] (the QM scans' ScanArgs::mask)
        qbias;       // shadow-8 scan: -C_q per padded query, the accumulators' start value (k_prep_q, ScanArgs::qbias)
    int64_t last_W = 0, last_Bp = 0;  // waves (per query group) and queries per group of the most recent FILTER
    int last_ng = 1;                  // query groups of that launch
    int last_capw = kCapW;            // candidate slots per (region, query) of that launch
    bool wtiles_valid = false;        // that launch was a k_scan FILTER (it wrote wtiles)
    hipEvent_t scanned = nullptr;     // scan stream: this set's FILTER is done
    hipEvent_t released = nullptr;    // tail stream: this set's select/rescore are done
    hipEvent_t sampled = nullptr;     // pre stream: this set's early query prep + SAMPLE are done
    hipStream_t scan = nullptr;       // early mode: this set's FILTER stream (created on first use)
    bool armed = false;               // `released` has been recorded at least once
    void release_all() {
        for (DevBuf* b : {&q32, &qfrag, &qerr, &mkeys, &floor_q, &cnt, &buf, &sel_rows, &sel_cnt, &bound_approx,
                          &overflow, &pbuf, &pcnt, &dyn_q, &tl, &tl_tmp, &wtiles, &cand8, &qunion, &qallow, &qbias})
            b->release();
        if (scanned) (void)hipEventDestroy(scanned);
        if (released) (void)hipEventDestroy(released);
        if (sampled) (void)hipEventDestroy(sampled);
        if (scan) (void)hipStreamDestroy(scan);
        scan = nullptr;
        scanned = released = sampled = nullptr;
    }
};
static constexpr int kSyncSet = 2;

struct hr_index {
    int dim = 0, dpad = 0, S = 0, dtype = BF16, metric = COSINE, device = 0;
    int64_t n = 0, cap = 0, n_live = 0;
    double max_norm2 = 0.0;
    uint8_t* rows = nullptr;        // tiled corpus
    // fp32 corpora: a 16-bit copy of the rows in the MFMA type (mfma_type), tiled as a 16-bit corpus, that the
    // approximate passes (SAMPLE, FILTER, collect) stream instead of the fp32 tiles -- the values they round every
    // fragment to anyway, at half the bytes; the exact rescoring and exhaustive passes keep reading the fp32 rows.
    // Maintained lazily: row writers lower shadow_lo (first stale tile) and the next search converts [shadow_lo,
    // tiles).  HIPRAG_F32_SHADOW=0 at create: none (the fp32 tiles are streamed and rounded in the kernels).
    uint8_t* rows16 = nullptr;
    bool shadow = false;
    int64_t shadow_lo = 0;
    // cosine corpora (any stored dtype): an 8-bit copy of the rows -- biased int8 (byte = round(x / scale) + 128,
    // |value| <= 127), one 1 KiB block per pair of k-steps (XFrag<F16, I8S>), slot swizzle and tile order as the
    // rows -- with one fp32 scale = max|x| / 127 per row (scale8[row]), built from the STORED rows.  The SAMPLE and
    // the 64-query FILTER of the main pass stream it instead of the 16-bit rows (half the bytes); the guard's
    // storage term is then u_x8 = err8 / max norm, err8 = max_r |x_r - scale_r i_r| over the stored rows (fp64,
    // device word err8_bits).  Maintained lazily like the 16-bit shadow (shadow8_lo: first stale tile); never
    // written to files.  shadow8: the corpus keeps one (cosine, allocation succeeded, HIPRAG_SHADOW8 != 0);
    // shadow8_mode (hr_index_set_shadow8): 0 never scanned, 1 where it measured faster, 2 wherever it is built.
    uint8_t* rows8 = nullptr;
    float* scale8 = nullptr;
    unsigned long long* err8_bits = nullptr;
    bool shadow8 = false;
    int shadow8_mode = 1;
    int64_t shadow8_lo = 0;
    double err8 = 0.0;
    float scale8_max = 0.0f;        // largest row scale of the shadow (device word err8_bits[1]): the bias fold's guard term
    int64_t n_shadow8 = 0;          // shadow-8 FILTER launches issued (diagnostics)
    int last_kc8 = 0;               // candidate depth the most recent shadow-8 scan planned (diagnostics)
    uint32_t* live = nullptr;       // one word per tile
    float* xnorm = nullptr;         // euclidean only: fp32 |x|^2 per stored row (approximate scan score)
    std::vector<uint32_t> live_host;
    unsigned long long* norm_bits = nullptr;  // device max stored norm² (as double bits)
    hipStream_t stream = nullptr;
    hipStream_t pre = nullptr;  // early query prep + SAMPLE of pipelined batches (created on first use)
    // per-launch timing of the main (SAMPLE, FILTER) scan pair: events are recorded on the
    // search stream and harvested later, so batches can be pipelined (see hr_index_take_scan_times)
    struct ScanEvents {
        hipEvent_t e[4];  // SAMPLE start, FILTER start (= SAMPLE end unless early), early SAMPLE end, FILTER end
        bool sampled, early;
        uint32_t pepoch;  // persistent FILTER: the batch's epoch (its FILTER time comes from the device's stamps)
    };
    std::vector<ScanEvents> ev_free;
    std::deque<ScanEvents> ev_pending;
    float last_sample_ms = 0.f, last_filter_ms = 0.f;
    int time_every = 0;               // record events around every Nth main pass (0 = never)
    int64_t main_passes = 0;
    bool isolate_next = false;        // dual-stream mode: the next FILTER waits for a timed one
    int n_cu = 256;                   // CUs the grids are sized from (hr_index_set_cu_mask: the mask's)
    int n_cu_dev = 256;               // CUs of the device, whatever the mask (region_slots)
    std::mutex mu;
    // tile list of the current selective-filter search (hr_index_search with a row mask that
    // leaves at most half the tiles): sorted tiles holding a live, allowed row; tl_n = -1: none
    // (a device mask builds its own), -2: the host evaluated the mask and chose the full scan
    DevBuf tl;
    int64_t tl_n = -1;
    std::vector<uint32_t> tl_host;
    // search workspace
    HostStage hs;
    DevBuf pool_s, pool_r;  // the derived searches' inner search: its B x P scores / rows (one at a time under mu)
    DevBuf cand, bound, kth, fail, fb_cand, fb_bound, fb_q, fb_out, exh;
    DevBuf ivf_coarse, ivf_probe, ivf_units, ivf_uoff, ivf_out;  // IVF lists search (hr_ivf.hip)
    Scratch scr[3];
    int flip = 0;                     // next ping-pong set of the pipelined path
    const Scratch* last_scr = nullptr;  // set of the most recent FILTER launch (diagnostics)
    int64_t n_exhaustive = 0;         // queries that needed the exhaustive exact pass (diagnostics)
    int64_t n_guard_fail = 0;         // queries that failed the exactness guard (collect fallback)
    int64_t n_wide = 0;               // 128-query FILTER launches issued (hr_wide.hip; not graph replays)
    int64_t n_q256 = 0;               // 256-query FILTER launches issued (hr_q256.hip)
    int64_t n_qmask = 0;              // FILTER launches that ran with per-query masks (hr_index_search_masks)
    bool qmask_timing = false;        // hr_index_set_qmask_timing: HIP events around the mask prep of every chunk
    hipEvent_t qm_ev[3] = {nullptr, nullptr, nullptr};
    double qm_ms[2] = {0.0, 0.0};     // union + tile list, allow table: summed over the most recent call's chunks
    bool q256 = true;                 // hr_index_set_q256: 129-256-query batches take the 256-query FILTER
    std::vector<float> floor_host;
    // ---- hr_index_search (host queries, no mask) replayed as one HIP graph per batch shape: H2D of
    // the queries from pinned staging, prep, SAMPLE, FILTER, select, rescore, merge, D2H of results
    // and guard flags.  Captured on a shape's second use (the first allocates every buffer); stale once
    // the corpus, its buffers or any work buffer changes (address / size snapshot below).
    struct SyncGraph {
        int B = 0, k = 0, uses = 0;
        bool disabled = false;
        int64_t n = -1;
        const void* rows = nullptr;
        const void* live = nullptr;
        const void* xnorm = nullptr;
        const void* rows8 = nullptr;
        double err8 = 0.0;
        float scale8_max = 0.0f;
        const void* pin = nullptr;
        double max_norm2 = 0.0;
        uint64_t buf_gen = 0;
        int chunks = 1;
        hipGraphExec_t exec = nullptr;
    };
    std::vector<SyncGraph> sync_graphs;
    void* pin = nullptr;      // pinned host staging of the graph path (hipHostMalloc)
    size_t pin_bytes = 0;
    DevBuf sync_out;          // device results of the graph path
    int64_t n_graph_replays = 0;
    // ---- asynchronous host-query search (hr_index_search_submit_host / _collect, hr_index.hip): up to two
    // batches in flight; each batch's completion is signalled to a file descriptor (an eventfd the caller's
    // event loop watches) by a host function queued behind its results' copy to pinned memory
    struct AsyncSlot {
        bool busy = false;
        int64_t ticket = 0;
        int B = 0, k = 0;
        uint8_t* pin = nullptr;  // pinned: queries in | scores | rows | guard flags | k-th scores out
        size_t pin_bytes = 0;
        size_t off_s = 0, off_r = 0, off_f = 0, off_k = 0;
        DevBuf q, cand, bound, kth, fail, s, r;
        hipEvent_t q_ready = nullptr, done = nullptr;
        // the batch's notify host function (hipLaunchHostFunc behind `done`) has not returned yet: collect and
        // destroy wait for it, so the caller never closes or reuses the fd number while that write is pending
        std::atomic<int> notify_pending{0};
        int notify_fd = -1;
    } aslot[2];
    int64_t aticket = 1;
    hipStream_t acopy = nullptr, atail = nullptr;
    // ---- multi-device handles (hr_index_create with n_dev > 1, hr_group.hip)
    // A group handle owns G shard handles (one per dev_ids entry, repeats allowed) and stripes its
    // rows over them by 32-row tile (stripe_row, hr_common.hpp); it holds no rows itself.  Its
    // device / stream are the primary's (dev_ids[0]): the shards' candidates are copied there
    // (hipMemcpyPeerAsync, xGMI) and merged by k_merge.  A shard knows its place in the stripe.
    int G = 1;                        // > 1: group handle
    std::vector<hr_index*> shards;
    int stripe_G = 1, stripe_s = 0;   // shard of a group: global row of local row L = stripe_row(L, G, s)
    bool shared_dev = false;          // shard of a group whose GPU also holds another shard of the group
    DevBuf g_cand, g_bound, g_kth, g_fail, g_out, g_q;  // group: gathered candidates / merge outputs (primary)
    DevBuf s_mask;                    // shard of a group: this shard's words of the caller's row mask
    std::vector<hipEvent_t> g_ev;     // group: one per shard (shard stream -> primary stream)
    hipEvent_t g_ev_q = nullptr;      // group: queries ready on the primary stream
    std::vector<char> g_peer;         // group: shard s's device has peer access with the primary
    struct GroupPipe* pipe = nullptr; // group: pipelined search (submit / finalize, hr_group.hip)
    struct Persist* ps = nullptr;     // persistent FILTER state (hr_index.hip; created on first use)
    // hr_index_set_cu_mask: the CUs this index's own streams may use (empty: all).  Every internal stream is then
    // created with hipExtStreamCreateWithCUMask and the launch grids are sized for popcount(mask) CUs
    std::vector<uint32_t> cu_mask;
    // ---- collapsed search (hr_collapse.hip): the group column -- one int32 id per row, -1 = no group -- allocated by
    // the first hr_index_set_groups and grown by doubling on its own (index_grow never sees it): entries
    // [0, groups_cap) exist, rows at or beyond groups_cap count as -1.  n_groups = largest id set so far + 1.
    int32_t* groups = nullptr;
    int64_t groups_cap = 0;
    int64_t n_groups = 0;
    DevBuf col_flag;                  // the probe's incomplete flags
    DevBuf col_keys, col_g, col_top;  // stage 2: score keys + rows of one query (12 n bytes), group tables, top-k
    int64_t n_collapse_probe = 0, n_collapse_all = 0;  // queries answered from the probe / by the all-rows pass
    bool collapse_timing = false;     // hr_index_set_collapse_timing: HIP events around the stages of every call
    hipEvent_t col_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double col_ms[3] = {0.0, 0.0, 0.0};  // probe search, prefix kernel, stage 2 of the most recent timed call
    // ---- MMR search (hr_mmr.hip)
    bool mmr_timing = false;          // hr_index_set_mmr_timing: HIP events around the two stages of every call
    hipEvent_t mmr_ev[3] = {nullptr, nullptr, nullptr};
    double mmr_ms[2] = {0.0, 0.0};    // probe search, selection kernel of the most recent timed call
    // ---- range search (hr_range.hip): every buffer allocated by the first call that needs it.  rng_arena: per query
    // of a chunk one region of cap float2 scan records and cap score keys; rng_keys: stage 2's score keys + rows of
    // ONE query (12 n bytes) or a large region's row-ordered copy; rng_sort: the hits of one query being sorted
    DevBuf rng_arena, rng_flag, rng_keys, rng_sort, rng_tmp;
    int64_t n_range_window = 0, n_range_all = 0;  // queries answered by stage 1 (window scan) / stage 2 (all rows)
    int64_t n_range_scans = 0;                    // window-scan launches (one per chunk of queries)
    DevBuf rng_wtiles;                            // diagnostics: tiles each wave of the most recent window scan scanned
    int64_t rng_waves = 0;                        // ... and how many waves that launch had (all query groups)
    // ---- search by example (hr_examples.hip): every buffer allocated by the first call that needs it.  ex_list: one
    // call's example lists as one block (offsets | rows | weights), packed in ex_host and copied once
    DevBuf ex_list, ex_q, ex_cand;  // lists, built queries, K' records of the exhaustive pass
    std::vector<uint8_t> ex_host;
    // ---- fused multi-query search (hr_fuse.hip): every buffer allocated by the first call that needs it.  fu_list:
    // one call's group offsets and weights as one block, packed in fu_host and copied once
    DevBuf fu_list;
    std::vector<uint8_t> fu_host;
    // ---- boosted search (hr_boost.hip): the boost columns -- one fp32 per row each, allocated by the first
    // hr_index_set_boost of the column and grown by doubling on their own, as the group column: entries [0, boost_cap)
    // exist, rows at or beyond it read 0.0.  boost_ext_*: the column's extrema over rows [0, n), valid while
    // boost_ext_n == n (-1: the column was written).  Work buffers allocated by the first call that needs them:
    // bst_win the window of one chunk of queries, bst_keys stage 2's keys / rows / fp32 scores / selection of ONE
    // query (20 n bytes), bst_sort the selected rows being sorted
    float* boost[HR_BOOST_MAX_COLS] = {nullptr, nullptr, nullptr, nullptr};
    int64_t boost_cap[HR_BOOST_MAX_COLS] = {0, 0, 0, 0};
    float boost_ext_lo[HR_BOOST_MAX_COLS] = {0.f, 0.f, 0.f, 0.f}, boost_ext_hi[HR_BOOST_MAX_COLS] = {0.f, 0.f, 0.f, 0.f};
    int64_t boost_ext_n[HR_BOOST_MAX_COLS] = {-1, -1, -1, -1};
    DevBuf bst_win, bst_keys, bst_sort, bst_tmp;
    int64_t n_boost_window = 0, n_boost_all = 0;  // queries answered by stage 1 (window) / stage 2 (all rows)
};

// an internal stream of h: on h's CU mask when one is set (priority is then not available), else high priority or
// the default one (hr_index.hip)
hipError_t index_stream_create(const hr_index* h, hipStream_t* s, bool high_priority);

// group-handle entry points (hr_group.hip); each public hr_index_* call forwards here when h->G > 1
int group_create(int dim, int dtype, int metric, int n_dev, const int* dev_ids, hr_index** out);
void group_destroy(hr_index* g);
int group_reserve(hr_index* g, int64_t rows);
int group_add_host(hr_index* g, const float* rows, int64_t n, int64_t* first);
int group_add_synthetic(hr_index* g, uint64_t seed, int64_t global_row0, int64_t n, int64_t* first);
int group_add_device(hr_index* g, const float* rows_dev, int64_t n, int64_t* first, hipStream_t st);
int group_remove(hr_index* g, const int64_t* rows, int64_t n);
int group_search_host(hr_index* g, const float* q, int B, int k, const uint64_t* mask, float* s_out, int64_t* r_out);
int group_search_device(hr_index* g, const float* q_dev, int B, int k, const uint64_t* mask_dev, float* s_out,
                        int64_t* r_out, hipStream_t st);
int group_get_rows(hr_index* g, const int64_t* rows, int64_t n, float* out);
// pipelined group search: enqueue a batch (every shard submitted by its own host thread), finalize =
// wait for its guard flags and run the exact fallback; group_drain finalizes everything in flight
int group_search_submit(hr_index* g, const float* q_dev, int B, int k, float* s_out, int64_t* r_out, hipStream_t st,
                        int64_t* ticket);
int group_search_finalize(hr_index* g, int64_t ticket);
int group_drain(hr_index* g);
int group_host_us(hr_index* g, double out[3]);
int group_save(hr_index* g, const char* path);
int group_load_into(hr_index* g, FILE* f, int64_t n, int64_t n_live, double max_norm2);
void group_stats(hr_index* g, int64_t out[3]);

// single-shard internals shared with hr_group.hip (hr_index.hip)
int index_grow(hr_index* h, int64_t need_rows);
int index_add_host(hr_index* h, const float* rows, int64_t n, int64_t* first);
int index_add_synthetic(hr_index* h, uint64_t seed, int64_t gen_base, int64_t n);
int index_remove_local(hr_index* h, const int64_t* rows, int64_t n);
int index_get_rows(hr_index* h, const int64_t* rows, int64_t n, float* out);
int index_update_row_norms(hr_index* h, int64_t r0, int64_t n);
// the group-max order statistic of the FILTER's starting threshold and k_select (ScanArgs::kj; hr_index.hip)
int hr_rank_for(int k, int kc, int dim);
int index_finish_load(hr_index* h);
// one batch of queries (device, on this shard's device) through the exact search of one shard:
// candidates (global rows) + bounds into cand_out / bound_out on `st`
int index_shard_search(hr_index* h, const float* q_dev, int B, int kc, int kj, const uint64_t* mask_dev, Cand* cand_out,
                       double* bound_out, hipStream_t st);
// the same, pipelined: scan on st, select + rescore on st_tail (outputs ready in st_tail order), the
// queries ready once q_ready completes (see hr_index_search_shard_async_ev)
int index_shard_search_async(hr_index* h, const float* q_dev, int B, int kc, int kj, Cand* cand_out, double* bound_out,
                             hipStream_t st, hipStream_t st_tail, hipEvent_t q_ready);
int index_shard_collect(hr_index* h, const float* q_dev, int B, const double* kth_host, int cap,
                        const uint64_t* mask_dev, Cand* cand_out, double* bound_out, hipStream_t st);
int index_exact_all(hr_index* h, const float* q_dev, int B, int m, const uint64_t* mask_dev, Cand* out_host,
                    hipStream_t st);
int index_host_tile_list(hr_index* h, const uint32_t* mask_words, hipStream_t st);
// collapsed search (hr_collapse.hip) over the single-shard search; the caller holds h->mu with h's device current.
// index_search_locked: hr_index_search_device without the lock (the full exact search, fallback included);
// index_prep_exact: the canonical fp32 queries of the all-rows exact pass (dpad floats each, at *q32_out) and
// their host-side terms (qerr_out[4 b + 2] = |q_b|^2); synchronises st.  collapse_free: hr_index_destroy's part.
int index_search_locked(hr_index* h, const float* q_dev, int B, int k, const uint64_t* mask_dev, float* s_out,
                        int64_t* r_out, hipStream_t st);
int index_prep_exact(hr_index* h, const float* q_dev, int B, hipStream_t st, const float** q32_out,
                     std::vector<double>* qerr_out);
void collapse_free(hr_index* h);
// range search (hr_range.hip) reaches the collect scan through shard_chunk's mode 2: query prep, floors from the
// caller's thresholds (range_floors, on the stream: no host wait), one SCAN_COLLECT pass appending into the caller's
// regions, and nothing after it -- the counts are left in the synchronous workspace's cnt (h->scr[kSyncSet]), its q32
// / qerr hold the chunk's processed queries.  index_range_chunk: one chunk of bc <= index_plan_bp(h, B) queries.
struct RangeScan {
    const float* min_score;  // device, one per query of the chunk
    float2* buf;             // [Bp][cap] records {approximate score, row bits}
    int cap;
};
int index_plan_bp(hr_index* h, int B, int* bp_out);
int index_range_chunk(hr_index* h, const float* q_dev, int bc, const uint64_t* mask_dev, const RangeScan* rs,
                      hipStream_t st);
int range_floors(const double* qerr, const float* min_score, int B, int Bp, double max_norm, double gamma, double u_x,
                 int metric, float* floor_q, hipStream_t st);
void range_free(hr_index* h);  // hr_index_destroy's part
// the range search itself (hr_range.hip), for the searches built on it (hr_boost.hip): queries, thresholds (no NaN),
// mask and outputs on h's device; the caller holds h->mu with the device current; returns with st idle
int range_impl(hr_index* h, const float* q_dev, int B, const float* t_dev, int max_hits, const uint64_t* mask_dev,
               float* s_out, int64_t* r_out, int64_t* c_out, hipStream_t st);
void boost_free(hr_index* h);  // hr_boost.hip: hr_index_destroy's part
void mmr_free(hr_index* h);  // hr_mmr.hip: hr_index_destroy's part
void examples_free(hr_index* h);  // hr_examples.hip: hr_index_destroy's part
void fused_free(hr_index* h);  // hr_fuse.hip: hr_index_destroy's part
// hr_index_search_masks_device without the lock and the argument checks (hr_fuse.hip): mask_of_host holds the B
// entries of mask_of_dev, already through index_validate_masks; 1 <= k <= HR_MAX_K (hr_index.hip)
int index_validate_masks(hr_index* h, int B, int D, int64_t stride, const int32_t* mask_of_host);
int index_search_masks_locked(hr_index* h, const float* q_dev, int B, int k, const uint64_t* masks_dev, int64_t stride,
                              const int32_t* mask_of_dev, const int32_t* mask_of_host, float* s_out, int64_t* r_out,
                              hipStream_t st);
// the exhaustive exact pass of a k > HR_MAX_K search into device records out_dev[B][m] (hr_index.hip)
int index_exact_dev(hr_index* h, const float* q_dev, int B, int m, const uint64_t* mask_dev, int64_t row_offset,
                    Cand* out_dev, hipStream_t st);
int launch_merge(int device, const Cand* cand, const double* bounds, int G, int B, int kc, int k, float* s_out,
                 int64_t* r_out, double* kth_out, int32_t* fail_out, hipStream_t st, int64_t cstride = 0,
                 int64_t bstride = 0);
static constexpr int kMergeMaxCand = 8192;  // G * kc of one launch_merge: its LDS holds that many 16-byte records
static constexpr int kFallbackCapMax = 1024;
inline int fallback_cap(int G) { return std::max(64, std::min(kFallbackCapMax, kMergeMaxCand / std::max(1, G))); }

struct FileHeader {
    char magic[8];
    int32_t version, dim, dtype, metric;
    int64_t n, n_live;
    double max_norm2;
};

inline size_t tile_bytes(const hr_index* h) { return (size_t)h->S * (h->dtype == F32 ? 2048 : 1024); }

inline int set_device(hr_index* h) {
    HIP_TRY(hipSetDevice(h->device));
    return HR_OK;
}

// ---------------------------------------------------------------- host-form staging (h->hs, on st, under h->mu)
// B host queries -> *q_dev
inline int stage_queries(hr_index* h, const float* q, int64_t B, hipStream_t st, float** q_dev) {
    const size_t bytes = (size_t)B * h->dim * 4;
    HIP_TRY(h->hs.q.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(h->hs.q.p, q, bytes, hipMemcpyHostToDevice, st));
    *q_dev = h->hs.q.as<float>();
    return HR_OK;
}
// one host row mask -> *m_dev: the words that cover the index; nullptr without a mask or on an index without rows
// (no zero-byte copy)
inline int stage_mask(hr_index* h, const uint64_t* row_mask, hipStream_t st, uint64_t** m_dev) {
    const size_t words = (size_t)((h->n + 63) / 64);
    *m_dev = nullptr;
    if (!row_mask || !words) return HR_OK;
    HIP_TRY(h->hs.mask.ensure(words * 8));
    HIP_TRY(hipMemcpyAsync(h->hs.mask.p, row_mask, words * 8, hipMemcpyHostToDevice, st));
    *m_dev = h->hs.mask.as<uint64_t>();
    return HR_OK;
}
// D host bitmaps, stride words apart, and the B entries of mask_of: only the words that cover the index go up,
// words64 = (n + 63) / 64 apart on the device.  D = 0 leaves *masks_dev a valid (8-byte) address nobody reads.
inline int stage_masks(hr_index* h, const uint64_t* masks, int D, int64_t stride, const int32_t* mask_of, int B,
                       hipStream_t st, uint64_t** masks_dev, int32_t** of_dev) {
    const size_t words64 = (size_t)((h->n + 63) / 64);
    HIP_TRY(h->hs.of.ensure((size_t)B * 4));
    HIP_TRY(h->hs.mask.ensure(std::max<size_t>(8, (size_t)D * words64 * 8)));
    HIP_TRY(hipMemcpyAsync(h->hs.of.p, mask_of, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (D > 0 && words64 > 0)
        HIP_TRY(hipMemcpy2DAsync(h->hs.mask.p, words64 * 8, masks, (size_t)stride * 8, words64 * 8, (size_t)D,
                                 hipMemcpyHostToDevice, st));
    *masks_dev = h->hs.mask.as<uint64_t>();
    *of_dev = h->hs.of.as<int32_t>();
    return HR_OK;
}
// one result block: stage_out lays the segments out in hs.out (dev: 256-byte aligned; nullptr for a segment the
// caller does not want, host == nullptr), stage_download copies every wanted, non-empty one to its host array
struct OutSeg {
    void* host;
    size_t bytes;
    void* dev;
    template <class T>
    T* as() const {
        return (T*)dev;
    }
};
template <int N>
inline int stage_out(hr_index* h, OutSeg (&seg)[N]) {
    size_t total = 0;
    for (const OutSeg& s : seg) total += s.host ? up256(s.bytes) : 0;
    HIP_TRY(h->hs.out.ensure(total));
    size_t off = 0;
    for (OutSeg& s : seg) {
        s.dev = s.host ? h->hs.out.as<uint8_t>() + off : nullptr;
        off += s.host ? up256(s.bytes) : 0;
    }
    return HR_OK;
}
template <int N>
inline int stage_download(const OutSeg (&seg)[N], hipStream_t st) {
    for (const OutSeg& s : seg)
        if (s.host && s.bytes) HIP_TRY(hipMemcpyAsync(s.host, s.dev, s.bytes, hipMemcpyDeviceToHost, st));
    return HR_OK;
}
// the selective-filter tile list of a host row mask (index_host_tile_list) lasts one call
struct TileListScope {
    hr_index* h;
    ~TileListScope() { h->tl_n = -1; }
};

// ---------------------------------------------------------------- dispatch helpers
template <class F>
inline int dispatch_dt(int dt, F&& f) {
    switch (dt) {
        case F32: return f(std::integral_constant<int, F32>{});
        case BF16: return f(std::integral_constant<int, BF16>{});
        case F16: return f(std::integral_constant<int, F16>{});
    }
    return set_err(HR_E_INVALID, "unknown dtype");
}

// MFMA operand type: f16 corpora use the f16 MFMA and bf16 corpora the bf16 one.  fp32 corpora are
// rounded to one of them on the fly: f16 (unit roundoff 2^-11, 8x finer than bf16, so the guard's window
// and the collect fallbacks shrink with it) when the rows are normalised (cosine: every element in
// [-1, 1], far inside f16's range), bf16 (fp32's range) for raw inner-product / euclidean rows
inline int mfma_type(const hr_index* h) {
    return (h->dtype == F16 || (h->dtype == F32 && h->metric == COSINE)) ? F16 : BF16;
}

// what the approximate passes stream: the 16-bit shadow of an fp32 corpus (as a corpus of the MFMA type), else the
// stored rows.  The exactness guard's storage term (storage_u) stays the fp32 one: the shadow holds exactly the
// RNE-rounded values the fp32 kernels would form on the fly.
inline int scan_dtype(const hr_index* h) { return h->rows16 ? mfma_type(h) : h->dtype; }
inline const uint8_t* scan_rows(const hr_index* h) { return h->rows16 ? h->rows16 : h->rows; }
// a row writer touched tiles from t0 on (INT64_MAX: the shadow is current)
inline void shadow_stale(hr_index* h, int64_t t0) {
    if (h->shadow && t0 < h->shadow_lo) h->shadow_lo = t0 < 0 ? 0 : t0;
    if (h->shadow8 && t0 < h->shadow8_lo) h->shadow8_lo = t0 < 0 ? 0 : t0;
}
int shadow_update(hr_index* h);

