// hr_collapse.hip -- collapsed search: the exact top-k DISTINCT groups of every query, each group represented by
// its best row (Milvus "group-by search", Elasticsearch "collapse").
//
// Every row may carry a group id (the group column, hr_index_set_groups; -1 = no group).  For one query, order the
// live, allowed rows with a group as every search does (canonical fp64 score desc, row asc), walk that order and keep
// a row only when its group has not been seen: the first k kept rows are the answer.
//
//   stage 1 (probe)     the exact search for P >= k rows, then k_collapse_prefix (one wave per query): drop records
//                       without a group, mark the first record of every group, compact the first k of them.  The
//                       query is INCOMPLETE when fewer than k groups came out of a probe that came back full (its
//                       last slot holds a row): a (k+1)-th document may sit just below the probe.
//   stage 2 (all rows)  incomplete queries only, one at a time: canonical score key of every live, allowed row
//                       (k_exact_all, hr_exhaustive.hip -- the arithmetic lives there alone), k_group_max (atomicMax
//                       of the key into gkey[g]), k_group_row (atomicMin of the row into grow[g] among the rows whose
//                       key equals gkey[g]), k_group_records ({score, row} per group), the exact record selector
//                       (hr_topk_records) for the top k groups, k_collapse_take (fp32 / int64 outputs).  No n-row
//                       sort.  A document's rows are appended together, so ids come in runs: both reductions first
//                       reduce every run of equal ids inside the wave and issue one atomic per run, and skip it when
//                       a plain read shows it cannot win.  Nothing depends on the runs: interleaved ids only cost
//                       more atomics.
//
// Stage-2 workspace (h->col_keys / col_g): 12 bytes per index row (the score keys and row numbers of ONE query) plus
// 32 bytes per group (gkey, grow, one record), whatever the batch size.
#include "hr_internal.hpp"

namespace {

// ---------------------------------------------------------------- stage 1
// One wave per query (four per workgroup), P <= 128 probe records per query, two per lane.
__global__ __launch_bounds__(256) void k_collapse_prefix(const float* __restrict__ s_in, const int64_t* __restrict__ r_in,
                                                         int B, int P, int k, const int32_t* __restrict__ groups,
                                                         int64_t gcap, float* __restrict__ s_out,
                                                         int64_t* __restrict__ r_out, int32_t* __restrict__ flags) {
    __shared__ int32_t sg[4][HR_MAX_K];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + w;
    const bool active = q < B;
    int32_t g[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int i = lane + 64 * hh;
        g[hh] = -1;
        if (active && i < P) {
            const int64_t r = r_in[(int64_t)q * P + i];
            if (r >= 0 && r < gcap) g[hh] = groups[r];
        }
        sg[w][i] = g[hh];
    }
    __syncthreads();
    bool first[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int i = lane + 64 * hh;
        first[hh] = g[hh] >= 0;
        if (first[hh])
            for (int j = 0; j < i; ++j)
                if (sg[w][j] == g[hh]) {
                    first[hh] = false;
                    break;
                }
    }
    const unsigned long long b0 = __ballot(first[0]), b1 = __ballot(first[1]);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int c0 = __popcll(b0), total = c0 + __popcll(b1);
    const int pos[2] = {(int)__popcll(b0 & lt), c0 + (int)__popcll(b1 & lt)};
    if (!active) return;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
        if (first[hh] && pos[hh] < k) {
            const int64_t src = (int64_t)q * P + lane + 64 * hh;
            s_out[(int64_t)q * k + pos[hh]] = s_in[src];
            r_out[(int64_t)q * k + pos[hh]] = r_in[src];
        }
    for (int i = total + lane; i < k; i += 64) {
        s_out[(int64_t)q * k + i] = -__builtin_inff();
        r_out[(int64_t)q * k + i] = -1;
    }
    if (lane == 0) flags[q] = (total < k && r_in[(int64_t)q * P + (P - 1)] >= 0) ? 1 : 0;
}

// ---------------------------------------------------------------- stage 2
// Lane i of a wave holds row 64 * wave + i.  A run = a maximal stretch of lanes with one id; start = its first
// lane, tail = this lane is its last.  Every lane of the wave must call.
__device__ inline void run_bounds(int32_t g, int lane, int* start, bool* tail) {
    const int32_t gp = __shfl_up(g, 1, 64), gn = __shfl_down(g, 1, 64);
    int s = (lane == 0 || gp != g) ? lane : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(s, off, 64);
        if (lane >= off && o > s) s = o;
    }
    *start = s;
    *tail = lane == 63 || gn != g;
}

__device__ inline int32_t row_group(const int32_t* __restrict__ groups, int64_t gcap, int64_t n_groups, int64_t r,
                                    int64_t n) {
    if (r >= n || r >= gcap) return -1;
    const int32_t g = groups[r];
    return (int64_t)g < n_groups ? g : -1;
}

__global__ __launch_bounds__(256) void k_group_max(const uint64_t* __restrict__ keys, int64_t n,
                                                   const int32_t* __restrict__ groups, int64_t gcap, int64_t n_groups,
                                                   unsigned long long* __restrict__ gkey) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t g = row_group(groups, gcap, n_groups, r, n);
    unsigned long long key = r < n ? keys[r] : 0ull;  // 0: deleted or masked out
    int start;
    bool tail;
    run_bounds(g, lane, &start, &tail);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(key, off, 64);
        if (lane - off >= start && o > key) key = o;
    }
    if (tail && g >= 0 && key != 0ull && key > __atomic_load_n(&gkey[g], __ATOMIC_RELAXED)) atomicMax(&gkey[g], key);
}

// after k_group_max (gkey final): the lowest row of every group among those that hold the group's best key
__global__ __launch_bounds__(256) void k_group_row(const uint64_t* __restrict__ keys, int64_t n,
                                                   const int32_t* __restrict__ groups, int64_t gcap, int64_t n_groups,
                                                   const unsigned long long* __restrict__ gkey,
                                                   unsigned long long* __restrict__ grow) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t g = row_group(groups, gcap, n_groups, r, n);
    const unsigned long long key = r < n ? keys[r] : 0ull;
    unsigned long long best = ~0ull;
    if (g >= 0 && key != 0ull && key == gkey[g]) best = (unsigned long long)r;
    int start;
    bool tail;
    run_bounds(g, lane, &start, &tail);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(best, off, 64);
        if (lane - off >= start && o < best) best = o;
    }
    if (tail && g >= 0 && best != ~0ull && best < __atomic_load_n(&grow[g], __ATOMIC_RELAXED)) atomicMin(&grow[g], best);
}

__global__ __launch_bounds__(256) void k_group_records(const unsigned long long* __restrict__ gkey,
                                                       const unsigned long long* __restrict__ grow, int64_t n_groups,
                                                       Cand* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const unsigned long long key = gkey[g];
    out[g] = key != 0ull ? Cand{key2d(key), (int64_t)grow[g]} : Cand{-__builtin_inf(), -1};
}

__global__ void k_collapse_take(const Cand* __restrict__ top, int k, float* __restrict__ s_out,
                                int64_t* __restrict__ r_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const Cand e = top[i];
    s_out[i] = e.row >= 0 ? (float)e.score : -__builtin_inff();
    r_out[i] = e.row >= 0 ? e.row : -1;
}

// one incomplete query through the all-rows pass; qv: its canonical fp32 query (dpad floats), qn2 = |q|^2
int collapse_all_rows(hr_index* h, const float* qv, double qn2, const uint64_t* mask_dev, int k, float* s_out,
                      int64_t* r_out, hipStream_t st) {
    const int64_t n = h->n, G = h->n_groups;
    if (n <= 0 || G <= 0) return pad_results(s_out, r_out, k, st);
    uint64_t* keys = h->col_keys.as<uint64_t>();
    uint32_t* vals = (uint32_t*)(h->col_keys.as<uint8_t>() + up256(8 * (size_t)n));
    unsigned long long* gkey = h->col_g.as<unsigned long long>();
    unsigned long long* grow = gkey + G;
    Cand* rec = (Cand*)(grow + G);
    if (int rc = exact_all_keys(h->rows, h->dtype, h->S, h->dpad, qv, h->metric, qn2, h->live, (const uint32_t*)mask_dev,
                                n, keys, vals, st))
        return set_err(rc, "all-rows exact pass failed");
    HIP_TRY(hipMemsetAsync(gkey, 0, (size_t)G * 8, st));
    HIP_TRY(hipMemsetAsync(grow, 0xFF, (size_t)G * 8, st));
    const dim3 rows_grid((unsigned)((n + 255) / 256)), grp_grid((unsigned)((G + 255) / 256));
    hipLaunchKernelGGL(k_group_max, rows_grid, dim3(256), 0, st, keys, n, h->groups, h->groups_cap, G, gkey);
    hipLaunchKernelGGL(k_group_row, rows_grid, dim3(256), 0, st, keys, n, h->groups, h->groups_cap, G, gkey, grow);
    hipLaunchKernelGGL(k_group_records, grp_grid, dim3(256), 0, st, gkey, grow, G, rec);
    HIP_TRY(hipGetLastError());
    if (int rc = hr_topk_records(rec, nullptr, G, 1, k, h->col_top.p, st)) return rc;
    hipLaunchKernelGGL(k_collapse_take, dim3((unsigned)((k + 127) / 128)), dim3(128), 0, st, h->col_top.as<Cand>(), k,
                       s_out, r_out);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

// The default probe (the sweep of tools/bench_collapse.py): the probe answers a query only when it
// reaches past the documents that own its top rows, one query in the all-rows stage costs about what the whole
// batch's probe does, and the deepest probe costs 0.5 ms more per 64-query batch than a 40-row one at 1M rows.  So
// the deepest it is; k = 1 is answered by the first row that has a group and keeps a shallow probe.
int default_probe(int k) { return k == 1 ? 32 : HR_MAX_K; }

// queries, mask and outputs on h's device; the caller holds h->mu with the device current.  Returns with st idle.
int collapsed_impl(hr_index* h, const float* q_dev, int B, int k, int probe, const uint64_t* mask_dev, float* s_out,
                   int64_t* r_out, hipStream_t st) {
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (k <= 0 || k > HR_MAX_K) return set_err(HR_E_INVALID, "k must be in [1, HR_MAX_K]");
    const int P = probe ? probe : default_probe(k);
    if (P < k || P > HR_MAX_K) return set_err(HR_E_INVALID, "probe must be 0 or in [k, HR_MAX_K]");
    if (!h->groups) return set_err(HR_E_INVALID, "the index has no group column (hr_index_set_groups)");
    if (h->n_live == 0) {  // empty index: padding, as hr_index_search
        if (int rc = pad_results(s_out, r_out, (int64_t)B * k, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        h->n_collapse_probe += B;
        return HR_OK;
    }
    const bool timed = h->collapse_timing;
    if (timed)
        for (auto& e : h->col_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(h->pool_s.ensure((size_t)B * P * 4));
    HIP_TRY(h->pool_r.ensure((size_t)B * P * 8));
    HIP_TRY(h->col_flag.ensure((size_t)B * 4));
    if (timed) HIP_TRY(hipEventRecord(h->col_ev[0], st));
    if (int rc = index_search_locked(h, q_dev, B, P, mask_dev, h->pool_s.as<float>(), h->pool_r.as<int64_t>(), st))
        return rc;
    if (timed) HIP_TRY(hipEventRecord(h->col_ev[1], st));
    hipLaunchKernelGGL(k_collapse_prefix, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, h->pool_s.as<float>(),
                       h->pool_r.as<int64_t>(), B, P, k, h->groups, h->groups_cap, s_out, r_out,
                       h->col_flag.as<int32_t>());
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(h->col_ev[2], st));
    std::vector<int32_t> flags((size_t)B);
    HIP_TRY(hipMemcpyAsync(flags.data(), h->col_flag.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int> todo;
    for (int b = 0; b < B; ++b)
        if (flags[(size_t)b]) todo.push_back(b);
    h->n_collapse_probe += B - (int64_t)todo.size();
    h->n_collapse_all += (int64_t)todo.size();
    if (!todo.empty()) {
        const float* q32 = nullptr;
        std::vector<double> qerr;
        if (int rc = index_prep_exact(h, q_dev, B, st, &q32, &qerr)) return rc;
        HIP_TRY(h->col_keys.ensure(up256(8 * (size_t)h->n) + up256(4 * (size_t)h->n)));
        HIP_TRY(h->col_g.ensure(std::max<size_t>(32, 32 * (size_t)h->n_groups)));
        HIP_TRY(h->col_top.ensure((size_t)HR_MAX_K * sizeof(Cand)));
        for (int b : todo)
            if (int rc = collapse_all_rows(h, q32 + (int64_t)b * h->dpad, qerr[4 * (size_t)b + 2], mask_dev, k,
                                           s_out + (int64_t)b * k, r_out + (int64_t)b * k, st))
                return rc;
    }
    if (timed) HIP_TRY(hipEventRecord(h->col_ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timed) {
        float ms[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], h->col_ev[i], h->col_ev[i + 1]));
        for (int i = 0; i < 3; ++i) h->col_ms[i] = ms[i];
    }
    return HR_OK;
}

int check_handle(hr_index* h) {
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "collapsed search needs a single-device handle");
    return HR_OK;
}

}  // namespace

void collapse_free(hr_index* h) {
    if (h->groups) (void)hipFree(h->groups);
    h->groups = nullptr;
    h->groups_cap = 0;
    for (DevBuf* b : {&h->col_flag, &h->col_keys, &h->col_g, &h->col_top}) b->release();
    for (auto& e : h->col_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int hr_index_set_groups(hr_index* h, int64_t row0, int64_t n, const int32_t* groups) {
    if (!h || (n > 0 && !groups)) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_handle(h)) return rc;
    if (int rc = set_device(h)) return rc;
    if (row0 < 0 || n < 0 || row0 > h->n || n > h->n - row0)
        return set_err(HR_E_INVALID, "rows [row0, row0 + n) must lie inside the index");
    int32_t top = -1;
    for (int64_t i = 0; i < n; ++i) {
        if (groups[i] < -1) return set_err(HR_E_INVALID, "group ids must be >= -1");
        top = std::max(top, groups[i]);
    }
    const int64_t need = std::max<int64_t>(row0 + n, 1);
    if (need > h->groups_cap) {  // grow by doubling: contents kept, new entries -1
        const int64_t cap = std::max(need, 2 * h->groups_cap);
        int32_t* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, (size_t)cap * 4));
        hipError_t e = hipMemsetAsync(p, 0xFF, (size_t)cap * 4, h->stream);
        if (e == hipSuccess && h->groups_cap > 0)
            e = hipMemcpyAsync(p, h->groups, (size_t)h->groups_cap * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_err(HR_E_HIP, std::string("group column: ") + hipGetErrorString(e));
        }
        if (h->groups) (void)hipFree(h->groups);
        h->groups = p;
        h->groups_cap = cap;
    }
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(h->groups + row0, groups, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->n_groups = std::max(h->n_groups, (int64_t)top + 1);
    return HR_OK;
}

extern "C" int hr_index_search_collapsed_device(hr_index* h, const float* q_dev, int B, int k, int probe,
                                                const uint64_t* row_mask_dev, float* scores_out_dev,
                                                int64_t* rows_out_dev, void* stream) {
    if (!h || !q_dev || !scores_out_dev || !rows_out_dev) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_handle(h)) return rc;
    if (int rc = set_device(h)) return rc;
    return collapsed_impl(h, q_dev, B, k, probe, row_mask_dev, scores_out_dev, rows_out_dev, (hipStream_t)stream);
}

extern "C" int hr_index_search_collapsed(hr_index* h, const float* q, int B, int k, int probe, const uint64_t* row_mask,
                                         float* scores_out, int64_t* rows_out) {
    if (!h || !q || !scores_out || !rows_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_handle(h)) return rc;
    if (int rc = set_device(h)) return rc;
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (k <= 0 || k > HR_MAX_K) return set_err(HR_E_INVALID, "k must be in [1, HR_MAX_K]");
    hipStream_t st = h->stream;
    OutSeg out[2] = {{scores_out, (size_t)B * k * 4}, {rows_out, (size_t)B * k * 8}};
    float* q_dev = nullptr;
    uint64_t* m_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    if (int rc = stage_mask(h, row_mask, st, &m_dev)) return rc;
    if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    if (int rc = collapsed_impl(h, q_dev, B, k, probe, m_dev, out[0].as<float>(), out[1].as<int64_t>(), st)) return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_collapse_stats(hr_index* h, int64_t out[2]) {
    if (!h || !out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->n_collapse_probe;
    out[1] = h->n_collapse_all;
    return HR_OK;
}

extern "C" int hr_index_set_collapse_timing(hr_index* h, int on) {
    if (!h) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->collapse_timing = on != 0;
    return HR_OK;
}

extern "C" int hr_index_collapse_last_ms(hr_index* h, double out[3]) {
    if (!h || !out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < 3; ++i) out[i] = h->col_ms[i];
    return HR_OK;
}
