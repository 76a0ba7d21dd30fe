// hr_boost.hip -- boosted search: the exact top-k of v(r) = alpha * s(r) + sum_c beta[c] * b_c(r) over the whole
// collection, s the canonical fp64 score and b_c per-row fp32 boost columns (Elasticsearch
// function_score / rank_feature, Qdrant's score-boosting formula, Vespa rank profiles; the reference's memory search
// re-ranks a guessed similarity window on the host, memory_toolkit.py:865-924; tests/boost_ref.py restates all of it).
//
//   columns    up to HR_BOOST_MAX_COLS device arrays of one fp32 per row, allocated by their first set, grown by
//              doubling, new entries 0.0; rows at or beyond a column's capacity read 0.0 (boost_at)
//   pilot      the exact search for P rows (index_search_locked); the pool's rows rescored in fp64 -> the keys of
//              their true v (k_boost_rescore); tau = the k-th largest (k_boost_floor), -inf with fewer than k rows
//   floor      bext_c = the column's largest (beta >= 0) or smallest (beta < 0) value over rows [0, n), a device
//              reduction without atomics (k_boost_extrema, two launches) cached on the handle; Vmax(x) = the blend
//              with every b_c := bext_c, non-decreasing in x and >= v(r) at x = s(r); t0 = the smallest fp32 with
//              Vmax(t0) >= tau by bisection over the ordered fp32 bit patterns (k_boost_floor, thread 0 of the
//              query's wave); t = nextafterf(t0, -inf): every row with v >= tau has (float)s >= t
//   stage 1    the range search at min_score = t with max_hits = window (range_impl, hr_range.hip): a query whose
//              exact count is <= window has every candidate in hand; k_boost_rescore (one wave per record) and
//              k_boost_order (one workgroup per query: bitonic sort by (v key desc, row asc) in LDS, first k out)
//   stage 2    a query whose count exceeds the window, one at a time: exact_all_keys, k_boost_rekey (score key ->
//              key of v in place, the fp32 score kept aside), rocPRIM select of the rows with v >= tau, a stable
//              descending radix sort of THOSE rows, k_boost_take.  No n-row sort.
//
// Every product and sum of the blend is rounded once (boost_blend: contraction off, operands opaque); no
// floating-point atomics; the LDS compaction's integer counter only decides where a record waits for the sort.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "hr_internal.hpp"

namespace {

constexpr int kBoostChunk = 256;        // queries of one pass: bounds the window workspace (20 bytes per slot)
constexpr int kBoostDefaultWindow = 4096;
constexpr int kBoostExtBlocks = 1024;   // partial extrema of the first reduction launch

struct BoostW {  // the weights, and for the floor kernel the columns' extrema
    double alpha;
    double beta[HR_BOOST_MAX_COLS];
    double bext[HR_BOOST_MAX_COLS];
    int n_cols;
};
struct BoostCols {
    const float* p[HR_BOOST_MAX_COLS];
    int64_t cap[HR_BOOST_MAX_COLS];
};

__device__ inline double boost_at(const BoostCols& c, int i, int64_t r) {
    return r < c.cap[i] ? (double)c.p[i][r] : 0.0;
}

// (...((alpha * s) + beta[0] * b[0]) + beta[1] * b[1]) ...): one rounding per product and per sum, in column order.
// The library is built with -ffp-contract=fast: contraction is off here and every product passes through an empty
// asm, as mmr_value (hr_mmr.hip), so nothing is left to fuse.
__device__ inline double boost_blend(const BoostW& w, double s, const double* b) {
#pragma clang fp contract(off)
    double v = w.alpha * s;
    asm volatile("" : "+v"(v));
    for (int c = 0; c < w.n_cols; ++c) {
        double p = w.beta[c] * b[c];
        asm volatile("" : "+v"(p));
        v = v + p;
        asm volatile("" : "+v"(v));
    }
    return v;
}

__device__ inline uint64_t boost_key(const BoostW& w, const BoostCols& cols, double s, int64_t r) {
    double b[HR_BOOST_MAX_COLS];
#pragma unroll
    for (int c = 0; c < HR_BOOST_MAX_COLS; ++c) b[c] = c < w.n_cols ? boost_at(cols, c, r) : 0.0;
    const double v = boost_blend(w, s, b);
    return v != v ? 0 : d2key(v);
}

// ---------------------------------------------------------------- extrema
// smallest of lo_in[0, m) and largest of hi_in[0, m) per block (m > 0): min / max are exact and order-free, so the
// wave shuffle and the LDS step give the same bits whatever the schedule.  The second launch (one block) reduces the
// first one's partials.
__global__ __launch_bounds__(256) void k_boost_extrema(const float* __restrict__ lo_in, const float* __restrict__ hi_in,
                                                       int64_t m, float* __restrict__ lo_out,
                                                       float* __restrict__ hi_out) {
    __shared__ float wl[4], wh[4];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        lo = fminf(lo, lo_in[i]);
        hi = fmaxf(hi, hi_in[i]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        wl[threadIdx.x >> 6] = lo;
        wh[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo_out[blockIdx.x] = fminf(fminf(wl[0], wl[1]), fminf(wl[2], wl[3]));
        hi_out[blockIdx.x] = fmaxf(fmaxf(wh[0], wh[1]), fmaxf(wh[2], wh[3]));
    }
}

// ---------------------------------------------------------------- rescore
// One wave per record: grid (gx, queries), the gx * 4 waves of a query stride over its records recs[q][0, m), m =
// cnt[q] (cnt == nullptr: stride); a query with cnt[q] > lim is stage 2's and skipped.  keys[q][i] = the key of v of
// record i, 0 for padding (row < 0) or a NaN v.
template <int DT>
__global__ __launch_bounds__(256) void k_boost_rescore(const uint8_t* __restrict__ rows, int S, int dpad,
                                                       const float* __restrict__ q32, const double* __restrict__ qerr,
                                                       int metric, const int64_t* __restrict__ recs, int stride,
                                                       const int64_t* __restrict__ cnt, int lim, int64_t n, BoostW w,
                                                       BoostCols cols, uint64_t* __restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.y;
    const int64_t c = cnt ? cnt[q] : (int64_t)stride;
    if (c > lim) return;
    const uint32_t m = (uint32_t)c;
    const double qn2 = qerr[4 * q + 2];
    const float* qv = q32 + (int64_t)q * dpad;
    const uint32_t step = gridDim.x * 4;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += step) {
        const int64_t r = recs[(int64_t)q * stride + i];
        uint64_t key = 0;
        if (r >= 0 && r < n) {  // (wave-uniform)
            const double s = canonical_score<DT>(rows, S, dpad, qv, metric, qn2, r, lane);
            key = boost_key(w, cols, s, r);
        }
        if (lane == 0) keys[(int64_t)q * stride + i] = key;
    }
}

// ---------------------------------------------------------------- tau and the similarity floor
// One wave per query.  pkeys[q][0, P): the v keys of the pilot pool (0: not a candidate).  tau = the k-th largest
// (rank by (key desc, position asc), every lane ranks the positions it owns), -inf when that key is 0; thread 0
// then finds t0 by bisection over the ordered fp32 keys [f2key(-inf), f2key(+inf)] -- Vmax(+inf) = +inf >= tau
// always, Vmax is non-decreasing -- and writes t = nextafterf(t0, -inf).
__global__ __launch_bounds__(64) void k_boost_floor(const uint64_t* __restrict__ pkeys, int P, int k, BoostW w,
                                                    double* __restrict__ tau_out, uint64_t* __restrict__ taukey_out,
                                                    float* __restrict__ t_out) {
    __shared__ uint64_t ks[HR_MAX_K];
    __shared__ uint64_t kth;
    const int q = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < P; i += 64) ks[i] = pkeys[(int64_t)q * P + i];
    __syncthreads();
    for (int i = lane; i < P; i += 64) {
        const uint64_t a = ks[i];
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const uint64_t b = ks[j];
            rank += (b > a || (b == a && j < i)) ? 1 : 0;
        }
        if (rank == k - 1) kth = a;  // exactly one position holds rank k - 1 (k <= P)
    }
    __syncthreads();
    if (lane != 0) return;
    const uint64_t tk = kth;
    const double tau = tk ? key2d(tk) : -__builtin_inf();
    uint32_t lo = HR_KEY_NEG_INF, hi = 0xFF800000u;  // f2key(-inf), f2key(+inf)
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (boost_blend(w, (double)key2f(mid), w.bext) >= tau)
            hi = mid;
        else
            lo = mid + 1;
    }
    tau_out[q] = tau;
    taukey_out[q] = d2key(tau);
    t_out[q] = nextafterf(key2f(lo), -__builtin_inff());
}

// ---------------------------------------------------------------- stage 1: order
// One workgroup per query; a query whose count exceeds lim is left to stage 2.  The window's records with a non-zero
// key are compacted into LDS -- key, row and window position, 16 bytes each, p2 (a power of two >= lim) slots: at most
// 128 KiB, dynamic -- sorted by (key desc, row asc), and the first k written: v, the fp32 score the range search
// returned at that position, the row; -inf / -inf / -1 after them.
__global__ __launch_bounds__(1024) void k_boost_order(const int64_t* __restrict__ cnt, int lim, int p2cap,
                                                      const uint64_t* __restrict__ keys,
                                                      const int64_t* __restrict__ win_r, const float* __restrict__ win_s,
                                                      int k, double* __restrict__ v_out, float* __restrict__ s_out,
                                                      int64_t* __restrict__ r_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int nh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t c = cnt[q];
    if (c > lim) return;
    const int m = (int)c;
    uint64_t* ks = (uint64_t*)smem;
    uint32_t* rs = (uint32_t*)(ks + p2cap);
    uint32_t* ps = rs + p2cap;
    if (tid == 0) nh = 0;
    __syncthreads();
    for (int i = tid; i < m; i += blockDim.x) {
        const uint64_t key = keys[(int64_t)q * lim + i];
        if (key) {
            const int pos = atomicAdd(&nh, 1);
            ks[pos] = key;
            rs[pos] = (uint32_t)win_r[(int64_t)q * lim + i];
            ps[pos] = (uint32_t)i;
        }
    }
    __syncthreads();
    const int hits = nh;
    int p2 = 1;
    while (p2 < hits) p2 <<= 1;
    for (int i = hits + tid; i < p2; i += blockDim.x) {
        ks[i] = 0;
        rs[i] = 0xFFFFFFFFu;
        ps[i] = 0;
    }
    __syncthreads();
    // records arrive in atomic order: (key desc, row asc) is established here, rows are distinct
    for (int kk = 2; kk <= p2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < p2; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = ks[i], b = ks[ixj];
                    const uint32_t ra = rs[i], rb = rs[ixj];
                    const bool a_first = a > b || (a == b && ra < rb);
                    const bool desc = (i & kk) == 0;
                    if (desc ? !a_first : a_first) {
                        const uint32_t pa = ps[i], pb = ps[ixj];
                        ks[i] = b;
                        ks[ixj] = a;
                        rs[i] = rb;
                        rs[ixj] = ra;
                        ps[i] = pb;
                        ps[ixj] = pa;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < k; i += blockDim.x) {
        const bool hit = i < hits;
        v_out[(int64_t)q * k + i] = hit ? key2d(ks[i]) : -__builtin_inf();
        s_out[(int64_t)q * k + i] = hit ? win_s[(int64_t)q * lim + ps[i]] : -__builtin_inff();
        r_out[(int64_t)q * k + i] = hit ? (int64_t)rs[i] : -1;
    }
}

// ---------------------------------------------------------------- stage 2
// keys[r]: d2key(canonical score) of a live, allowed row, else 0 (exact_all_keys) -> the key of v(r), 0 stays 0 and a
// NaN v becomes 0; s32[r] = the fp32 score hr_index_search returns for the row
__global__ __launch_bounds__(256) void k_boost_rekey(uint64_t* __restrict__ keys, int64_t n, BoostW w, BoostCols cols,
                                                     float* __restrict__ s32) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t key = keys[r];
    if (!key) return;
    const double s = key2d(key);
    s32[r] = (float)s;
    keys[r] = boost_key(w, cols, s, r);
}

struct BoostHit {  // row i has v >= tau
    const uint64_t* keys;
    const uint64_t* taukey;
    __device__ bool operator()(uint32_t i) const {
        const uint64_t key = keys[i];
        return key != 0 && key >= *taukey;
    }
};

__global__ __launch_bounds__(256) void k_boost_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                      int64_t hits, uint64_t* __restrict__ k_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < hits) k_out[i] = keys[idx[i]];
}

// the first k of the sorted hits, padding after them (keys == nullptr: padding only)
__global__ __launch_bounds__(256) void k_boost_take(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    int64_t hits, int k, const float* __restrict__ s32,
                                                    double* __restrict__ v_out, float* __restrict__ s_out,
                                                    int64_t* __restrict__ r_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const bool hit = keys && i < hits;
    v_out[i] = hit ? key2d(keys[i]) : -__builtin_inf();
    s_out[i] = hit ? s32[vals[i]] : -__builtin_inff();
    r_out[i] = hit ? (int64_t)vals[i] : -1;
}

dim3 grid_for(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)); }

int pad_boosted(double* v_out, float* s_out, int64_t* r_out, int64_t slots, hipStream_t st) {
    for (int64_t i = 0; i < slots; i += HR_MAX_K) {  // (k_boost_take pads one list of <= HR_MAX_K slots)
        const int m = (int)std::min<int64_t>(HR_MAX_K, slots - i);
        hipLaunchKernelGGL(k_boost_take, dim3(1), dim3(256), 0, st, (const uint64_t*)nullptr, (const uint32_t*)nullptr,
                           (int64_t)0, m, (const float*)nullptr, v_out + i, s_out + i, r_out + i);
    }
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

// the extrema of column c over rows [0, n): cached until the column is written or the index grows
int column_extrema(hr_index* h, int c, hipStream_t st) {
    if (h->boost_ext_n[c] == h->n) return HR_OK;
    float lo = 0.f, hi = 0.f;
    const int64_t m = std::min(h->n, h->boost_cap[c]);
    if (m > 0) {
        HIP_TRY(h->bst_tmp.ensure((size_t)(2 * kBoostExtBlocks + 2) * 4));
        float* part = h->bst_tmp.as<float>();
        const int blocks = (int)std::min<int64_t>(kBoostExtBlocks, (m + 255) / 256);
        hipLaunchKernelGGL(k_boost_extrema, dim3((unsigned)blocks), dim3(256), 0, st, h->boost[c], h->boost[c], m, part,
                           part + kBoostExtBlocks);
        hipLaunchKernelGGL(k_boost_extrema, dim3(1), dim3(256), 0, st, part, part + kBoostExtBlocks, (int64_t)blocks,
                           part + 2 * kBoostExtBlocks, part + 2 * kBoostExtBlocks + 1);
        HIP_TRY(hipGetLastError());
        float two[2];
        HIP_TRY(hipMemcpyAsync(two, part + 2 * kBoostExtBlocks, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lo = two[0];
        hi = two[1];
    }
    if (m < h->n || m == 0) {  // rows the column does not cover read 0.0
        lo = m > 0 ? std::min(lo, 0.f) : 0.f;
        hi = m > 0 ? std::max(hi, 0.f) : 0.f;
    }
    h->boost_ext_lo[c] = lo;
    h->boost_ext_hi[c] = hi;
    h->boost_ext_n[c] = h->n;
    return HR_OK;
}

// one stage-2 query: keys / vals / s32 of the n rows are in h->bst_keys; the rows with v >= tau sorted, first k out
int all_rows_tail(hr_index* h, uint64_t* keys, const float* s32, uint32_t* idx, void* sel_tmp_p, size_t sel_tmp,
                  const uint64_t* taukey, int k, double* v_out, float* s_out, int64_t* r_out, hipStream_t st) {
    uint32_t* sel_count = h->bst_tmp.as<uint32_t>();
    const BoostHit pred{keys, taukey};
    HIP_TRY(rocprim::select(sel_tmp_p, sel_tmp, rocprim::counting_iterator<uint32_t>(0), idx, sel_count, (size_t)h->n,
                            pred, st));
    uint32_t hits = 0;
    HIP_TRY(hipMemcpyAsync(&hits, sel_count, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hits == 0) return pad_boosted(v_out, s_out, r_out, k, st);
    size_t sort_tmp = 0;
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (size_t)hits, 0, 64, st));
    const size_t k8 = up256(8 * (size_t)hits), v4 = up256(4 * (size_t)hits);
    HIP_TRY(h->bst_sort.ensure(2 * k8 + v4 + up256(sort_tmp)));
    uint8_t* p = h->bst_sort.as<uint8_t>();
    uint64_t* k_a = (uint64_t*)p;
    uint64_t* k_b = (uint64_t*)(p + k8);
    uint32_t* v_b = (uint32_t*)(p + 2 * k8);
    hipLaunchKernelGGL(k_boost_gather, grid_for(hits), dim3(256), 0, st, keys, idx, (int64_t)hits, k_a);
    HIP_TRY(hipGetLastError());
    // idx is row-ascending and the sort stable: equal keys keep row-ascending order
    HIP_TRY(rocprim::radix_sort_pairs_desc(p + 2 * k8 + v4, sort_tmp, k_a, k_b, idx, v_b, (size_t)hits, 0, 64, st));
    hipLaunchKernelGGL(k_boost_take, dim3(1), dim3(256), 0, st, k_b, v_b, (int64_t)hits, k, s32, v_out, s_out, r_out);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

// at most kBoostChunk queries; everything on h's device, the caller holds h->mu with the device current and has
// checked the arguments.  Returns with st idle.
int boost_chunk(hr_index* h, const float* q_dev, int B, int k, const BoostW& w, const BoostCols& cols, int P, int W,
                const uint64_t* mask_dev, double* v_out, float* s_out, int64_t* r_out, hipStream_t st) {
    // ---- pilot
    HIP_TRY(h->pool_s.ensure((size_t)B * P * 4));
    HIP_TRY(h->pool_r.ensure((size_t)B * P * 8));
    if (int rc = index_search_locked(h, q_dev, B, P, mask_dev, h->pool_s.as<float>(), h->pool_r.as<int64_t>(), st))
        return rc;
    const size_t o_wr = 0, o_wk = o_wr + up256((size_t)B * W * 8), o_ws = o_wk + up256((size_t)B * W * 8),
                 o_pk = o_ws + up256((size_t)B * W * 4), o_c = o_pk + up256((size_t)B * P * 8),
                 o_tau = o_c + up256((size_t)B * 8), o_tk = o_tau + up256((size_t)B * 8),
                 o_t = o_tk + up256((size_t)B * 8), total = o_t + up256((size_t)B * 4);
    HIP_TRY(h->bst_win.ensure(total));
    uint8_t* base = h->bst_win.as<uint8_t>();
    int64_t* win_r = (int64_t*)(base + o_wr);
    uint64_t* win_k = (uint64_t*)(base + o_wk);
    float* win_s = (float*)(base + o_ws);
    uint64_t* pkeys = (uint64_t*)(base + o_pk);
    int64_t* win_c = (int64_t*)(base + o_c);
    double* tau = (double*)(base + o_tau);
    uint64_t* taukey = (uint64_t*)(base + o_tk);
    float* t_dev = (float*)(base + o_t);
    const float* q32 = nullptr;
    std::vector<double> qerr;
    if (int rc = index_prep_exact(h, q_dev, B, st, &q32, &qerr)) return rc;
    const double* qerr_dev = h->scr[kSyncSet].qerr.as<double>();
    auto rescore = [&](const int64_t* recs, int stride, const int64_t* cnt, int lim, uint64_t* keys) -> int {
        const dim3 grid((unsigned)std::min(256, (stride + 3) / 4), (unsigned)B);
        return dispatch_dt(h->dtype, [&](auto dt) -> int {
            hipLaunchKernelGGL((k_boost_rescore<decltype(dt)::value>), grid, dim3(256), 0, st, h->rows, h->S, h->dpad,
                               q32, qerr_dev, h->metric, recs, stride, cnt, lim, h->n, w, cols, keys);
            HIP_TRY(hipGetLastError());
            return HR_OK;
        });
    };
    if (int rc = rescore(h->pool_r.as<int64_t>(), P, nullptr, P, pkeys)) return rc;
    // ---- tau and the floor
    hipLaunchKernelGGL(k_boost_floor, dim3((unsigned)B), dim3(64), 0, st, pkeys, P, k, w, tau, taukey, t_dev);
    HIP_TRY(hipGetLastError());
    // ---- stage 1: the window (returns with st idle; its own stages keep the count exact whatever it is)
    if (int rc = range_impl(h, q_dev, B, t_dev, W, mask_dev, win_s, win_r, win_c, st)) return rc;
    std::vector<int64_t> cnt((size_t)B);
    HIP_TRY(hipMemcpyAsync(cnt.data(), win_c, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    if (int rc = index_prep_exact(h, q_dev, B, st, &q32, &qerr)) return rc;  // (the scans reused the workspace)
    qerr_dev = h->scr[kSyncSet].qerr.as<double>();
    std::vector<int> todo;
    for (int b = 0; b < B; ++b)
        if (cnt[(size_t)b] > W) todo.push_back(b);
    h->n_boost_window += B - (int64_t)todo.size();
    h->n_boost_all += (int64_t)todo.size();
    if ((int)todo.size() < B) {
        if (int rc = rescore(win_r, W, win_c, W, win_k)) return rc;
        int p2 = 1024;
        while (p2 < W) p2 <<= 1;
        static bool order_attr[64] = {};  // per device, set once
        if (!order_attr[h->device & 63]) {
            HIP_TRY(hipFuncSetAttribute((const void*)k_boost_order, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        HR_BOOST_MAX_WINDOW * 16));
            order_attr[h->device & 63] = true;
        }
        hipLaunchKernelGGL(k_boost_order, dim3((unsigned)B), dim3(1024), (size_t)p2 * 16, st, win_c, W, p2, win_k, win_r,
                           win_s, k, v_out, s_out, r_out);
        HIP_TRY(hipGetLastError());
    }
    // ---- stage 2
    if (!todo.empty()) {
        const int64_t n = h->n;
        size_t sel_tmp = 0;
        HIP_TRY(rocprim::select(nullptr, sel_tmp, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr,
                                (uint32_t*)nullptr, (size_t)n, BoostHit{nullptr, nullptr}, st));
        const size_t k8 = up256(8 * (size_t)n), v4 = up256(4 * (size_t)n);
        HIP_TRY(h->bst_keys.ensure(k8 + 3 * v4 + up256(sel_tmp)));
        HIP_TRY(h->bst_tmp.ensure((size_t)(2 * kBoostExtBlocks + 2) * 4));
        uint8_t* p = h->bst_keys.as<uint8_t>();
        uint64_t* akeys = (uint64_t*)p;
        uint32_t* avals = (uint32_t*)(p + k8);
        float* s32 = (float*)(p + k8 + v4);
        uint32_t* idx = (uint32_t*)(p + k8 + 2 * v4);
        void* sel_tmp_p = p + k8 + 3 * v4;
        for (int b : todo) {
            if (int rc = exact_all_keys(h->rows, h->dtype, h->S, h->dpad, q32 + (int64_t)b * h->dpad, h->metric,
                                        qerr[4 * (size_t)b + 2], h->live, (const uint32_t*)mask_dev, n, akeys, avals, st))
                return set_err(rc, "all-rows exact pass failed");
            hipLaunchKernelGGL(k_boost_rekey, grid_for(n), dim3(256), 0, st, akeys, n, w, cols, s32);
            HIP_TRY(hipGetLastError());
            if (int rc = all_rows_tail(h, akeys, s32, idx, sel_tmp_p, sel_tmp, taukey + b, k, v_out + (int64_t)b * k,
                                       s_out + (int64_t)b * k, r_out + (int64_t)b * k, st))
                return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

int boost_impl(hr_index* h, const float* q_dev, int B, int k, double alpha, const double* beta, int n_cols, int probe,
               int window, const uint64_t* mask_dev, double* v_out, float* s_out, int64_t* r_out, hipStream_t st) {
    if (h->n_live == 0 || h->n <= 0) {  // empty index: padding
        if (int rc = pad_boosted(v_out, s_out, r_out, (int64_t)B * k, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        h->n_boost_window += B;
        return HR_OK;
    }
    const int P = probe ? probe : std::min(HR_MAX_K, std::max(32, 4 * k));
    const int W = window ? window : std::max(k, kBoostDefaultWindow);
    BoostW w{};
    BoostCols cols{};
    w.alpha = alpha;
    w.n_cols = n_cols;
    for (int c = 0; c < n_cols; ++c) {
        if (int rc = column_extrema(h, c, st)) return rc;
        w.beta[c] = beta[c];
        w.bext[c] = (double)(beta[c] >= 0.0 ? h->boost_ext_hi[c] : h->boost_ext_lo[c]);
        cols.p[c] = h->boost[c];
        cols.cap[c] = h->boost_cap[c];
    }
    for (int b0 = 0; b0 < B; b0 += kBoostChunk) {
        const int bc = std::min(kBoostChunk, B - b0);
        if (int rc = boost_chunk(h, q_dev + (int64_t)b0 * h->dim, bc, k, w, cols, P, W, mask_dev, v_out + (int64_t)b0 * k,
                                 s_out + (int64_t)b0 * k, r_out + (int64_t)b0 * k, st))
            return rc;
    }
    return HR_OK;
}

// every limit that needs no handle, before the handle is looked at
int check_args(int B, int k, double alpha, const double* beta, int n_cols, int probe, int window) {
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (k <= 0 || k > HR_MAX_K) return set_err(HR_E_INVALID, "k must be in [1, HR_MAX_K]");
    if (!(alpha >= 0x1p-64 && alpha <= 0x1p64)) return set_err(HR_E_INVALID, "alpha must be in [2^-64, 2^64]");
    if (n_cols < 0 || n_cols > HR_BOOST_MAX_COLS) return set_err(HR_E_INVALID, "n_cols must be in [0, HR_BOOST_MAX_COLS]");
    if (n_cols > 0 && !beta) return set_err(HR_E_INVALID, "null argument");
    for (int c = 0; c < n_cols; ++c)
        if (!(std::fabs(beta[c]) <= 0x1p64)) return set_err(HR_E_INVALID, "|beta| must be at most 2^64");
    if (probe != 0 && (probe < k || probe > HR_MAX_K)) return set_err(HR_E_INVALID, "probe must be 0 or in [k, HR_MAX_K]");
    if (window != 0 && (window < k || window > HR_BOOST_MAX_WINDOW))
        return set_err(HR_E_INVALID, "window must be 0 or in [k, HR_BOOST_MAX_WINDOW]");
    return HR_OK;
}

}  // namespace

void boost_free(hr_index* h) {
    for (int c = 0; c < HR_BOOST_MAX_COLS; ++c) {
        if (h->boost[c]) (void)hipFree(h->boost[c]);
        h->boost[c] = nullptr;
        h->boost_cap[c] = 0;
        h->boost_ext_n[c] = -1;
    }
    for (DevBuf* b : {&h->bst_win, &h->bst_keys, &h->bst_sort, &h->bst_tmp}) b->release();
}

extern "C" int hr_index_set_boost(hr_index* h, int col, int64_t row0, int64_t n, const float* values) {
    if (col < 0 || col >= HR_BOOST_MAX_COLS) return set_err(HR_E_INVALID, "col must be in [0, HR_BOOST_MAX_COLS)");
    if (n > 0 && values)
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(values[i])) return set_err(HR_E_INVALID, "boost values must be finite");
    if (!h || (n > 0 && !values)) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "boosted search needs a single-device handle");
    if (row0 < 0 || n < 0 || row0 > h->n || n > h->n - row0)
        return set_err(HR_E_INVALID, "rows [row0, row0 + n) must lie inside the index");
    if (int rc = set_device(h)) return rc;
    const int64_t need = std::max<int64_t>(row0 + n, 1);
    if (need > h->boost_cap[col]) {  // grow by doubling: contents kept, new entries 0.0
        const int64_t cap = std::max(need, 2 * h->boost_cap[col]);
        float* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, (size_t)cap * 4));
        hipError_t e = hipMemsetAsync(p, 0, (size_t)cap * 4, h->stream);
        if (e == hipSuccess && h->boost_cap[col] > 0)
            e = hipMemcpyAsync(p, h->boost[col], (size_t)h->boost_cap[col] * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_err(HR_E_HIP, std::string("boost column: ") + hipGetErrorString(e));
        }
        if (h->boost[col]) (void)hipFree(h->boost[col]);
        h->boost[col] = p;
        h->boost_cap[col] = cap;
    }
    h->boost_ext_n[col] = -1;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(h->boost[col] + row0, values, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return HR_OK;
}

extern "C" int hr_index_search_boosted_device(hr_index* h, const float* q_dev, int B, int k, double alpha,
                                              const double* beta, int n_cols, int probe, int window,
                                              const uint64_t* row_mask_dev, double* blended_out_dev,
                                              float* scores_out_dev, int64_t* rows_out_dev, void* stream) {
    if (int rc = check_args(B, k, alpha, beta, n_cols, probe, window)) return rc;
    if (!h || !q_dev || !blended_out_dev || !scores_out_dev || !rows_out_dev)
        return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "boosted search needs a single-device handle");
    if (int rc = set_device(h)) return rc;
    return boost_impl(h, q_dev, B, k, alpha, beta, n_cols, probe, window, row_mask_dev, blended_out_dev, scores_out_dev,
                      rows_out_dev, (hipStream_t)stream);
}

extern "C" int hr_index_search_boosted(hr_index* h, const float* q, int B, int k, double alpha, const double* beta,
                                       int n_cols, int probe, int window, const uint64_t* row_mask, double* blended_out,
                                       float* scores_out, int64_t* rows_out) {
    if (int rc = check_args(B, k, alpha, beta, n_cols, probe, window)) return rc;
    if (!h || !q || !blended_out || !scores_out || !rows_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "boosted search needs a single-device handle");
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    const size_t nk = (size_t)B * k;
    OutSeg out[3] = {{blended_out, nk * 8}, {scores_out, nk * 4}, {rows_out, nk * 8}};
    float* q_dev = nullptr;
    uint64_t* m_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    if (int rc = stage_mask(h, row_mask, st, &m_dev)) return rc;
    if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    if (int rc = boost_impl(h, q_dev, B, k, alpha, beta, n_cols, probe, window, m_dev, out[0].as<double>(),
                            out[1].as<float>(), out[2].as<int64_t>(), st))
        return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_boost_stats(hr_index* h, int64_t out[2]) {
    if (!h || !out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->n_boost_window;
    out[1] = h->n_boost_all;
    return HR_OK;
}
