// hr_range.hip -- range search: every live, allowed row whose fp32 score is at least the caller's threshold, with
// the exact count, in the order every search uses (FAISS range_search, Milvus / Qdrant score-threshold
// search).
//
//   stage 1 (window)    per chunk of Plan::Bp queries: query prep, k_range_floors (floor = the largest fp64 value
//                       below the threshold, minus the guard's E_q, in scan-score space, rounded down to fp32 -- on
//                       the stream, nothing waits on the host), ONE collect pass of the 16-bit rows appending every
//                       row with approx >= floor into the query's region of cap = max(1024, 2 max_hits) records
//                       (shard_chunk mode 2), then the ragged tail: k_range_rescore (one wave per appended record:
//                       canonical fp64 score -> order-preserving key, 0 below the threshold or NaN) and
//                       k_range_order (one workgroup per query: hits compacted into LDS, bitonic sort by (key desc,
//                       row asc), first max_hits out, padding, the count).  A region holding more than kRangeLds
//                       records is ordered through rocPRIM instead (row-ascending sort, then stage 2's tail).  A
//                       region that overflowed is never used: the query goes to stage 2.
//   stage 2 (all rows)  flagged queries only, one at a time: the canonical key of every live, allowed row
//                       (exact_all_keys, hr_exhaustive.hip -- the arithmetic stays there alone), k_range_count (the
//                       exact count; a count-only call ends here), rocPRIM select of the hits in row order, a stable
//                       descending radix sort of the HITS (stability keeps row-ascending order), k_range_take.
//
// Workspace: 16 bytes per region record (h->rng_arena); stage 2 12 bytes per index row (h->rng_keys) plus 28 bytes
// per hit of the one query being sorted (h->rng_sort).
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "hr_internal.hpp"

namespace {

constexpr int kRangeLds = 8192;  // records one workgroup orders in LDS (12 bytes each: 96 KiB of the CU's 160)

// ---------------------------------------------------------------- floors
// One thread per padded query.  Every hit has fp64 score > lo = nextafterf(t, -inf) (the fp32 cast is monotone), and
// approx >= exact - E_q, so approx >= floor: what mode 1 of shard_chunk does with kth - E on the host.
__global__ __launch_bounds__(256) void k_range_floors(const double* __restrict__ qerr, const float* __restrict__ t,
                                                      int B, int Bp, double max_norm, double gamma, double u_x,
                                                      int metric, float* __restrict__ floor_q) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= Bp) return;
    if (b >= B) {  // padded queries never collect
        floor_q[b] = __builtin_inff();
        return;
    }
    const double E = guard_e(qerr + 4 * b, max_norm, gamma, u_x, metric);
    double lo = (double)nextafterf(t[b], -__builtin_inff());
    if (metric == L2) {  // similarity -> scan-score space, minus the rounding slack
        const double qn2 = qerr[4 * b + 2];
        lo = (lo - (1.0 - qn2)) - E - euclid_slack(qn2, max_norm);
    } else {
        lo = lo - E;
    }
    float f = (float)lo;
    if ((double)f > lo) f = nextafterf(f, -__builtin_inff());
    floor_q[b] = f;
}

// ---------------------------------------------------------------- stage 1 tail
// One wave per appended record, ragged over the per-query counts: grid (gx, chunk queries), the gx * 4 waves of a
// query stride over its cnt[q] records; an overflowed region (cnt > cap) is skipped.  keys[q][i] = d2key(score) of
// record i, or 0 when its fp32 cast is below the threshold or the score is NaN.
template <int DT>
__global__ __launch_bounds__(256) void k_range_rescore(const uint8_t* __restrict__ rows, int S, int dpad,
                                                       const float* __restrict__ q32, const double* __restrict__ qerr,
                                                       int metric, const uint32_t* __restrict__ cnt,
                                                       const float2* __restrict__ buf, int cap,
                                                       const float* __restrict__ t, int64_t n,
                                                       uint64_t* __restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.y;
    const uint32_t m = cnt[q];
    if (m > (uint32_t)cap) return;
    const float tq = t[q];
    const double qn2 = qerr[4 * q + 2];
    const float* qv = q32 + (int64_t)q * dpad;
    const uint32_t stride = gridDim.x * 4;
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < m; i += stride) {
        const int64_t r = (int64_t)__builtin_bit_cast(uint32_t, buf[(int64_t)q * cap + i].y);
        uint64_t key = 0;
        if (r < n) {
            const double p = canonical_score<DT>(rows, S, dpad, qv, metric, qn2, r, lane);
            if ((float)p >= tq) key = d2key(p);  // (false for a NaN score)
        }
        if (lane == 0) keys[(int64_t)q * cap + i] = key;
    }
}

// One workgroup per query of the chunk.  flags[q]: 0 answered here, 1 region overflowed (stage 2), 2 region beyond
// lds_cap records (ordered through rocPRIM by the host).  LDS: lds_p2 (lds_cap rounded up to a power of two) keys and
// as many rows (dynamic), and the hit counter.
__global__ __launch_bounds__(1024) void k_range_order(const uint32_t* __restrict__ cnt, const float2* __restrict__ buf,
                                                      const uint64_t* __restrict__ keys, int cap, int lds_cap,
                                                      int lds_p2, int max_hits, float* __restrict__ s_out,
                                                      int64_t* __restrict__ r_out, int64_t* __restrict__ c_out,
                                                      int32_t* __restrict__ flags, uint32_t* __restrict__ cnt_out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int nh;
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = cnt[q];
    if (tid == 0) {
        cnt_out[q] = m;
        flags[q] = m > (uint32_t)cap ? 1 : (m > (uint32_t)lds_cap ? 2 : 0);
        nh = 0;
    }
    if (m > (uint32_t)cap || m > (uint32_t)lds_cap) return;
    uint64_t* ks = (uint64_t*)smem;
    uint32_t* rs = (uint32_t*)(ks + lds_p2);
    __syncthreads();
    for (uint32_t i = tid; i < m; i += blockDim.x) {
        const uint64_t key = keys[(int64_t)q * cap + i];
        if (key) {
            const int pos = atomicAdd(&nh, 1);
            ks[pos] = key;
            rs[pos] = __builtin_bit_cast(uint32_t, buf[(int64_t)q * cap + i].y);
        }
    }
    __syncthreads();
    const int hits = nh;
    if (tid == 0) c_out[q] = hits;
    if (max_hits == 0) return;
    int p2 = 1;
    while (p2 < hits) p2 <<= 1;
    for (int i = hits + tid; i < p2; i += blockDim.x) {
        ks[i] = 0;
        rs[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    // records arrive in atomic order: (key desc, row asc) is established here, rows included
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
                        ks[i] = b;
                        ks[ixj] = a;
                        rs[i] = rb;
                        rs[ixj] = ra;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < max_hits; i += blockDim.x) {
        const bool hit = i < hits;
        s_out[(int64_t)q * max_hits + i] = hit ? (float)key2d(ks[i]) : -__builtin_inff();
        r_out[(int64_t)q * max_hits + i] = hit ? (int64_t)rs[i] : -1;
    }
}

// ---------------------------------------------------------------- stage 2 (and regions beyond the LDS)
struct RangeHit {  // element i of a key array is a hit
    const uint64_t* keys;
    const float* t;
    __device__ bool operator()(uint32_t i) const {
        const uint64_t key = keys[i];
        return key != 0 && (float)key2d(key) >= *t;
    }
};

__global__ __launch_bounds__(256) void k_range_count(const uint64_t* __restrict__ keys, int64_t n,
                                                     const float* __restrict__ t,
                                                     unsigned long long* __restrict__ total) {
    const RangeHit hit{keys, t};
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        c += hit((uint32_t)i) ? 1 : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, c);
}

__global__ __launch_bounds__(256) void k_range_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                      const uint32_t* __restrict__ idx, int64_t hits,
                                                      uint64_t* __restrict__ k_out, uint32_t* __restrict__ v_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hits) return;
    const uint32_t j = idx[i];
    k_out[i] = keys[j];
    v_out[i] = vals[j];
}

// the first max_hits of the sorted hits as fp32 / int64, padding after them (keys == nullptr: padding only)
__global__ __launch_bounds__(256) void k_range_take(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    int64_t hits, int max_hits, float* __restrict__ s_out,
                                                    int64_t* __restrict__ r_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= max_hits) return;
    const bool hit = keys && i < hits;
    s_out[i] = hit ? (float)key2d(keys[i]) : -__builtin_inff();
    r_out[i] = hit ? (int64_t)vals[i] : -1;
}

__global__ __launch_bounds__(256) void k_range_rows(const float2* __restrict__ buf, int64_t m, uint32_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) rows[i] = __builtin_bit_cast(uint32_t, buf[i].y);
}

__global__ __launch_bounds__(256) void k_range_zero(int64_t* __restrict__ c_out, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) c_out[i] = 0;
}

dim3 grid_for(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + 255) / 256)); }

// keys[i] / vals[i], i in [0, n), vals ascending: the exact count of the hits into *c_out, and (max_hits > 0) the
// first max_hits of them by (key desc, val asc) with padding.  Waits for the count on the host; t: device threshold.
int hits_sorted(hr_index* h, const uint64_t* keys, const uint32_t* vals, int64_t n, const float* t, int max_hits,
                float* s_out, int64_t* r_out, int64_t* c_out, hipStream_t st) {
    HIP_TRY(h->rng_tmp.ensure(64));
    unsigned long long* total = h->rng_tmp.as<unsigned long long>();
    uint32_t* sel_count = (uint32_t*)(total + 1);
    HIP_TRY(hipMemsetAsync(total, 0, 8, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_range_count, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, st, keys,
                           n, t, total);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long hits = 0;
    HIP_TRY(hipMemcpyAsync(c_out, total, 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(&hits, total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (max_hits == 0) return HR_OK;
    if (hits == 0) return pad_results(s_out, r_out, max_hits, st);
    size_t sel_tmp = 0, sort_tmp = 0;
    const RangeHit pred{keys, t};
    HIP_TRY(rocprim::select(nullptr, sel_tmp, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr,
                            (uint32_t*)nullptr, (size_t)n, pred, st));
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (size_t)hits, 0, 64, st));
    const size_t k8 = up256(8 * (size_t)hits), v4 = up256(4 * (size_t)hits), tmp = up256(std::max(sel_tmp, sort_tmp));
    HIP_TRY(h->rng_sort.ensure(2 * k8 + 3 * v4 + tmp));
    uint8_t* p = h->rng_sort.as<uint8_t>();
    uint64_t* k_a = (uint64_t*)p;
    uint64_t* k_b = (uint64_t*)(p + k8);
    uint32_t* v_a = (uint32_t*)(p + 2 * k8);
    uint32_t* v_b = (uint32_t*)(p + 2 * k8 + v4);
    uint32_t* idx = (uint32_t*)(p + 2 * k8 + 2 * v4);
    void* tmp_p = p + 2 * k8 + 3 * v4;
    // the count above is exact and the predicate is the same, so the selection writes `hits` entries
    HIP_TRY(rocprim::select(tmp_p, sel_tmp, rocprim::counting_iterator<uint32_t>(0), idx, sel_count, (size_t)n, pred, st));
    hipLaunchKernelGGL(k_range_gather, grid_for((int64_t)hits), dim3(256), 0, st, keys, vals, idx, (int64_t)hits, k_a, v_a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs_desc(tmp_p, sort_tmp, k_a, k_b, v_a, v_b, (size_t)hits, 0, 64, st));
    hipLaunchKernelGGL(k_range_take, grid_for(max_hits), dim3(256), 0, st, k_b, v_b, (int64_t)hits, max_hits, s_out, r_out);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

// a stage-1 region of m > kRangeLds records (not overflowed): rows ascending first, then stage 2's tail
int order_large_region(hr_index* h, const float2* buf, const uint64_t* keys, int64_t m, const float* t, int max_hits,
                       float* s_out, int64_t* r_out, int64_t* c_out, hipStream_t st) {
    size_t sort_tmp = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint64_t*)nullptr,
                                      (uint64_t*)nullptr, (size_t)m, 0, 32, st));
    const size_t k8 = up256(8 * (size_t)m), v4 = up256(4 * (size_t)m);
    HIP_TRY(h->rng_keys.ensure(k8 + 2 * v4 + up256(sort_tmp)));
    uint8_t* p = h->rng_keys.as<uint8_t>();
    uint64_t* k_sorted = (uint64_t*)p;
    uint32_t* r_sorted = (uint32_t*)(p + k8);
    uint32_t* r_in = (uint32_t*)(p + k8 + v4);
    hipLaunchKernelGGL(k_range_rows, grid_for(m), dim3(256), 0, st, buf, m, r_in);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(p + k8 + 2 * v4, sort_tmp, r_in, r_sorted, keys, k_sorted, (size_t)m, 0, 32, st));
    return hits_sorted(h, k_sorted, r_sorted, m, t, max_hits, s_out, r_out, c_out, st);
}

}  // namespace

// queries, thresholds (already validated), mask and outputs on h's device.  The caller holds h->mu with the device
// current.  Returns with st idle.  (hr_internal.hpp: the boosted search's window is this call.)
int range_impl(hr_index* h, const float* q_dev, int B, const float* t_dev, int max_hits, const uint64_t* mask_dev,
               float* s_out, int64_t* r_out, int64_t* c_out, hipStream_t st) {
    if (h->n_live == 0 || h->n <= 0) {  // empty index: counts 0 and padding
        hipLaunchKernelGGL(k_range_zero, grid_for(B), dim3(256), 0, st, c_out, B);
        HIP_TRY(hipGetLastError());
        if (max_hits > 0)
            if (int rc = pad_results(s_out, r_out, (int64_t)B * max_hits, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        h->n_range_window += B;
        return HR_OK;
    }
    const int cap = std::max(1024, 2 * max_hits);
    const int lds_cap = std::min(cap, kRangeLds);
    int Bp = 0;
    if (int rc = index_plan_bp(h, B, &Bp)) return rc;
    const size_t rec = (size_t)Bp * cap;
    HIP_TRY(h->rng_arena.ensure(rec * 16));
    HIP_TRY(h->rng_flag.ensure((size_t)B * 8));
    uint64_t* keys = h->rng_arena.as<uint64_t>();
    float2* buf = (float2*)(keys + rec);
    int32_t* flags = h->rng_flag.as<int32_t>();
    uint32_t* cnts = (uint32_t*)(flags + B);
    int lds_p2 = 1024;
    while (lds_p2 < lds_cap) lds_p2 <<= 1;
    const int lds = lds_p2 * 12;
    static bool order_attr[64] = {};  // per device, set once
    if (!order_attr[h->device & 63]) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_range_order, hipFuncAttributeMaxDynamicSharedMemorySize, kRangeLds * 12));
        order_attr[h->device & 63] = true;
    }
    const Scratch& sc = h->scr[kSyncSet];
    std::vector<int32_t> fl((size_t)B, 0);
    std::vector<uint32_t> cn((size_t)B, 0);
    for (int b0 = 0; b0 < B; b0 += Bp) {
        const int bc = std::min(Bp, B - b0);
        const RangeScan rs{t_dev + b0, buf, cap};
        if (int rc = index_range_chunk(h, q_dev + (int64_t)b0 * h->dim, bc, mask_dev, &rs, st)) return rc;
        const dim3 rgrid((unsigned)std::min(256, (cap + 3) / 4), (unsigned)bc);
        int rc = dispatch_dt(h->dtype, [&](auto dt) -> int {
            hipLaunchKernelGGL((k_range_rescore<decltype(dt)::value>), rgrid, dim3(256), 0, st, h->rows, h->S, h->dpad,
                               sc.q32.as<float>(), sc.qerr.as<double>(), h->metric, sc.cnt.as<uint32_t>(), buf, cap,
                               t_dev + b0, h->n, keys);
            HIP_TRY(hipGetLastError());
            return HR_OK;
        });
        if (rc) return rc;
        hipLaunchKernelGGL(k_range_order, dim3((unsigned)bc), dim3(1024), lds, st, sc.cnt.as<uint32_t>(), buf, keys, cap,
                           lds_cap, lds_p2, max_hits, max_hits ? s_out + (int64_t)b0 * max_hits : nullptr,
                           max_hits ? r_out + (int64_t)b0 * max_hits : nullptr, c_out + b0, flags + b0, cnts + b0);
        HIP_TRY(hipGetLastError());
        if (cap > kRangeLds) {  // a region may be beyond the LDS: it is ordered before the next chunk reuses the arena
            HIP_TRY(hipMemcpyAsync(&fl[(size_t)b0], flags + b0, (size_t)bc * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&cn[(size_t)b0], cnts + b0, (size_t)bc * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int i = 0; i < bc; ++i) {
                if (fl[(size_t)(b0 + i)] != 2) continue;
                const int b = b0 + i;
                if (int rc2 = order_large_region(h, buf + (int64_t)i * cap, keys + (int64_t)i * cap, cn[(size_t)b],
                                                 t_dev + b, max_hits, max_hits ? s_out + (int64_t)b * max_hits : nullptr,
                                                 max_hits ? r_out + (int64_t)b * max_hits : nullptr, c_out + b, st))
                    return rc2;
            }
        }
    }
    if (cap <= kRangeLds) {
        HIP_TRY(hipMemcpyAsync(fl.data(), flags, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    std::vector<int> todo;
    for (int b = 0; b < B; ++b)
        if (fl[(size_t)b] == 1) todo.push_back(b);
    h->n_range_window += B - (int64_t)todo.size();
    h->n_range_all += (int64_t)todo.size();
    if (!todo.empty()) {
        const float* q32 = nullptr;
        std::vector<double> qerr;
        if (int rc = index_prep_exact(h, q_dev, B, st, &q32, &qerr)) return rc;
        const size_t k8 = up256(8 * (size_t)h->n);
        HIP_TRY(h->rng_keys.ensure(k8 + up256(4 * (size_t)h->n)));
        uint64_t* akeys = h->rng_keys.as<uint64_t>();
        uint32_t* avals = (uint32_t*)(h->rng_keys.as<uint8_t>() + k8);
        for (int b : todo) {
            if (int rc = exact_all_keys(h->rows, h->dtype, h->S, h->dpad, q32 + (int64_t)b * h->dpad, h->metric,
                                        qerr[4 * (size_t)b + 2], h->live, (const uint32_t*)mask_dev, h->n, akeys, avals, st))
                return set_err(rc, "all-rows exact pass failed");
            if (int rc = hits_sorted(h, akeys, avals, h->n, t_dev + b, max_hits,
                                     max_hits ? s_out + (int64_t)b * max_hits : nullptr,
                                     max_hits ? r_out + (int64_t)b * max_hits : nullptr, c_out + b, st))
                return rc;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

namespace {

int check_args(hr_index* h, int B, int max_hits) {
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "range search needs a single-device handle");
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (max_hits < 0 || max_hits > HR_RANGE_MAX_HITS)
        return set_err(HR_E_INVALID, "max_hits must be in [0, HR_RANGE_MAX_HITS]");
    return HR_OK;
}

int check_thresholds(const float* t, int B) {
    for (int b = 0; b < B; ++b)
        if (std::isnan(t[b])) return set_err(HR_E_INVALID, "min_score must not be NaN");
    return HR_OK;
}

}  // namespace

int range_floors(const double* qerr, const float* min_score, int B, int Bp, double max_norm, double gamma, double u_x,
                 int metric, float* floor_q, hipStream_t st) {
    hipLaunchKernelGGL(k_range_floors, grid_for(Bp), dim3(256), 0, st, qerr, min_score, B, Bp, max_norm, gamma, u_x,
                       metric, floor_q);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

void range_free(hr_index* h) {
    for (DevBuf* b : {&h->rng_arena, &h->rng_flag, &h->rng_keys, &h->rng_sort, &h->rng_tmp, &h->rng_wtiles})
        b->release();
}

extern "C" int hr_index_search_range_device(hr_index* h, const float* q_dev, int B, const float* min_score_dev,
                                            int max_hits, const uint64_t* row_mask_dev, float* scores_out_dev,
                                            int64_t* rows_out_dev, int64_t* counts_out_dev, void* stream) {
    if (!h || !q_dev || !min_score_dev || !counts_out_dev) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_args(h, B, max_hits)) return rc;
    if (max_hits > 0 && (!scores_out_dev || !rows_out_dev)) return set_err(HR_E_INVALID, "null argument");
    if (int rc = set_device(h)) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> t((size_t)B);
    HIP_TRY(hipMemcpyAsync(t.data(), min_score_dev, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = check_thresholds(t.data(), B)) return rc;
    return range_impl(h, q_dev, B, min_score_dev, max_hits, row_mask_dev, scores_out_dev, rows_out_dev, counts_out_dev,
                      st);
}

extern "C" int hr_index_search_range(hr_index* h, const float* q, int B, const float* min_score, int max_hits,
                                     const uint64_t* row_mask, float* scores_out, int64_t* rows_out,
                                     int64_t* counts_out) {
    if (!h || !q || !min_score || !counts_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_args(h, B, max_hits)) return rc;
    if (max_hits > 0 && (!scores_out || !rows_out)) return set_err(HR_E_INVALID, "null argument");
    if (int rc = check_thresholds(min_score, B)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    const size_t nk = (size_t)B * max_hits;  // (count only: no score / row segments)
    OutSeg out[3] = {{scores_out, nk * 4}, {rows_out, nk * 8}, {counts_out, (size_t)B * 8}};
    float* q_dev = nullptr;
    uint64_t* m_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    HIP_TRY(h->hs.aux.ensure((size_t)B * 4));
    if (int rc = stage_mask(h, row_mask, st, &m_dev)) return rc;
    if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    HIP_TRY(hipMemcpyAsync(h->hs.aux.p, min_score, (size_t)B * 4, hipMemcpyHostToDevice, st));
    TileListScope tl_scope{h};  // the selective-filter tile list of a host mask, as hr_index_search
    if (m_dev && h->n_live > 0)
        if (int rc = index_host_tile_list(h, (const uint32_t*)row_mask, st)) return rc;
    if (int rc = range_impl(h, q_dev, B, h->hs.aux.as<float>(), max_hits, m_dev, out[0].as<float>(),
                            out[1].as<int64_t>(), out[2].as<int64_t>(), st))
        return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_range_stats(hr_index* h, int64_t out[3]) {
    if (!h || !out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    out[0] = h->n_range_window;
    out[1] = h->n_range_all;
    out[2] = h->n_range_scans;
    return HR_OK;
}

// diagnostics: tiles each wave of the most recent window scan (the last chunk's) scanned, [group][wave]; blocking
extern "C" int hr_index_range_wave_tiles(hr_index* h, uint32_t* out, int cap, int* n_out) {
    if (!h || !out || !n_out || cap < 0) return set_err(HR_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    *n_out = 0;
    if (!h->rng_wtiles.p || h->rng_waves <= 0) return HR_OK;
    if (int rc = set_device(h)) return rc;
    const int n = (int)std::min<int64_t>(cap, h->rng_waves);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->rng_wtiles.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    *n_out = n;
    return HR_OK;
}
