// hr_mmr.hip -- MMR search: k rows of every query chosen by maximal marginal relevance from the exact top-P pool
// (LangChain's max_marginal_relevance_search, with every step pinned so that the host restatement in
// tests/mmr_ref.py gives the same bits).
//
//   pool       the exact search for P rows (index_search_locked), in its order (canonical score desc, row asc);
//              rel[j] = the fp32 score of position j widened to fp64; row -1 = padding, never a candidate
//   sim(s, j)  the canonical fp64 score of stored row j against stored row s in the QUERY role (its components
//              widened to fp32): lane l accumulates the elements d = l (mod 64) in increasing d, wave_butterfly_sum,
//              euclid_score(|s|^2, dot, |j|^2) for l2 -- the arithmetic of k_exact_all / k_rescore, on h->rows
//   greedy     step 0 takes position 0; maxsim[j] = max over the selected s of sim(s, j); every further step takes
//              the largest v[j] = lambda * rel[j] - (1 - lambda) * maxsim[j] (three roundings, NO fused multiply-add:
//              mmr_value below; NaN counts as -inf), ties to the lowest position
//   output     the rows in selection order with their fp32 relevance (so not monotone), then -inf / -1
//
// k_mmr_select: one workgroup per query, min(16, P) waves.  The lazy form: a round computes only
// sim(newly selected, j) for the unselected candidates -- (k - 1) P dots, not a P x P Gram matrix.  Per round the
// selected row is staged once as fp32 in LDS (dpad * 4 bytes), wave w takes the candidates j = w (mod waves), one
// canonical dot each -- ILP of them side by side, independent chains for the scheduler -- updates maxsim[j] and v
// and keeps the wave's best (v desc, position asc); the waves' bests meet in LDS and every thread reduces them to
// the same pick: two barriers per round.  The candidate rows are re-read from the tiled corpus every round
// (through L2: at P = 128 and 1024 bf16 dims they are 256 KB, beyond LDS; at 16 waves a lane has 128 registers,
// which do not hold a wave's 8 rows of 16 elements beside the dots' own state).
#include <climits>

#include "hr_internal.hpp"

namespace {

constexpr int kMmrWaves = 16;

// lambda * rel - one_minus * maxsim as three separately rounded fp64 operations.  The library is built with
// -ffp-contract=fast, and the header's __dmul_rn is a plain product that contracts like any other; so contraction is
// switched off for this function and each product also passes through an empty asm that makes it opaque, which
// leaves the compiler nothing to fuse the subtraction with.  (The one place in the feature where an FMA changes
// bits: the dots multiply two stored values, exact in fp64.)
__device__ inline double mmr_value(double lambda, double rel, double one_minus, double maxsim) {
#pragma clang fp contract(off)
    double a = lambda * rel;
    double b = one_minus * maxsim;
    asm volatile("" : "+v"(a));
    asm volatile("" : "+v"(b));
    return a - b;
}

template <int DT, int ILP>
__global__ __launch_bounds__(64 * kMmrWaves) void k_mmr_select(const uint8_t* __restrict__ rows, int S, int dpad,
                                                               int metric, int64_t n, const float* __restrict__ s_in,
                                                               const int64_t* __restrict__ r_in, int P, int k,
                                                               double lambda, double one_minus,
                                                               float* __restrict__ s_out, int64_t* __restrict__ r_out) {
    extern __shared__ __attribute__((aligned(16))) float sel[];  // the selected row, dpad floats
    __shared__ double rel[HR_MAX_K], maxsim[HR_MAX_K];
    __shared__ int64_t rowid[HR_MAX_K];
    __shared__ int taken[HR_MAX_K];  // selected, or padding
    __shared__ double wave_v[kMmrWaves];
    __shared__ int wave_j[kMmrWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
    const int64_t q = blockIdx.x;
    bool valid = false;
    if (tid < P) {
        const int64_t r = r_in[q * P + tid];
        valid = r >= 0 && r < n;
        rowid[tid] = valid ? r : -1;
        rel[tid] = (double)s_in[q * P + tid];
        maxsim[tid] = -__builtin_inf();
        taken[tid] = valid ? 0 : 1;
    }
    if (tid < kMmrWaves) {
        wave_v[tid] = -__builtin_inf();
        wave_j[tid] = INT_MAX;
    }
    const int n_valid = __syncthreads_count(valid);  // (blockDim.x >= P)
    const int n_pick = k < n_valid ? k : n_valid;
    int first = INT_MAX;  // the lowest candidate position: 0 (the pool's padding is at its end)
    for (int j = P - 1; j >= 0; --j)
        if (!taken[j]) first = j;
    __syncthreads();  // (taken is written below)
    for (int t = 0; t < n_pick; ++t) {
        // step 0 takes the first position; afterwards every thread reduces the waves' bests of the round before to
        // the same pick (value desc, position asc)
        double bv = -__builtin_inf();
        int pick = first;
        if (t > 0) {
            pick = INT_MAX;
            for (int i = 0; i < W; ++i) {
                const double v = wave_v[i];
                const int j = wave_j[i];
                if (v > bv || (v == bv && j < pick)) {
                    bv = v;
                    pick = j;
                }
            }
        }
        if (tid == 0) {
            s_out[q * k + t] = s_in[q * P + pick];
            r_out[q * k + t] = rowid[pick];
            taken[pick] = 1;
        }
        if (t + 1 == n_pick) break;
        const int64_t rs = rowid[pick];
        for (int d = tid; d < dpad; d += blockDim.x) sel[d] = load_elem<DT>(rows, S, rs, d);
        __syncthreads();
        double qn2 = 0.0;
        if (metric == L2) {  // the canonical |s|^2, by every wave for itself
            for (int d = lane; d < dpad; d += 64) {
                const double x = (double)sel[d];
                qn2 = qn2 + x * x;
            }
            qn2 = wave_butterfly_sum(qn2);
        }
        double best_v = -__builtin_inf();
        int best_j = INT_MAX;
        // ILP of the wave's candidates at a time: their loads, accumulations and butterflies are independent
        // chains the scheduler interleaves (each dot keeps its own canonical order).  A slot without a candidate
        // (beyond P, selected, padding) reads the selected row again and is dropped.
        for (int j0 = w; j0 < P; j0 += ILP * W) {
            int64_t r[ILP];
            bool act[ILP], any = false;
#pragma unroll
            for (int u = 0; u < ILP; ++u) {
                const int j = j0 + u * W;
                act[u] = j < P && !taken[j];  // (wave-uniform)
                r[u] = act[u] ? rowid[j] : rs;
                any = any || act[u];
            }
            if (!any) continue;
            double p[ILP], x2[ILP];
#pragma unroll
            for (int u = 0; u < ILP; ++u) p[u] = x2[u] = 0.0;
            for (int d = lane; d < dpad; d += 64) {
                const double qd = (double)sel[d];
#pragma unroll
                for (int u = 0; u < ILP; ++u) {
                    const double x = (double)load_elem<DT>(rows, S, r[u], d);
                    p[u] = p[u] + x * qd;
                    if (metric == L2) x2[u] = x2[u] + x * x;
                }
            }
#pragma unroll
            for (int u = 0; u < ILP; ++u) {
                p[u] = wave_butterfly_sum(p[u]);
                if (metric == L2) p[u] = euclid_score(qn2, p[u], wave_butterfly_sum(x2[u]));
            }
#pragma unroll
            for (int u = 0; u < ILP; ++u) {
                const int j = j0 + u * W;
                if (!act[u]) continue;
                double m = maxsim[j];
                if (p[u] > m) m = p[u];
                double v = mmr_value(lambda, rel[j], one_minus, m);
                if (v != v) v = -__builtin_inf();
                if (lane == 0) maxsim[j] = m;
                if (v > best_v || (v == best_v && j < best_j)) {
                    best_v = v;
                    best_j = j;
                }
            }
        }
        if (lane == 0) {
            wave_v[w] = best_v;
            wave_j[w] = best_j;
        }
        __syncthreads();
    }
    for (int i = n_pick + tid; i < k; i += blockDim.x) {
        s_out[q * k + i] = -__builtin_inff();
        r_out[q * k + i] = -1;
    }
}

int default_fetch(int k) { return std::min(HR_MAX_K, std::max(32, 4 * k)); }

int check_args(hr_index* h, int B, int k, int fetch_k, double lambda) {
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "MMR search needs a single-device handle");
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (k <= 0 || k > HR_MAX_K) return set_err(HR_E_INVALID, "k must be in [1, HR_MAX_K]");
    if (fetch_k != 0 && (fetch_k < k || fetch_k > HR_MAX_K))
        return set_err(HR_E_INVALID, "fetch_k must be 0 or in [k, HR_MAX_K]");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return set_err(HR_E_INVALID, "lambda must be in [0, 1]");
    return HR_OK;
}

// queries, mask and outputs on h's device; the caller holds h->mu with the device current and has checked the
// arguments.  Returns with st idle.
int mmr_impl(hr_index* h, const float* q_dev, int B, int k, int fetch_k, double lambda, const uint64_t* mask_dev,
             float* s_out, int64_t* r_out, hipStream_t st) {
    const int P = fetch_k ? fetch_k : default_fetch(k);
    if (h->n_live == 0) {  // empty index: padding, as hr_index_search
        if (int rc = pad_results(s_out, r_out, (int64_t)B * k, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return HR_OK;
    }
    const bool timed = h->mmr_timing;
    if (timed)
        for (auto& e : h->mmr_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(h->pool_s.ensure((size_t)B * P * 4));
    HIP_TRY(h->pool_r.ensure((size_t)B * P * 8));
    float* ps = h->pool_s.as<float>();
    int64_t* pr = h->pool_r.as<int64_t>();
    if (timed) HIP_TRY(hipEventRecord(h->mmr_ev[0], st));
    if (int rc = index_search_locked(h, q_dev, B, P, mask_dev, ps, pr, st)) return rc;
    if (timed) HIP_TRY(hipEventRecord(h->mmr_ev[1], st));
    const dim3 grid((unsigned)B), block((unsigned)(64 * std::min(kMmrWaves, P)));
    const size_t lds = (size_t)h->dpad * 4;
    const double om = 1.0 - lambda;
    // candidates a wave scores side by side: four where it owns more than two (P > 32), else two -- a slot without a
    // candidate still reads a row: at P = 32, 64 queries and 768 bf16 dims the four-wide form took 0.086 ms, the
    // two-wide one 0.064 ms (one at a time: 0.077 ms; at P = 128 one at a time 0.35 ms, four-wide 0.19 ms)
    if (int rc = dispatch_dt(h->dtype, [&](auto dt) {
            constexpr int DT = decltype(dt)::value;
            auto kern = P > 2 * kMmrWaves ? k_mmr_select<DT, 4> : k_mmr_select<DT, 2>;
            hipLaunchKernelGGL(kern, grid, block, lds, st, h->rows, h->S, h->dpad, h->metric, h->n, ps, pr, P, k, lambda,
                               om, s_out, r_out);
            return HR_OK;
        }))
        return rc;
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(h->mmr_ev[2], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timed) {
        float ms[2] = {0.f, 0.f};
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], h->mmr_ev[i], h->mmr_ev[i + 1]));
        for (int i = 0; i < 2; ++i) h->mmr_ms[i] = ms[i];
    }
    return HR_OK;
}

}  // namespace

void mmr_free(hr_index* h) {
    for (auto& e : h->mmr_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int hr_index_search_mmr_device(hr_index* h, const float* q_dev, int B, int k, int fetch_k, double lambda,
                                          const uint64_t* row_mask_dev, float* scores_out_dev, int64_t* rows_out_dev,
                                          void* stream) {
    if (!h || !q_dev || !scores_out_dev || !rows_out_dev) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_args(h, B, k, fetch_k, lambda)) return rc;
    if (int rc = set_device(h)) return rc;
    return mmr_impl(h, q_dev, B, k, fetch_k, lambda, row_mask_dev, scores_out_dev, rows_out_dev, (hipStream_t)stream);
}

extern "C" int hr_index_search_mmr(hr_index* h, const float* q, int B, int k, int fetch_k, double lambda,
                                   const uint64_t* row_mask, float* scores_out, int64_t* rows_out) {
    if (!h || !q || !scores_out || !rows_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_args(h, B, k, fetch_k, lambda)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    OutSeg out[2] = {{scores_out, (size_t)B * k * 4}, {rows_out, (size_t)B * k * 8}};
    float* q_dev = nullptr;
    uint64_t* m_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    if (int rc = stage_mask(h, row_mask, st, &m_dev)) return rc;
    if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    if (int rc = mmr_impl(h, q_dev, B, k, fetch_k, lambda, m_dev, out[0].as<float>(), out[1].as<int64_t>(), st))
        return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_set_mmr_timing(hr_index* h, int on) {
    if (!h) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->mmr_timing = on != 0;
    return HR_OK;
}

extern "C" int hr_index_mmr_last_ms(hr_index* h, double out[2]) {
    if (!h || !out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (int i = 0; i < 2; ++i) out[i] = h->mmr_ms[i];
    return HR_OK;
}
