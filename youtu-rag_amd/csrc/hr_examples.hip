// hr_examples.hip -- search by example: queries built on the device from stored rows, searched exactly, the examples
// dropped from the answer (Qdrant's recommend, Weaviate's nearObject, Pinecone's query by id; the
// contract is in include/hiprag.h and restated by tests/examples_ref.py).
//
//   lists      query b's examples are ex_rows[ex_off[b] .. ex_off[b + 1]) with the fp32 weights ex_weights[...]: host
//              arrays, validated on the host (range, live bit, finite weight, 0 <= m_b <= HR_EX_MAX, m_b = 0 only with
//              a base vector), packed as offsets | rows | weights and copied to the device once per call
//   build      k_build_queries: acc = (double)q[b][d] (0.0 without q), then per example in list order
//              acc = acc + (double)w * (double)x[d], built[b][d] = (float)acc -- on h->rows, in their tiled layout
//   search     index_search_locked for K' = k + M rows, M = the largest m_b (K' > HR_MAX_K: the exhaustive pass)
//   drop       k_drop_examples: the positions holding one of the query's examples leave the list, order kept; the
//              first k remain, -inf / -1 after them.  At most m_b <= M of the K' rows leave, so k of the remainder
//              are always among them: exact, without a fallback stage.  HR_EX_KEEP: K' = k and no drop.
#include "hr_internal.hpp"

namespace {

constexpr int kExAbreast = 8;  // examples whose row chunks one thread has in flight before it accumulates them

// element j of an 8-element chunk (lo: its 16 bytes; fp32 rows: elements 4..7 in hi), widened to fp32 as load_elem does
template <int DT>
__device__ inline float chunk_elem(const u32x4& lo, const u32x4& hi, int j) {
    if (DT == F32) return __builtin_bit_cast(float, j < 4 ? lo[j] : hi[j - 4]);
    const uint16_t v = (uint16_t)((j & 1) ? lo[j >> 1] >> 16 : lo[j >> 1] & 0xFFFFu);
    return DT == BF16 ? bf16_to_f32(v) : f16_to_f32(v);
}

// One workgroup per query; a thread owns the 8-element chunks c = tid (mod 256) of the padded dim -- chunk c is k-step
// c / 2, half c % 2 of a row's slot (16 bytes, 2 x 16 for fp32 rows; the addressing of k_copy_rows).  Its examples'
// chunks are loaded kExAbreast at a time, all issued before the first is used, then accumulated in LIST order in
// fp64.  The product of two fp32 values is exact in fp64, so the fused multiply-add the compiler forms here
// (-ffp-contract=fast) and a separate multiply and add round once, to the same bits: unlike mmr_value this needs no
// contraction guard.  A slot without an example is skipped, not added as zero (-0.0 + 0.0 would lose a base vector's
// sign).  Rows outside [0, n) never reach the kernel (the host refuses them); the test here keeps a stray one from
// being read.  Registers only: no LDS, no scratch.
template <int DT>
__global__ __launch_bounds__(256) void k_build_queries(const uint8_t* __restrict__ rows, int S, int dim, int64_t n,
                                                       const int64_t* __restrict__ ex_off,
                                                       const int64_t* __restrict__ ex_rows,
                                                       const float* __restrict__ ex_w, const float* __restrict__ q,
                                                       float* __restrict__ out) {
    constexpr int64_t CB = DT == F32 ? 2048 : 1024;
    const int64_t b = blockIdx.x;
    const int64_t e0 = ex_off[b], e1 = ex_off[b + 1];
    for (int c = threadIdx.x; c < 2 * S; c += blockDim.x) {
        const int s = c >> 1, hf = c & 1, d0 = 8 * c;
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = (q && d0 + j < dim) ? (double)q[b * dim + d0 + j] : 0.0;
        for (int64_t e = e0; e < e1; e += kExAbreast) {
            u32x4 lo[kExAbreast], hi[kExAbreast];
            float w[kExAbreast];
            bool on[kExAbreast];
#pragma unroll
            for (int u = 0; u < kExAbreast; ++u) {  // (e, e1 and the rows are workgroup-uniform)
                const int64_t r = e + u < e1 ? ex_rows[e + u] : -1;
                on[u] = r >= 0 && r < n;
                w[u] = on[u] ? ex_w[e + u] : 0.0f;
                lo[u] = hi[u] = u32x4{0, 0, 0, 0};
                if (on[u]) {
                    const uint8_t* p = rows + ((r >> 5) * S + s) * CB + (row_slot(r) + 32 * hf) * 16;
                    lo[u] = *(const u32x4*)p;
                    if (DT == F32) hi[u] = *(const u32x4*)(p + 1024);
                }
            }
#pragma unroll
            for (int u = 0; u < kExAbreast; ++u) {
                if (!on[u]) continue;
                const double wd = (double)w[u];
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = acc[j] + wd * (double)chunk_elem<DT>(lo[u], hi[u], j);
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (d0 + j < dim) out[b * dim + d0 + j] = (float)acc[j];
    }
}

// One wave per query over its Kp results (s_in / r_in, or the exhaustive pass's records c_in), 64 positions a step: a
// position stays when it holds a row (>= 0) that is none of the query's m <= HR_EX_MAX examples; a ballot prefix
// gives it its place, so the order is kept; the first k are written, -inf / -1 after them.  ex_off == nullptr: no
// examples (Kp = 0 then pads every slot: the empty index).
__global__ __launch_bounds__(256) void k_drop_examples(const float* __restrict__ s_in, const int64_t* __restrict__ r_in,
                                                       const Cand* __restrict__ c_in, int Kp, int k, int B,
                                                       const int64_t* __restrict__ ex_off,
                                                       const int64_t* __restrict__ ex_rows, float* __restrict__ s_out,
                                                       int64_t* __restrict__ r_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;  // (wave-uniform)
    const int64_t e0 = ex_off ? ex_off[b] : 0;
    const int m = ex_off ? (int)(ex_off[b + 1] - e0) : 0;
    int base = 0;  // rows kept so far
    for (int i0 = 0; i0 < Kp && base < k; i0 += 64) {
        const int i = i0 + lane;
        int64_t r = -1;
        float s = -__builtin_inff();
        if (i < Kp) {
            if (c_in) {
                const Cand c = c_in[b * Kp + i];
                r = c.row;
                s = (float)c.score;
            } else {
                r = r_in[b * Kp + i];
                s = s_in[b * Kp + i];
            }
        }
        bool keep = r >= 0;
        for (int j = 0; j < m; ++j) keep = keep && r != ex_rows[e0 + j];
        const uint64_t kept = __ballot(keep);
        const int pos = base + __popcll(kept & ((1ull << lane) - 1ull));
        if (keep && pos < k) {
            s_out[b * k + pos] = s;
            r_out[b * k + pos] = r;
        }
        base += __popcll(kept);
    }
    for (int i = (base < k ? base : k) + lane; i < k; i += 64) {
        s_out[b * k + i] = -__builtin_inff();
        r_out[b * k + i] = -1;
    }
}

struct Lists {  // one call's example lists on the device (h->ex_list)
    const int64_t* off = nullptr;
    const int64_t* rows = nullptr;
    const float* w = nullptr;
    int M = 0;  // the largest m_b
};

// everything the contract refuses, before any device call
int check_lists(hr_index* h, const int64_t* ex_rows, const float* ex_w, const int64_t* ex_off, int B, bool has_q) {
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "search by example needs a single-device handle");
    if (B <= 0) return set_err(HR_E_INVALID, "B must be positive");
    if (ex_off[0] < 0) return set_err(HR_E_INVALID, "ex_off must start at or above 0");
    for (int b = 0; b < B; ++b) {
        const int64_t m = ex_off[b + 1] - ex_off[b];
        if (m < 0 || m > HR_EX_MAX) return set_err(HR_E_INVALID, "a query takes 0 to HR_EX_MAX examples");
        if (m == 0 && !has_q) return set_err(HR_E_INVALID, "a query without examples needs a base vector");
    }
    if (ex_off[B] > ex_off[0] && (!ex_rows || !ex_w)) return set_err(HR_E_INVALID, "null argument");
    for (int64_t e = ex_off[0]; e < ex_off[B]; ++e) {
        const int64_t r = ex_rows[e];
        if (r < 0 || r >= h->n) return set_err(HR_E_INVALID, "example row out of range");
        if (!(h->live_host[(size_t)(r >> 5)] >> (r & 31) & 1u)) return set_err(HR_E_INVALID, "example row was removed");
        if (!std::isfinite(ex_w[e])) return set_err(HR_E_INVALID, "example weights must be finite");
    }
    return HR_OK;
}

// the validated lists, rebased to offset 0, as ONE block and one copy on st (h->ex_host keeps the host side alive)
int stage_lists(hr_index* h, const int64_t* ex_rows, const float* ex_w, const int64_t* ex_off, int B, hipStream_t st,
                Lists* out) {
    const int64_t first = ex_off[0], tot = ex_off[B] - first;
    const size_t off_r = (size_t)(B + 1) * 8, off_w = off_r + (size_t)tot * 8, bytes = off_w + (size_t)tot * 4;
    h->ex_host.resize(bytes);
    int64_t* o = (int64_t*)h->ex_host.data();
    out->M = 0;
    for (int b = 0; b <= B; ++b) o[b] = ex_off[b] - first;
    for (int b = 0; b < B; ++b) out->M = std::max(out->M, (int)(o[b + 1] - o[b]));
    if (tot) {
        std::memcpy(h->ex_host.data() + off_r, ex_rows + first, (size_t)tot * 8);
        std::memcpy(h->ex_host.data() + off_w, ex_w + first, (size_t)tot * 4);
    }
    HIP_TRY(h->ex_list.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(h->ex_list.p, h->ex_host.data(), bytes, hipMemcpyHostToDevice, st));
    const uint8_t* p = h->ex_list.as<uint8_t>();
    out->off = (const int64_t*)p;
    out->rows = (const int64_t*)(p + off_r);
    out->w = (const float*)(p + off_w);
    return HR_OK;
}

int launch_build(hr_index* h, const Lists& L, int B, const float* q_dev, float* q_out, hipStream_t st) {
    return dispatch_dt(h->dtype, [&](auto dt) -> int {
        hipLaunchKernelGGL((k_build_queries<decltype(dt)::value>), dim3((unsigned)B), dim3(256), 0, st, h->rows, h->S,
                           h->dim, h->n, L.off, L.rows, L.w, q_dev, q_out);
        HIP_TRY(hipGetLastError());
        return HR_OK;
    });
}

int launch_drop(const float* s_in, const int64_t* r_in, const Cand* c_in, int Kp, int k, int B, const Lists* L,
                float* s_out, int64_t* r_out, hipStream_t st) {
    hipLaunchKernelGGL(k_drop_examples, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, s_in, r_in, c_in, Kp, k, B,
                       L ? L->off : nullptr, L ? L->rows : nullptr, s_out, r_out);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

// lists staged, base queries, mask and outputs on h's device; the caller holds h->mu with the device current and has
// checked the arguments.  Returns with st idle.
int examples_impl(hr_index* h, const Lists& L, const float* q_dev, int B, int k, int flags, const uint64_t* mask_dev,
                  float* s_out, int64_t* r_out, hipStream_t st) {
    if (h->n_live == 0) {  // empty index (only base vectors pass the checks): padding, as hr_index_search
        if (int rc = pad_results(s_out, r_out, (int64_t)B * k, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return HR_OK;
    }
    HIP_TRY(h->ex_q.ensure((size_t)B * h->dim * 4));
    float* built = h->ex_q.as<float>();
    if (int rc = launch_build(h, L, B, q_dev, built, st)) return rc;
    const int M = (flags & HR_EX_KEEP) ? 0 : L.M;
    if ((int64_t)k + M > INT32_MAX) return set_err(HR_E_INVALID, "k too large");
    const int Kp = k + M;
    if (Kp > HR_MAX_K) {  // as hr_index_search: the exhaustive exact pass, its records dropped from
        HIP_TRY(h->ex_cand.ensure((size_t)B * Kp * sizeof(Cand)));
        if (int rc = index_exact_dev(h, built, B, Kp, mask_dev, 0, h->ex_cand.as<Cand>(), st)) return rc;
        if (int rc = launch_drop(nullptr, nullptr, h->ex_cand.as<Cand>(), Kp, k, B, M ? &L : nullptr, s_out, r_out, st))
            return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return HR_OK;
    }
    if (M == 0) return index_search_locked(h, built, B, k, mask_dev, s_out, r_out, st);  // nothing to drop
    HIP_TRY(h->pool_s.ensure((size_t)B * Kp * 4));
    HIP_TRY(h->pool_r.ensure((size_t)B * Kp * 8));
    if (int rc = index_search_locked(h, built, B, Kp, mask_dev, h->pool_s.as<float>(), h->pool_r.as<int64_t>(), st))
        return rc;
    if (int rc = launch_drop(h->pool_s.as<float>(), h->pool_r.as<int64_t>(), nullptr, Kp, k, B, &L, s_out, r_out, st))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

int check_search(int k, int flags) {
    if (k <= 0) return set_err(HR_E_INVALID, "k must be positive");
    if (flags & ~HR_EX_KEEP) return set_err(HR_E_INVALID, "unknown flags");
    return HR_OK;
}

}  // namespace

void examples_free(hr_index* h) {
    for (DevBuf* b : {&h->ex_list, &h->ex_q, &h->ex_cand}) b->release();
}

extern "C" int hr_index_build_queries_device(hr_index* h, const int64_t* ex_rows, const float* ex_weights,
                                             const int64_t* ex_off, int B, const float* q_dev, float* q_out_dev,
                                             void* stream) {
    if (!h || !ex_off || !q_out_dev) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_lists(h, ex_rows, ex_weights, ex_off, B, q_dev != nullptr)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Lists L;
    if (int rc = stage_lists(h, ex_rows, ex_weights, ex_off, B, st, &L)) return rc;
    if (int rc = launch_build(h, L, B, q_dev, q_out_dev, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_build_queries(hr_index* h, const int64_t* ex_rows, const float* ex_weights,
                                      const int64_t* ex_off, int B, const float* q, float* q_out) {
    if (!h || !ex_off || !q_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_lists(h, ex_rows, ex_weights, ex_off, B, q != nullptr)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    const size_t qb = (size_t)B * h->dim * 4;
    Lists L;
    if (int rc = stage_lists(h, ex_rows, ex_weights, ex_off, B, st, &L)) return rc;
    HIP_TRY(h->ex_q.ensure(qb));
    float* q_dev = nullptr;
    if (q)
        if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    if (int rc = launch_build(h, L, B, q_dev, h->ex_q.as<float>(), st)) return rc;
    HIP_TRY(hipMemcpyAsync(q_out, h->ex_q.p, qb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

extern "C" int hr_index_search_examples_device(hr_index* h, const float* q_dev, const int64_t* ex_rows,
                                               const float* ex_weights, const int64_t* ex_off, int B, int k, int flags,
                                               const uint64_t* row_mask_dev, float* scores_out_dev,
                                               int64_t* rows_out_dev, void* stream) {
    if (!h || !ex_off || !scores_out_dev || !rows_out_dev) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_lists(h, ex_rows, ex_weights, ex_off, B, q_dev != nullptr)) return rc;
    if (int rc = check_search(k, flags)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = (hipStream_t)stream;
    Lists L;
    if (int rc = stage_lists(h, ex_rows, ex_weights, ex_off, B, st, &L)) return rc;
    return examples_impl(h, L, q_dev, B, k, flags, row_mask_dev, scores_out_dev, rows_out_dev, st);
}

extern "C" int hr_index_search_examples(hr_index* h, const float* q, const int64_t* ex_rows, const float* ex_weights,
                                        const int64_t* ex_off, int B, int k, int flags, const uint64_t* row_mask,
                                        float* scores_out, int64_t* rows_out) {
    if (!h || !ex_off || !scores_out || !rows_out) return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc = check_lists(h, ex_rows, ex_weights, ex_off, B, q != nullptr)) return rc;
    if (int rc = check_search(k, flags)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    Lists L;
    if (int rc = stage_lists(h, ex_rows, ex_weights, ex_off, B, st, &L)) return rc;
    OutSeg out[2] = {{scores_out, (size_t)B * k * 4}, {rows_out, (size_t)B * k * 8}};
    float* q_dev = nullptr;
    uint64_t* m_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    if (q)
        if (int rc = stage_queries(h, q, B, st, &q_dev)) return rc;
    if (int rc = stage_mask(h, row_mask, st, &m_dev)) return rc;
    if (int rc = examples_impl(h, L, q_dev, B, k, flags, m_dev, out[0].as<float>(), out[1].as<int64_t>(), st))
        return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}
