// hr_fuse.hip -- fused multi-query search: several exact ranked lists per question fused on the device by reciprocal
// rank (RRF) or by the largest score (MAX) (Elasticsearch's rrf retriever, Qdrant's fusion query,
// LangChain's MultiQueryRetriever / EnsembleRetriever; the contract is in include/hiprag.h and restated by
// tests/fused_ref.py).
//
//   lists      Q = grp_off[G] ranked lists of P slots (rows int64, scores fp32; row < 0 = padding), the format every
//              search writes; group g owns the lists [grp_off[g], grp_off[g + 1]): its 1..16 members
//   RRF        fused(r) = 0.0, then per member i holding r, in member order: fused = fused + (double)w_i / (rrf_k +
//              (double)p_i), p_i the 1-based position -- one division and one addition per term, each rounded once
//   MAX        fused(r) = the largest fp32 score among the members holding r (NaN counts as -inf), widened
//   order      fused desc, row asc; the first min(k, distinct rows) are written, then -inf / -1 / 0
//   members    bit j of members_out: member grp_off[g] + j holds the row
//
// k_fuse_lists: one workgroup per group, everything in LDS (60 KiB, static).  The group's m * P <= 2048 entries are
// sorted by (row asc, entry asc) -- entry = member * P + position, so the entries of one row come out in member order
// --; one thread per segment head walks its at most 16 entries, which gives the ordered fp64 sum without an atomic or
// anything that depends on scheduling; the heads are sorted again by (fused desc, head position asc) -- the heads'
// positions ascend with their rows -- and the first k are written.  Both sorts are one bitonic network over pairs
// (u64 key desc, u16 value asc); the first sorts ~row, so descending keys are ascending rows and key 0 is padding.
//
// hr_index_search_fused: the Q members through ONE batched exact search for fetch_k rows each (the per-query-mask
// search when the members name different bitmaps, else the plain / single-mask search), then k_fuse_lists on the
// pools where they lie.  The pools are exact and the answer a function of them: no fallback stage of its own.
#include "hr_internal.hpp"

namespace {

constexpr int kFuseEntries = HR_FUSE_MAX_MEMBERS * HR_MAX_K;  // 2048: the entries of the largest group
constexpr uint16_t kFuseNone = 0xFFFF;                        // the value of a padding pair: it sorts last
static_assert(kFuseEntries < kFuseNone, "entries are u16 values");

// n (a power of two) pairs in LDS by (key desc, value asc); thread t owns one compare-exchange per step.  Ends with a
// barrier.
__device__ inline void fuse_sort(uint64_t* ks, uint16_t* vs, int n) {
    for (int kk = 2; kk <= n; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ixj = i | j;
                const uint64_t a = ks[i], b = ks[ixj];
                const uint16_t va = vs[i], vb = vs[ixj];
                const bool a_first = a > b || (a == b && va < vb);
                const bool desc = (i & kk) == 0;
                if (desc ? !a_first : a_first) {
                    ks[i] = b;
                    ks[ixj] = a;
                    vs[i] = vb;
                    vs[ixj] = va;
                }
            }
            __syncthreads();
        }
    }
}

// one RRF term added: a division and an addition, each rounded once (there is no product to contract; the pragma keeps
// it so whatever the build's -ffp-contract says)
__device__ inline double rrf_add(double fused, float w, double rrf_k, int pos1) {
#pragma clang fp contract(off)
    const double term = (double)w / (rrf_k + (double)pos1);
    return fused + term;
}

__global__ __launch_bounds__(1024) void k_fuse_lists(const int64_t* __restrict__ rows, const float* __restrict__ scores,
                                                     int P, const int64_t* __restrict__ grp_off,
                                                     const float* __restrict__ weights, int k, int mode, double rrf_k,
                                                     double* __restrict__ fused_out, int64_t* __restrict__ rows_out,
                                                     uint32_t* __restrict__ members_out) {
    __shared__ uint64_t rkey[kFuseEntries];  // ~row of an entry, 0 = padding
    __shared__ uint16_t ent[kFuseEntries];   // member * P + position of the entry
    __shared__ uint64_t fkey[kFuseEntries];  // d2key(fused) of a segment head, 0 elsewhere
    __shared__ uint16_t head[kFuseEntries];  // the head's place in rkey / ent
    __shared__ double fval[kFuseEntries];    // fused score of the head at that place
    __shared__ uint16_t memb[kFuseEntries];  // its member bits
    const int64_t g = blockIdx.x, q0 = grp_off[g], m = grp_off[g + 1] - q0;
    // (the host refuses anything else; the test keeps a stray group inside the LDS arrays)
    const int N = (m >= 1 && m <= HR_FUSE_MAX_MEMBERS && P >= 1 && P <= HR_MAX_K) ? (int)m * P : 0;
    int p2 = 1;
    while (p2 < N) p2 <<= 1;
    const int64_t* grows = rows + q0 * P;
    for (int i = threadIdx.x; i < p2; i += blockDim.x) {
        const int64_t r = i < N ? grows[i] : -1;
        rkey[i] = r >= 0 ? ~(uint64_t)r : 0;
        ent[i] = r >= 0 ? (uint16_t)i : kFuseNone;
    }
    __syncthreads();
    fuse_sort(rkey, ent, p2);
    for (int i = threadIdx.x; i < p2; i += blockDim.x) {
        const uint64_t rk = rkey[i];
        const bool is_head = ent[i] != kFuseNone && (i == 0 || rkey[i - 1] != rk);
        double f = mode == HR_FUSE_RRF ? 0.0 : -__builtin_inf();
        uint32_t bits = 0;
        if (is_head) {
            for (int j = i; j < p2 && ent[j] != kFuseNone && rkey[j] == rk; ++j) {  // in member order
                const int e = ent[j], mb = e / P, pos = e - mb * P;
                bits |= 1u << mb;
                if (mode == HR_FUSE_RRF) {
                    f = rrf_add(f, weights ? weights[q0 + mb] : 1.0f, rrf_k, pos + 1);
                } else {
                    float s = scores[q0 * P + e];
                    if (s != s) s = -__builtin_inff();
                    if ((double)s > f) f = (double)s;
                }
            }
        }
        fkey[i] = is_head ? d2key(f) : 0;
        head[i] = is_head ? (uint16_t)i : kFuseNone;
        fval[i] = f;
        memb[i] = (uint16_t)bits;
    }
    __syncthreads();
    fuse_sort(fkey, head, p2);
    for (int t = threadIdx.x; t < k; t += blockDim.x) {
        const int at = t < p2 ? head[t] : kFuseNone;
        const bool on = at != kFuseNone;
        fused_out[g * k + t] = on ? fval[at] : -__builtin_inf();
        rows_out[g * k + t] = on ? (int64_t)~rkey[at] : -1;
        if (members_out) members_out[g * k + t] = on ? memb[at] : 0u;
    }
}

__global__ void k_fuse_pad(double* __restrict__ fused_out, int64_t* __restrict__ rows_out,
                           uint32_t* __restrict__ members_out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fused_out[i] = -__builtin_inf();
    rows_out[i] = -1;
    if (members_out) members_out[i] = 0u;
}

// everything hr_fuse_lists refuses, before any device call
int check_fuse(int P, const int64_t* grp_off, const float* weights, int G, int k, int mode, double rrf_k) {
    if (!grp_off) return set_err(HR_E_INVALID, "null argument");
    if (G <= 0) return set_err(HR_E_INVALID, "G must be positive");
    if (mode != HR_FUSE_RRF && mode != HR_FUSE_MAX) return set_err(HR_E_INVALID, "mode must be HR_FUSE_RRF or HR_FUSE_MAX");
    if (P <= 0 || P > HR_MAX_K) return set_err(HR_E_INVALID, "P must be in [1, HR_MAX_K]");
    if (k <= 0 || k > P) return set_err(HR_E_INVALID, "k must be in [1, P]");
    if (!(std::isfinite(rrf_k) && rrf_k >= 0.0)) return set_err(HR_E_INVALID, "rrf_k must be finite and not negative");
    if (grp_off[0] != 0) return set_err(HR_E_INVALID, "grp_off must start at 0");
    for (int g = 0; g < G; ++g) {
        const int64_t m = grp_off[g + 1] - grp_off[g];
        if (m < 1 || m > HR_FUSE_MAX_MEMBERS) return set_err(HR_E_INVALID, "a group takes 1 to HR_FUSE_MAX_MEMBERS members");
    }
    if (weights) {
        if (mode == HR_FUSE_MAX) return set_err(HR_E_INVALID, "HR_FUSE_MAX takes no weights");
        for (int64_t i = 0; i < grp_off[G]; ++i)
            if (!std::isfinite(weights[i])) return set_err(HR_E_INVALID, "weights must be finite");
    }
    return HR_OK;
}

// the checked lists fused on st: offsets and weights go up as ONE block through *host (kept alive by the caller until
// st is idle) into *list
int launch_fuse(const int64_t* rows_dev, const float* scores_dev, int P, const int64_t* grp_off, const float* weights,
                int G, int k, int mode, double rrf_k, double* fused_out, int64_t* rows_out, uint32_t* members_out,
                hipStream_t st, DevBuf* list, std::vector<uint8_t>* host) {
    const int64_t Q = grp_off[G];
    const size_t off_w = (size_t)(G + 1) * 8, bytes = off_w + (weights ? (size_t)Q * 4 : 0);
    host->resize(bytes);
    std::memcpy(host->data(), grp_off, off_w);
    if (weights) std::memcpy(host->data() + off_w, weights, (size_t)Q * 4);
    HIP_TRY(list->ensure(bytes));
    HIP_TRY(hipMemcpyAsync(list->p, host->data(), bytes, hipMemcpyHostToDevice, st));
    int64_t m_max = 1;
    for (int g = 0; g < G; ++g) m_max = std::max(m_max, grp_off[g + 1] - grp_off[g]);
    int p2 = 1;
    while (p2 < m_max * P) p2 <<= 1;
    const unsigned threads = (unsigned)std::min(1024, std::max(64, p2 / 2));  // one compare-exchange per thread
    hipLaunchKernelGGL(k_fuse_lists, dim3((unsigned)G), dim3(threads), 0, st, rows_dev, scores_dev, P,
                       (const int64_t*)list->p, weights ? (const float*)(list->as<uint8_t>() + off_w) : nullptr, k, mode,
                       rrf_k, fused_out, rows_out, members_out);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

int launch_pad(double* fused_out, int64_t* rows_out, uint32_t* members_out, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_fuse_pad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fused_out, rows_out, members_out,
                       n);
    HIP_TRY(hipGetLastError());
    return HR_OK;
}

int default_fetch(int k, int mode) { return mode == HR_FUSE_MAX ? k : std::min(HR_MAX_K, std::max(4 * k, 50)); }

// everything hr_index_search_fused refuses apart from the masks; *P_out: the pool depth
int check_search(hr_index* h, const int64_t* grp_off, const float* weights, int G, int k, int fetch_k, int mode,
                 double rrf_k, int* P_out) {
    if (h->G > 1) return set_err(HR_E_UNSUPPORTED, "a fused search needs a single-device handle");
    if (mode != HR_FUSE_RRF && mode != HR_FUSE_MAX) return set_err(HR_E_INVALID, "mode must be HR_FUSE_RRF or HR_FUSE_MAX");
    if (k <= 0 || k > HR_MAX_K) return set_err(HR_E_INVALID, "k must be in [1, HR_MAX_K]");
    if (fetch_k != 0 && (fetch_k < k || fetch_k > HR_MAX_K))
        return set_err(HR_E_INVALID, "fetch_k must be 0 or in [k, HR_MAX_K]");
    *P_out = fetch_k ? fetch_k : default_fetch(k, mode);
    if (int rc = check_fuse(*P_out, grp_off, weights, G, k, mode, rrf_k)) return rc;
    if (grp_off[G] > INT32_MAX / HR_MAX_K) return set_err(HR_E_INVALID, "too many queries");
    return HR_OK;
}

// queries, bitmaps, mask_of and outputs on h's device; the caller holds h->mu with the device current and has checked
// the arguments (of: the Q host entries of mask_of, nullptr = no masks).  Returns with st idle.
int fused_impl(hr_index* h, const float* q_dev, const int64_t* grp_off, const float* weights, int G, int k, int P,
               int mode, double rrf_k, const uint64_t* masks_dev, int64_t stride, const int32_t* mask_of_dev,
               const int32_t* of, double* fused_out, int64_t* rows_out, uint32_t* members_out, hipStream_t st) {
    const int Q = (int)grp_off[G];
    if (h->n_live == 0) {  // empty index: padding, as hr_index_search
        if (int rc = launch_pad(fused_out, rows_out, members_out, (int64_t)G * k, st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return HR_OK;
    }
    HIP_TRY(h->pool_s.ensure((size_t)Q * P * 4));
    HIP_TRY(h->pool_r.ensure((size_t)Q * P * 8));
    float* ps = h->pool_s.as<float>();
    int64_t* pr = h->pool_r.as<int64_t>();
    bool same = true;  // every member names the same bitmap (or none): the single-mask search, identical by contract
    for (int i = 1; of && i < Q; ++i) same = same && of[i] == of[0];
    if (!of || same) {
        const uint64_t* one = of && of[0] >= 0 ? masks_dev + (int64_t)of[0] * stride : nullptr;
        if (int rc = index_search_locked(h, q_dev, Q, P, one, ps, pr, st)) return rc;
    } else if (int rc = index_search_masks_locked(h, q_dev, Q, P, masks_dev, stride, mask_of_dev, of, ps, pr, st)) {
        return rc;
    }
    if (int rc = launch_fuse(pr, ps, P, grp_off, weights, G, k, mode, rrf_k, fused_out, rows_out, members_out, st,
                             &h->fu_list, &h->fu_host))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}

std::mutex g_fuse_mu;  // hr_fuse_lists: the staging of one call at a time
DevBuf g_fuse_list[64];
std::vector<uint8_t> g_fuse_host;

}  // namespace

void fused_free(hr_index* h) {
    h->fu_list.release();
}

extern "C" int hr_fuse_lists(int device, const int64_t* rows_dev, const float* scores_dev, int P, const int64_t* grp_off,
                             const float* weights, int G, int k, int mode, double rrf_k, double* fused_out_dev,
                             int64_t* rows_out_dev, uint32_t* members_out_dev, void* stream) {
    if (!rows_dev || !scores_dev || !grp_off || !fused_out_dev || !rows_out_dev) return set_err(HR_E_INVALID, "null argument");
    if (device < 0) return set_err(HR_E_INVALID, "device must not be negative");
    if (int rc = check_fuse(P, grp_off, weights, G, k, mode, rrf_k)) return rc;
    std::lock_guard<std::mutex> lk(g_fuse_mu);
    HIP_TRY(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_fuse(rows_dev, scores_dev, P, grp_off, weights, G, k, mode, rrf_k, fused_out_dev, rows_out_dev,
                             members_out_dev, st, &g_fuse_list[device & 63], &g_fuse_host))
        return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the staged offsets are read until here)
    return HR_OK;
}

extern "C" int hr_index_search_fused_device(hr_index* h, const float* q_dev, const int64_t* grp_off, const float* weights,
                                            int G, int k, int fetch_k, int mode, double rrf_k,
                                            const uint64_t* masks_dev, int D, int64_t mask_stride,
                                            const int32_t* mask_of_dev, double* fused_out_dev, int64_t* rows_out_dev,
                                            uint32_t* members_out_dev, void* stream) {
    if (!h || !q_dev || !grp_off || !fused_out_dev || !rows_out_dev || (D > 0 && (!masks_dev || !mask_of_dev)))
        return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    int P = 0;
    if (int rc = check_search(h, grp_off, weights, G, k, fetch_k, mode, rrf_k, &P)) return rc;
    if (D < 0) return set_err(HR_E_INVALID, "D must not be negative");
    if (int rc = set_device(h)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int Q = (int)grp_off[G];
    std::vector<int32_t> of;
    if (D > 0) {
        of.resize((size_t)Q);
        HIP_TRY(hipMemcpyAsync(of.data(), mask_of_dev, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (int rc = index_validate_masks(h, Q, D, mask_stride, of.data())) return rc;
    }
    return fused_impl(h, q_dev, grp_off, weights, G, k, P, mode, rrf_k, masks_dev, mask_stride, mask_of_dev,
                      D > 0 ? of.data() : nullptr, fused_out_dev, rows_out_dev, members_out_dev, st);
}

extern "C" int hr_index_search_fused(hr_index* h, const float* q, const int64_t* grp_off, const float* weights, int G,
                                     int k, int fetch_k, int mode, double rrf_k, const uint64_t* masks, int D,
                                     int64_t mask_stride, const int32_t* mask_of, double* fused_out, int64_t* rows_out,
                                     uint32_t* members_out) {
    if (!h || !q || !grp_off || !fused_out || !rows_out || (D > 0 && (!masks || !mask_of)))
        return set_err(HR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    int P = 0;
    if (int rc = check_search(h, grp_off, weights, G, k, fetch_k, mode, rrf_k, &P)) return rc;
    if (D < 0) return set_err(HR_E_INVALID, "D must not be negative");
    const int Q = (int)grp_off[G];
    if (D > 0)
        if (int rc = index_validate_masks(h, Q, D, mask_stride, mask_of)) return rc;
    if (int rc = set_device(h)) return rc;
    hipStream_t st = h->stream;
    const size_t nk = (size_t)G * k;
    OutSeg out[3] = {{fused_out, nk * 8}, {rows_out, nk * 8}, {members_out, nk * 4}};
    float* q_dev = nullptr;
    uint64_t* masks_dev = nullptr;
    int32_t* of_dev = nullptr;
    if (int rc = stage_out(h, out)) return rc;
    if (int rc = stage_queries(h, q, Q, st, &q_dev)) return rc;
    const int64_t words64 = (h->n + 63) / 64;
    const bool masked = D > 0 && words64 > 0;  // else: the plain search, and no pointer of an earlier call's masks
    if (masked)
        if (int rc = stage_masks(h, masks, D, mask_stride, mask_of, Q, st, &masks_dev, &of_dev)) return rc;
    if (int rc = fused_impl(h, q_dev, grp_off, weights, G, k, P, mode, rrf_k, masks_dev, words64, of_dev,
                            masked ? mask_of : nullptr, out[0].as<double>(), out[1].as<int64_t>(), out[2].as<uint32_t>(), st))
        return rc;
    if (int rc = stage_download(out, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return HR_OK;
}
