// hr_lex.hip -- the lexical (BM25) index: an hr_lex handle holding a forward index in CSR form on one device, and
// its scan.  Scoring definition and the bit-exact contract: DESIGN.md "Keyword search"; host half (packing, the
// fp64 tables): hr_lex_host.cpp.
//
//   k_lex_score  streams the entries once per sub-batch of <= 64 queries.  A workgroup takes blocks of 64
//                consecutive rows (their entries are adjacent in CSR: one contiguous range, read with 16-byte
//                loads); every entry's term is looked up in an LDS hash table of the sub-batch's distinct terms;
//                a hit adds llrint(c * 2^32) to the 64-bit LDS accumulator of every (row, query) asking for the
//                term (integer adds: any order gives the same sum).  After the block, each (row, query) that
//                matched and whose row is live and allowed becomes a {score, row} record in the query's segment
//                (one global counter add per block and query).  No B x n score matrix exists anywhere.
//   k_lex_pad    marks the unused tail of every segment absent (row -1).
//   k_topk_cand  (hr_topk_records) the exact top-k of every segment, (score desc, row asc).
#include <map>

#include "hr_internal.hpp"
#include "hr_lex.hpp"

using namespace hrlex;

namespace {

constexpr int kRowsPerBlock = 64;
constexpr int kLexThreads = 256;
constexpr int kLoads = 4;                    // 16-byte loads a lane issues back to back
constexpr int kMaxSub = 64;                  // queries per sub-batch (one bit each in a row's 64-bit hit word)
constexpr size_t kLdsBudget = 64 * 1024;     // dynamic LDS of k_lex_score (no opt-in above 64 KiB needed)
constexpr int64_t kMinWorkspace = 16 << 20;  // candidate records a sub-batch may fill: max(n, this)
constexpr uint32_t kEmpty = 0xFFFFFFFFu;

struct LexArgs {
    const int64_t* off;     // n + 1 CSR offsets
    const uint32_t* ent;    // term << 10 | tf
    const uint16_t* dl;
    const uint32_t* live;   // bit r of word r / 32
    const uint32_t* mask;   // same layout, nullable
    const double* ktab;     // K[dl]
    int64_t n, n_blocks;
    int Bs, H, hshift, P;   // sub-batch queries; hash slots (power of two) and 32 - log2 H; (term, query) pairs
    const int64_t* seg_off;            // Bs + 1
    unsigned long long* cnt;           // Bs
    const double* pair_A;              // P
    const uint32_t* ht_key;            // H
    const uint32_t* ht_rng;            // H: first pair << 16 | pairs
    const uint16_t* pair_q;            // P
    Cand* ws;
};

// LDS layout of k_lex_score (bytes), shared by the kernel and the host's sub-batch planning
struct LexLds {
    size_t acc, hit, offs, seg, base, pA, hk, hr, lcnt, lpos, pq, flag, total;
    __host__ __device__ LexLds(int Bs, int H, int P) {
        size_t o = 0;
        acc = o, o += (size_t)8 * kRowsPerBlock * Bs;
        hit = o, o += 8 * kRowsPerBlock;
        offs = o, o += 8 * (kRowsPerBlock + 2);
        seg = o, o += (size_t)8 * (Bs + 1);
        base = o, o += (size_t)8 * Bs;
        pA = o, o += (size_t)8 * P;
        hk = o, o += (size_t)4 * H;
        hr = o, o += (size_t)4 * H;
        lcnt = o, o += (size_t)4 * Bs;
        flag = o, o += 4;
        lpos = o, o += (size_t)2 * kRowsPerBlock * Bs;
        pq = o, o += (size_t)2 * P;
        total = (o + 15) & ~(size_t)15;
    }
};

__global__ __launch_bounds__(kLexThreads) void k_lex_score(LexArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    const LexLds L(a.Bs, a.H, a.P);
    long long* acc = (long long*)(smem + L.acc);
    unsigned long long* hit = (unsigned long long*)(smem + L.hit);
    int64_t* offs = (int64_t*)(smem + L.offs);
    int64_t* seg = (int64_t*)(smem + L.seg);
    unsigned long long* base = (unsigned long long*)(smem + L.base);
    double* pA = (double*)(smem + L.pA);
    uint32_t* hk = (uint32_t*)(smem + L.hk);
    uint32_t* hr = (uint32_t*)(smem + L.hr);
    uint32_t* lcnt = (uint32_t*)(smem + L.lcnt);
    int* flag = (int*)(smem + L.flag);
    uint16_t* lpos = (uint16_t*)(smem + L.lpos);
    uint16_t* pq = (uint16_t*)(smem + L.pq);
    const int tid = threadIdx.x, Bs = a.Bs, H = a.H, nacc = kRowsPerBlock * Bs;

    for (int i = tid; i < nacc; i += kLexThreads) acc[i] = 0;
    for (int i = tid; i <= Bs; i += kLexThreads) seg[i] = a.seg_off[i];
    for (int i = tid; i < a.P; i += kLexThreads) {
        pA[i] = a.pair_A[i];
        pq[i] = a.pair_q[i];
    }
    for (int i = tid; i < H; i += kLexThreads) {
        hk[i] = a.ht_key[i];
        hr[i] = a.ht_rng[i];
    }

    for (int64_t blk = blockIdx.x; blk < a.n_blocks; blk += gridDim.x) {
        const int64_t r0 = blk * kRowsPerBlock;
        if (tid <= kRowsPerBlock) {
            const int64_t r = r0 + tid;
            offs[tid] = a.off[r < a.n ? r : a.n];  // rows past n: empty
        }
        if (tid < kRowsPerBlock) hit[tid] = 0;
        if (tid < Bs) lcnt[tid] = 0;
        if (tid == 0) *flag = 0;
        __syncthreads();
        const int64_t e0 = offs[0], e1 = offs[kRowsPerBlock];
        // 16-byte loads from the aligned address at or below e0 (the array's capacity is a multiple of 4 entries),
        // kLoads of them in flight per lane before the first is used
        for (int64_t i0 = (e0 & ~(int64_t)3) + 4 * tid; i0 < e1; i0 += 4 * kLexThreads * kLoads) {
            uint4 v[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int64_t i = i0 + (int64_t)u * 4 * kLexThreads;
                v[u] = i < e1 ? *(const uint4*)(a.ent + i) : uint4{0, 0, 0, 0};
            }
#pragma unroll
            for (int uc = 0; uc < 4 * kLoads; ++uc) {
                const int u = uc >> 2, c = uc & 3;
                const int64_t idx = i0 + (int64_t)u * 4 * kLexThreads + c;
                if (idx < e0 || idx >= e1) continue;
                const uint32_t ev = c == 0 ? v[u].x : c == 1 ? v[u].y : c == 2 ? v[u].z : v[u].w;
                const uint32_t term = ev >> kTfBits;
                uint32_t slot = (term * 2654435761u) >> a.hshift;
                uint32_t key = hk[slot];
                while (key != term && key != kEmpty) {  // (at most half the slots are taken)
                    slot = (slot + 1) & (H - 1);
                    key = hk[slot];
                }
                if (key != term) continue;
                int lo = 0, hi = kRowsPerBlock;  // the row: offs[lo] <= idx < offs[lo + 1]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (offs[mid] <= idx) lo = mid;
                    else hi = mid;
                }
                const double tf = (double)(ev & kTfMax);
                const double den = tf + a.ktab[a.dl[r0 + lo]];
                const uint32_t rng = hr[slot];
                const int p0 = rng >> 16, np = rng & 0xFFFF;
                unsigned long long bits = 0;
                for (int j = 0; j < np; ++j) {
                    const double cval = (pA[p0 + j] * tf) / den;  // (contraction is off in this function)
                    const long long fx = __double2ll_rn(cval * 4294967296.0);  // round half to even
                    const int q = pq[p0 + j];
                    atomicAdd((unsigned long long*)&acc[lo * Bs + q], (unsigned long long)fx);
                    bits |= 1ull << q;
                }
                atomicOr(&hit[lo], bits);
                *flag = 1;
            }
        }
        __syncthreads();
        if (*flag) {  // (block-uniform)
            // a slot in its query's segment for every (row, query) that matched on a live, allowed row: first
            // within the block (LDS counter), then one global add per query
            for (int i = tid; i < nacc; i += kLexThreads) {
                const int row = i / Bs, q = i - row * Bs;
                uint16_t lp = 0xFFFF;
                if ((hit[row] >> q) & 1) {
                    const int64_t r = r0 + row;
                    bool ok = r < a.n && ((a.live[r >> 5] >> (r & 31)) & 1);
                    if (ok && a.mask) ok = (a.mask[r >> 5] >> (r & 31)) & 1;
                    if (ok) lp = (uint16_t)atomicAdd(&lcnt[q], 1u);
                }
                lpos[i] = lp;
            }
            __syncthreads();
            if (tid < Bs) base[tid] = lcnt[tid] ? atomicAdd(&a.cnt[tid], (unsigned long long)lcnt[tid]) : 0ull;
            __syncthreads();
            for (int i = tid; i < nacc; i += kLexThreads) {
                const int row = i / Bs, q = i - row * Bs;
                const uint16_t lp = lpos[i];
                if (lp != 0xFFFF) {
                    const int64_t pos = (int64_t)base[q] + lp, cap = seg[q + 1] - seg[q];
                    if (pos < cap)  // (always: the capacity is the sum of the query's document frequencies)
                        a.ws[seg[q] + pos] = Cand{(double)acc[i] * (1.0 / 4294967296.0), r0 + row};
                }
                acc[i] = 0;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_lex_pad(const int64_t* __restrict__ seg_off,
                                                 const unsigned long long* __restrict__ cnt, Cand* __restrict__ ws) {
    const int q = blockIdx.x;
    const int64_t lo = seg_off[q], cap = seg_off[q + 1] - lo;
    const int64_t c = (int64_t)cnt[q] < cap ? (int64_t)cnt[q] : cap;
    for (int64_t i = c + (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.y * blockDim.x)
        ws[lo + i] = Cand{-__builtin_inf(), -1};
}

// a device array that grows by doubling and keeps its contents
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    hipError_t ensure(size_t need, size_t used, size_t initial, hipStream_t st) {
        if (need <= cap) return hipSuccess;
        size_t want = std::max(std::max(need, 2 * cap), initial);
        want = (want + 15) & ~(size_t)15;
        void* np = nullptr;
        hipError_t e = hipMalloc(&np, want);
        if (e != hipSuccess) return e;
        if (p && used) e = hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(np);
            return e;
        }
        if (p) (void)hipFree(p);
        p = np;
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

struct hr_lex {
    int device = 0, n_cu = 256;
    hipStream_t st = nullptr;
    std::mutex mu;
    int64_t n = 0, n_live = 0, sum_dl = 0, n_entries = 0;
    int max_dl = 0;
    std::vector<int64_t> h_off{0};   // host mirrors of the offsets, dl and the live bitmap
    std::vector<uint16_t> h_dl;
    std::vector<uint32_t> h_live;
    std::vector<int32_t> df;         // 2^22 document frequencies over live rows
    GrowBuf d_off, d_ent, d_dl, d_live;
    DevBuf d_mask, d_ktab, d_tab, d_ws, d_out;
    std::vector<hipEvent_t> evs;
    // the K table on the device is valid for these
    double kt_k1 = -1, kt_b = -1;
    int64_t kt_sum = -1, kt_n = -1;
    int kt_max = -1;
    double last_ms[3] = {0, 0, 0};
};

extern "C" int hr_lex_create(int device, hr_lex** out) {
    if (!out || device < 0) return set_err(HR_E_INVALID, "hr_lex_create: bad arguments");
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device >= n_dev) return set_err(HR_E_INVALID, "hr_lex_create: no such device");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    auto* h = new hr_lex;
    h->device = device;
    h->n_cu = std::max(1, prop.multiProcessorCount);
    hipError_t e = hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return set_err(HR_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    h->df.assign(kTermSpan, 0);
    *out = h;
    return HR_OK;
}

extern "C" void hr_lex_destroy(hr_lex* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    for (hipEvent_t e : h->evs) (void)hipEventDestroy(e);
    h->d_off.release(), h->d_ent.release(), h->d_dl.release(), h->d_live.release();
    h->d_mask.release(), h->d_ktab.release(), h->d_tab.release(), h->d_ws.release(), h->d_out.release();
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
}

extern "C" int hr_lex_add(hr_lex* h, const uint32_t* tokens, const int64_t* offsets, int64_t n,
                          int64_t* first_row_out) {
    if (!h || n < 0 || (n > 0 && !offsets)) return set_err(HR_E_INVALID, "hr_lex_add: bad arguments");
    std::lock_guard<std::mutex> g(h->mu);
    if (first_row_out) *first_row_out = h->n;
    if (n == 0) return HR_OK;
    if (offsets[0] < 0 || offsets[n] < offsets[0]) return set_err(HR_E_INVALID, "hr_lex_add: bad offsets");
    const int64_t n_tok = offsets[n] - offsets[0];
    std::vector<uint32_t> ent((size_t)std::max<int64_t>(n_tok, 1));
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<uint16_t> dl((size_t)n);
    std::vector<int64_t> rel((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) rel[i] = offsets[i] - offsets[0];
    int rc = hr_lex_pack(tokens ? tokens + offsets[0] : nullptr, rel.data(), n, ent.data(), n_tok, off.data(),
                         dl.data());
    if (rc != HR_OK) return rc;
    const int64_t n_ent = off[n], n_new = h->n + n;
    HIP_TRY(hipSetDevice(h->device));
    // (4 entries of slack: the scan reads whole 16-byte groups)
    HIP_TRY(h->d_ent.ensure((size_t)(h->n_entries + n_ent + 4) * 4, (size_t)h->n_entries * 4, (size_t)16384 * 4, h->st));
    HIP_TRY(h->d_off.ensure((size_t)(n_new + 1) * 8, (size_t)(h->n + 1) * 8, 1025 * 8, h->st));
    HIP_TRY(h->d_dl.ensure((size_t)n_new * 2, (size_t)h->n * 2, 1024 * 2, h->st));
    const size_t w_old = (size_t)(h->n + 31) / 32, w_new = (size_t)(n_new + 31) / 32;
    HIP_TRY(h->d_live.ensure(w_new * 4, w_old * 4, 1024 / 8, h->st));
    for (int64_t i = 0; i <= n; ++i) off[i] += h->n_entries;
    if (n_ent)
        HIP_TRY(hipMemcpyAsync((uint32_t*)h->d_ent.p + h->n_entries, ent.data(), (size_t)n_ent * 4,
                               hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemcpyAsync((int64_t*)h->d_off.p + h->n, off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemcpyAsync((uint16_t*)h->d_dl.p + h->n, dl.data(), (size_t)n * 2, hipMemcpyHostToDevice, h->st));
    h->h_live.resize(w_new, 0u);
    for (int64_t r = h->n; r < n_new; ++r) h->h_live[r >> 5] |= 1u << (r & 31);
    const size_t w0 = (size_t)h->n / 32;
    HIP_TRY(hipMemcpyAsync((uint32_t*)h->d_live.p + w0, h->h_live.data() + w0, (w_new - w0) * 4, hipMemcpyHostToDevice,
                           h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    // the device holds the rows: now the host state
    h->h_off.insert(h->h_off.end(), off.begin() + 1, off.end());
    h->h_dl.insert(h->h_dl.end(), dl.begin(), dl.end());
    for (int64_t i = 0; i < n_ent; ++i) ++h->df[ent[i] >> kTfBits];
    for (int64_t i = 0; i < n; ++i) {
        h->sum_dl += dl[i];
        h->max_dl = std::max(h->max_dl, (int)dl[i]);
    }
    h->n = n_new;
    h->n_live += n;
    h->n_entries += n_ent;
    return HR_OK;
}

extern "C" int hr_lex_remove(hr_lex* h, const int64_t* rows, int64_t n) {
    if (!h || n < 0 || (n > 0 && !rows)) return set_err(HR_E_INVALID, "hr_lex_remove: bad arguments");
    std::lock_guard<std::mutex> g(h->mu);
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= h->n) return set_err(HR_E_INVALID, "hr_lex_remove: row out of range");
    if (n == 0) return HR_OK;
    HIP_TRY(hipSetDevice(h->device));
    std::vector<uint32_t> ent;
    size_t w_lo = SIZE_MAX, w_hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rows[i];
        if (!((h->h_live[r >> 5] >> (r & 31)) & 1)) continue;  // already dead (or repeated in this call)
        const int64_t e0 = h->h_off[r], e1 = h->h_off[r + 1];
        ent.resize((size_t)(e1 - e0));
        if (e1 > e0) {  // the row's terms, from the device arrays
            HIP_TRY(hipMemcpyAsync(ent.data(), (const uint32_t*)h->d_ent.p + e0, (size_t)(e1 - e0) * 4,
                                   hipMemcpyDeviceToHost, h->st));
            HIP_TRY(hipStreamSynchronize(h->st));
        }
        for (uint32_t e : ent) --h->df[e >> kTfBits];
        h->sum_dl -= h->h_dl[r];
        h->h_live[r >> 5] &= ~(1u << (r & 31));
        --h->n_live;
        w_lo = std::min(w_lo, (size_t)(r >> 5));
        w_hi = std::max(w_hi, (size_t)(r >> 5));
    }
    if (w_lo != SIZE_MAX) {
        HIP_TRY(hipMemcpyAsync((uint32_t*)h->d_live.p + w_lo, h->h_live.data() + w_lo, (w_hi - w_lo + 1) * 4,
                               hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipStreamSynchronize(h->st));
    }
    return HR_OK;
}

extern "C" int hr_lex_size(hr_lex* h, int64_t* n_out, int64_t* n_live_out) {
    if (!h) return set_err(HR_E_INVALID, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    if (n_out) *n_out = h->n;
    if (n_live_out) *n_live_out = h->n_live;
    return HR_OK;
}

extern "C" int hr_lex_stats(hr_lex* h, int64_t* n_live_out, int64_t* sum_dl_out) {
    if (!h) return set_err(HR_E_INVALID, "null handle");
    std::lock_guard<std::mutex> g(h->mu);
    if (n_live_out) *n_live_out = h->n_live;
    if (sum_dl_out) *sum_dl_out = h->sum_dl;
    return HR_OK;
}

extern "C" int hr_lex_df(hr_lex* h, const uint32_t* terms, int64_t n_terms, int32_t* df_out) {
    if (!h || n_terms < 0 || (n_terms > 0 && (!terms || !df_out))) return set_err(HR_E_INVALID, "hr_lex_df: bad arguments");
    std::lock_guard<std::mutex> g(h->mu);
    for (int64_t i = 0; i < n_terms; ++i) {
        if (terms[i] >= kTermSpan) return set_err(HR_E_INVALID, "hr_lex_df: term id beyond HR_LEX_TERM_BITS");
        df_out[i] = h->df[terms[i]];
    }
    return HR_OK;
}

extern "C" int hr_lex_last_ms(hr_lex* h, double* out) {
    if (!h || !out) return set_err(HR_E_INVALID, "hr_lex_last_ms: bad arguments");
    std::lock_guard<std::mutex> g(h->mu);
    for (int i = 0; i < 3; ++i) out[i] = h->last_ms[i];
    return HR_OK;
}

namespace {

struct SubBatch {
    std::vector<int> queries;          // indices into the call's batch
    std::map<uint32_t, int> terms;     // distinct term -> number of queries asking for it
    int64_t records = 0;
    int pairs = 0;
};

int hash_slots(int n_terms) {
    int H = 16;
    while (H < 2 * n_terms) H <<= 1;
    return H;
}

}  // namespace

extern "C" int hr_lex_search(hr_lex* h, const uint32_t* q_terms, const int64_t* q_off, int B, int k, double k1,
                             double b, const uint64_t* row_mask, double* scores_out, int64_t* rows_out) {
    if (!h || B < 0 || (B > 0 && (!q_off || !scores_out || !rows_out)))
        return set_err(HR_E_INVALID, "hr_lex_search: bad arguments");
    if (k < 1 || k > HR_LEX_MAX_K) return set_err(HR_E_INVALID, "hr_lex_search: need 1 <= k <= 1024");
    if (!(k1 >= 0.0) || !std::isfinite(k1) || !(b >= 0.0 && b <= 1.0))
        return set_err(HR_E_INVALID, "hr_lex_search: need k1 >= 0 and 0 <= b <= 1");
    std::lock_guard<std::mutex> g(h->mu);
    for (int64_t i = 0; i < (int64_t)B * k; ++i) {
        scores_out[i] = -__builtin_inf();
        rows_out[i] = -1;
    }
    h->last_ms[0] = h->last_ms[1] = h->last_ms[2] = 0;
    // the queries' terms: distinct, the HR_LEX_MAX_QTERMS smallest ids, those some live row holds
    std::vector<std::vector<uint32_t>> qt((size_t)B);
    std::vector<int64_t> cap((size_t)B, 0);
    std::vector<int> active;
    for (int i = 0; i < B; ++i) {
        const int64_t a0 = q_off[i], a1 = q_off[i + 1];
        if (a0 < 0 || a1 < a0 || (a1 > a0 && !q_terms)) return set_err(HR_E_INVALID, "hr_lex_search: bad query offsets");
        std::vector<uint32_t> t(q_terms + a0, q_terms + a1);
        for (uint32_t x : t)
            if (x >= kTermSpan) return set_err(HR_E_INVALID, "hr_lex_search: term id beyond HR_LEX_TERM_BITS");
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        if (t.size() > HR_LEX_MAX_QTERMS) t.resize(HR_LEX_MAX_QTERMS);
        for (uint32_t x : t)
            if (h->df[x] > 0) {
                qt[i].push_back(x);
                cap[i] += h->df[x];
            }
        cap[i] = std::min(cap[i], h->n);  // an exact upper bound on the query's hits
        if (!qt[i].empty()) active.push_back(i);
    }
    if (active.empty() || h->n_live == 0) return HR_OK;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st;

    // K[dl] for this (k1, b) and the current statistics (kept while they stay the same)
    if (h->kt_k1 != k1 || h->kt_b != b || h->kt_sum != h->sum_dl || h->kt_n != h->n_live || h->kt_max != h->max_dl) {
        std::vector<double> kt((size_t)h->max_dl + 1);
        bm25_K_table(k1, b, (double)h->sum_dl / (double)h->n_live, h->max_dl, kt.data());  // (sum_dl > 0: a df is)
        HIP_TRY(h->d_ktab.ensure(kt.size() * 8));
        HIP_TRY(hipMemcpyAsync(h->d_ktab.p, kt.data(), kt.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        h->kt_k1 = k1, h->kt_b = b, h->kt_sum = h->sum_dl, h->kt_n = h->n_live, h->kt_max = h->max_dl;
    }
    if (row_mask) {
        const size_t words = (size_t)(h->n + 63) / 64;
        HIP_TRY(h->d_mask.ensure(words * 8));
        HIP_TRY(hipMemcpyAsync(h->d_mask.p, row_mask, words * 8, hipMemcpyHostToDevice, st));
    }

    // sub-batches: <= 64 queries whose tables fit the LDS budget and whose segments fit the workspace
    const int64_t ws_budget = std::max(h->n, kMinWorkspace);
    std::vector<SubBatch> subs;
    for (int qi : active) {
        bool fits = false;
        if (!subs.empty()) {
            SubBatch& s = subs.back();
            int new_terms = 0;
            for (uint32_t t : qt[qi]) new_terms += !s.terms.count(t);
            const LexLds L((int)s.queries.size() + 1, hash_slots((int)s.terms.size() + new_terms),
                           s.pairs + (int)qt[qi].size());
            fits = (int)s.queries.size() < kMaxSub && L.total <= kLdsBudget && s.records + cap[qi] <= ws_budget;
        }
        if (!fits) subs.emplace_back();
        SubBatch& s = subs.back();
        s.queries.push_back(qi);
        for (uint32_t t : qt[qi]) ++s.terms[t];
        s.pairs += (int)qt[qi].size();
        s.records += cap[qi];
    }
    const int n_sub = (int)subs.size();
    while ((int)h->evs.size() < 3 * n_sub) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->evs.push_back(e);
    }
    HIP_TRY(h->d_out.ensure((size_t)active.size() * k * sizeof(Cand)));
    int64_t max_records = 0;
    size_t max_tab = 0;
    std::vector<std::vector<unsigned char>> blobs((size_t)n_sub);  // alive until the stream has copied them
    std::vector<size_t> tab_off((size_t)n_sub);
    struct TabLayout { size_t seg, cnt, pA, hk, hr, pq, total; };
    std::vector<TabLayout> lay((size_t)n_sub);
    for (int s = 0; s < n_sub; ++s) {
        const SubBatch& sb = subs[s];
        const int Bs = (int)sb.queries.size(), P = sb.pairs, H = hash_slots((int)sb.terms.size());
        TabLayout& t = lay[s];
        size_t o = 0;
        t.seg = o, o += (size_t)8 * (Bs + 1);
        t.cnt = o, o += (size_t)8 * Bs;
        t.pA = o, o += (size_t)8 * P;
        t.hk = o, o += (size_t)4 * H;
        t.hr = o, o += (size_t)4 * H;
        t.pq = o, o += (size_t)2 * P;
        t.total = (o + 255) & ~(size_t)255;
        tab_off[s] = max_tab;  // every sub-batch its own region: the uploads need not wait for the kernels
        max_tab += t.total;
        max_records = std::max(max_records, sb.records);
        std::vector<unsigned char>& blob = blobs[s];
        blob.assign(t.total, 0);
        int64_t* seg = (int64_t*)(blob.data() + t.seg);
        double* pA = (double*)(blob.data() + t.pA);
        uint32_t* hk = (uint32_t*)(blob.data() + t.hk);
        uint32_t* hr = (uint32_t*)(blob.data() + t.hr);
        uint16_t* pq = (uint16_t*)(blob.data() + t.pq);
        seg[0] = 0;
        for (int j = 0; j < Bs; ++j) seg[j + 1] = seg[j] + cap[sb.queries[j]];
        for (int j = 0; j < H; ++j) hk[j] = kEmpty;
        int hshift = 32;
        for (int x = H; x > 1; x >>= 1) --hshift;
        int p = 0;
        std::map<uint32_t, int> first;  // term -> its first pair
        for (const auto& kv : sb.terms) {
            first[kv.first] = p;
            uint32_t slot = (kv.first * 2654435761u) >> hshift;
            while (hk[slot] != kEmpty) slot = (slot + 1) & (uint32_t)(H - 1);
            hk[slot] = kv.first;
            hr[slot] = ((uint32_t)p << 16) | (uint32_t)kv.second;
            p += kv.second;
        }
        std::map<uint32_t, int> fill;
        for (int j = 0; j < Bs; ++j)
            for (uint32_t term : qt[sb.queries[j]]) {
                const int at = first[term] + fill[term]++;
                pA[at] = bm25_A(h->n_live, h->df[term], k1);
                pq[at] = (uint16_t)j;
            }
    }
    HIP_TRY(h->d_tab.ensure(max_tab));
    HIP_TRY(h->d_ws.ensure((size_t)std::max<int64_t>(max_records, 1) * sizeof(Cand)));
    const int64_t n_blocks = (h->n + kRowsPerBlock - 1) / kRowsPerBlock;
    int64_t done = 0;
    for (int s = 0; s < n_sub; ++s) {
        const SubBatch& sb = subs[s];
        const int Bs = (int)sb.queries.size(), P = sb.pairs, H = hash_slots((int)sb.terms.size());
        const TabLayout& t = lay[s];
        unsigned char* tab = (unsigned char*)h->d_tab.p + tab_off[s];
        HIP_TRY(hipMemcpyAsync(tab, blobs[s].data(), t.total, hipMemcpyHostToDevice, st));
        LexArgs a;
        a.off = (const int64_t*)h->d_off.p, a.ent = (const uint32_t*)h->d_ent.p, a.dl = (const uint16_t*)h->d_dl.p;
        a.live = (const uint32_t*)h->d_live.p, a.mask = row_mask ? h->d_mask.as<uint32_t>() : nullptr;
        a.ktab = h->d_ktab.as<double>();
        a.n = h->n, a.n_blocks = n_blocks;
        a.Bs = Bs, a.H = H, a.P = P;
        a.hshift = 32;
        for (int x = H; x > 1; x >>= 1) --a.hshift;
        a.seg_off = (const int64_t*)(tab + t.seg), a.cnt = (unsigned long long*)(tab + t.cnt);
        a.pair_A = (const double*)(tab + t.pA), a.ht_key = (const uint32_t*)(tab + t.hk);
        a.ht_rng = (const uint32_t*)(tab + t.hr), a.pair_q = (const uint16_t*)(tab + t.pq);
        a.ws = h->d_ws.as<Cand>();
        const LexLds L(Bs, H, P);
        if (L.total > kLdsBudget) return set_err(HR_E_UNSUPPORTED, "hr_lex_search: a query's tables exceed the LDS budget");
        const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / L.total));
        const int grid = (int)std::min<int64_t>(n_blocks, (int64_t)h->n_cu * per_cu);
        HIP_TRY(hipEventRecord(h->evs[3 * s], st));
        hipLaunchKernelGGL(k_lex_score, dim3(grid), dim3(kLexThreads), L.total, st, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_lex_pad, dim3(Bs, 16), dim3(256), 0, st, a.seg_off, a.cnt, a.ws);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(h->evs[3 * s + 1], st));
        int rc = hr_topk_records(a.ws, a.seg_off, 0, Bs, k, h->d_out.as<Cand>() + done * k, st);
        if (rc != HR_OK) return rc;
        HIP_TRY(hipEventRecord(h->evs[3 * s + 2], st));
        done += Bs;
    }
    std::vector<Cand> out((size_t)active.size() * k);
    HIP_TRY(hipMemcpyAsync(out.data(), h->d_out.p, out.size() * sizeof(Cand), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int s = 0; s < n_sub; ++s) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->evs[3 * s], h->evs[3 * s + 1]));
        h->last_ms[0] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->evs[3 * s + 1], h->evs[3 * s + 2]));
        h->last_ms[1] += ms;
    }
    h->last_ms[2] = n_sub;
    size_t j = 0;
    for (const SubBatch& sb : subs)
        for (int qi : sb.queries) {
            for (int i = 0; i < k; ++i) {
                scores_out[(size_t)qi * k + i] = out[j * k + i].score;
                rows_out[(size_t)qi * k + i] = out[j * k + i].row;
            }
            ++j;
        }
    return HR_OK;
}
