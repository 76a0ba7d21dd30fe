// hr_qmask.hip -- prep kernels of a search with per-query row masks (hr_index_search_masks, DESIGN.md "Mixed-filter
// batches"): a chunk of up to 64 queries, each with its own row bitmap (or none), shares ONE corpus pass.
//
//   k_qmask_union   OR of the bitmaps the chunk references, one u32 word per tile: the existing tile-list builder
//                   (build_tile_list, hr_exhaustive.hip) then finds the tiles SOME query of the chunk allows.
//   k_qallow_build  the lane-order allow words the QM scans read (through ScanArgs::mask): for every visited tile, one u32
//                   per lane whose bit qb*16+i says "the row this lane's slot holds is live and allowed for the query
//                   in accumulator register (qb, i)".  The 64 query words x 32 rows of a tile are transposed here,
//                   once, by 16*QB lane shuffles per lane -- not in the FILTER's epilogue.  The table is indexed by
//                   tile (8 bytes per index row); with a tile list only the listed tiles are written and read.
#include "hr_internal.hpp"
#include "hr_kernels.hpp"

namespace hr {

namespace {

__global__ __launch_bounds__(256) void k_qmask_union(const uint64_t* __restrict__ masks, int64_t stride, QMaskRefs refs,
                                                     int nref, int64_t n_tiles, uint32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t w = 0;
    for (int r = 0; r < nref; ++r) w |= ((const uint32_t*)(masks + (int64_t)refs.d[r] * stride))[t];
    out[t] = w;
}

// one wave per visited unit, four per workgroup; B <= QB * 32 queries, mask_of[q] in [-1, D) (checked by the host)
__global__ __launch_bounds__(256) void k_qallow_build(const uint64_t* __restrict__ masks, int64_t stride,
                                                      const int32_t* __restrict__ mask_of, int B, int QB,
                                                      const uint32_t* __restrict__ live,
                                                      const uint32_t* __restrict__ tile_list, int64_t n_units,
                                                      uint32_t* __restrict__ qallow) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_units) return;  // (the whole wave)
    const int64_t t = tile_list ? (int64_t)tile_list[u] : u;
    // lane q: query q's word of this tile (all ones without a mask, 0 for a padded query), live rows only
    uint32_t w = 0;
    if (lane < B) {
        const int d = mask_of[lane];
        w = d < 0 ? 0xFFFFFFFFu : ((const uint32_t*)(masks + (int64_t)d * stride))[t];
    }
    w &= live[t];
    const int half = lane >> 5;
    const int r = slot_row(t, lane & 31);
    uint32_t aw = 0;
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t wq = (uint32_t)__shfl((int)w, acc_query(qb, i, half), 64);
            aw |= ((wq >> r) & 1u) << (qb * 16 + i);
        }
    qallow[t * 64 + lane] = aw;
}

}  // namespace

int launch_qmask_union(const uint64_t* masks, int64_t stride, const QMaskRefs& refs, int nref, int64_t n_tiles,
                       uint32_t* out, hipStream_t st) {
    if (n_tiles <= 0) return HR_OK;
    hipLaunchKernelGGL(k_qmask_union, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, st, masks, stride, refs, nref,
                       n_tiles, out);
    return hipGetLastError() == hipSuccess ? HR_OK : HR_E_HIP;
}

int launch_qallow_build(const uint64_t* masks, int64_t stride, const int32_t* mask_of, int B, int QB, const uint32_t* live,
                        const uint32_t* tile_list, int64_t n_units, uint32_t* qallow, hipStream_t st) {
    if (n_units <= 0) return HR_OK;
    hipLaunchKernelGGL(k_qallow_build, dim3((unsigned)((n_units + 3) / 4)), dim3(256), 0, st, masks, stride, mask_of, B, QB,
                       live, tile_list, n_units, qallow);
    return hipGetLastError() == hipSuccess ? HR_OK : HR_E_HIP;
}

}  // namespace hr
