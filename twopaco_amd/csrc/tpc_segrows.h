// tpc_segrows.h -- the ROW of every event of the segment table: the index of its segment among the first bits in event order.
// Shared by the stages that group the events of the last tpc_segments_build_* by segment (tpc_colors.hip, tpc_links.hip,
// tpc_bubbles.hip).  The build's first-sight table is gone by the time they run, so it is made again:
//   k_col_flags    rank[e] = first bit of e; one exclusive scan makes it the row of every first event (the total is the row count)
//   k_col_min      table[|name[e]|] = min(e), as k_seg_min of tpc_segments.hip ('N'-named events, names >= 2^34, are their own row)
// and the row of event e is rank[table[|name[e]|]], or rank[e] for an 'N'-named one.  Every including unit gets its own copy of
// the kernels (anonymous namespace).  link_side: the SIDE of an event, row << 1 | (name < 0), as the link table and the bubble
// table hold an oriented segment in 32 bits.
#pragma once
#include "tpc_ctx.h"

namespace {

constexpr int64_t COL_FRESH = (int64_t)1 << 34;  // first fresh name (tpc_segments.hip: SEG_FRESH)

__device__ __forceinline__ uint64_t col_mag(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// n_events + 1 entries: the scan's last element is the row count
__global__ void k_col_flags(const uint32_t *__restrict__ first, uint64_t n_events, uint32_t *__restrict__ rank)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n_events; e += stride)
        rank[e] = e < n_events ? (first[e >> 5] >> (e & 31)) & 1u : 0u;
}

__global__ void k_col_min(const int64_t *__restrict__ name, uint64_t n_events, uint32_t *__restrict__ table, uint64_t n_table)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        const int64_t nm = name[e];
        if (nm >= COL_FRESH) continue;
        const uint64_t m = col_mag(nm);
        if (m < n_table) atomicMin(&table[m], (uint32_t)e);
    }
}

// row << 1 | strand of event e, 0xFFFFFFFF when the table does not know its segment (cannot happen after a good build)
__device__ __forceinline__ uint32_t link_side(const int64_t *__restrict__ name, uint64_t e, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table,
                                              const uint32_t *__restrict__ rank, uint64_t n_rows)
{
    const int64_t nm = name[e];
    const uint64_t m = col_mag(nm);
    const uint32_t e0 = (nm >= COL_FRESH || m >= n_table) ? (uint32_t)e : table[m];
    const uint32_t row = e0 < n_events ? rank[e0] : 0xFFFFFFFFu;
    return row < n_rows ? (row << 1) | (nm < 0 ? 1u : 0u) : 0xFFFFFFFFu;
}

unsigned col_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

}  // namespace
