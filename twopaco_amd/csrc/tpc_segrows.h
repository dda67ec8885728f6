// tpc_segrows.h -- the ROW of every event of the segment table: the index of its segment among the first bits in event order.
// Shared by the stages that group the events of the last tpc_segments_build_* by segment (tpc_colors.hip, tpc_links.hip,
// tpc_bubbles.hip, tpc_components.hip, tpc_superbubbles.hip, tpc_anchors.hip) and by the edge index (tpc_locate.hip: the rank of a first event alone).  The build's first-sight table is gone by the time they run, so it is made again:
//   k_col_flags    rank[e] = first bit of e; one exclusive scan makes it the row of every first event (the total is the row count)
//   k_col_min      table[|name[e]|] = min(e), as k_seg_min of tpc_segments.hip ('N'-named events, names >= 2^34, are their own row)
// and the row of event e is rank[table[|name[e]|]], or rank[e] for an 'N'-named one.  Every including unit gets its own copy of
// the kernels (anonymous namespace).  link_side: the SIDE of an event, row << 1 | (name < 0), as the link table and the bubble
// table hold an oriented segment in 32 bits.  SegRows owns the index's three buffers for the length of one stage call: every
// stage builds its own inside its own call, none is kept between stages.
#pragma once
#include "tpc_stage.h"

#include <rocprim/rocprim.hpp>

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

// how many entries of seq_begin[0 .. n_rec] are <= e: one more than the sequence of event e (sequences without events share their
// entry with the next one that has some); 0 or n_rec + 1 when no sequence holds e
__device__ __forceinline__ uint32_t col_seq_end(const uint32_t *__restrict__ seq_begin, uint32_t n_rec, uint32_t e)
{
    uint32_t lo = 0, hi = n_rec + 1;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (seq_begin[mid] <= e) lo = mid + 1; else hi = mid; }
    return lo;
}

// HOT ROWS: the lanes of the run a head lane leads, from the ballots of the wave's head lanes and of its active lanes: this lane and
// the active ones above it, up to the next head
__device__ __forceinline__ unsigned long long col_run(uint32_t lane, unsigned long long heads, unsigned long long actives)
{
    const unsigned long long from = ~0ull << lane;
    const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
    return from & actives & (above ? ((1ull << (__ffsll((long long)above) - 1)) - 1) : ~0ull);
}

unsigned col_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

// The row index of one stage call: rank[n_events + 1], the first-sight table[n_table] and the scan's scratch.
struct SegRows {
    uint32_t *rank = nullptr, *table = nullptr;
    void *scan_tmp = nullptr;
    uint64_t n_events = 0, n_table = 0;
    size_t rank_bytes = 0, table_bytes = 0, scan_bytes = 0;
    size_t scan_alloc = 0;   // the scratch's size, the stage may raise it for a scan of its own over the same scratch
    uint32_t scanned = 0;    // the scan's total as read back by total(): the rows the first bits hold

    // the sizes alone, for the sum before the first allocation; false: the scan could not be sized
    bool size(tpc_ctx *c)
    {
        n_events = c->seg.events; n_table = c->seg.table_bytes / sizeof(uint32_t);
        rank_bytes = ((size_t)n_events + 1) * 4; table_bytes = (size_t)n_table * 4 + 16;
        const bool ok = rocprim::exclusive_scan(nullptr, scan_bytes, rank, rank, 0u, n_events + 1, rocprim::plus<uint32_t>(), c->stream) == hipSuccess;
        scan_alloc = scan_bytes;
        return ok;
    }
    uint64_t bytes() const { return (uint64_t)rank_bytes + table_bytes + scan_alloc; }
    bool alloc(tpc_ctx *c, StageTemps &temps) { return temps.get(c, &rank, rank_bytes) && temps.get(c, &table, table_bytes) && temps.get(c, &scan_tmp, scan_alloc + 16); }
    // no event seen yet: all ones
    bool fill(hipStream_t s) { return hipMemsetAsync(table, 0xFF, table_bytes, s) == hipSuccess; }
    // k_col_flags, the scan, k_col_min: after them the row of event e is rank[table[|name[e]|]]
    bool enqueue(tpc_ctx *c)
    {
        hipStream_t s = c->stream;
        hipLaunchKernelGGL(k_col_flags, dim3(col_grid(n_events + 1)), dim3(256), 0, s, c->seg.first, n_events, rank);
        if (rocprim::exclusive_scan(scan_tmp, scan_bytes, rank, rank, 0u, n_events + 1, rocprim::plus<uint32_t>(), s) != hipSuccess) return false;
        if (n_events) hipLaunchKernelGGL(k_col_min, dim3(col_grid(n_events)), dim3(256), 0, s, c->seg.name, n_events, table, n_table);
        return true;
    }
    bool total(hipStream_t s) { return hipMemcpyAsync(&scanned, rank + n_events, sizeof scanned, hipMemcpyDeviceToHost, s) == hipSuccess; }
};

}  // namespace
