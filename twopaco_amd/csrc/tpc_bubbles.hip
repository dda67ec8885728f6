// tpc_bubbles.hip -- the SIMPLE BUBBLES of the compacted graph: the places where two segments leave one side of a segment, touch
// nothing else and meet again at one side of another segment -- a substitution or a short insertion / deletion between genomes.
// Kernels and the C-ABI of the tpc_segments_bubbles_* group of include/twopaco_hip.h, which defines side, arc, degree, bubble,
// canonical orientation and the order of arms and rows.  No counterpart in the reference; host/graphformat.h: ComputeBubbles is
// the serial statement.
//
// Input: the event table of the last tpc_segments_build_* and the link rows of the last tpc_segments_links_build (first_event[r]:
// the row is spelled (name[e - 1], name[e])).  The link stage keeps no sides, so the row of every event's segment is made again:
//   k_col_flags, scan, k_col_min   tpc_segrows.h, shared with tpc_colors.hip and tpc_links.hip
//   k_bub_arcs    one thread per link row.  from = side(e - 1), to = side(e) give the arcs from -> to and to ^ 1 -> from ^ 1; when
//                 both are one arc (to == from ^ 1) it counts once.  Per arc u -> v: atomicAdd(deg[u], 1), atomicMin(lo[u], v),
//                 atomicMax(hi[u], v).  The link table holds every class once, so every arc arrives once: nothing to fold, and
//                 whatever the order of the atomics deg / lo / hi end up the same.  No adjacency list: the definition only ever
//                 reads sides of degree 1 (lo is the neighbour) and 2 (lo and hi are the two).
//   k_bub_find    one thread per side: the definition, by at most ten dependent loads, and the canonical orientation; a flag
//   scan          exclusive, over the flags: the rank of every bubble, the total is their number
//   k_bub_rows    one thread per side: source, arm_a, arm_b, sink at the side's rank (ascending source code by construction)
//   k_bub_hist    sides by degree 0, 1, 2, 3, 4, 5+: counted per workgroup in LDS, then one atomic per bin and workgroup
// Memory: kept until the next segment, link or bubble build 16 B / bubble, 12 B / side (deg, lo, hi) and 48 B of histogram; during
// the call 4 B / event of ranks, the first-sight table (counts[3] of tpc_segments_counts), 4 B / side of flags and the scan's
// scratch.  None of it exists in a context that never asks for bubbles, and the segment, colour and link outputs are what they were.
// What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint64_t BUB_MAX_ROWS = ((uint64_t)1 << 31) - 1;   // a side is row << 1 | strand in 32 bits, all ones is no side (link_side, lo of degree 0)
constexpr uint32_t BUB_FLAG_ROW = 1u, BUB_FLAG_EVENT = 2u;
constexpr int BUB_BINS = 6;                             // degree 0 .. 4, 5 or more

__device__ __forceinline__ void bub_arc(uint32_t *__restrict__ deg, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, uint32_t u, uint32_t v)
{
    atomicAdd(&deg[u], 1u);
    atomicMin(&lo[u], v);
    atomicMax(&hi[u], v);
}

// deg / lo / hi: [n_sides], deg and hi zero, lo all ones.  counters[0]: the link rows that are their own reverse (one arc, not two)
__global__ void k_bub_arcs(const uint32_t *__restrict__ first_event, uint64_t n_links, const int64_t *__restrict__ name, uint64_t n_events,
                           const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows,
                           uint32_t *__restrict__ deg, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, unsigned long long *__restrict__ counters,
                           uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_links; r += stride) {
        const uint64_t e = first_event[r];
        if (e == 0 || e >= n_events) { atomicOr(flags, BUB_FLAG_EVENT); continue; }
        const uint32_t from = link_side(name, e - 1, n_events, table, n_table, rank, n_rows), to = link_side(name, e, n_events, table, n_table, rank, n_rows);
        if (from == 0xFFFFFFFFu || to == 0xFFFFFFFFu) { atomicOr(flags, BUB_FLAG_ROW); continue; }  // (a side is below 2 x n_rows otherwise)
        bub_arc(deg, lo, hi, from, to);
        if (to == (from ^ 1u)) atomicAdd(&counters[0], 1ull);   // a+ a-: its own reverse
        else bub_arc(deg, lo, hi, to ^ 1u, from ^ 1u);
    }
}

// the sink of the simple bubble whose source is s, by the definition of include/twopaco_hip.h; false when there is none
__device__ __forceinline__ bool bub_at(const uint32_t *__restrict__ deg, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint32_t s,
                                       uint32_t *arm_a, uint32_t *arm_b, uint32_t *sink)
{
    if (deg[s] != 2) return false;
    const uint32_t a = lo[s], b = hi[s];                 // out(s) = {a, b}, a < b
    if (deg[a ^ 1u] != 1 || deg[b ^ 1u] != 1) return false;   // s is the only way in to each arm
    if (deg[a] != 1 || deg[b] != 1) return false;
    const uint32_t t = lo[a];
    if (lo[b] != t) return false;                        // out(a) == out(b) == {t}
    if (deg[t ^ 1u] != 2) return false;
    const uint32_t rs = s >> 1, ra = a >> 1, rb = b >> 1, rt = t >> 1;
    if (rs == ra || rs == rb || rs == rt || ra == rb || ra == rt || rb == rt) return false;
    *arm_a = a; *arm_b = b; *sink = t;
    return true;
}

// n_sides + 1 entries: the scan's last element is the number of bubbles
__global__ void k_bub_find(const uint32_t *__restrict__ deg, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint64_t n_sides,
                           uint32_t *__restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_sides; i += stride) {
        uint32_t a, b, t;
        // reported once: the same bubble is found at t ^ 1 as well, the orientation with the smaller source code is the one kept
        flag[i] = i < n_sides && bub_at(deg, lo, hi, (uint32_t)i, &a, &b, &t) && (uint32_t)i < (t ^ 1u) ? 1u : 0u;
    }
}

// rows: [0, B) source, [B, 2B) arm_a, [2B, 3B) arm_b, [3B, 4B) sink.  where[i] is the exclusive scan of the flags: side i holds a
// bubble when where[i + 1] > where[i]
__global__ void k_bub_rows(const uint32_t *__restrict__ deg, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ hi, uint64_t n_sides,
                           const uint32_t *__restrict__ where, uint32_t *__restrict__ rows, uint64_t n_bubbles, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_sides; i += stride) {
        const uint64_t at = where[i];
        if (where[i + 1] == at) continue;
        uint32_t a, b, t;
        if (at >= n_bubbles || !bub_at(deg, lo, hi, (uint32_t)i, &a, &b, &t)) { atomicOr(flags, BUB_FLAG_ROW); continue; }
        rows[at] = (uint32_t)i;
        rows[n_bubbles + at] = a;
        rows[2 * n_bubbles + at] = b;
        rows[3 * n_bubbles + at] = t;
    }
}

__global__ void k_bub_hist(const uint32_t *__restrict__ deg, uint64_t n_sides, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned long long s_bins[BUB_BINS];
    if (threadIdx.x < BUB_BINS) s_bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_sides; i += stride) {
        const uint32_t d = deg[i];
        atomicAdd(&s_bins[d < BUB_BINS - 1 ? d : BUB_BINS - 1], 1ull);
    }
    __syncthreads();
    if (threadIdx.x < BUB_BINS && s_bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_bins[threadIdx.x]);
}

}  // namespace

extern "C" {

int tpc_segments_bubbles_build(tpc_ctx *c)
{
    if (!c) return -1;
    bubbles_drop(c);
    if (int rc = stage_needs_segments(c, "bubbles", "join")) return rc;
    if (!c->lnk.valid) return fail(c, -1, "segment bubbles: build the link table first (tpc_segments_links_build)");
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments, n_links = c->lnk.n_rows;
    if (n_rows > BUB_MAX_ROWS) return fail(c, -1, "segment bubbles: %llu segments, a side holds at most %llu", (unsigned long long)n_rows, (unsigned long long)BUB_MAX_ROWS);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n_sides = 2 * n_rows;

    // sizes in 64 bits, summed before the first allocation; the rows are not counted yet: their bound is one per two sides
    const uint64_t sides_bytes = n_sides * 12 + 16, hist_bytes = BUB_BINS * 8, flag_bytes = (n_sides + 1) * 4;
    const uint64_t rows_bound = n_rows * 16 + 16;
    size_t scan_flag = 0;
    uint32_t *flag = nullptr, *flags = nullptr;
    SegRows idx;
    if (!idx.size(c) || rocprim::exclusive_scan(nullptr, scan_flag, flag, flag, 0u, n_sides + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess)
        return fail(c, -10, "segment bubbles: the scan could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, scan_flag);   // one scratch for both scans
    const uint64_t need = sides_bytes + hist_bytes + flag_bytes + rows_bound + idx.bytes() + 16 + 64;
    if (int rc = stage_fits(c, "bubbles", need, "%llu of them the degree, smallest and largest neighbour of %llu sides", (unsigned long long)sides_bytes, (unsigned long long)n_sides))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) bubbles_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->bub.sides, sides_bytes) != hipSuccess || dev_malloc(c, (void **)&c->bub.hist, hist_bytes) != hipSuccess || !idx.alloc(c, temps) ||
        !temps.get(c, &flag, flag_bytes) || !temps.get(c, &flags, 64))
        return done(fail(c, -10, "segment bubbles: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    uint32_t *deg = c->bub.sides, *lo = deg + n_sides, *hi = lo + n_sides;
    unsigned long long *counters = (unsigned long long *)(flags + 2);   // 8 bytes into the 64: flags[0], then counters[0]
    hipStream_t s = c->stream;
    // degrees and largest neighbours zero, smallest neighbours all ones
    bool ok = hipMemsetAsync(c->bub.sides, 0, sides_bytes, s) == hipSuccess && (!n_sides || hipMemsetAsync(lo, 0xFF, n_sides * 4, s) == hipSuccess) &&
              hipMemsetAsync(c->bub.hist, 0, hist_bytes, s) == hipSuccess && idx.fill(s) &&
              hipMemsetAsync(flags, 0, 64, s) == hipSuccess;
    uint32_t n_bubbles = 0, raised = 0;
    unsigned long long own_reverse = 0;
    if (ok) {
        Timed t(c, TPC_K_BUBBLES);   // the whole stage on the stream, the wait for the bubble count included (as TPC_K_LINKS)
        ok = idx.enqueue(c);
        if (ok && n_links)
            hipLaunchKernelGGL(k_bub_arcs, dim3(col_grid(n_links)), dim3(256), 0, s, c->lnk.rows, n_links, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, deg, lo, hi,
                               counters, flags);
        if (ok) {
            hipLaunchKernelGGL(k_bub_find, dim3(col_grid(n_sides + 1)), dim3(256), 0, s, deg, lo, hi, n_sides, flag);
            ok = rocprim::exclusive_scan(idx.scan_tmp, scan_flag, flag, flag, 0u, n_sides + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        if (ok && n_sides) hipLaunchKernelGGL(k_bub_hist, dim3(std::min(col_grid(n_sides), 1024u)), dim3(256), 0, s, deg, n_sides, c->bub.hist);
        // the number of bubbles decides the size of what is kept: the one wait in the middle
        ok = ok && idx.total(s) && hipMemcpyAsync(&n_bubbles, flag + n_sides, sizeof n_bubbles, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&own_reverse, counters, sizeof own_reverse, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "bubbles", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment bubbles: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (raised & BUB_FLAG_EVENT) return done(fail(c, -10, "segment bubbles: a link row's first event lies outside the event table"));
        if (raised & BUB_FLAG_ROW) return done(fail(c, -10, "segment bubbles: an event's segment is missing from the first-sight table"));
        if (2 * (uint64_t)n_bubbles > n_sides || own_reverse > n_links)
            return done(fail(c, -10, "segment bubbles: %u bubbles on %llu sides", n_bubbles, (unsigned long long)n_sides));
        const uint64_t rows_bytes = (uint64_t)n_bubbles * 16 + 16;
        if (dev_malloc(c, (void **)&c->bub.rows, rows_bytes) != hipSuccess) return done(fail(c, -10, "segment bubbles: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        if (n_bubbles) hipLaunchKernelGGL(k_bub_rows, dim3(col_grid(n_sides)), dim3(256), 0, s, deg, lo, hi, n_sides, flag, c->bub.rows, (uint64_t)n_bubbles, flags);
        ok = hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->bub.peak_bytes = need - rows_bound + rows_bytes;
    }
    if (int rc = stage_wait(c, "bubbles", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment bubbles: a flagged side holds no bubble"));
    c->bub.n_rows = n_bubbles; c->bub.n_sides = n_sides; c->bub.arcs = 2 * n_links - own_reverse;
    c->bub.valid = true;
    return 0;
}

int tpc_segments_bubbles_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->bub.valid) return fail(c, -1, "segment bubbles: tpc_segments_bubbles_build first");
    if (!info) return fail(c, -1, "segment bubbles: info required");
    info[0] = c->bub.n_rows; info[1] = c->bub.n_sides; info[2] = c->bub.arcs; info[3] = c->bub.peak_bytes;
    return 0;
}

int tpc_segments_bubbles_fetch_rows(tpc_ctx *c, uint64_t b0, uint64_t n, uint32_t *source_host, uint32_t *arm_a_host, uint32_t *arm_b_host, uint32_t *sink_host)
{
    if (!c) return -1;
    if (!c->bub.valid) return fail(c, -1, "segment bubbles: tpc_segments_bubbles_build first");
    return fetch_planes(c, "bubbles", "row", c->bub.rows, c->bub.n_rows, b0, n, { source_host, arm_a_host, arm_b_host, sink_host });
}

int tpc_segments_bubbles_fetch_sides(tpc_ctx *c, uint64_t c0, uint64_t n, uint32_t *deg_host, uint32_t *lo_host, uint32_t *hi_host)
{
    if (!c) return -1;
    if (!c->bub.valid) return fail(c, -1, "segment bubbles: tpc_segments_bubbles_build first");
    return fetch_planes(c, "bubbles", "side", c->bub.sides, c->bub.n_sides, c0, n, { deg_host, lo_host, hi_host });
}

int tpc_segments_bubbles_fetch_hist(tpc_ctx *c, uint64_t *hist_host)
{
    if (!c) return -1;
    if (!c->bub.valid) return fail(c, -1, "segment bubbles: tpc_segments_bubbles_build first");
    if (!hist_host) return fail(c, -1, "segment bubbles: the histogram array is required");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(hist_host, c->bub.hist, BUB_BINS * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
