// tpc_colors.hip -- the segment colour table: which colours (genomes, files, sequences -- the caller's map) hold each segment
// of the compacted graph, how often, on which strand; and the histogram of segments by their number of colours.  Kernels and
// the C-ABI of the tpc_segments_colors_* group of include/twopaco_hip.h.  No counterpart in the reference: its gfa1 defines the
// table (an S line with a body is a row, a C line one occurrence of a row in a sequence), host/graphformat.h: ComputeColors is
// the serial statement of it.
//
// Input: the event table the last tpc_segments_build_* left in the context (name[e], first[] bits, begin / end,
// seq_event_begin[]; tpc_segments.hip).  What that table lacks is the ROW of every event, the index of its segment among the
// first bits in event order.  The build's first-sight table is gone by then, so it is made again (tpc_segrows.h, shared with tpc_links.hip):
//   k_col_flags    rank[e] = first bit of e; one exclusive scan makes it the row of every first event (the total is the row count)
//   k_col_min      table[|name[e]|] = min(e), as k_seg_min of tpc_segments.hip ('N'-named events, names >= 2^34, are their own row)
//   k_col_scatter  one thread per event: row = rank[table[|name|]], colour = color_of_seq[sequence of e] (the sequence by binary
//                  search in seq_event_begin), then occurrences[row] += 1, forward[row] += name > 0, presence[row] |= bit(colour).
//                  HOT ROWS: a poly-A tract gives thousands of consecutive events of one segment in one sequence; one atomic per
//                  lane would queue a whole wave on one address.  Lanes compare their (row, colour) with the lane below (shuffle),
//                  the lanes that differ are run leaders (ballot), and a leader issues the run's atomics once: the add of the run
//                  length (popcount of the ballot between this leader and the next), the add of the run's forward lanes, one OR.
//   k_col_rows     one thread per row: n_colors = popcount of the row's presence words, length = end - begin + k of its first
//                  event, and the histogram bins [n_colors] += 1 / += length (64 bits both).  The bins are privatised in LDS while
//                  C + 1 of them fit (COL_LDS_BINS, 16 B each) and flushed once per block; beyond that they are global atomics.
// Memory: kept until the next build or the context's end 16 B / row (first event, occurrences, forward, n_colors), 4 B x ceil(C / 32)
// per row of presence, 16 B x (C + 1) of histogram; during the call also the first-sight table (counts[3] of tpc_segments_counts),
// 4 B / event of ranks, 4 B / sequence of colours.  None of it exists in a context that never asks for colours, and
// tpc_segments_counts reports what it reported before.  What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint32_t COL_MAX_COLORS = 1u << 31;     // the most colours of one build
constexpr uint32_t COL_LDS_BINS = 2048;          // histogram bins a block keeps in LDS: 2 x 8 B x 2048 = 32 KiB

// rows: [0, S) first event, [S, 2S) occurrences, [2S, 3S) forward.  A whole wave runs every iteration (the stride is a multiple of
// 64), lanes past the last event take part in the shuffles and ballots and nothing else.
__global__ void k_col_scatter(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table,
                              const uint32_t *__restrict__ rank, const uint32_t *__restrict__ seq_begin, uint32_t n_rec, const uint32_t *__restrict__ color,
                              uint32_t *__restrict__ rows, uint64_t n_rows, uint32_t *__restrict__ presence, uint32_t words)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e - lane < n_events; e += stride) {
        bool active = e < n_events, forward = false;
        uint32_t row = 0xFFFFFFFFu, col = 0xFFFFFFFFu;
        if (active) {
            const int64_t nm = name[e];
            const uint64_t m = col_mag(nm);
            const uint32_t e0 = (nm >= COL_FRESH || m >= n_table) ? (uint32_t)e : table[m];
            row = e0 < n_events ? rank[e0] : 0xFFFFFFFFu;
            const uint32_t lo = col_seq_end(seq_begin, n_rec, (uint32_t)e);
            active = row < n_rows && lo >= 1 && lo <= n_rec;  // (the build's caller checked that every event has a sequence)
            if (active) {
                col = color[lo - 1];
                forward = nm > 0;
                if (e0 == (uint32_t)e) rows[row] = (uint32_t)e;
            }
        }
        const uint32_t row_below = __shfl_up(row, 1), col_below = __shfl_up(col, 1);
        const bool head = active && (lane == 0 || row_below != row || col_below != col);
        const unsigned long long heads = __ballot(head), actives = __ballot(active), forwards = __ballot(active && forward);
        if (head) {
            const unsigned long long run = col_run(lane, heads, actives);
            // (inactive lanes sit between runs only behind the last event, or where a row was refused: they cut no run short that matters)
            atomicAdd(&rows[n_rows + row], (uint32_t)__popcll(run));
            const uint32_t nf = (uint32_t)__popcll(run & forwards);
            if (nf) atomicAdd(&rows[2 * n_rows + row], nf);
            atomicOr(&presence[(uint64_t)row * words + (col >> 5)], 1u << (col & 31));
        }
    }
}

// hist: [0, C] segments, [C + 1, 2C + 1] bases.  LDS: 2 x (C + 1) 64-bit bins of dynamic shared memory, or none.
template <bool LDS>
__global__ void k_col_rows(uint32_t *__restrict__ rows, uint64_t n_rows, const uint32_t *__restrict__ presence, uint32_t words, const uint32_t *__restrict__ begin,
                           const uint32_t *__restrict__ end, uint32_t k, unsigned long long *__restrict__ hist, uint32_t n_colors)
{
    extern __shared__ unsigned long long s_bins[];
    const uint32_t bins = n_colors + 1;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) s_bins[i] = 0;
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < words; w++) n += (uint32_t)__popc(presence[r * words + w]);
        rows[3 * n_rows + r] = n;
        const uint32_t e0 = rows[r];
        const unsigned long long length = (unsigned long long)end[e0] - begin[e0] + k;
        if (n > n_colors) continue;  // (cannot happen: every colour is below n_colors)
        if (LDS) { atomicAdd(&s_bins[n], 1ull); atomicAdd(&s_bins[bins + n], length); }
        else { atomicAdd(&hist[n], 1ull); atomicAdd(&hist[bins + n], length); }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 2 * bins; i += blockDim.x) if (s_bins[i]) atomicAdd(&hist[i], s_bins[i]);
    }
}

}  // namespace

extern "C" {

int tpc_segments_colors_build(tpc_ctx *c, const uint32_t *color_of_seq, uint32_t n_colors)
{
    if (!c) return -1;
    colors_drop(c);
    if (int rc = stage_needs_segments(c, "colours", "colour")) return rc;
    if (n_colors == 0) return fail(c, -1, "segment colours: at least one colour is required");
    // C + 1 bins and ceil(C / 32) words are 32-bit quantities in the kernels: neither may wrap
    if (n_colors > COL_MAX_COLORS) return fail(c, -1, "segment colours: %u colours, at most %u are supported", n_colors, COL_MAX_COLORS);
    const uint32_t n_rec = c->seg.n_rec;
    if (n_rec && !color_of_seq) return fail(c, -1, "segment colours: the colour of every one of the %u sequences is required", n_rec);
    for (uint32_t s = 0; s < n_rec; s++)
        if (color_of_seq[s] >= n_colors) return fail(c, -1, "segment colours: sequence %u has colour %u, there are %u colours", s, color_of_seq[s], n_colors);
    HIPCHK(c, hipSetDevice(c->device));
    // the table's own consistency: every event belongs to one of the n_rec sequences
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != c->seg.events) return fail(c, -1, "segment colours: the stream holds events of more sequences than the %u given", n_rec);

    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments;
    // sizes in 64 bits: S x W x 4 B of presence is the large term, and the refusal below must see it whole
    const uint32_t words = (uint32_t)(((uint64_t)n_colors + 31) / 32), bins = n_colors + 1;
    const uint64_t presence_words = n_rows * (uint64_t)words;  // below 2^32 x 2^26
    const size_t rows_bytes = (size_t)n_rows * 16 + 16, presence_bytes = (size_t)presence_words * 4 + 16, hist_bytes = (size_t)bins * 16;
    const size_t color_bytes = (size_t)n_rec * 4 + 16;
    SegRows idx;
    if (!idx.size(c)) return fail(c, -10, "segment colours: the scan could not be sized");
    const size_t need = rows_bytes + presence_bytes + hist_bytes + color_bytes + idx.bytes();
    if (int rc = stage_fits(c, "colours", need, "%zu of them the presence bits of %llu segments x %u colours", presence_bytes, (unsigned long long)n_rows, n_colors)) return rc;
    StageTemps temps;
    uint32_t *color = nullptr;
    auto done = [&](int code) {
        if (code) colors_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->col.rows, rows_bytes) != hipSuccess || dev_malloc(c, (void **)&c->col.presence, presence_bytes) != hipSuccess ||
        dev_malloc(c, (void **)&c->col.hist, hist_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &color, color_bytes))
        return done(fail(c, -10, "segment colours: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(c->col.rows, 0, rows_bytes, s) == hipSuccess && hipMemsetAsync(c->col.presence, 0, presence_bytes, s) == hipSuccess &&
              hipMemsetAsync(c->col.hist, 0, hist_bytes, s) == hipSuccess && idx.fill(s) &&
              (!n_rec || hipMemcpyAsync(color, color_of_seq, (size_t)n_rec * 4, hipMemcpyHostToDevice, s) == hipSuccess);
    if (ok) {
        Timed t(c, TPC_K_COLORS);
        ok = idx.enqueue(c);
        if (ok && n_events)
            hipLaunchKernelGGL(k_col_scatter, dim3(col_grid(n_events)), dim3(256), 0, s, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, c->seg.ev[2], n_rec, color,
                               c->col.rows, n_rows, c->col.presence, words);
        if (ok && n_rows) {
            if (bins <= COL_LDS_BINS)
                hipLaunchKernelGGL(k_col_rows<true>, dim3(std::min(col_grid(n_rows), 1024u)), dim3(256), (size_t)bins * 16, s, c->col.rows, n_rows, c->col.presence, words,
                                   c->seg.ev[0], c->seg.ev[1], (uint32_t)c->seg.k, c->col.hist, n_colors);
            else
                hipLaunchKernelGGL(k_col_rows<false>, dim3(col_grid(n_rows)), dim3(256), 0, s, c->col.rows, n_rows, c->col.presence, words, c->seg.ev[0], c->seg.ev[1],
                                   (uint32_t)c->seg.k, c->col.hist, n_colors);
        }
    }
    ok = ok && idx.total(s);
    if (int rc = stage_wait(c, "colours", ok)) return done(rc);
    if (idx.scanned != n_rows) return done(fail(c, -10, "segment colours: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
    c->col.n_rows = n_rows; c->col.n_colors = n_colors; c->col.words = words;
    c->col.valid = true;
    return 0;
}

int tpc_segments_colors_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->col.valid) return fail(c, -1, "segment colours: tpc_segments_colors_build first");
    if (!info) return fail(c, -1, "segment colours: info required");
    info[0] = c->col.n_rows; info[1] = c->col.n_colors; info[2] = c->col.words;
    return 0;
}

int tpc_segments_colors_fetch_rows(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *first_event_host, uint32_t *occ_host, uint32_t *fwd_host, uint32_t *ncol_host)
{
    if (!c) return -1;
    if (!c->col.valid) return fail(c, -1, "segment colours: tpc_segments_colors_build first");
    return fetch_planes(c, "colours", "row", c->col.rows, c->col.n_rows, r0, n, { first_event_host, occ_host, fwd_host, ncol_host });
}

int tpc_segments_colors_fetch_presence(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *words_host)
{
    if (!c) return -1;
    if (!c->col.valid) return fail(c, -1, "segment colours: tpc_segments_colors_build first");
    if ((n && !words_host) || r0 > c->col.n_rows || n > c->col.n_rows - r0)
        return fail(c, -1, "segment colours: bad presence range (%llu rows at %llu of %llu)", (unsigned long long)n, (unsigned long long)r0, (unsigned long long)c->col.n_rows);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(words_host, c->col.presence + r0 * c->col.words, n * c->col.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_colors_fetch_hist(tpc_ctx *c, uint64_t *segments_host, uint64_t *bases_host)
{
    if (!c) return -1;
    if (!c->col.valid) return fail(c, -1, "segment colours: tpc_segments_colors_build first");
    if (!segments_host || !bases_host) return fail(c, -1, "segment colours: both histogram arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bins = (size_t)c->col.n_colors + 1;
    HIPCHK(c, hipMemcpy(segments_host, c->col.hist, bins * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(bases_host, c->col.hist + bins, bins * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
