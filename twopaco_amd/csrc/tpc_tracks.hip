// tpc_tracks.hip -- the PRESENCE TRACKS of the input sequences: the colour rows projected onto the coordinates of every sequence, with
// neighbouring occurrences of equal presence merged into one interval.  Kernels and the C-ABI of the tpc_segments_tracks_* group of
// include/twopaco_hip.h, which defines selected, continues, interval and the sums.  No counterpart in the reference;
// host/graphformat.h: ComputeTracks is the serial statement.
//
// Input: the event table of the last tpc_segments_build_* (name, first bits, begin, end, the sequences' event ranges), the colour table
// of the last tpc_segments_colors_build (presence[S][W], n_colors per row) and the caller's colour of every sequence.
//   SegRows              the row of every first event (tpc_segrows.h)
//   k_trk_rows           row_of[e] for every event: rank[table[|name[e]|]], or rank[e] for an 'N'-named one
//   k_trk_heads_thread   W <= 8: one thread per event.  Its sequence by a binary search over the sequences' event ranges (col_seq_end),
//                        its colour, whether it is selected, and whether it CONTINUES e - 1: e - 1 lies in the same sequence and the rows
//                        are equal (the shortcut) or their W words are.  flag[e] = selected | head << 1.  The selected events are counted
//                        per lane and added once per wave.
//   k_trk_heads_wave     W > 8: one wave per event, lane j compares words j, j + 64, .. and the wave votes; only when the rows differ.
//   scan                 one rocprim exclusive scan over the head bits numbers the intervals; its total is the host's one wait
//   k_trk_place          one thread per event: a head writes first_event and row of interval id[e]; a tail -- a selected event whose
//                        successor is no selected event that continues it -- writes last_event of interval id[e + 1] - 1
//   k_trk_sums           one thread per interval: edges = end[last] - begin[first], the colour of its sequence, n = the row's n_colors.
//                        HOT KEYS: one colour takes every add of a whole genome and the core depth nearly every add of a real input,
//                        so neighbouring lanes of one colour are one run (col_run) and those of one depth another, each summed by a
//                        segmented scan over the wave and added once by the run's leader, as tpc_classes.hip folds its sums: four
//                        vector atomics per colour run and two per depth run.  Where every stretch has a depth of its own the depth
//                        runs are one lane long: the bins are kept in LDS while C <= 512 (24 KiB) and flushed once per block, so
//                        those adds never reach the global bins one by one.
// Integers and commutative sums: the result is exact and does not depend on the schedule.
// Memory: kept until the next segment, colour or track build 12 B per interval (first_event, last_event, row) and 32 B + 16 B per colour
// of sums (16 B more for depth C); during the call 12 B per event (the row, the flags, and the first-bit ranks that become the interval
// ids), 4 B per name of the first-sight table, 4 B per sequence and the scan's scratch.  None of it exists in a context that never asks
// for tracks.  What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint32_t TRK_ALL = 0xFFFFFFFFu;        // only_color: every colour
constexpr uint32_t TRK_NONE = 0xFFFFFFFFu;
constexpr uint32_t TRK_THREAD_WORDS = 8;         // up to here one thread compares two rows, beyond one wave does (as tpc_classes.hip)
constexpr uint32_t TRK_SELECTED = 1u, TRK_HEAD = 2u;
constexpr int TRK_COLOR_SUMS = 4;                // planes per colour: intervals, edges, core_edges, private_edges
constexpr uint32_t TRK_LDS_COLORS = 512;         // up to here a block keeps all bins of the sums in LDS: 8 B x (6 x 512 + 2) = 24 KiB

__device__ __forceinline__ unsigned long long trk_wave_sum(unsigned long long v)
{
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ void k_trk_rows(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank,
                           uint64_t n_rows, uint32_t *__restrict__ row_of)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        const uint32_t side = link_side(name, e, n_events, table, n_table, rank, n_rows);
        row_of[e] = side == 0xFFFFFFFFu ? TRK_NONE : side >> 1;
    }
}

// the sequence of event e, or TRK_NONE; begins: e is the first event of its sequence
__device__ __forceinline__ uint32_t trk_seq(const uint32_t *__restrict__ seq_begin, uint32_t n_rec, uint32_t e, bool &begins)
{
    const uint32_t lo = col_seq_end(seq_begin, n_rec, e);
    if (lo < 1 || lo > n_rec) { begins = true; return TRK_NONE; }
    begins = seq_begin[lo - 1] == e;
    return lo - 1;
}

// flag: n_events + 1 entries, the last one 0.  bad: raised when an event has no sequence or no row (cannot happen after a good build).
__global__ void k_trk_heads_thread(const uint32_t *__restrict__ row_of, uint64_t n_events, uint64_t n_rows, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                                   const uint32_t *__restrict__ color, uint32_t only, const uint32_t *__restrict__ presence, uint32_t words, uint32_t *__restrict__ flag,
                                   unsigned long long *__restrict__ selected_total, uint32_t *__restrict__ bad)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n_events; e += stride) {
        uint32_t f = 0;
        if (e < n_events) {
            bool begins = true;
            const uint32_t seq = trk_seq(seq_begin, n_rec, (uint32_t)e, begins), r = row_of[e];
            if (seq == TRK_NONE || r >= n_rows) atomicOr(bad, 1u);
            else if (only == TRK_ALL || color[seq] == only) {
                bool continues = !begins;
                if (continues) {
                    const uint32_t below = row_of[e - 1];
                    if (below >= n_rows) continues = false;
                    else if (below != r)
                        for (uint32_t w = 0; continues && w < words; w++) continues = presence[(uint64_t)r * words + w] == presence[(uint64_t)below * words + w];
                }
                f = TRK_SELECTED | (continues ? 0u : TRK_HEAD);
                mine++;
            }
        }
        flag[e] = f;
    }
    mine = trk_wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(selected_total, mine);
}

// one wave per event: the event is uniform over the wave, and so is every branch around the vote
__global__ void k_trk_heads_wave(const uint32_t *__restrict__ row_of, uint64_t n_events, uint64_t n_rows, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                                 const uint32_t *__restrict__ color, uint32_t only, const uint32_t *__restrict__ presence, uint32_t words, uint32_t *__restrict__ flag,
                                 unsigned long long *__restrict__ selected_total, uint32_t *__restrict__ bad)
{
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * waves;
    unsigned long long mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); e <= n_events; e += stride) {
        uint32_t f = 0;
        if (e < n_events) {
            bool begins = true;
            const uint32_t seq = trk_seq(seq_begin, n_rec, (uint32_t)e, begins), r = row_of[e];
            if (seq == TRK_NONE || r >= n_rows) { if (lane == 0) atomicOr(bad, 1u); }
            else if (only == TRK_ALL || color[seq] == only) {
                bool continues = !begins;
                if (continues) {
                    const uint32_t below = row_of[e - 1];
                    if (below >= n_rows) continues = false;
                    else if (below != r) {
                        bool differs = false;
                        for (uint32_t w = lane; w < words; w += 64) differs = differs || presence[(uint64_t)r * words + w] != presence[(uint64_t)below * words + w];
                        continues = !__any(differs);
                    }
                }
                f = TRK_SELECTED | (continues ? 0u : TRK_HEAD);
                if (lane == 0) mine++;
            }
        }
        if (lane == 0) flag[e] = f;
    }
    mine = trk_wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(selected_total, mine);
}

// head[e] = the head bit of flag[e], n_events + 1 entries: the input of the scan
__global__ void k_trk_bits(const uint32_t *__restrict__ flag, uint64_t n_events, uint32_t *__restrict__ head)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n_events; e += stride) head[e] = (flag[e] & TRK_HEAD) ? 1u : 0u;
}

// id: the exclusive scan of the head bits, n_events + 1 entries.  rows: [3][n_intervals] first_event, last_event, row.
__global__ void k_trk_place(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ id, const uint32_t *__restrict__ row_of, uint64_t n_events,
                            uint32_t *__restrict__ rows, uint64_t n_intervals)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        const uint32_t f = flag[e];
        if (!(f & TRK_SELECTED)) continue;
        if (f & TRK_HEAD) {
            const uint32_t i = id[e];
            if (i < n_intervals) { rows[i] = (uint32_t)e; rows[2 * n_intervals + i] = row_of[e]; }
        }
        const uint32_t after = flag[e + 1];   // (flag[n_events] = 0)
        if (!(after & TRK_SELECTED) || (after & TRK_HEAD)) {
            const uint32_t i = id[e + 1] - 1u;   // (e is selected: a head lies at or below it)
            if (i < n_intervals) rows[n_intervals + i] = (uint32_t)e;
        }
    }
}

// the sum of v over the lanes start .. lane of this lane's run (start: the run's first lane)
__device__ __forceinline__ unsigned long long trk_run_sum(unsigned long long v, uint32_t lane, uint32_t start)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long below = __shfl_up(v, d);
        if (lane >= start + d) v += below;
    }
    return v;
}

// A RUN of neighbouring lanes with one key, from the wave's ballots (col_run): whether this lane leads one, its first and last lane and
// its lanes.  The lanes that are not active hold the key all ones; they are runs of their own and lead nothing.
struct TrkRun {
    bool leads;
    uint32_t start, last;
    unsigned long long lanes;
};

__device__ __forceinline__ TrkRun trk_runs(unsigned long long key, bool active, uint32_t lane)
{
    const unsigned long long key_below = __shfl_up(key, 1);
    const bool head = lane == 0 || key_below != key;
    const unsigned long long heads = __ballot(head), actives = __ballot(active);
    TrkRun r;
    r.start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
    r.lanes = col_run(lane, heads, actives);
    r.last = r.lanes ? 63u - (uint32_t)__clzll((long long)r.lanes) : lane;
    r.leads = head && active;
    return r;
}

// of a leader: the sum of v over its run
__device__ __forceinline__ unsigned long long trk_total(unsigned long long v, uint32_t lane, const TrkRun &r) { return __shfl(trk_run_sum(v, lane, r.start), r.last); }

// sums: [4][n_colors] intervals, edges, core_edges, private_edges, then [2][n_colors + 1] depth_intervals, depth_edges.  col_n: n_colors of
// every colour row.  The intervals ascend by their first event, so a wave holds neighbouring stretches of one sequence: the lanes of
// one COLOUR are one run (as a rule the whole wave) and its leader adds the four per-colour sums once; the lanes of one DEPTH are another
// kind of run -- long where the genomes agree, short where every stretch has a set of its own -- and its leader adds the two per-depth
// sums.  LDS: all bins in dynamic shared memory, 8 B x (6 n_colors + 2), flushed once per block; without, the leaders add to the global
// bins.  A whole wave runs every iteration (the stride is a multiple of 64), lanes past the last interval take part in the shuffles and
// ballots and nothing else.
template <bool LDS>
__global__ void k_trk_sums(const uint32_t *__restrict__ rows, uint64_t n_intervals, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint64_t n_events,
                           const uint32_t *__restrict__ seq_begin, uint32_t n_rec, const uint32_t *__restrict__ color, const uint32_t *__restrict__ col_n, uint64_t n_rows,
                           uint32_t n_colors, unsigned long long *__restrict__ sums, uint32_t *__restrict__ bad)
{
    extern __shared__ unsigned long long s_trk[];
    const uint32_t total = TRK_COLOR_SUMS * n_colors + 2 * (n_colors + 1);
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) s_trk[i] = 0;
        __syncthreads();
    }
    unsigned long long *per_color = LDS ? s_trk : sums, *depth = per_color + (uint64_t)TRK_COLOR_SUMS * n_colors;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i - lane < n_intervals; i += stride) {
        bool active = i < n_intervals;
        unsigned long long edges = 0;
        uint32_t c = 0, n = 0;
        if (active) {
            const uint32_t first = rows[i], last = rows[n_intervals + i], r = rows[2 * n_intervals + i];
            bool begins = true;
            const uint32_t seq = first < n_events ? trk_seq(seq_begin, n_rec, first, begins) : TRK_NONE;
            active = seq != TRK_NONE && last < n_events && last >= first && r < n_rows && end[last] >= begin[first];
            if (active) {
                c = color[seq];
                n = col_n[r];
                active = c < n_colors && n <= n_colors;
            }
            if (!active) atomicOr(bad, 2u);
            else edges = (unsigned long long)end[last] - begin[first];
        }
        const TrkRun by_color = trk_runs(active ? (unsigned long long)c : ~0ull, active, lane);
        const unsigned long long color_edges = trk_total(edges, lane, by_color), core = trk_total(active && n == n_colors ? edges : 0ull, lane, by_color),
                                 alone = trk_total(active && n == 1 ? edges : 0ull, lane, by_color);
        if (by_color.leads) {
            atomicAdd(&per_color[c], (unsigned long long)__popcll(by_color.lanes));
            atomicAdd(&per_color[(uint64_t)n_colors + c], color_edges);
            if (core) atomicAdd(&per_color[2 * (uint64_t)n_colors + c], core);
            if (alone) atomicAdd(&per_color[3 * (uint64_t)n_colors + c], alone);
        }
        const TrkRun by_depth = trk_runs(active ? (unsigned long long)n : ~0ull, active, lane);
        const unsigned long long depth_edges = trk_total(edges, lane, by_depth);
        if (by_depth.leads) {
            atomicAdd(&depth[n], (unsigned long long)__popcll(by_depth.lanes));
            atomicAdd(&depth[(uint64_t)n_colors + 1 + n], depth_edges);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) if (s_trk[i]) atomicAdd(&sums[i], s_trk[i]);
    }
}

int trk_needs(tpc_ctx *c)
{
    if (!c->trk.valid) return fail(c, -1, "segment tracks: tpc_segments_tracks_build first");
    return 0;
}

// the test option holds for one build: whichever way it returns, the next one runs on its own
struct TrkOptions {
    tpc_ctx *c;
    int grid;
    explicit TrkOptions(tpc_ctx *c_) : c(c_), grid(c_->opt_tracks_grid) {}
    ~TrkOptions() { c->opt_tracks_grid = 0; }
};

}  // namespace

extern "C" {

int tpc_segments_tracks_build(tpc_ctx *c, const uint32_t *color_of_seq, uint32_t n_colors, uint32_t only_color)
{
    if (!c) return -1;
    tracks_drop(c);
    const TrkOptions opt(c);
    if (int rc = stage_needs_segments(c, "tracks", "project")) return rc;
    if (!c->col.valid) return fail(c, -1, "segment tracks: build the colour table first (tpc_segments_colors_build)");
    if (c->col.n_colors != n_colors) return fail(c, -1, "segment tracks: the colour table holds %u colours, the caller gives %u", c->col.n_colors, n_colors);
    if (only_color != TRK_ALL && only_color >= n_colors) return fail(c, -1, "segment tracks: the one colour is %u, there are %u colours", only_color, n_colors);
    const uint32_t n_rec = c->seg.n_rec;
    if (n_rec && !color_of_seq) return fail(c, -1, "segment tracks: the colour of every one of the %u sequences is required", n_rec);
    for (uint32_t s = 0; s < n_rec; s++)
        if (color_of_seq[s] >= n_colors) return fail(c, -1, "segment tracks: sequence %u has colour %u, there are %u colours", s, color_of_seq[s], n_colors);
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments;
    if (n_events >= TRK_NONE) return fail(c, -1, "segment tracks: %llu events, an interval holds events below %u", (unsigned long long)n_events, TRK_NONE);
    if (n_rows >= ((uint64_t)1 << 31)) return fail(c, -1, "segment tracks: %llu segments, a row holds at most %llu", (unsigned long long)n_rows, (unsigned long long)(((uint64_t)1 << 31) - 1));
    if (c->col.n_rows != n_rows) return fail(c, -10, "segment tracks: the colour table holds %llu rows, the build counted %llu segments", (unsigned long long)c->col.n_rows, (unsigned long long)n_rows);
    HIPCHK(c, hipSetDevice(c->device));
    // the table's own consistency: every event belongs to one of the n_rec sequences
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != n_events) return fail(c, -1, "segment tracks: the stream holds events of more sequences than the %u given", n_rec);
    const uint32_t words = c->col.words;
    auto grid = [&](uint64_t n) { return dim3(opt.grid > 0 ? std::min<unsigned>(col_grid(n), (unsigned)opt.grid) : col_grid(n)); };

    // sizes in 64 bits, summed before the first allocation; the intervals are not counted yet: at most one per event
    const uint64_t event_bytes = (n_events + 1) * 4 + 16, color_bytes = (uint64_t)n_rec * 4 + 16, rows_bound = n_events * 12 + 16;
    const uint64_t sums_bytes = ((uint64_t)TRK_COLOR_SUMS * n_colors + 2 * ((uint64_t)n_colors + 1)) * 8;
    SegRows idx;
    if (!idx.size(c)) return fail(c, -10, "segment tracks: the scan could not be sized");
    const uint64_t need = 2 * event_bytes + color_bytes + sums_bytes + rows_bound + idx.bytes() + 64;
    if (int rc = stage_fits(c, "tracks", need, "%llu of them the rows, flags and ranks of %llu events, up to %llu the intervals", (unsigned long long)(2 * event_bytes + idx.rank_bytes),
                            (unsigned long long)n_events, (unsigned long long)rows_bound))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) tracks_drop(c);
        return code;
    };
    uint32_t *row_of = nullptr, *flag = nullptr, *color = nullptr, *scalars = nullptr;
    if (dev_malloc(c, (void **)&c->trk.sums, sums_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &row_of, event_bytes) || !temps.get(c, &flag, event_bytes) ||
        !temps.get(c, &color, color_bytes) || !temps.get(c, &scalars, 64))
        return done(fail(c, -10, "segment tracks: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    // 64 bytes of scalars: the raised bits, then the selected events
    unsigned long long *selected = (unsigned long long *)(scalars + 2);
    unsigned long long *sums = c->trk.sums;
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(scalars, 0, 64, s) == hipSuccess && hipMemsetAsync(sums, 0, sums_bytes, s) == hipSuccess && idx.fill(s) &&
              (!n_rec || hipMemcpyAsync(color, color_of_seq, (size_t)n_rec * 4, hipMemcpyHostToDevice, s) == hipSuccess);
    uint32_t n_intervals = 0, raised = 0;
    unsigned long long selected_host = 0;
    if (ok) {
        Timed t(c, TPC_K_TRACKS);   // the whole stage on the stream, the wait for the interval count included (as TPC_K_CLASSES)
        ok = idx.enqueue(c) && idx.total(s);
        if (ok && n_events) hipLaunchKernelGGL(k_trk_rows, grid(n_events), dim3(256), 0, s, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, row_of);
        if (ok) {
            // (a wave per event: four events per workgroup of 256)
            if (words > TRK_THREAD_WORDS)
                hipLaunchKernelGGL(k_trk_heads_wave, grid((n_events + 1) * 64), dim3(256), 0, s, row_of, n_events, n_rows, c->seg.ev[2], n_rec, color, only_color, c->col.presence, words, flag,
                                   selected, scalars);
            else
                hipLaunchKernelGGL(k_trk_heads_thread, grid(n_events + 1), dim3(256), 0, s, row_of, n_events, n_rows, c->seg.ev[2], n_rec, color, only_color, c->col.presence, words, flag,
                                   selected, scalars);
            // the ranks were read for the last time by k_trk_rows (and their total is on its way to the host): the buffer takes the ids
            hipLaunchKernelGGL(k_trk_bits, grid(n_events + 1), dim3(256), 0, s, flag, n_events, idx.rank);
            ok = rocprim::exclusive_scan(idx.scan_tmp, idx.scan_bytes, idx.rank, idx.rank, 0u, n_events + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the number of intervals decides the size of what is kept: the one wait in the middle
        ok = ok && hipMemcpyAsync(&n_intervals, idx.rank + n_events, sizeof n_intervals, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, scalars, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&selected_host, selected, sizeof selected_host, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "tracks", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment tracks: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (raised) return done(fail(c, -10, "segment tracks: an event lies in no sequence or in no segment"));
        if (n_intervals > n_events) return done(fail(c, -10, "segment tracks: %u intervals over %llu events", n_intervals, (unsigned long long)n_events));
        const uint64_t rows_bytes = (uint64_t)n_intervals * 12 + 16;
        if (dev_malloc(c, (void **)&c->trk.rows, rows_bytes) != hipSuccess) return done(fail(c, -10, "segment tracks: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->trk.rows, 0xFF, rows_bytes, s) == hipSuccess;
        if (ok && n_intervals) {
            hipLaunchKernelGGL(k_trk_place, grid(n_events), dim3(256), 0, s, flag, idx.rank, row_of, n_events, c->trk.rows, (uint64_t)n_intervals);
            if (n_colors <= TRK_LDS_COLORS)
                hipLaunchKernelGGL(k_trk_sums<true>, dim3(std::min(grid(n_intervals).x, 1024u)), dim3(256), sums_bytes, s, c->trk.rows, (uint64_t)n_intervals, c->seg.ev[0], c->seg.ev[1],
                                   n_events, c->seg.ev[2], n_rec, color, c->col.rows + 3 * n_rows, n_rows, n_colors, sums, scalars);
            else
                hipLaunchKernelGGL(k_trk_sums<false>, grid(n_intervals), dim3(256), 0, s, c->trk.rows, (uint64_t)n_intervals, c->seg.ev[0], c->seg.ev[1], n_events, c->seg.ev[2], n_rec,
                                   color, c->col.rows + 3 * n_rows, n_rows, n_colors, sums, scalars);
        }
        ok = ok && hipMemcpyAsync(&raised, scalars, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->trk.peak_bytes = need - rows_bound + rows_bytes;
    }
    if (int rc = stage_wait(c, "tracks", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment tracks: an interval lies outside the tables"));
    c->trk.n_intervals = n_intervals; c->trk.selected = selected_host; c->trk.n_colors = n_colors; c->trk.only = only_color;
    c->trk.valid = true;
    return 0;
}

int tpc_segments_tracks_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = trk_needs(c)) return rc;
    if (!info) return fail(c, -1, "segment tracks: info required");
    info[0] = c->trk.n_intervals; info[1] = c->trk.selected; info[2] = c->trk.n_colors; info[3] = c->trk.only; info[4] = c->trk.peak_bytes;
    return 0;
}

int tpc_segments_tracks_fetch_rows(tpc_ctx *c, uint64_t i0, uint64_t n, uint32_t *first_event, uint32_t *last_event, uint32_t *row)
{
    if (!c) return -1;
    if (int rc = trk_needs(c)) return rc;
    return fetch_planes(c, "tracks", "interval", c->trk.rows, c->trk.n_intervals, i0, n, { first_event, last_event, row });
}

int tpc_segments_tracks_fetch_colors(tpc_ctx *c, uint64_t *intervals, uint64_t *edges, uint64_t *core_edges, uint64_t *private_edges)
{
    if (!c) return -1;
    if (int rc = trk_needs(c)) return rc;
    if (!intervals || !edges || !core_edges || !private_edges) return fail(c, -1, "segment tracks: all four per-colour arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = c->trk.n_colors;
    uint64_t *dst[TRK_COLOR_SUMS] = {intervals, edges, core_edges, private_edges};
    for (int i = 0; i < TRK_COLOR_SUMS; i++) HIPCHK(c, hipMemcpy(dst[i], c->trk.sums + (size_t)i * n, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_tracks_fetch_depth(tpc_ctx *c, uint64_t *intervals, uint64_t *edges)
{
    if (!c) return -1;
    if (int rc = trk_needs(c)) return rc;
    if (!intervals || !edges) return fail(c, -1, "segment tracks: both per-depth arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = c->trk.n_colors, bins = n + 1;
    HIPCHK(c, hipMemcpy(intervals, c->trk.sums + TRK_COLOR_SUMS * n, bins * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(edges, c->trk.sums + TRK_COLOR_SUMS * n + bins, bins * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
