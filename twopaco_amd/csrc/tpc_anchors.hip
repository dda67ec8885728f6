// tpc_anchors.hip -- the anchor blocks: where the sequence a colour shares with a reference colour lies in both, in which order and
// on which strand.  Kernels and the C-ABI of the tpc_segments_anchors_* group of include/twopaco_hip.h, which states the
// definition (count, anchor, mate, reverse, continues, block); host/graphformat.h: ComputeAnchors is the serial statement of it.
// No counterpart in the reference.
//
// Input: the event table of the last tpc_segments_build_* (name[e], first[] bits, begin / end, seq_event_begin[]) and the
// caller's colour of every sequence.  The row of every event is made again (tpc_segrows.h).  Then:
//   k_anc_keys     one thread per event: key = row << colour_bits | colour, value = the event; the colour by binary search in
//                  seq_event_begin (col_seq_end).  An event without a row gets the key of row n_rows and sorts last.  The
//                  reference colour's events add end - begin to ref_edges: a sum per lane, one shuffle reduction and one atomic
//                  per wave.
//   the sort       rocprim::radix_sort_pairs over the key bits in use (colour_bits + row_bits).  A poly-A row with thousands of
//                  events is one long run of equal keys: nothing queues on one address.
//   k_anc_runs     one thread per sorted entry compares its key with both neighbours ACROSS THE ARRAY (not the wave): the head of
//                  a run in the reference colour writes ref_event[row] = its event when it is also the run's tail (count 1), the
//                  "many" sentinel otherwise.  One writer per row: a (row, colour) pair is one run.
//   k_anc_mates    one thread per sorted entry of another colour whose run has length 1: mate[event] = ref_event[row] when that
//                  holds an event.  mate[] is preset to none.
//   k_anc_heads    one thread per event evaluates the continue rule for itself and for the event after it -- the names of both
//                  events and of both mates, the sequence ranges on both sides -- and writes head | tail << 1; the head bit alone
//                  goes to the array that is scanned.
//   the scan       exclusive, over n_events + 1 head flags: the slot of every block and, as the last element, their number.  The
//                  host waits for that number once: it is the size of what is kept.
//   k_anc_place    one thread per event: a head writes query_first and its mate's end of the reference range into slot
//                  scan[e], a tail writes query_last and the other end into slot scan[e + 1] - 1 (the heads at or before it,
//                  less one).  Heads and tails alternate in event order, so block b pairs the b-th head with the b-th tail.
//   k_anc_sums     one thread per block adds 1, anchors, edges and, reverse, edges again to its colour's four sums.  Blocks
//                  ascend by query event, so with the usual colour maps all blocks of a wave belong to one colour: lanes compare
//                  their colour with the lane below, the lanes that differ are run leaders (col_run of tpc_segrows.h), and a
//                  leader issues the run's four atomics once, the run's sums taken from a wave prefix sum.  The bins are
//                  privatised in LDS while 4 x 8 B x C fits ANC_LDS_BYTES and flushed once per block; beyond that they are
//                  global atomics (the pattern of k_col_rows).
// Memory: kept until the next segment build or anchor build 4 B / event of mates, 16 B / block of rows, 32 B / colour of sums
// and the one word of ref_edges; during the call also the row index, 24 B / event of keys and values in two buffers each, the
// sort's scratch, 8 B / event of flags, 4 B / row of reference events and 4 B / sequence of colours.  None of it exists in a
// context that never asks for anchors.  What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint32_t ANC_NONE = 0xFFFFFFFFu;       // mate[]: no mate; ref_event[]: no event of the reference colour
constexpr uint32_t ANC_MANY = 0xFFFFFFFEu;       // ref_event[]: more than one event of the reference colour
constexpr uint32_t ANC_LDS_BYTES = 32768;        // the LDS a block of k_anc_sums may spend on its bins: 4 x 8 B x 1024 colours
constexpr uint32_t ANC_LDS_COLORS = ANC_LDS_BYTES / 32;
constexpr uint32_t ANC_MAX_COLORS = 1u << 31;    // as COL_MAX_COLORS of tpc_colors.hip

inline uint32_t anc_bits(uint64_t largest) { uint32_t b = 0; while (b < 64 && (largest >> b)) b++; return b; }

__device__ __forceinline__ unsigned long long anc_wave_sum(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the inclusive prefix sum of v over the lanes of the wave
__device__ __forceinline__ unsigned long long anc_wave_prefix(unsigned long long v, uint32_t lane)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long below = __shfl_up(v, d);
        if (lane >= d) v += below;
    }
    return v;
}

// A whole wave runs every iteration (the stride is a multiple of 64): the reduction of ref_edges needs all lanes.
__global__ void k_anc_keys(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank,
                           uint64_t n_rows, const uint32_t *__restrict__ seq_begin, uint32_t n_rec, const uint32_t *__restrict__ color, uint32_t ref_color,
                           const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint32_t color_bits, unsigned long long *__restrict__ keys,
                           uint32_t *__restrict__ vals, unsigned long long *__restrict__ ref_edges)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        const int64_t nm = name[e];
        const uint64_t mag = col_mag(nm);
        const uint32_t e0 = (nm >= COL_FRESH || mag >= n_table) ? (uint32_t)e : table[mag];
        const uint32_t row = e0 < n_events ? rank[e0] : 0xFFFFFFFFu;
        const uint32_t lo = col_seq_end(seq_begin, n_rec, (uint32_t)e);
        const bool known = row < n_rows && lo >= 1 && lo <= n_rec;  // (the build's caller checked that every event has a sequence)
        const uint32_t col = known ? color[lo - 1] : 0u;
        keys[e] = ((known ? (unsigned long long)row : (unsigned long long)n_rows) << color_bits) | col;
        vals[e] = (uint32_t)e;
        if (known && col == ref_color) mine += (unsigned long long)end[e] - begin[e];
    }
    mine = anc_wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(ref_edges, mine);
}

__global__ void k_anc_runs(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n_events, uint64_t n_rows, uint32_t color_bits,
                           uint32_t ref_color, uint32_t *__restrict__ ref_event)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const unsigned long long color_mask = (1ull << color_bits) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_events; i += stride) {
        const unsigned long long key = keys[i];
        const uint64_t row = key >> color_bits;
        if (row >= n_rows || (uint32_t)(key & color_mask) != ref_color) continue;
        if (i > 0 && keys[i - 1] == key) continue;  // not the head of its run
        const bool alone = i + 1 == n_events || keys[i + 1] != key;
        ref_event[row] = alone ? vals[i] : ANC_MANY;
    }
}

__global__ void k_anc_mates(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n_events, uint64_t n_rows, uint32_t color_bits,
                            uint32_t ref_color, const uint32_t *__restrict__ ref_event, uint32_t *__restrict__ mate)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const unsigned long long color_mask = (1ull << color_bits) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_events; i += stride) {
        const unsigned long long key = keys[i];
        const uint64_t row = key >> color_bits;
        if (row >= n_rows || (uint32_t)(key & color_mask) == ref_color) continue;
        if ((i > 0 && keys[i - 1] == key) || (i + 1 < n_events && keys[i + 1] == key)) continue;  // count[row][colour] above 1
        const uint32_t m = ref_event[row], e = vals[i];
        if (m < n_events && e < n_events) mate[e] = m;
    }
}

// the mate of event e when it is an anchor (ANC_NONE otherwise) and its reverse flag
__device__ __forceinline__ uint32_t anc_mate(const uint32_t *__restrict__ mate, const int64_t *__restrict__ name, uint64_t n_events, uint64_t e, bool &reverse)
{
    const uint32_t m = mate[e];
    reverse = false;
    if (m >= n_events) return ANC_NONE;
    reverse = (name[e] < 0) != (name[m] < 0);
    return m;
}

// e is an anchor with mate m and flag reverse: does it continue e - 1?
__device__ __forceinline__ bool anc_continues(const uint32_t *__restrict__ mate, const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ seq_begin,
                                              uint32_t n_rec, uint64_t e, uint32_t m, bool reverse)
{
    if (e == 0) return false;
    const uint32_t lo = col_seq_end(seq_begin, n_rec, (uint32_t)e);
    if (lo < 1 || lo > n_rec || seq_begin[lo - 1] > e - 1) return false;        // e begins its sequence
    bool reverse_before;
    const uint32_t m_before = anc_mate(mate, name, n_events, e - 1, reverse_before);
    if (m_before == ANC_NONE || reverse_before != reverse) return false;
    if (reverse ? m_before != m + 1 : m != m_before + 1) return false;
    return col_seq_end(seq_begin, n_rec, m) == col_seq_end(seq_begin, n_rec, m_before);  // both mates in one reference sequence
}

// flags[e] = head | tail << 1; heads[e] = the head bit, heads[n_events] = 0: the scan's last element is the block count
__global__ void k_anc_heads(const uint32_t *__restrict__ mate, const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                            uint32_t *__restrict__ flags, uint32_t *__restrict__ heads)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n_events; e += stride) {
        uint32_t head = 0, tail = 0;
        bool reverse;
        if (e < n_events) {
            const uint32_t m = anc_mate(mate, name, n_events, e, reverse);
            if (m != ANC_NONE) {
                head = anc_continues(mate, name, n_events, seq_begin, n_rec, e, m, reverse) ? 0u : 1u;
                tail = 1;
                if (e + 1 < n_events) {
                    bool reverse_after;
                    const uint32_t m_after = anc_mate(mate, name, n_events, e + 1, reverse_after);
                    if (m_after != ANC_NONE && anc_continues(mate, name, n_events, seq_begin, n_rec, e + 1, m_after, reverse_after)) tail = 0;
                }
            }
            flags[e] = head | tail << 1;
        }
        heads[e] = head;
    }
}

// rows: [0, B) query_first, [B, 2B) query_last, [2B, 3B) ref_first, [3B, 4B) ref_last; slot[] the scanned head flags
__global__ void k_anc_place(const uint32_t *__restrict__ mate, const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ flags,
                            const uint32_t *__restrict__ slot, uint32_t *__restrict__ rows, uint64_t n_blocks)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        const uint32_t f = flags[e];
        if (!f) continue;
        bool reverse;
        const uint32_t m = anc_mate(mate, name, n_events, e, reverse);
        if (m == ANC_NONE) continue;
        if (f & 1u) {
            const uint64_t b = slot[e];
            if (b < n_blocks) { rows[b] = (uint32_t)e; rows[(reverse ? 3 : 2) * n_blocks + b] = m; }
        }
        if (f & 2u) {
            const uint64_t b = (uint64_t)slot[e + 1] - 1;  // (a tail has its head at or before it: slot[e + 1] >= 1)
            if (slot[e + 1] >= 1 && b < n_blocks) { rows[n_blocks + b] = (uint32_t)e; rows[(reverse ? 2 : 3) * n_blocks + b] = m; }
        }
    }
}

// sums: [0, C) blocks, [C, 2C) anchors, [2C, 3C) edges, [3C, 4C) reverse_edges.  LDS: 4 x C 64-bit bins of dynamic shared memory, or
// none.  A whole wave runs every iteration, lanes past the last block take part in the shuffles and ballots and nothing else.
template <bool LDS>
__global__ void k_anc_sums(const uint32_t *__restrict__ rows, uint64_t n_blocks, const uint32_t *__restrict__ mate, const int64_t *__restrict__ name, uint64_t n_events,
                           const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                           const uint32_t *__restrict__ color, uint32_t n_colors, unsigned long long *__restrict__ sums)
{
    extern __shared__ unsigned long long s_sums[];
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < 4 * n_colors; i += blockDim.x) s_sums[i] = 0;
        __syncthreads();
    }
    unsigned long long *bins = LDS ? s_sums : sums;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b - lane < n_blocks; b += stride) {
        bool active = b < n_blocks;
        uint32_t col = 0xFFFFFFFFu;
        unsigned long long anchors = 0, edges = 0, reverse_edges = 0;
        if (active) {
            const uint32_t qf = rows[b], ql = rows[n_blocks + b];
            const uint32_t lo = qf < n_events ? col_seq_end(seq_begin, n_rec, qf) : 0u;
            active = qf <= ql && ql < n_events && lo >= 1 && lo <= n_rec;
            if (active) {
                col = color[lo - 1];
                active = col < n_colors;
            }
            if (active) {
                bool reverse;
                (void)anc_mate(mate, name, n_events, qf, reverse);
                anchors = (unsigned long long)ql - qf + 1;
                edges = (unsigned long long)end[ql] - begin[qf];
                reverse_edges = reverse ? edges : 0ull;
            }
        }
        const uint32_t col_below = __shfl_up(col, 1);
        const bool head = active && (lane == 0 || col_below != col);
        const unsigned long long heads = __ballot(head), actives = __ballot(active);
        const unsigned long long p_anchors = anc_wave_prefix(anchors, lane), p_edges = anc_wave_prefix(edges, lane), p_reverse = anc_wave_prefix(reverse_edges, lane);
        // every lane names the lane whose prefix closes its run, and the lane below the run (an inactive lane adds 0: it may lie inside)
        const unsigned long long run = head ? col_run(lane, heads, actives) : 0ull;
        const uint32_t last = run ? 63u - (uint32_t)__clzll((long long)run) : lane;
        const unsigned long long a1 = __shfl(p_anchors, last), e1 = __shfl(p_edges, last), r1 = __shfl(p_reverse, last);
        const unsigned long long a0 = __shfl_up(p_anchors, 1), e0 = __shfl_up(p_edges, 1), r0 = __shfl_up(p_reverse, 1);
        if (head) {
            const unsigned long long n = (unsigned long long)__popcll(run), a = a1 - (lane ? a0 : 0ull), ed = e1 - (lane ? e0 : 0ull), rv = r1 - (lane ? r0 : 0ull);
            atomicAdd(&bins[col], n);
            atomicAdd(&bins[n_colors + col], a);
            atomicAdd(&bins[2 * n_colors + col], ed);
            if (rv) atomicAdd(&bins[3 * n_colors + col], rv);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 4 * n_colors; i += blockDim.x) if (s_sums[i]) atomicAdd(&sums[i], s_sums[i]);
    }
}

int anc_needs(tpc_ctx *c)
{
    if (!c->anc.valid) return fail(c, -1, "segment anchors: tpc_segments_anchors_build first");
    return 0;
}

}  // namespace

extern "C" {

int tpc_segments_anchors_build(tpc_ctx *c, const uint32_t *color_of_seq, uint32_t n_colors, uint32_t ref_color)
{
    if (!c) return -1;
    anchors_drop(c);
    if (int rc = stage_needs_segments(c, "anchors", "pair")) return rc;
    if (n_colors == 0) return fail(c, -1, "segment anchors: at least one colour is required");
    if (n_colors > ANC_MAX_COLORS) return fail(c, -1, "segment anchors: %u colours, at most %u are supported", n_colors, ANC_MAX_COLORS);
    if (ref_color >= n_colors) return fail(c, -1, "segment anchors: the reference colour is %u, there are %u colours", ref_color, n_colors);
    const uint32_t n_rec = c->seg.n_rec;
    if (n_rec && !color_of_seq) return fail(c, -1, "segment anchors: the colour of every one of the %u sequences is required", n_rec);
    for (uint32_t s = 0; s < n_rec; s++)
        if (color_of_seq[s] >= n_colors) return fail(c, -1, "segment anchors: sequence %u has colour %u, there are %u colours", s, color_of_seq[s], n_colors);
    HIPCHK(c, hipSetDevice(c->device));
    // the table's own consistency: every event belongs to one of the n_rec sequences
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != c->seg.events) return fail(c, -1, "segment anchors: the stream holds events of more sequences than the %u given", n_rec);

    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments;
    if (n_events >= ANC_MANY) return fail(c, -1, "segment anchors: %llu events, a mate holds at most %u", (unsigned long long)n_events, ANC_MANY - 1);
    // the key: the row above the colour, in as few bits as hold them (row n_rows stands for "no row"); at most 32 + 31 bits
    const uint32_t color_bits = std::max(1u, anc_bits(n_colors - 1)), key_bits = color_bits + std::max(1u, anc_bits(n_rows));
    // sizes in 64 bits, summed before the first allocation; the blocks are not counted yet: at most one per event
    const uint64_t mate_bytes = n_events * 4 + 16, keys_bytes = n_events * 8 + 16, flag_bytes = (n_events + 1) * 4 + 16, ref_bytes = n_rows * 4 + 16;
    const uint64_t sums_bytes = (uint64_t)n_colors * 32 + 8, color_bytes = (uint64_t)n_rec * 4 + 16, rows_bound = n_events * 16 + 16;
    unsigned long long *keys = nullptr, *sorted = nullptr;
    uint32_t *vals = nullptr, *sorted_vals = nullptr, *ref_event = nullptr, *flags = nullptr, *heads = nullptr, *color = nullptr;
    size_t sort_bytes = 0;
    SegRows idx;
    if (!idx.size(c) || rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, sorted, vals, sorted_vals, n_events, 0, key_bits, c->stream) != hipSuccess)
        return fail(c, -10, "segment anchors: the scan and the sort could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, sort_bytes);   // one scratch for the scans and the sort
    const uint64_t need = mate_bytes + 2 * keys_bytes + 2 * mate_bytes + 2 * flag_bytes + ref_bytes + sums_bytes + color_bytes + rows_bound + idx.bytes();
    if (int rc = stage_fits(c, "anchors", need, "%llu of them the keys and values of %llu events in two buffers each, %llu the mates, flags and rows", (unsigned long long)(2 * keys_bytes + 2 * mate_bytes),
                            (unsigned long long)n_events, (unsigned long long)(mate_bytes + 2 * flag_bytes + rows_bound)))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) anchors_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->anc.mate, mate_bytes) != hipSuccess || dev_malloc(c, (void **)&c->anc.sums, sums_bytes) != hipSuccess || !idx.alloc(c, temps) ||
        !temps.get(c, &keys, keys_bytes) || !temps.get(c, &sorted, keys_bytes) || !temps.get(c, &vals, mate_bytes) || !temps.get(c, &sorted_vals, mate_bytes) ||
        !temps.get(c, &ref_event, ref_bytes) || !temps.get(c, &flags, flag_bytes) || !temps.get(c, &heads, flag_bytes) || !temps.get(c, &color, color_bytes))
        return done(fail(c, -10, "segment anchors: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    uint32_t *mate = c->anc.mate;
    unsigned long long *sums = c->anc.sums;
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(mate, 0xFF, mate_bytes, s) == hipSuccess && hipMemsetAsync(sums, 0, sums_bytes, s) == hipSuccess &&
              hipMemsetAsync(ref_event, 0xFF, ref_bytes, s) == hipSuccess && idx.fill(s) &&
              (!n_rec || hipMemcpyAsync(color, color_of_seq, (size_t)n_rec * 4, hipMemcpyHostToDevice, s) == hipSuccess);
    uint32_t n_blocks = 0;
    if (ok) {
        Timed t(c, TPC_K_ANCHORS);   // the whole stage on the stream, the wait for the block count included (as TPC_K_SUPERBUBBLES)
        ok = idx.enqueue(c);
        if (ok && n_events) {
            hipLaunchKernelGGL(k_anc_keys, dim3(col_grid(n_events)), dim3(256), 0, s, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, c->seg.ev[2], n_rec, color,
                               ref_color, c->seg.ev[0], c->seg.ev[1], color_bits, keys, vals, sums + 4 * (uint64_t)n_colors);
            ok = rocprim::radix_sort_pairs(idx.scan_tmp, sort_bytes, keys, sorted, vals, sorted_vals, n_events, 0, key_bits, s) == hipSuccess;
        }
        if (ok && n_events) {
            hipLaunchKernelGGL(k_anc_runs, dim3(col_grid(n_events)), dim3(256), 0, s, sorted, sorted_vals, n_events, n_rows, color_bits, ref_color, ref_event);
            hipLaunchKernelGGL(k_anc_mates, dim3(col_grid(n_events)), dim3(256), 0, s, sorted, sorted_vals, n_events, n_rows, color_bits, ref_color, ref_event, mate);
        }
        if (ok) {
            hipLaunchKernelGGL(k_anc_heads, dim3(col_grid(n_events + 1)), dim3(256), 0, s, mate, c->seg.name, n_events, c->seg.ev[2], n_rec, flags, heads);
            ok = rocprim::exclusive_scan(idx.scan_tmp, idx.scan_bytes, heads, heads, 0u, n_events + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the number of blocks decides the size of what is kept: the one wait in the middle
        ok = ok && idx.total(s) && hipMemcpyAsync(&n_blocks, heads + n_events, sizeof n_blocks, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "anchors", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment anchors: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (n_blocks > n_events) return done(fail(c, -10, "segment anchors: %u blocks over %llu events", n_blocks, (unsigned long long)n_events));
        const uint64_t rows_bytes = (uint64_t)n_blocks * 16 + 16;
        if (dev_malloc(c, (void **)&c->anc.rows, rows_bytes) != hipSuccess) return done(fail(c, -10, "segment anchors: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->anc.rows, 0xFF, rows_bytes, s) == hipSuccess;
        if (ok && n_blocks) {
            hipLaunchKernelGGL(k_anc_place, dim3(col_grid(n_events)), dim3(256), 0, s, mate, c->seg.name, n_events, flags, heads, c->anc.rows, (uint64_t)n_blocks);
            if (n_colors <= ANC_LDS_COLORS)
                hipLaunchKernelGGL(k_anc_sums<true>, dim3(std::min(col_grid(n_blocks), 1024u)), dim3(256), (size_t)n_colors * 32, s, c->anc.rows, (uint64_t)n_blocks, mate, c->seg.name,
                                   n_events, c->seg.ev[0], c->seg.ev[1], c->seg.ev[2], n_rec, color, n_colors, sums);
            else
                hipLaunchKernelGGL(k_anc_sums<false>, dim3(col_grid(n_blocks)), dim3(256), 0, s, c->anc.rows, (uint64_t)n_blocks, mate, c->seg.name, n_events, c->seg.ev[0],
                                   c->seg.ev[1], c->seg.ev[2], n_rec, color, n_colors, sums);
        }
        c->anc.peak_bytes = need - rows_bound + rows_bytes;
    }
    if (int rc = stage_wait(c, "anchors", ok)) return done(rc);
    unsigned long long totals[2] = {0, 0};   // the anchors are the sum over the colours; ref_edges the word behind the sums
    std::vector<unsigned long long> per_color(n_colors);
    HIPCHK(c, hipMemcpy(per_color.data(), sums + n_colors, (size_t)n_colors * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&totals[1], sums + 4 * (uint64_t)n_colors, 8, hipMemcpyDeviceToHost));
    for (unsigned long long a : per_color) totals[0] += a;
    c->anc.n_blocks = n_blocks; c->anc.n_anchors = totals[0]; c->anc.ref_edges = totals[1]; c->anc.n_events = n_events;
    c->anc.n_colors = n_colors; c->anc.ref_color = ref_color;
    c->anc.valid = true;
    return 0;
}

int tpc_segments_anchors_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = anc_needs(c)) return rc;
    if (!info) return fail(c, -1, "segment anchors: info required");
    info[0] = c->anc.n_blocks; info[1] = c->anc.n_anchors; info[2] = c->anc.n_colors; info[3] = c->anc.ref_color; info[4] = c->anc.ref_edges; info[5] = c->anc.peak_bytes;
    return 0;
}

int tpc_segments_anchors_fetch_mates(tpc_ctx *c, uint64_t e0, uint64_t n, uint32_t *mate_host)
{
    if (!c) return -1;
    if (int rc = anc_needs(c)) return rc;
    return fetch_planes(c, "anchors", "event", c->anc.mate, c->anc.n_events, e0, n, { mate_host });
}

int tpc_segments_anchors_fetch_rows(tpc_ctx *c, uint64_t b0, uint64_t n, uint32_t *query_first, uint32_t *query_last, uint32_t *ref_first, uint32_t *ref_last)
{
    if (!c) return -1;
    if (int rc = anc_needs(c)) return rc;
    return fetch_planes(c, "anchors", "block", c->anc.rows, c->anc.n_blocks, b0, n, { query_first, query_last, ref_first, ref_last });
}

int tpc_segments_anchors_fetch_shared(tpc_ctx *c, uint64_t *blocks, uint64_t *anchors, uint64_t *edges, uint64_t *reverse_edges)
{
    if (!c) return -1;
    if (int rc = anc_needs(c)) return rc;
    if (!blocks || !anchors || !edges || !reverse_edges) return fail(c, -1, "segment anchors: all four per-colour arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = c->anc.n_colors;
    uint64_t *dst[4] = {blocks, anchors, edges, reverse_edges};
    for (int i = 0; i < 4; i++) HIPCHK(c, hipMemcpy(dst[i], c->anc.sums + (size_t)i * n, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
