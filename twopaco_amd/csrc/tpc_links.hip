// tpc_links.hip -- the link table of the compacted graph: every distinct link between two segments once, with the number of
// its occurrences, and the bit of every event that closes the first occurrence of its link.  Kernels and the C-ABI of the
// tpc_segments_links_* group of include/twopaco_hip.h, which defines occurrence, class, rows and bits.  No counterpart in the
// reference: its gfa1 prints one L line per occurrence; host/graphformat.h: ComputeLinks is the serial statement.
//
// Input: the event table the last tpc_segments_build_* left in the context (name[e], first[] bits, seq_event_begin[]).
//   k_col_flags, k_col_min, scan   the row of every event's segment (tpc_segrows.h, shared with tpc_colors.hip)
//   k_link_insert  one thread per event.  An event that is not the first of its sequence (binary search in seq_event_begin) closes
//                  an occurrence (name[e - 1], name[e]).  A side is (row << 1 | name < 0), 32 bits, so the spelling is 64 bits,
//                  from << 32 | to; the reversed spelling is (to ^ 1) << 32 | (from ^ 1); the KEY of the class is the smaller of the
//                  two (a class that is its own reverse has both equal).  The key goes into an open-addressed table: 64-bit
//                  atomicCAS on the slot's key from the hash on, linear probing, at most `slots` probes; then atomicMin of e on
//                  the slot's first event, atomicAdd on its count, atomicAdd on its count of occurrences spelled as the key.
//                  HOT KEYS: a poly-A tract gives thousands of consecutive occurrences of one self-loop; lanes compare their key
//                  with the lane below (shuffle), the lanes that differ lead a run (ballot), and the leader alone probes and issues
//                  the three atomics with the run's length, as k_col_scatter of tpc_colors.hip does.  A table without a free slot
//                  raises a flag and the call ends with an error text, never with a wrong table.
//   k_link_bits    one thread per slot: link_first bit of the slot's first event (atomicOr on 32-bit words)
//   k_col_flags, scan   over link_first: the row of every first occurrence, the total is the row count
//   k_link_rows    one thread per slot: first_event, count, same at the slot's row; same = the stored counter when the first
//                  occurrence is spelled as the key, count - counter otherwise
// Memory: kept until the next segment build or link build 12 B / row and 1 bit / event; during the call 20 B / slot (key, first
// event, two counters), 2 x 4 B / event of ranks, the first-sight table (counts[3] of tpc_segments_counts) and the scan's scratch.
// slots = the smallest power of two >= 2 x occurrences, at least 1024.  None of it exists in a context that never asks for links,
// and tpc_segments_counts reports what it reported before.  What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr unsigned long long LINK_EMPTY = ~0ull;        // no key: both spellings of a link cannot be all ones (they differ in bit 0 and bit 32)
constexpr uint64_t LINK_MAX_ROWS = (uint64_t)1 << 31;   // a side is row << 1 | strand in 32 bits
constexpr uint32_t LINK_FLAG_FULL = 1u, LINK_FLAG_ROW = 2u;

__device__ __forceinline__ uint64_t link_hash(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

// the spelling of the occurrence event e closes, LINK_EMPTY when e begins its sequence (or a side is unknown: *bad is set)
__device__ __forceinline__ unsigned long long link_spelling(const int64_t *__restrict__ name, uint64_t e, uint64_t n_events, const uint32_t *__restrict__ table,
                                                            uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows,
                                                            const uint32_t *__restrict__ seq_begin, uint32_t n_rec, bool *bad)
{
    const uint32_t lo = col_seq_end(seq_begin, n_rec, (uint32_t)e);
    if (lo == 0 || seq_begin[lo - 1] == (uint32_t)e) return LINK_EMPTY;
    const uint32_t a = link_side(name, e - 1, n_events, table, n_table, rank, n_rows), b = link_side(name, e, n_events, table, n_table, rank, n_rows);
    if (a == 0xFFFFFFFFu || b == 0xFFFFFFFFu) { *bad = true; return LINK_EMPTY; }
    return ((unsigned long long)a << 32) | b;
}

__device__ __forceinline__ unsigned long long link_key(unsigned long long spelled)
{
    const unsigned long long reversed = ((spelled & 0xFFFFFFFFull) ^ 1ull) << 32 | ((spelled >> 32) ^ 1ull);
    return spelled < reversed ? spelled : reversed;
}

// A whole wave runs every iteration (the stride is a multiple of 64), lanes past the last event take part in the shuffles and
// ballots and nothing else.  slot arrays: key[slots], first[slots] (0xFFFFFFFF), count[slots], canon[slots].
__global__ void k_link_insert(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table,
                              const uint32_t *__restrict__ rank, uint64_t n_rows, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                              unsigned long long *key_of, uint32_t *first_of, uint32_t *count_of, uint32_t *canon_of, uint64_t slots, uint32_t *flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e - lane < n_events; e += stride) {
        unsigned long long key = LINK_EMPTY;
        bool canon = false;
        if (e < n_events) {
            bool bad = false;
            const unsigned long long spelled = link_spelling(name, e, n_events, table, n_table, rank, n_rows, seq_begin, n_rec, &bad);
            if (bad) atomicOr(flags, LINK_FLAG_ROW);
            if (spelled != LINK_EMPTY) { key = link_key(spelled); canon = key == spelled; }
        }
        const bool active = key != LINK_EMPTY;
        const uint32_t lo_below = __shfl_up((uint32_t)key, 1), hi_below = __shfl_up((uint32_t)(key >> 32), 1);
        const bool head = active && (lane == 0 || lo_below != (uint32_t)key || hi_below != (uint32_t)(key >> 32));
        const unsigned long long heads = __ballot(head), actives = __ballot(active), canons = __ballot(active && canon);
        if (head) {
            // (an inactive lane has no key, so the active lane above it leads a run of its own: no run spans one)
            const unsigned long long run = col_run(lane, heads, actives);
            uint64_t at = link_hash(key) & (slots - 1);
            bool placed = false;
            for (uint64_t probes = 0; probes < slots; probes++) {
                unsigned long long seen = key_of[at];
                if (seen == LINK_EMPTY) seen = atomicCAS(&key_of[at], LINK_EMPTY, key);
                if (seen == LINK_EMPTY || seen == key) { placed = true; break; }
                at = (at + 1) & (slots - 1);
            }
            if (placed) {
                atomicMin(&first_of[at], (uint32_t)e);  // the leader's event is the run's first
                atomicAdd(&count_of[at], (uint32_t)__popcll(run));
                const uint32_t nc = (uint32_t)__popcll(run & canons);
                if (nc) atomicAdd(&canon_of[at], nc);
            }
            else atomicOr(flags, LINK_FLAG_FULL);
        }
    }
}

__global__ void k_link_bits(const unsigned long long *__restrict__ key_of, const uint32_t *__restrict__ first_of, uint64_t slots, uint64_t n_events,
                            uint32_t *__restrict__ link_first)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
        if (key_of[i] == LINK_EMPTY) continue;
        const uint32_t e = first_of[i];
        if (e < n_events) atomicOr(&link_first[e >> 5], 1u << (e & 31));
    }
}

// rows: [0, N) first event, [N, 2N) count, [2N, 3N) same
__global__ void k_link_rows(const unsigned long long *__restrict__ key_of, const uint32_t *__restrict__ first_of, const uint32_t *__restrict__ count_of,
                            const uint32_t *__restrict__ canon_of, uint64_t slots, const uint32_t *__restrict__ link_rank, const int64_t *__restrict__ name,
                            uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows,
                            const uint32_t *__restrict__ seq_begin, uint32_t n_rec, uint32_t *__restrict__ rows, uint64_t n_links, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
        const unsigned long long key = key_of[i];
        if (key == LINK_EMPTY) continue;
        const uint32_t e = first_of[i];
        const uint64_t r = e < n_events ? link_rank[e] : n_links;
        bool bad = false;
        const unsigned long long spelled = e < n_events ? link_spelling(name, e, n_events, table, n_table, rank, n_rows, seq_begin, n_rec, &bad) : LINK_EMPTY;
        if (r >= n_links || spelled == LINK_EMPTY || link_key(spelled) != key) { atomicOr(flags, LINK_FLAG_ROW); continue; }
        rows[r] = e;
        rows[n_links + r] = count_of[i];
        rows[2 * n_links + r] = spelled == key ? canon_of[i] : count_of[i] - canon_of[i];
    }
}

}  // namespace

extern "C" {

int tpc_segments_links_build(tpc_ctx *c)
{
    if (!c) return -1;
    links_drop(c);
    if (int rc = stage_needs_segments(c, "links", "link")) return rc;
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments;
    const uint32_t n_rec = c->seg.n_rec;
    if (n_rows > LINK_MAX_ROWS) return fail(c, -1, "segment links: %llu segments, a link's key holds at most %llu", (unsigned long long)n_rows, (unsigned long long)LINK_MAX_ROWS);
    if (c->opt_links_slots_log2 < 0 || c->opt_links_slots_log2 > 40) return fail(c, -1, "segment links: option test_links_slots_log2 = %d is not in 0 .. 40", c->opt_links_slots_log2);
    HIPCHK(c, hipSetDevice(c->device));
    // occurrences: every event but the first of its sequence; the table's own consistency: every event belongs to one of the n_rec sequences
    std::vector<uint32_t> seq_begin((size_t)n_rec + 1);
    HIPCHK(c, hipMemcpy(seq_begin.data(), c->seg.ev[2], seq_begin.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (seq_begin[0] != 0 || seq_begin[n_rec] != n_events) return fail(c, -1, "segment links: the stream holds events of more sequences than the %u given", n_rec);
    uint64_t with_events = 0;
    for (uint32_t s = 0; s < n_rec; s++) {
        if (seq_begin[s] > seq_begin[s + 1]) return fail(c, -1, "segment links: the sequences' event ranges must ascend");
        with_events += seq_begin[s + 1] > seq_begin[s];
    }
    const uint64_t occurrences = n_events - with_events;
    uint64_t slots = 1024;
    if (c->opt_links_slots_log2) slots = (uint64_t)1 << c->opt_links_slots_log2;
    else while (slots < 2 * occurrences) slots <<= 1;

    // sizes in 64 bits, summed before the first allocation; the rows are not counted yet: their bound is one per occurrence
    const uint64_t first_words = (n_events + 31) / 32;
    const uint64_t slot_bytes = slots * 20 + 64, first_bytes = first_words * 4 + 16;
    const uint64_t rows_bound = occurrences * 12 + 16;
    SegRows idx;
    if (!idx.size(c)) return fail(c, -10, "segment links: the scan could not be sized");
    // (the second rank_bytes: link_rank, scanned over the same scratch)
    const uint64_t need = slot_bytes + idx.bytes() + idx.rank_bytes + first_bytes + rows_bound + 16 + 64;
    if (int rc = stage_fits(c, "links", need, "%llu of them the %llu slots of the link set", (unsigned long long)slot_bytes, (unsigned long long)slots)) return rc;
    StageTemps temps;
    uint32_t *link_rank = nullptr, *flags = nullptr;
    unsigned long long *key_of = nullptr;
    auto done = [&](int code) {
        if (code) links_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->lnk.first, first_bytes) != hipSuccess || !temps.get(c, &key_of, slot_bytes) || !idx.alloc(c, temps) ||
        !temps.get(c, &link_rank, idx.rank_bytes) || !temps.get(c, &flags, 64))
        return done(fail(c, -10, "segment links: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    uint32_t *first_of = (uint32_t *)(key_of + slots), *count_of = first_of + slots, *canon_of = count_of + slots;
    hipStream_t s = c->stream;
    // keys and first events all ones (no key, no event), the counters zero
    bool ok = hipMemsetAsync(key_of, 0xFF, slots * 12, s) == hipSuccess && hipMemsetAsync(count_of, 0, slots * 8, s) == hipSuccess &&
              hipMemsetAsync(c->lnk.first, 0, first_bytes, s) == hipSuccess && idx.fill(s) &&
              hipMemsetAsync(flags, 0, 64, s) == hipSuccess;
    uint32_t n_links = 0, raised = 0;
    if (ok) {
        Timed t(c, TPC_K_LINKS);
        ok = idx.enqueue(c);
        if (ok && n_events) {
            hipLaunchKernelGGL(k_link_insert, dim3(col_grid(n_events)), dim3(256), 0, s, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, c->seg.ev[2], n_rec,
                               key_of, first_of, count_of, canon_of, slots, flags);
            hipLaunchKernelGGL(k_link_bits, dim3(col_grid(slots)), dim3(256), 0, s, key_of, first_of, slots, n_events, c->lnk.first);
        }
        if (ok) {
            hipLaunchKernelGGL(k_col_flags, dim3(col_grid(n_events + 1)), dim3(256), 0, s, c->lnk.first, n_events, link_rank);
            ok = rocprim::exclusive_scan(idx.scan_tmp, idx.scan_bytes, link_rank, link_rank, 0u, n_events + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the row count decides the size of what is kept: one wait in the middle
        ok = ok && idx.total(s) && hipMemcpyAsync(&n_links, link_rank + n_events, sizeof n_links, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "links", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment links: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (raised & LINK_FLAG_FULL)
            return done(fail(c, -21, "segment links: the link set of %llu slots is full (%llu occurrences); no table was made", (unsigned long long)slots, (unsigned long long)occurrences));
        if (raised & LINK_FLAG_ROW) return done(fail(c, -10, "segment links: an event's segment is missing from the first-sight table"));
        if (n_links > occurrences) return done(fail(c, -10, "segment links: %u links out of %llu occurrences", n_links, (unsigned long long)occurrences));
        const uint64_t rows_bytes = (uint64_t)n_links * 12 + 16;
        if (dev_malloc(c, (void **)&c->lnk.rows, rows_bytes) != hipSuccess) return done(fail(c, -10, "segment links: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        if (n_links)
            hipLaunchKernelGGL(k_link_rows, dim3(col_grid(slots)), dim3(256), 0, s, key_of, first_of, count_of, canon_of, slots, link_rank, c->seg.name, n_events, idx.table, idx.n_table,
                               idx.rank, n_rows, c->seg.ev[2], n_rec, c->lnk.rows, (uint64_t)n_links, flags);
        ok = hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->lnk.peak_bytes = need - rows_bound + rows_bytes;
    }
    if (int rc = stage_wait(c, "links", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment links: a slot's first occurrence does not spell its key"));
    c->lnk.n_rows = n_links; c->lnk.occurrences = occurrences; c->lnk.slots = slots;
    c->lnk.valid = true;
    return 0;
}

int tpc_segments_links_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->lnk.valid) return fail(c, -1, "segment links: tpc_segments_links_build first");
    if (!info) return fail(c, -1, "segment links: info required");
    info[0] = c->lnk.n_rows; info[1] = c->lnk.occurrences; info[2] = c->lnk.slots; info[3] = c->lnk.peak_bytes;
    return 0;
}

int tpc_segments_links_fetch_rows(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *first_event_host, uint32_t *count_host, uint32_t *same_host)
{
    if (!c) return -1;
    if (!c->lnk.valid) return fail(c, -1, "segment links: tpc_segments_links_build first");
    return fetch_planes(c, "links", "row", c->lnk.rows, c->lnk.n_rows, r0, n, { first_event_host, count_host, same_host });
}

int tpc_segments_links_fetch_first(tpc_ctx *c, uint64_t word0, uint64_t n_words, uint32_t *bits_host)
{
    if (!c) return -1;
    if (!c->lnk.valid) return fail(c, -1, "segment links: tpc_segments_links_build first");
    const uint64_t words = (c->seg.events + 31) / 32;
    if ((n_words && !bits_host) || word0 > words || n_words > words - word0)
        return fail(c, -1, "segment links: bad first-bit range (%llu words at %llu of %llu)", (unsigned long long)n_words, (unsigned long long)word0, (unsigned long long)words);
    HIPCHK(c, hipSetDevice(c->device));
    if (n_words) HIPCHK(c, hipMemcpy(bits_host, c->lnk.first + word0, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
