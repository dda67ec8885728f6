// tpc_superbubbles.hip -- the SUPERBUBBLES of the compacted graph (Onodera, Sadakane, Shibuya 2013), bounded to 64 sides: the places
// where the paths that leave one side of a segment meet again at one side of another and touch nothing else on their way -- two
// substitutions closer than k, a substitution beside an indel, three alleles at one site, and the simple bubble as the smallest case.
// Kernels and the C-ABI of the tpc_segments_superbubbles_* group of include/twopaco_hip.h, which defines U(s, t), matching, acyclic,
// one strand per segment, minimal, bounded, the reporting rule and what a row carries.  No counterpart in the reference;
// host/graphformat.h states the same definition for the serial program.
//
// Input: the event table of the last tpc_segments_build_*, the link rows of the last tpc_segments_links_build and the colour rows of
// the last tpc_segments_colors_build (first event -> weight end - begin, presence).  The row of every event's segment is made again
// (tpc_segrows.h); a side is link_side(..).
//   ADJACENCY
//   k_sb_arcs     one thread per link row: the arcs from -> to and to ^ 1 -> from ^ 1 as 64-bit keys tail << 32 | head at 2 r and
//                 2 r + 1 (a link that is its own reverse gives one arc, its second key is all ones), atomicAdd(deg[tail], 1)
//   scan          exclusive, over deg: the CSR offsets [2 S + 1], the total is the number of arcs
//   radix sort    of the keys: every side's heads lie together and ascend, the all-ones keys last.  The lists do not depend on the
//                 schedule, and a hub is sorted by the whole device like everything else: no lane walks a long list.
//   k_sb_heads    heads[a] = the low half of key a
//   SEARCH
//   k_sb_flag, scan, k_sb_compact   the sides of degree 2 or more, compacted: most sides have degree 1
//   k_sb_search   one thread per candidate s: sb_walk, Onodera's per-entrance procedure.  A work list of the sides seen, each with the
//                 number of its in-neighbours not visited yet; a side all of whose in-neighbours are visited is visited next; the walk
//                 fails on a dead end, an arc back to s, a side whose other strand is in the list, a side of degree above 64 (in or
//                 out), and on an entry beyond max_inside + 2; it stops when one side is left unvisited and that side is ready, and
//                 then fails if that side has an arc to s (a binary search of its sorted list).  EVERY LOOP IS A for TO A BOUND: at
//                 most 63 sides are visited, each has at most 64 arcs, the list holds at most 64 entries, the binary search takes at
//                 most 32 steps.  Nothing waits on another lane.  The list lives in LDS, 4 B of code and 1 B of pending count per
//                 entry, entry e of lane l at [e][l] so that the lanes of a wave hit different banks: 20 KiB per workgroup of 64.
//                 Writes exit[s] (all ones: none) and, for the one wait below, the list's length.
//   REPORT
//   k_sb_keep     one thread per side: the reporting rule -- exit(s) = t and (s < rev(t) or exit(rev(t)) != rev(s)); a flag and the
//                 size of the inside; entrances whose mirror is missing are counted
//   two scans     the rank of every reported row and the offset of its members; the host waits once, for both totals
//   k_sb_place    entrance, exit and the member offset at the row's rank (ascending entrance code by construction)
//   k_sb_report   one wave per reported row: lane 0 walks again and leaves the list and the order of the visits -- a topological
//                 order of U -- in LDS; then lane j owns list entry j, and the wave goes through the visited sides in that order and
//                 through their arcs, all lanes in step: the lane that owns the head adds the tail's paths, and takes the smaller and
//                 the larger sum of weights.  inside, arcs, paths, min_edges, max_edges at the exit's lane; the members by counting
//                 the smaller codes; the presence words by an OR over the wave.
// Integers, commutative sums, minima, maxima and ORs over sets that do not depend on the schedule: the arrays are exact.
// Memory: kept until the next segment, link, colour or superbubble build 4 B / side of offsets, 4 B / arc of heads, 4 B / side of
// exits, per row 20 B + 24 B + 4 W B + 4 B of offset, 4 B per member; during the call 16 B / arc of keys and the sort's scratch, 20 B /
// side of degrees, flags, candidates and sizes, and the row index.  What does not fit the free device memory is refused.
#include "tpc_segrows.h"

namespace {

constexpr uint64_t SB_MAX_ROWS = ((uint64_t)1 << 31) - 1;   // a side is row << 1 | strand in 32 bits, all ones is no side
constexpr uint32_t SB_NONE = 0xFFFFFFFFu;
constexpr uint32_t SB_FLAG_ROW = 1u, SB_FLAG_EVENT = 2u, SB_FLAG_WALK = 4u;
constexpr int SB_LIST = 64;         // entries of a work list: entrance, at most 62 inside, exit
constexpr int SB_U32_PLANES = 5;    // entrance, exit, inside, arcs, n_colors
constexpr int SB_U64_PLANES = 3;    // paths, min_edges, max_edges

__device__ __forceinline__ unsigned long long sb_bit(uint32_t i) { return 1ull << i; }

// keys: [2 n_links], all ones beforehand.  deg: [n_sides + 1], zero beforehand (the scan's last element is the number of arcs)
__global__ void k_sb_arcs(const uint32_t *__restrict__ first_event, uint64_t n_links, const int64_t *__restrict__ name, uint64_t n_events,
                          const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows,
                          unsigned long long *__restrict__ keys, uint32_t *__restrict__ deg, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_links; r += stride) {
        const uint64_t e = first_event[r];
        if (e == 0 || e >= n_events) { atomicOr(flags, SB_FLAG_EVENT); continue; }
        const uint32_t from = link_side(name, e - 1, n_events, table, n_table, rank, n_rows), to = link_side(name, e, n_events, table, n_table, rank, n_rows);
        if (from == SB_NONE || to == SB_NONE) { atomicOr(flags, SB_FLAG_ROW); continue; }  // (a side is below 2 x n_rows otherwise)
        keys[2 * r] = (unsigned long long)from << 32 | to;
        atomicAdd(&deg[from], 1u);
        if (to != (from ^ 1u)) {   // a+ a- is its own reverse: one arc
            keys[2 * r + 1] = (unsigned long long)(to ^ 1u) << 32 | (from ^ 1u);
            atomicAdd(&deg[to ^ 1u], 1u);
        }
    }
}

__global__ void k_sb_heads(const unsigned long long *__restrict__ keys, uint64_t n_keys, const uint32_t *__restrict__ off, uint64_t n_sides, uint32_t *__restrict__ heads)
{
    const uint64_t n_arcs = off[n_sides];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n_arcs && a < n_keys; a += stride) heads[a] = (uint32_t)keys[a];
}

// n_sides + 1 entries: the scan's last element is the number of candidates
__global__ void k_sb_flag(const uint32_t *__restrict__ off, uint64_t n_sides, uint32_t *__restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_sides; i += stride) flag[i] = i < n_sides && off[i + 1] - off[i] >= 2 ? 1u : 0u;
}

__global__ void k_sb_compact(const uint32_t *__restrict__ where, uint64_t n_sides, uint32_t *__restrict__ cand)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_sides; i += stride)
        if (where[i + 1] != where[i]) cand[where[i]] = (uint32_t)i;
}

// Onodera's per-entrance procedure from s.  list / pend / ord: this walk's arrays, entry e at [e * STRIDE].  Returns the exit or
// SB_NONE; *n_list is the list's length (|U|) and *n_visited the number of entries of ord (U without the exit, in a topological order).
template <int STRIDE, bool RECORD>
__device__ __forceinline__ uint32_t sb_walk(uint32_t s, const uint32_t *__restrict__ off, const uint32_t *__restrict__ heads, uint32_t max_entries,
                                            uint32_t *list, uint8_t *pend, uint8_t *ord, uint32_t *n_list, uint32_t *n_visited)
{
    *n_list = 0; *n_visited = 0;
    const uint32_t ds = off[s + 1] - off[s];
    if (ds < 2 || ds > SB_LIST) return SB_NONE;   // more than 64 out-neighbours cannot lie within 64 sides
    uint32_t n = 1, exit_at = SB_NONE;
    unsigned long long visited = 0, ready = 1;
    list[0] = s;
    pend[0] = 0;
    for (uint32_t step = 0; step < SB_LIST - 1 && exit_at == SB_NONE; step++) {   // the exit is never visited: 63 visits at most
        if (!ready) return SB_NONE;               // sides are seen but none has all its in-neighbours visited: a way in from outside, or a cycle
        const uint32_t i = (uint32_t)__ffsll((long long)ready) - 1;
        ready &= ~sb_bit(i);
        visited |= sb_bit(i);
        if (RECORD) ord[step * STRIDE] = (uint8_t)i;
        const uint32_t v = list[i * STRIDE], a0 = off[v], d = off[v + 1] - a0;
        if (d == 0 || d > SB_LIST) return SB_NONE;   // a dead end; a hub
        for (uint32_t a = 0; a < d; a++) {
            const uint32_t u = heads[a0 + a];
            uint32_t j = SB_NONE;
            bool other_strand = false;
            for (uint32_t q = 0; q < n; q++) {
                const uint32_t code = list[q * STRIDE];
                if (code == u) j = q;
                other_strand = other_strand || code == (u ^ 1u);
            }
            // an arc back to s; both strands of a row (list[0] is s, so rev(s) as well)
            if (u == s || other_strand) return SB_NONE;
            if (j == SB_NONE) {
                if (n >= max_entries) return SB_NONE;
                const uint32_t in_degree = off[(u ^ 1u) + 1] - off[u ^ 1u];   // in(u) = rev(out(rev(u)))
                if (in_degree > SB_LIST) return SB_NONE;
                j = n++;
                list[j * STRIDE] = u;
                pend[j * STRIDE] = (uint8_t)in_degree;
            }
            const uint32_t left = pend[j * STRIDE];
            if ((visited & sb_bit(j)) || left == 0) return SB_NONE;   // (every in-neighbour arrives once: cannot happen)
            pend[j * STRIDE] = (uint8_t)(left - 1);
            if (left == 1) ready |= sb_bit(j);
        }
        const unsigned long long unvisited = (n == 64 ? ~0ull : sb_bit(n) - 1) & ~visited;
        *n_visited = step + 1;
        if (__popcll(unvisited) == 1 && ready == unvisited) exit_at = (uint32_t)__ffsll((long long)unvisited) - 1;
    }
    if (exit_at == SB_NONE) return SB_NONE;
    const uint32_t t = list[exit_at * STRIDE];
    // an arc t -> s closes a cycle: out(t) ascends
    uint32_t lo = off[t], hi = off[t + 1];
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (heads[mid] < s) lo = mid + 1; else hi = mid;
    }
    if (lo < off[t + 1] && heads[lo] == s) return SB_NONE;
    *n_list = n;
    return t;
}

// exit: [n_sides], all ones beforehand.  size: [n_sides], zero beforehand: |U| of the sides that are entrances
__global__ __launch_bounds__(64) void k_sb_search(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ n_cand_at, const uint32_t *__restrict__ off,
                                                  const uint32_t *__restrict__ heads, uint32_t max_entries, uint32_t *__restrict__ exit_of, uint32_t *__restrict__ size)
{
    __shared__ uint32_t s_list[SB_LIST * 64];
    __shared__ uint8_t s_pend[SB_LIST * 64];
    const uint64_t n_cand = *n_cand_at;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cand; i += stride) {
        const uint32_t s = cand[i];
        uint32_t n_list, n_visited;
        const uint32_t t = sb_walk<64, false>(s, off, heads, max_entries, s_list + threadIdx.x, s_pend + threadIdx.x, nullptr, &n_list, &n_visited);
        exit_of[s] = t;
        size[s] = t == SB_NONE ? 0u : n_list;
    }
}

// flag / members: n_sides + 1 entries each: the scans' last elements are the rows and the members in total.  counters[0]: the entrances
// whose mirror is missing
__global__ void k_sb_keep(const uint32_t *__restrict__ exit_of, const uint32_t *__restrict__ size, uint64_t n_sides, uint32_t *__restrict__ flag,
                          uint32_t *__restrict__ members, unsigned long long *__restrict__ counters)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_sides; i += stride) {
        uint32_t keep = 0, inside = 0;
        if (i < n_sides) {
            const uint32_t s = (uint32_t)i, t = exit_of[i];
            if (t != SB_NONE && t < n_sides) {
                const bool mirrored = exit_of[t ^ 1u] == (s ^ 1u);
                if (!mirrored) atomicAdd(&counters[0], 1ull);
                keep = s < (t ^ 1u) || !mirrored ? 1u : 0u;
                inside = keep ? size[i] - 2 : 0u;
            }
        }
        flag[i] = keep;
        members[i] = inside;
    }
}

// u32: [SB_U32_PLANES][n_rows]; member_off: [n_rows + 1]
__global__ void k_sb_place(const uint32_t *__restrict__ exit_of, uint64_t n_sides, const uint32_t *__restrict__ where, const uint32_t *__restrict__ member_where,
                           uint32_t *__restrict__ u32, uint32_t *__restrict__ member_off, uint64_t n_rows, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_sides; i += stride) {
        if (i == n_sides) { member_off[n_rows] = member_where[n_sides]; continue; }
        const uint64_t at = where[i];
        if (where[i + 1] == at) continue;
        if (at >= n_rows) { atomicOr(flags, SB_FLAG_WALK); continue; }
        u32[at] = (uint32_t)i;
        u32[n_rows + at] = exit_of[i];
        member_off[at] = member_where[i];
    }
}

// One wave per row.  col_rows: the colour table's first plane, the first event of every row.
__global__ __launch_bounds__(64) void k_sb_report(const uint32_t *__restrict__ off, const uint32_t *__restrict__ heads, uint32_t max_entries, uint64_t n_rows,
                                                  uint64_t n_segments, const uint32_t *__restrict__ col_rows, const uint32_t *__restrict__ col_presence, uint32_t words,
                                                  const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint64_t n_events, uint32_t *__restrict__ u32,
                                                  unsigned long long *__restrict__ u64, uint32_t *__restrict__ presence, const uint32_t *__restrict__ member_off,
                                                  uint32_t *__restrict__ members, uint64_t n_members, uint32_t *__restrict__ flags)
{
    __shared__ uint32_t s_list[SB_LIST];
    __shared__ uint8_t s_pend[SB_LIST], s_ord[SB_LIST];
    __shared__ uint32_t s_head[4];   // exit, |U|, visits
    const uint32_t lane = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < n_rows; b += gridDim.x) {
        __syncthreads();   // the previous row's arrays are read no more
        const uint32_t s = u32[b];
        if (lane == 0) {
            uint32_t n_list, n_visited;
            s_head[0] = sb_walk<1, true>(s, off, heads, max_entries, s_list, s_pend, s_ord, &n_list, &n_visited);
            s_head[1] = n_list; s_head[2] = n_visited;
        }
        __syncthreads();
        const uint32_t t = s_head[0], n = s_head[1], n_visited = s_head[2];
        const uint64_t m0 = member_off[b], m1 = member_off[b + 1];
        // what the search found is found again, or nothing is written
        if (t == SB_NONE || t != u32[n_rows + b] || n < 3 || n > SB_LIST || n_visited != n - 1 || m1 - m0 != n - 2 || m1 > n_members) {
            if (lane == 0) atomicOr(flags, SB_FLAG_WALK);
            continue;
        }
        const bool owns = lane < n;
        const uint32_t code = owns ? s_list[lane] : SB_NONE;
        const bool inside = owns && code != s && code != t;
        unsigned long long weight = 0;
        if (inside) {
            const uint32_t e0 = col_rows[code >> 1];
            if (e0 < n_events) weight = (unsigned long long)end[e0] - begin[e0];
            else atomicOr(flags, SB_FLAG_EVENT);
        }
        unsigned long long paths = lane == 0 ? 1ull : 0ull, low = lane == 0 ? 0ull : ~0ull, high = 0;
        uint32_t arcs = 0;
        for (uint32_t step = 0; step < n_visited; step++) {   // all lanes in step: the bounds are the wave's
            const uint32_t iv = s_ord[step];
            const unsigned long long paths_v = __shfl(paths, iv), low_v = __shfl(low, iv), high_v = __shfl(high, iv);
            const uint32_t v = s_list[iv], a0 = off[v], d = off[v + 1] - a0;
            arcs += d;   // every arc that leaves a side of U other than the exit ends in U
            for (uint32_t a = 0; a < d; a++) {
                if (heads[a0 + a] != code) continue;
                paths += paths_v;
                low = min(low, low_v + weight);
                high = max(high, high_v + weight);
            }
        }
        if (owns && code == t) {
            u32[2 * n_rows + b] = n - 2;
            u32[3 * n_rows + b] = arcs;
            u64[b] = paths;
            u64[n_rows + b] = low;
            u64[2 * n_rows + b] = high;
        }
        if (inside) {
            uint32_t smaller = 0;
            for (uint32_t q = 0; q < n; q++) {
                const uint32_t other = s_list[q];
                smaller += other != s && other != t && other < code ? 1u : 0u;
            }
            members[m0 + smaller] = code;
        }
        uint32_t colors = 0;
        for (uint32_t w = 0; w < words; w++) {
            uint32_t bits = inside && (code >> 1) < n_segments ? col_presence[(uint64_t)(code >> 1) * words + w] : 0u;
            for (uint32_t dlt = 1; dlt < 64; dlt <<= 1) bits |= __shfl_xor(bits, dlt);
            if (lane == 0) presence[b * words + w] = bits;
            colors += __popc(bits);
        }
        if (lane == 0) u32[4 * n_rows + b] = colors;
    }
}

int sb_fetch_check(tpc_ctx *c, const char *what, uint64_t total, uint64_t at, uint64_t n, bool missing)
{
    if ((n && missing) || at > total || n > total - at)
        return fail(c, -1, "segment superbubbles: bad %s range (%llu %ss at %llu of %llu)", what, (unsigned long long)n, what, (unsigned long long)at, (unsigned long long)total);
    return 0;
}

int sb_needs(tpc_ctx *c)
{
    if (!c->sbb.valid) return fail(c, -1, "segment superbubbles: tpc_segments_superbubbles_build first");
    return 0;
}

}  // namespace

extern "C" {

int tpc_segments_superbubbles_build(tpc_ctx *c, uint32_t max_inside)
{
    if (!c) return -1;
    superbubbles_drop(c);
    if (int rc = stage_needs_segments(c, "superbubbles", "join")) return rc;
    if (!c->lnk.valid) return fail(c, -1, "segment superbubbles: build the link table first (tpc_segments_links_build)");
    if (!c->col.valid) return fail(c, -1, "segment superbubbles: build the colour table first (tpc_segments_colors_build)");
    if (max_inside < 2 || max_inside > SB_LIST - 2)
        return fail(c, -1, "segment superbubbles: max_inside = %u, allowed are 2 .. %d", max_inside, SB_LIST - 2);
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments, n_links = c->lnk.n_rows;
    const uint32_t words = c->col.words;
    if (n_rows > SB_MAX_ROWS) return fail(c, -1, "segment superbubbles: %llu segments, a side holds at most %llu", (unsigned long long)n_rows, (unsigned long long)SB_MAX_ROWS);
    if (c->col.n_rows != n_rows) return fail(c, -10, "segment superbubbles: the colour table holds %llu rows, the build counted %llu segments", (unsigned long long)c->col.n_rows, (unsigned long long)n_rows);
    if (2 * n_links > 0xFFFFFFFEull) return fail(c, -1, "segment superbubbles: %llu links, an offset holds at most %llu arcs", (unsigned long long)n_links, 0xFFFFFFFEull);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n_sides = 2 * n_rows, n_keys = 2 * n_links;

    // sizes in 64 bits, summed before the first allocation; the rows and members are not counted yet: their bounds are one row per two
    // sides and max_inside members per row
    const uint64_t side_bytes = (n_sides + 1) * 4 + 16, keys_bytes = n_keys * 8 + 16, heads_bytes = n_keys * 4 + 16;
    const uint64_t per_row = SB_U32_PLANES * 4 + SB_U64_PLANES * 8 + (uint64_t)words * 4 + 4 + (uint64_t)max_inside * 4, rows_bound = n_rows * per_row + 64;
    size_t scan_side = 0, sort_bytes = 0;
    uint32_t *deg = nullptr, *flag = nullptr, *cand = nullptr, *size = nullptr, *msize = nullptr, *flags = nullptr;
    unsigned long long *keys = nullptr, *sorted = nullptr;
    SegRows idx;
    if (!idx.size(c) || rocprim::exclusive_scan(nullptr, scan_side, flag, flag, 0u, n_sides + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess ||
        rocprim::radix_sort_keys(nullptr, sort_bytes, keys, sorted, n_keys, 0, 64, c->stream) != hipSuccess)
        return fail(c, -10, "segment superbubbles: the scan and the sort could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, std::max(scan_side, sort_bytes));   // one scratch for the scans and the sort
    const uint64_t kept_sides = 2 * side_bytes;   // offsets, exits
    const uint64_t need = kept_sides + heads_bytes + 5 * side_bytes + 2 * keys_bytes + rows_bound + idx.bytes() + 64;
    if (int rc = stage_fits(c, "superbubbles", need, "%llu of them the keys of %llu arcs, %llu the offsets, exits and temporaries of %llu sides", (unsigned long long)(2 * keys_bytes),
                            (unsigned long long)n_keys, (unsigned long long)(7 * side_bytes), (unsigned long long)n_sides))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) superbubbles_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->sbb.off, side_bytes) != hipSuccess || dev_malloc(c, (void **)&c->sbb.heads, heads_bytes) != hipSuccess ||
        dev_malloc(c, (void **)&c->sbb.exit_of, side_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &deg, side_bytes) || !temps.get(c, &flag, side_bytes) ||
        !temps.get(c, &cand, side_bytes) || !temps.get(c, &size, side_bytes) || !temps.get(c, &msize, side_bytes) || !temps.get(c, &keys, keys_bytes) ||
        !temps.get(c, &sorted, keys_bytes) || !temps.get(c, &flags, 64))
        return done(fail(c, -10, "segment superbubbles: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    uint32_t *off = c->sbb.off, *heads = c->sbb.heads, *exit_of = c->sbb.exit_of;
    unsigned long long *counters = (unsigned long long *)(flags + 2);   // 8 bytes into the 64: flags[0], then counters[0]
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(deg, 0, side_bytes, s) == hipSuccess && hipMemsetAsync(keys, 0xFF, keys_bytes, s) == hipSuccess &&
              hipMemsetAsync(exit_of, 0xFF, side_bytes, s) == hipSuccess && hipMemsetAsync(size, 0, side_bytes, s) == hipSuccess && idx.fill(s) &&
              hipMemsetAsync(flags, 0, 64, s) == hipSuccess;
    uint32_t n_found = 0, n_members = 0, n_arcs = 0, raised = 0;
    unsigned long long unmirrored = 0;
    if (ok) {
        Timed t(c, TPC_K_SUPERBUBBLES);   // the whole stage on the stream, the wait for the two totals included (as TPC_K_BUBBLES)
        ok = idx.enqueue(c);
        if (ok && n_links)
            hipLaunchKernelGGL(k_sb_arcs, dim3(col_grid(n_links)), dim3(256), 0, s, c->lnk.rows, n_links, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, keys, deg, flags);
        ok = ok && rocprim::exclusive_scan(idx.scan_tmp, scan_side, deg, off, 0u, n_sides + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        if (ok && n_keys) {
            ok = rocprim::radix_sort_keys(idx.scan_tmp, sort_bytes, keys, sorted, n_keys, 0, 64, s) == hipSuccess;
            if (ok) hipLaunchKernelGGL(k_sb_heads, dim3(col_grid(n_keys)), dim3(256), 0, s, sorted, n_keys, off, n_sides, heads);
        }
        if (ok) {
            hipLaunchKernelGGL(k_sb_flag, dim3(col_grid(n_sides + 1)), dim3(256), 0, s, off, n_sides, flag);
            ok = rocprim::exclusive_scan(idx.scan_tmp, scan_side, flag, flag, 0u, n_sides + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        if (ok && n_sides) {
            hipLaunchKernelGGL(k_sb_compact, dim3(col_grid(n_sides)), dim3(256), 0, s, flag, n_sides, cand);
            // the candidates are few and uneven: one wave per workgroup, the grid by the sides
            hipLaunchKernelGGL(k_sb_search, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_sides + 63) / 64, 8192))), dim3(64), 0, s, cand, flag + n_sides, off, heads,
                               max_inside + 2, exit_of, size);
        }
        if (ok) {
            hipLaunchKernelGGL(k_sb_keep, dim3(col_grid(n_sides + 1)), dim3(256), 0, s, exit_of, size, n_sides, flag, msize, counters);
            ok = rocprim::exclusive_scan(idx.scan_tmp, scan_side, flag, flag, 0u, n_sides + 1, rocprim::plus<uint32_t>(), s) == hipSuccess &&
                 rocprim::exclusive_scan(idx.scan_tmp, scan_side, msize, msize, 0u, n_sides + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the number of rows and of members decide the size of what is kept: the one wait in the middle
        ok = ok && idx.total(s) && hipMemcpyAsync(&n_found, flag + n_sides, sizeof n_found, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&n_members, msize + n_sides, sizeof n_members, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&n_arcs, off + n_sides, sizeof n_arcs, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&unmirrored, counters, sizeof unmirrored, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "superbubbles", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment superbubbles: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (raised & SB_FLAG_EVENT) return done(fail(c, -10, "segment superbubbles: a link row's first event lies outside the event table"));
        if (raised & SB_FLAG_ROW) return done(fail(c, -10, "segment superbubbles: an event's segment is missing from the first-sight table"));
        if (n_arcs > n_keys || n_found > n_sides || (uint64_t)n_members > (uint64_t)n_found * max_inside || unmirrored > n_sides)
            return done(fail(c, -10, "segment superbubbles: %u superbubbles with %u members over %u arcs on %llu sides", n_found, n_members, n_arcs, (unsigned long long)n_sides));
        const uint64_t u32_bytes = (uint64_t)n_found * SB_U32_PLANES * 4 + 16, u64_bytes = (uint64_t)n_found * SB_U64_PLANES * 8 + 16;
        const uint64_t presence_bytes = (uint64_t)n_found * words * 4 + 16, moff_bytes = ((uint64_t)n_found + 1) * 4 + 16, members_bytes = (uint64_t)n_members * 4 + 16;
        if (dev_malloc(c, (void **)&c->sbb.u32, u32_bytes) != hipSuccess || dev_malloc(c, (void **)&c->sbb.u64, u64_bytes) != hipSuccess ||
            dev_malloc(c, (void **)&c->sbb.presence, presence_bytes) != hipSuccess || dev_malloc(c, (void **)&c->sbb.member_off, moff_bytes) != hipSuccess ||
            dev_malloc(c, (void **)&c->sbb.members, members_bytes) != hipSuccess)
            return done(fail(c, -10, "segment superbubbles: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->sbb.u32, 0, u32_bytes, s) == hipSuccess && hipMemsetAsync(c->sbb.u64, 0, u64_bytes, s) == hipSuccess &&
             hipMemsetAsync(c->sbb.presence, 0, presence_bytes, s) == hipSuccess && hipMemsetAsync(c->sbb.member_off, 0, moff_bytes, s) == hipSuccess &&
             hipMemsetAsync(c->sbb.members, 0xFF, members_bytes, s) == hipSuccess;
        if (ok) hipLaunchKernelGGL(k_sb_place, dim3(col_grid(n_sides + 1)), dim3(256), 0, s, exit_of, n_sides, flag, msize, c->sbb.u32, c->sbb.member_off, (uint64_t)n_found, flags);
        if (ok && n_found)
            hipLaunchKernelGGL(k_sb_report, dim3((unsigned)std::min<uint64_t>(n_found, 65535)), dim3(64), 0, s, off, heads, max_inside + 2, (uint64_t)n_found, n_rows, c->col.rows,
                               c->col.presence, words, c->seg.ev[0], c->seg.ev[1], n_events, c->sbb.u32, c->sbb.u64, c->sbb.presence, c->sbb.member_off, c->sbb.members,
                               (uint64_t)n_members, flags);
        ok = ok && hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->sbb.peak_bytes = need - rows_bound + u32_bytes + u64_bytes + presence_bytes + moff_bytes + members_bytes;
    }
    if (int rc = stage_wait(c, "superbubbles", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment superbubbles: a reported entrance was not found again by the second walk"));
    c->sbb.n_rows = n_found; c->sbb.n_sides = n_sides; c->sbb.n_members = n_members; c->sbb.n_arcs = n_arcs; c->sbb.unmirrored = unmirrored;
    c->sbb.words = words; c->sbb.max_inside = max_inside;
    c->sbb.valid = true;
    return 0;
}

int tpc_segments_superbubbles_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    if (!info) return fail(c, -1, "segment superbubbles: info required");
    info[0] = c->sbb.n_rows; info[1] = c->sbb.n_sides; info[2] = c->sbb.n_members; info[3] = c->sbb.unmirrored; info[4] = c->sbb.peak_bytes; info[5] = c->sbb.n_arcs;
    info[6] = c->sbb.max_inside;
    return 0;
}

int tpc_segments_superbubbles_fetch_adjacency(tpc_ctx *c, uint32_t *offsets_host, uint32_t *heads_host)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    if (!offsets_host || (c->sbb.n_arcs && !heads_host)) return fail(c, -1, "segment superbubbles: the offset and head arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(offsets_host, c->sbb.off, (c->sbb.n_sides + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (c->sbb.n_arcs) HIPCHK(c, hipMemcpy(heads_host, c->sbb.heads, c->sbb.n_arcs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_superbubbles_fetch_exits(tpc_ctx *c, uint64_t c0, uint64_t n, uint32_t *exit_host)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    return fetch_planes(c, "superbubbles", "side", c->sbb.exit_of, c->sbb.n_sides, c0, n, { exit_host });
}

int tpc_segments_superbubbles_fetch_rows(tpc_ctx *c, uint64_t b0, uint64_t n, uint32_t *entrance_host, uint32_t *exit_host, uint32_t *inside_host, uint32_t *arcs_host,
                                         uint32_t *n_colors_host, uint64_t *paths_host, uint64_t *min_edges_host, uint64_t *max_edges_host)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    uint64_t *const wide[SB_U64_PLANES] = { paths_host, min_edges_host, max_edges_host };
    bool missing = false;
    for (uint64_t *d : wide) missing = missing || !d;
    if (int rc = sb_fetch_check(c, "row", c->sbb.n_rows, b0, n, missing)) return rc;
    if (int rc = fetch_planes(c, "superbubbles", "row", c->sbb.u32, c->sbb.n_rows, b0, n, { entrance_host, exit_host, inside_host, arcs_host, n_colors_host })) return rc;
    for (int i = 0; i < SB_U64_PLANES && n; i++)
        HIPCHK(c, hipMemcpy(wide[i], c->sbb.u64 + (uint64_t)i * c->sbb.n_rows + b0, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_superbubbles_fetch_members(tpc_ctx *c, uint32_t *offsets_host, uint32_t *sides_host)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    if (!offsets_host || (c->sbb.n_members && !sides_host)) return fail(c, -1, "segment superbubbles: the offset and side arrays are required");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(offsets_host, c->sbb.member_off, (c->sbb.n_rows + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (c->sbb.n_members) HIPCHK(c, hipMemcpy(sides_host, c->sbb.members, c->sbb.n_members * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_superbubbles_fetch_presence(tpc_ctx *c, uint64_t b0, uint64_t n, uint32_t *words_host)
{
    if (!c) return -1;
    if (int rc = sb_needs(c)) return rc;
    if (int rc = sb_fetch_check(c, "row", c->sbb.n_rows, b0, n, !words_host)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(words_host, c->sbb.presence + b0 * c->sbb.words, n * c->sbb.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
