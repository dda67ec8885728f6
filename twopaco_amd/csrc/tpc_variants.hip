// tpc_variants.hip -- the VARIANTS: every input sequence walked through every superbubble, the walks grouped into alleles.  Kernels and
// the C-ABI of the tpc_segments_variants_* group of include/twopaco_hip.h, which defines walk, traversal, allele, site and reference.
// No counterpart in the reference; host/graphformat.h: ComputeVariants is the serial statement.
//
// Input: the event table of the last tpc_segments_build_* (name, first bits, begin, end, the sequences' event ranges), the rows and
// member lists of the last tpc_segments_superbubbles_build, the colour count of the last tpc_segments_colors_build and the caller's
// colour of every sequence.
//   SegRows              the row of every first event (tpc_segrows.h)
//   k_var_sides          side_of[e] for every event (link_side)
//   k_var_entrances      row_of_entrance[entrance[b]] = b, one thread per superbubble row (a side is the entrance of at most one row)
//   k_var_walk           one thread per SLOT 2 e + d: the row whose entrance is side_of[e] ^ d, the sequence of e by a binary search
//                        over the sequences' event ranges, then at most max_inside + 1 steps inside that range; every side read is the
//                        exit (the walk is a traversal) or is looked up in the row's ascending members by a binary search of at most
//                        6 steps (its bit of the mask) or is a stray.  Writes flag, row, last and mask of the slot.  Every loop is
//                        counted.
//   scan                 an exclusive scan over the slots' flags numbers the traversals in the order (e, d); its total is the first wait
//   k_var_compact        a flagged slot writes start, last, d, row, edges and mask of its traversal
//   two sorts            rocprim::radix_sort_pairs of the traversal indices by mask, then by row: radix sorts are stable, so the order is
//                        (row, mask, traversal) and the first of every run of one (row, mask) is the allele's smallest traversal
//   k_var_heads + scan   the runs' heads, numbered: the GROUPS, in the order (row, mask); the total is the second wait
//   k_var_groups + sort  key (row << 32 | first) and the run's first position per group, sorted: the alleles in the order (row, first)
//   k_var_alleles        one thread per allele: row, mask, sides, edges, first, traversals = the run's length (no atomics: the hot
//                        allele of a site that nearly every genome walks is one subtraction), the allele of its group, and the
//                        per-site counts by atomicAdd (one per allele)
//   scan                 the alleles' offset of every superbubble row
//   k_var_presence       one thread per traversal in sorted order: its allele, the colour of its sequence, the presence bit by
//                        atomicOr unless a read shows it set (the lanes of a hot allele mostly find it set), allele_of[traversal], and
//                        for the reference colour atomicMin of the traversal and atomicAdd of the count per site
//   k_var_sites          one thread per superbubble row: ref_allele from the smallest reference traversal, the sites, the largest
//                        number of alleles (the third wait sizes the histogram); k_var_ncolors, k_var_hist
// Integers, minima, ORs and commutative sums: the result is exact and does not depend on the schedule.
// Memory: kept until the next segment, colour, link, superbubble or variant build 28 B per traversal, 36 B + 4 W B per allele, 24 B per
// superbubble row and the histogram; during the call 44 B per event (the sides and, per slot, flag, row, last and mask), 4 B per side,
// 28 B per traversal, 24 B per group, the row index and the scans' and sorts' scratch.  None of it exists in a context that never asks
// for variants.  What does not fit the free device memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint32_t VAR_NONE = 0xFFFFFFFFu;
constexpr int VAR_TRV_PLANES = 5;   // start, last, d, row, edges
constexpr int VAR_ALL_PLANES = 5;   // row, sides, edges, first, n_colors
// scalars (uint64 each)
constexpr int VAR_BAD = 0, VAR_STRAYS = 1, VAR_SITES = 2, VAR_MOST = 3, VAR_SCALARS = 8;

__global__ void k_var_sides(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank,
                            uint64_t n_rows, uint32_t *__restrict__ side_of)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) side_of[e] = link_side(name, e, n_events, table, n_table, rank, n_rows);
}

__global__ void k_var_entrances(const uint32_t *__restrict__ entrance, uint64_t n_sbb, uint64_t n_sides, uint32_t *__restrict__ row_of_entrance, unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_sbb; b += stride) {
        const uint32_t s = entrance[b];
        if (s >= n_sides || atomicMin(&row_of_entrance[s], (uint32_t)b) != VAR_NONE) atomicOr(&scalars[VAR_BAD], 1ull);   // outside the sides, or the entrance of two rows
    }
}

// flag: 2 n_events + 1 entries, the last one 0.  sbb: [5][n_sbb] entrance, exit, inside, .. of the superbubble stage.
__global__ void k_var_walk(const uint32_t *__restrict__ side_of, uint64_t n_events, const uint32_t *__restrict__ seq_begin, uint32_t n_rec, const uint32_t *__restrict__ row_of_entrance,
                           uint64_t n_sides, const uint32_t *__restrict__ sbb, uint64_t n_sbb, const uint32_t *__restrict__ member_off, const uint32_t *__restrict__ members,
                           uint64_t n_members, uint32_t max_inside, uint32_t *__restrict__ flag, uint32_t *__restrict__ slot_row, uint32_t *__restrict__ slot_last,
                           unsigned long long *__restrict__ slot_mask, unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_slots = 2 * n_events;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_slots; i += stride) {
        uint32_t f = 0;
        if (i < n_slots) {
            const uint64_t e = i >> 1;
            const uint32_t d = (uint32_t)(i & 1), own = side_of[e];
            const uint32_t b = own < n_sides ? row_of_entrance[own ^ d] : VAR_NONE;
            if (own >= n_sides) atomicOr(&scalars[VAR_BAD], 2ull);
            else if (b < n_sbb) {
                const uint32_t at = col_seq_end(seq_begin, n_rec, (uint32_t)e);
                const uint32_t m0 = member_off[b], m1 = member_off[b + 1], exit = sbb[n_sbb + b];
                if (at < 1 || at > n_rec || m1 < m0 || m1 > n_members || m1 - m0 > 64) atomicOr(&scalars[VAR_BAD], 4ull);
                else {
                    const uint64_t lowest = seq_begin[at - 1], beyond = std::min<uint64_t>(seq_begin[at], n_events);
                    unsigned long long mask = 0;
                    uint64_t x = e;
                    bool reached = false;
                    for (uint32_t step = 0; step <= max_inside; step++) {
                        if (d ? x <= lowest : x + 1 >= beyond) break;   // the sequence ends inside the superbubble
                        x = d ? x - 1 : x + 1;
                        const uint32_t read = side_of[x] ^ d;
                        if (read == exit) { reached = true; break; }
                        // the member's index: a binary search over at most 64 ascending sides
                        uint32_t lo = m0, hi = m1;
                        for (int turn = 0; turn < 7 && lo < hi; turn++) { const uint32_t mid = lo + ((hi - lo) >> 1); if (members[mid] < read) lo = mid + 1; else hi = mid; }
                        if (lo >= m1 || members[lo] != read) { atomicAdd(&scalars[VAR_STRAYS], 1ull); break; }
                        mask |= 1ull << (lo - m0);
                    }
                    if (reached) {
                        f = 1;
                        slot_row[i] = b; slot_last[i] = (uint32_t)x; slot_mask[i] = mask;
                    }
                }
            }
        }
        flag[i] = f;
    }
}

// id: the exclusive scan of the flags.  trv: [5][n_trav] start, last, d, row, edges.
__global__ void k_var_compact(const uint32_t *__restrict__ id, const uint32_t *__restrict__ slot_row, const uint32_t *__restrict__ slot_last, const unsigned long long *__restrict__ slot_mask,
                              uint64_t n_events, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint32_t *__restrict__ trv, unsigned long long *__restrict__ trv_mask,
                              uint32_t *__restrict__ order, uint64_t n_trav)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n_slots = 2 * n_events;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const uint32_t t = id[i];
        if (id[i + 1] == t || t >= n_trav) continue;   // not flagged
        const uint32_t start = (uint32_t)(i >> 1), last = slot_last[i];
        const uint32_t lo = std::min(start, last), hi = std::max(start, last);
        const uint32_t from = end[lo], to = begin[hi];
        trv[t] = start; trv[n_trav + t] = last; trv[2 * n_trav + t] = (uint32_t)(i & 1); trv[3 * n_trav + t] = slot_row[i]; trv[4 * n_trav + t] = to >= from ? to - from : from - to;
        trv_mask[t] = slot_mask[i];
        order[t] = t;
    }
}

__global__ void k_var_gather(const uint32_t *__restrict__ order, const uint32_t *__restrict__ row, uint64_t n_trav, uint32_t *__restrict__ key)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_trav; i += stride) key[i] = order[i] < n_trav ? row[order[i]] : VAR_NONE;
}

// head: n_trav + 1 entries, the last one 0
__global__ void k_var_heads(const uint32_t *__restrict__ order, const uint32_t *__restrict__ row, const unsigned long long *__restrict__ mask, uint64_t n_trav, uint32_t *__restrict__ head,
                            unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_trav; i += stride) {
        uint32_t h = 0;
        if (i < n_trav) {
            const uint32_t t = order[i], below = i ? order[i - 1] : 0;
            if (t >= n_trav || below >= n_trav) atomicOr(&scalars[VAR_BAD], 8ull);
            else h = i == 0 || row[t] != row[below] || mask[t] != mask[below];
        }
        head[i] = h;
    }
}

// gid: the exclusive scan of the heads, n_trav + 1 entries: position i lies in group gid[i + 1] - 1 and is its head when gid[i + 1] != gid[i]
__global__ void k_var_groups(const uint32_t *__restrict__ gid, const uint32_t *__restrict__ order, const uint32_t *__restrict__ row, uint64_t n_trav, uint64_t n_groups,
                             unsigned long long *__restrict__ key, uint32_t *__restrict__ val, uint32_t *__restrict__ pos)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_trav; i += stride) {
        if (i == n_trav) { pos[n_groups] = (uint32_t)n_trav; continue; }
        const uint32_t g = gid[i];
        if (gid[i + 1] == g || g >= n_groups) continue;
        const uint32_t t = order[i];
        key[g] = (unsigned long long)row[t] << 32 | t;
        val[g] = g;
        pos[g] = (uint32_t)i;
    }
}

// all: [5][n_all] row, sides, edges, first, n_colors; all64: [2][n_all] mask, traversals.  count: [n_sbb + 1] the alleles of every row;
// site64: [2][n_sbb] traversals, ref_traversals.
__global__ void k_var_alleles(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ pos, uint64_t n_all,
                              const uint32_t *__restrict__ trv, const unsigned long long *__restrict__ trv_mask, uint64_t n_trav, uint64_t n_sbb, uint32_t *__restrict__ all,
                              unsigned long long *__restrict__ all64, uint32_t *__restrict__ allele_of_group, uint32_t *__restrict__ count, unsigned long long *__restrict__ site64,
                              unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n_all; a += stride) {
        const uint32_t g = val[a], first = (uint32_t)key[a], row = (uint32_t)(key[a] >> 32);
        if (g >= n_all || first >= n_trav || row >= n_sbb || pos[g + 1] < pos[g]) { atomicOr(&scalars[VAR_BAD], 16ull); continue; }
        const unsigned long long mask = trv_mask[first], n = (unsigned long long)pos[g + 1] - pos[g];
        all[a] = row; all[n_all + a] = (uint32_t)__popcll(mask); all[2 * n_all + a] = trv[4 * n_trav + first]; all[3 * n_all + a] = first; all[4 * n_all + a] = 0;
        all64[a] = mask; all64[n_all + a] = n;
        allele_of_group[g] = (uint32_t)a;
        atomicAdd(&count[row], 1u);
        atomicAdd(&site64[row], n);
    }
}

__global__ void k_var_presence(const uint32_t *__restrict__ gid, const uint32_t *__restrict__ order, const uint32_t *__restrict__ allele_of_group, uint64_t n_all,
                               const uint32_t *__restrict__ trv, uint64_t n_trav, uint64_t n_events, const uint32_t *__restrict__ seq_begin, uint32_t n_rec,
                               const uint32_t *__restrict__ color, uint32_t n_colors, uint32_t words, uint32_t ref, uint64_t n_sbb, uint32_t *__restrict__ presence,
                               uint32_t *__restrict__ allele_of, uint32_t *__restrict__ ref_first, unsigned long long *__restrict__ site64, unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_trav; i += stride) {
        const uint32_t g = gid[i + 1] - 1u, t = order[i];
        const uint32_t a = g < n_all ? allele_of_group[g] : VAR_NONE;
        const uint32_t start = t < n_trav ? trv[t] : VAR_NONE, row = t < n_trav ? trv[3 * n_trav + t] : VAR_NONE;
        const uint32_t at = start < n_events ? col_seq_end(seq_begin, n_rec, start) : 0;
        const uint32_t col = at >= 1 && at <= n_rec ? color[at - 1] : VAR_NONE;
        if (a >= n_all || row >= n_sbb || col >= n_colors) { atomicOr(&scalars[VAR_BAD], 32ull); continue; }
        allele_of[t] = a;
        uint32_t *word = &presence[(uint64_t)a * words + (col >> 5)];
        const uint32_t bit = 1u << (col & 31);
        if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
        if (col == ref) {
            atomicMin(&ref_first[row], t);
            atomicAdd(&site64[n_sbb + row], 1ull);
        }
    }
}

__global__ void k_var_ncolors(const uint32_t *__restrict__ presence, uint32_t words, uint64_t n_all, uint32_t *__restrict__ n_colors)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n_all; a += stride) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < words; w++) n += (uint32_t)__popc(presence[a * words + w]);
        n_colors[a] = n;
    }
}

// off: the exclusive scan of the counts, n_sbb + 1 entries.  ref_first becomes ref_allele in place.
__global__ void k_var_sites(const uint32_t *__restrict__ off, uint64_t n_sbb, const uint32_t *__restrict__ allele_of, uint64_t n_trav, uint32_t *__restrict__ ref_first,
                            unsigned long long *__restrict__ scalars)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_sbb; b += stride) {
        const uint32_t t = ref_first[b], n = off[b + 1] - off[b];
        if (t != VAR_NONE) ref_first[b] = t < n_trav ? allele_of[t] : VAR_NONE;
        if (n) { atomicAdd(&scalars[VAR_SITES], 1ull); atomicMax(&scalars[VAR_MOST], (unsigned long long)n); }
    }
}

__global__ void k_var_hist(const uint32_t *__restrict__ off, uint64_t n_sbb, unsigned long long *__restrict__ hist, uint64_t bins)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_sbb; b += stride) {
        const uint32_t n = off[b + 1] - off[b];
        if (n && n < bins) atomicAdd(&hist[n], 1ull);
    }
}

int var_needs(tpc_ctx *c)
{
    if (!c->var.valid) return fail(c, -1, "segment variants: tpc_segments_variants_build first");
    return 0;
}

uint32_t var_bits(uint64_t v) { uint32_t b = 0; while (v) { b++; v >>= 1; } return b; }

// the test option holds for one build: whichever way it returns, the next one runs on its own
struct VarOptions {
    tpc_ctx *c;
    int grid;
    explicit VarOptions(tpc_ctx *c_) : c(c_), grid(c_->opt_variants_grid) {}
    ~VarOptions() { c->opt_variants_grid = 0; }
};

}  // namespace

extern "C" {

int tpc_segments_variants_build(tpc_ctx *c, const uint32_t *color_of_seq, uint32_t n_colors, uint32_t ref_color)
{
    if (!c) return -1;
    variants_drop(c);
    const VarOptions opt(c);
    if (int rc = stage_needs_segments(c, "variants", "walk")) return rc;
    if (!c->col.valid) return fail(c, -1, "segment variants: build the colour table first (tpc_segments_colors_build)");
    if (!c->lnk.valid) return fail(c, -1, "segment variants: build the link table first (tpc_segments_links_build)");
    if (!c->sbb.valid) return fail(c, -1, "segment variants: build the superbubble table first (tpc_segments_superbubbles_build)");
    if (n_colors == 0) return fail(c, -1, "segment variants: at least one colour is required");
    if (c->col.n_colors != n_colors) return fail(c, -1, "segment variants: the colour table holds %u colours, the caller gives %u", c->col.n_colors, n_colors);
    if (ref_color != VAR_NONE && ref_color >= n_colors) return fail(c, -1, "segment variants: the reference colour is %u, there are %u colours", ref_color, n_colors);
    const uint32_t n_rec = c->seg.n_rec;
    if (n_rec && !color_of_seq) return fail(c, -1, "segment variants: the colour of every one of the %u sequences is required", n_rec);
    for (uint32_t s = 0; s < n_rec; s++)
        if (color_of_seq[s] >= n_colors) return fail(c, -1, "segment variants: sequence %u has colour %u, there are %u colours", s, color_of_seq[s], n_colors);
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments, n_sbb = c->sbb.n_rows, n_sides = c->sbb.n_sides, n_slots = 2 * n_events;
    if (n_events >= VAR_NONE) return fail(c, -1, "segment variants: %llu events, a traversal holds events below %u", (unsigned long long)n_events, VAR_NONE);
    if (n_slots >= VAR_NONE) return fail(c, -1, "segment variants: %llu walks of %llu events, a traversal is numbered below %u", (unsigned long long)n_slots, (unsigned long long)n_events, VAR_NONE);
    if (n_sides != 2 * n_rows || n_sbb >= VAR_NONE) return fail(c, -10, "segment variants: the superbubble table holds %llu sides, the build counted %llu segments", (unsigned long long)n_sides, (unsigned long long)n_rows);
    HIPCHK(c, hipSetDevice(c->device));
    // the table's own consistency: every event belongs to one of the n_rec sequences
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != n_events) return fail(c, -1, "segment variants: the stream holds events of more sequences than the %u given", n_rec);
    const uint32_t words = (n_colors + 31) / 32, max_inside = c->sbb.max_inside;
    auto grid = [&](uint64_t n) { return dim3(opt.grid > 0 ? std::min<unsigned>(col_grid(n), (unsigned)opt.grid) : col_grid(n)); };

    // sizes in 64 bits, summed before the first allocation; the traversals are not counted yet: at most one per slot
    const uint64_t side_bytes = n_events * 4 + 16, slot4 = (n_slots + 1) * 4 + 16, slot8 = n_slots * 8 + 16, ent_bytes = n_sides * 4 + 16, color_bytes = (uint64_t)n_rec * 4 + 16;
    const uint64_t site_bytes = (n_sbb + 1) * 4 + 16, site64_bytes = 2 * n_sbb * 8 + 16;
    SegRows idx;
    size_t slot_scan = 0;
    uint32_t *flag = nullptr;
    if (!idx.size(c) || rocprim::exclusive_scan(nullptr, slot_scan, flag, flag, 0u, n_slots + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess)
        return fail(c, -10, "segment variants: the scans could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, slot_scan);
    const uint64_t walk_need = side_bytes + 3 * slot4 + slot8 + ent_bytes + color_bytes + 2 * site_bytes + site64_bytes + idx.bytes() + 64;
    if (int rc = stage_fits(c, "variants", walk_need, "%llu of them the sides of %llu events and the flag, row, last event and mask of two walks each", (unsigned long long)(side_bytes + 3 * slot4 + slot8),
                            (unsigned long long)n_events))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) variants_drop(c);
        return code;
    };
    auto no_memory = [&]() { return done(fail(c, -10, "segment variants: hipMalloc failed: %s", hipGetErrorString(hipGetLastError()))); };
    uint32_t *side_of = nullptr, *slot_row = nullptr, *slot_last = nullptr, *row_of_entrance = nullptr, *color = nullptr;
    unsigned long long *slot_mask = nullptr, *scalars = nullptr;
    if (dev_malloc(c, (void **)&c->var.site_off, site_bytes) != hipSuccess || dev_malloc(c, (void **)&c->var.ref_allele, site_bytes) != hipSuccess ||
        dev_malloc(c, (void **)&c->var.site64, site64_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &side_of, side_bytes) || !temps.get(c, &flag, slot4) ||
        !temps.get(c, &slot_row, slot4) || !temps.get(c, &slot_last, slot4) || !temps.get(c, &slot_mask, slot8) || !temps.get(c, &row_of_entrance, ent_bytes) ||
        !temps.get(c, &color, color_bytes) || !temps.get(c, &scalars, VAR_SCALARS * 8))
        return no_memory();
    hipStream_t s = c->stream;
    const uint32_t *sbb = c->sbb.u32;
    bool ok = hipMemsetAsync(scalars, 0, VAR_SCALARS * 8, s) == hipSuccess && hipMemsetAsync(row_of_entrance, 0xFF, ent_bytes, s) == hipSuccess &&
              hipMemsetAsync(c->var.site_off, 0, site_bytes, s) == hipSuccess && hipMemsetAsync(c->var.ref_allele, 0xFF, site_bytes, s) == hipSuccess &&
              hipMemsetAsync(c->var.site64, 0, site64_bytes, s) == hipSuccess && idx.fill(s) &&
              (!n_rec || hipMemcpyAsync(color, color_of_seq, (size_t)n_rec * 4, hipMemcpyHostToDevice, s) == hipSuccess);
    uint32_t n_trav = 0, n_all = 0;
    unsigned long long host_scalars[VAR_SCALARS] = {0};
    uint64_t peak = walk_need;
    if (ok) {
        Timed t(c, TPC_K_VARIANTS);   // the whole stage on the stream, its waits for the counts included (as TPC_K_TRACKS)
        ok = idx.enqueue(c) && idx.total(s);
        if (ok && n_events) hipLaunchKernelGGL(k_var_sides, grid(n_events), dim3(256), 0, s, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, side_of);
        if (ok && n_sbb) hipLaunchKernelGGL(k_var_entrances, grid(n_sbb), dim3(256), 0, s, sbb, n_sbb, n_sides, row_of_entrance, scalars);
        if (ok) {
            hipLaunchKernelGGL(k_var_walk, grid(n_slots + 1), dim3(256), 0, s, side_of, n_events, c->seg.ev[2], n_rec, row_of_entrance, n_sides, sbb, n_sbb, c->sbb.member_off,
                               c->sbb.members, c->sbb.n_members, max_inside, flag, slot_row, slot_last, slot_mask, scalars);
            ok = rocprim::exclusive_scan(idx.scan_tmp, slot_scan, flag, flag, 0u, n_slots + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the number of traversals decides the size of what is kept: the first wait
        ok = ok && hipMemcpyAsync(&n_trav, flag + n_slots, sizeof n_trav, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(host_scalars, scalars, sizeof host_scalars, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "variants", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment variants: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (host_scalars[VAR_BAD]) return done(fail(c, -10, "segment variants: the tables disagree about the sides, the sequences or the members (%llu)", host_scalars[VAR_BAD]));
        if (n_trav > n_slots) return done(fail(c, -10, "segment variants: %u traversals over %llu events", n_trav, (unsigned long long)n_events));

        // the traversals, and their order by (row, mask)
        const uint64_t T = n_trav, trv_bytes = T * 4 * VAR_TRV_PLANES + 16, t4 = (T + 1) * 4 + 16, t8 = T * 8 + 16;
        const uint32_t mask_bits = std::max(1u, std::min(64u, max_inside)), row_bits = std::max(1u, var_bits(n_sbb));
        unsigned long long *mask_sorted = nullptr;
        uint32_t *order = nullptr, *order2 = nullptr, *key = nullptr, *key2 = nullptr, *gid = nullptr, *allele_of = nullptr;
        size_t sort_a = 0, sort_b = 0, t_scan = 0;
        if (rocprim::radix_sort_pairs(nullptr, sort_a, slot_mask, mask_sorted, order, order2, T, 0, mask_bits, s) != hipSuccess ||
            rocprim::radix_sort_pairs(nullptr, sort_b, key, key2, order2, order, T, 0, row_bits, s) != hipSuccess ||
            rocprim::exclusive_scan(nullptr, t_scan, gid, gid, 0u, T + 1, rocprim::plus<uint32_t>(), s) != hipSuccess)
            return done(fail(c, -10, "segment variants: the sorts could not be sized"));
        const uint64_t sort_bytes = std::max<uint64_t>(std::max(sort_a, sort_b), t_scan) + 16;
        const uint64_t group_need = trv_bytes + 2 * t8 + 6 * t4 + sort_bytes;
        if (int rc = stage_fits(c, "variants", group_need, "%llu traversals, their order by row and mask", (unsigned long long)T)) return done(rc);
        void *sort_tmp = nullptr;
        if (dev_malloc(c, (void **)&c->var.trv, trv_bytes) != hipSuccess || dev_malloc(c, (void **)&c->var.trv_mask, t8) != hipSuccess || !temps.get(c, &mask_sorted, t8) ||
            !temps.get(c, &order, t4) || !temps.get(c, &order2, t4) || !temps.get(c, &key, t4) || !temps.get(c, &key2, t4) || !temps.get(c, &gid, t4) || !temps.get(c, &allele_of, t4) ||
            !temps.get(c, &sort_tmp, sort_bytes))
            return no_memory();
        peak = std::max(peak, walk_need + group_need);
        uint32_t *trv = c->var.trv;
        unsigned long long *trv_mask = c->var.trv_mask;
        ok = true;
        if (T) {
            hipLaunchKernelGGL(k_var_compact, grid(n_slots), dim3(256), 0, s, flag, slot_row, slot_last, slot_mask, n_events, c->seg.ev[0], c->seg.ev[1], trv, trv_mask, order, T);
            ok = rocprim::radix_sort_pairs(sort_tmp, sort_a, trv_mask, mask_sorted, order, order2, T, 0, mask_bits, s) == hipSuccess;
            if (ok) {
                hipLaunchKernelGGL(k_var_gather, grid(T), dim3(256), 0, s, order2, trv + 3 * T, T, key);
                ok = rocprim::radix_sort_pairs(sort_tmp, sort_b, key, key2, order2, order, T, 0, row_bits, s) == hipSuccess;
            }
        }
        if (ok) {
            hipLaunchKernelGGL(k_var_heads, grid(T + 1), dim3(256), 0, s, order, trv + 3 * T, trv_mask, T, gid, scalars);
            ok = rocprim::exclusive_scan(sort_tmp, t_scan, gid, gid, 0u, T + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        // the number of alleles: the second wait
        ok = ok && hipMemcpyAsync(&n_all, gid + T, sizeof n_all, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(host_scalars, scalars, sizeof host_scalars, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "variants", ok)) return done(rc);
        if (host_scalars[VAR_BAD] || n_all > T) return done(fail(c, -10, "segment variants: the sorted traversals lie outside the table (%llu)", host_scalars[VAR_BAD]));

        // the alleles in the order (row, first)
        const uint64_t A = n_all, all_bytes = A * 4 * VAR_ALL_PLANES + 16, a4 = (A + 1) * 4 + 16, a8 = A * 8 + 16, all64_bytes = 2 * A * 8 + 16, pres_bytes = A * words * 4 + 16;
        unsigned long long *gkey = nullptr, *gkey2 = nullptr;
        uint32_t *gval = nullptr, *gval2 = nullptr, *gpos = nullptr, *allele_of_group = nullptr;
        size_t sort_c = 0, site_scan = 0;
        if (rocprim::radix_sort_pairs(nullptr, sort_c, gkey, gkey2, gval, gval2, A, 0, 64, s) != hipSuccess ||
            rocprim::exclusive_scan(nullptr, site_scan, gval, gval, 0u, n_sbb + 1, rocprim::plus<uint32_t>(), s) != hipSuccess)
            return done(fail(c, -10, "segment variants: the sorts could not be sized"));
        const uint64_t tmp_c = std::max<uint64_t>(sort_c, site_scan) + 16;
        const uint64_t allele_need = all_bytes + all64_bytes + pres_bytes + 2 * a8 + 4 * a4 + tmp_c;
        if (int rc = stage_fits(c, "variants", allele_need, "%llu alleles of %u presence words", (unsigned long long)A, words)) return done(rc);
        void *tmp3 = nullptr;
        if (dev_malloc(c, (void **)&c->var.all, all_bytes) != hipSuccess || dev_malloc(c, (void **)&c->var.all64, all64_bytes) != hipSuccess ||
            dev_malloc(c, (void **)&c->var.presence, pres_bytes) != hipSuccess || !temps.get(c, &gkey, a8) || !temps.get(c, &gkey2, a8) || !temps.get(c, &gval, a4) ||
            !temps.get(c, &gval2, a4) || !temps.get(c, &gpos, a4) || !temps.get(c, &allele_of_group, a4) || !temps.get(c, &tmp3, tmp_c))
            return no_memory();
        peak = std::max(peak, walk_need + group_need + allele_need);
        ok = hipMemsetAsync(c->var.presence, 0, pres_bytes, s) == hipSuccess;
        if (ok && A) {
            hipLaunchKernelGGL(k_var_groups, grid(T + 1), dim3(256), 0, s, gid, order, trv + 3 * T, T, A, gkey, gval, gpos);
            ok = rocprim::radix_sort_pairs(tmp3, sort_c, gkey, gkey2, gval, gval2, A, 0, 64, s) == hipSuccess;
            if (ok)
                hipLaunchKernelGGL(k_var_alleles, grid(A), dim3(256), 0, s, gkey2, gval2, gpos, A, trv, trv_mask, T, n_sbb, c->var.all, c->var.all64, allele_of_group, c->var.site_off,
                                   c->var.site64, scalars);
        }
        ok = ok && rocprim::exclusive_scan(tmp3, site_scan, c->var.site_off, c->var.site_off, 0u, n_sbb + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        if (ok && A) {
            hipLaunchKernelGGL(k_var_presence, grid(T), dim3(256), 0, s, gid, order, allele_of_group, A, trv, T, n_events, c->seg.ev[2], n_rec, color, n_colors, words, ref_color, n_sbb,
                               c->var.presence, allele_of, c->var.ref_allele, c->var.site64, scalars);
            hipLaunchKernelGGL(k_var_ncolors, grid(A), dim3(256), 0, s, c->var.presence, words, A, c->var.all + 4 * A);
        }
        if (ok && n_sbb) hipLaunchKernelGGL(k_var_sites, grid(n_sbb), dim3(256), 0, s, c->var.site_off, n_sbb, allele_of, T, c->var.ref_allele, scalars);
        // the largest number of alleles at one site sizes the histogram: the third wait
        ok = ok && hipMemcpyAsync(host_scalars, scalars, sizeof host_scalars, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "variants", ok)) return done(rc);
        if (host_scalars[VAR_BAD]) return done(fail(c, -10, "segment variants: an allele lies outside the tables (%llu)", host_scalars[VAR_BAD]));
        const uint64_t bins = host_scalars[VAR_MOST] + 1, hist_bytes = bins * 8 + 16;
        if (bins > A + 1) return done(fail(c, -10, "segment variants: a site of %llu alleles among %llu", host_scalars[VAR_MOST], (unsigned long long)A));
        if (dev_malloc(c, (void **)&c->var.hist, hist_bytes) != hipSuccess) return no_memory();
        ok = hipMemsetAsync(c->var.hist, 0, hist_bytes, s) == hipSuccess;
        if (ok && n_sbb) hipLaunchKernelGGL(k_var_hist, grid(n_sbb), dim3(256), 0, s, c->var.site_off, n_sbb, c->var.hist, bins);
        c->var.hist_bins = bins;
        peak += hist_bytes;
    }
    if (int rc = stage_wait(c, "variants", ok)) return done(rc);
    c->var.n_trav = n_trav; c->var.n_all = n_all; c->var.n_sbb = n_sbb; c->var.sites = host_scalars[VAR_SITES]; c->var.strays = host_scalars[VAR_STRAYS];
    c->var.n_colors = n_colors; c->var.words = words; c->var.ref = ref_color; c->var.peak_bytes = peak;
    c->var.valid = true;
    return 0;
}

int tpc_segments_variants_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    if (!info) return fail(c, -1, "segment variants: info required");
    info[0] = c->var.sites; info[1] = c->var.n_all; info[2] = c->var.n_trav; info[3] = c->var.strays; info[4] = c->var.peak_bytes; info[5] = c->var.n_colors;
    info[6] = c->var.ref; info[7] = c->var.hist_bins; info[8] = c->var.n_sbb;
    return 0;
}

int tpc_segments_variants_fetch_traversals(tpc_ctx *c, uint64_t t0, uint64_t n, uint32_t *start, uint32_t *last, uint32_t *dir, uint32_t *row, uint32_t *edges, uint64_t *mask)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    if (int rc = fetch_planes(c, "variants", "traversal", c->var.trv, c->var.n_trav, t0, n, { start, last, dir, row, edges })) return rc;
    if (n && !mask) return fail(c, -1, "segment variants: the masks are required");
    if (n) HIPCHK(c, hipMemcpy(mask, c->var.trv_mask + t0, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_variants_fetch_alleles(tpc_ctx *c, uint64_t a0, uint64_t n, uint32_t *row, uint32_t *sides, uint32_t *edges, uint32_t *first, uint32_t *n_colors, uint64_t *mask,
                                        uint64_t *traversals)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    if (int rc = fetch_planes(c, "variants", "allele", c->var.all, c->var.n_all, a0, n, { row, sides, edges, first, n_colors })) return rc;
    if (n && (!mask || !traversals)) return fail(c, -1, "segment variants: the masks and the traversal counts are required");
    if (n) HIPCHK(c, hipMemcpy(mask, c->var.all64 + a0, n * 8, hipMemcpyDeviceToHost));
    if (n) HIPCHK(c, hipMemcpy(traversals, c->var.all64 + c->var.n_all + a0, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_variants_fetch_presence(tpc_ctx *c, uint64_t a0, uint64_t n, uint32_t *words_host)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    if ((n && !words_host) || a0 > c->var.n_all || n > c->var.n_all - a0)
        return fail(c, -1, "segment variants: bad allele range (%llu alleles at %llu of %llu)", (unsigned long long)n, (unsigned long long)a0, (unsigned long long)c->var.n_all);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(words_host, c->var.presence + a0 * c->var.words, n * c->var.words * 4, hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_variants_fetch_sites(tpc_ctx *c, uint64_t b0, uint64_t n, uint32_t *allele_offset, uint64_t *traversals, uint32_t *ref_allele, uint64_t *ref_traversals)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    const uint64_t rows = c->var.n_sbb;
    if (!allele_offset || (n && (!traversals || !ref_allele || !ref_traversals)) || b0 > rows || n > rows - b0)
        return fail(c, -1, "segment variants: bad site range (%llu sites at %llu of %llu)", (unsigned long long)n, (unsigned long long)b0, (unsigned long long)rows);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(allele_offset, c->var.site_off + b0, (n + 1) * 4, hipMemcpyDeviceToHost));
    if (n) {
        HIPCHK(c, hipMemcpy(traversals, c->var.site64 + b0, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ref_allele, c->var.ref_allele + b0, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(ref_traversals, c->var.site64 + rows + b0, n * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

int tpc_segments_variants_fetch_hist(tpc_ctx *c, uint64_t *sites_host)
{
    if (!c) return -1;
    if (int rc = var_needs(c)) return rc;
    if (!sites_host) return fail(c, -1, "segment variants: the histogram is required");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(sites_host, c->var.hist, c->var.hist_bins * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
