// tpc_classes.hip -- the COLOUR CLASSES of the compacted graph: the distinct sets of colours that segments have, which segments have
// each, and what every class holds.  Kernels and the C-ABI of the tpc_segments_classes_* group of include/twopaco_hip.h, which defines
// row, class, first, class id and the per-class sums.  No counterpart in the reference; host/graphformat.h: ComputeClasses is the serial
// statement.
//
// Input: the colour table of the last tpc_segments_colors_build (rows: first event, occurrences; presence[S][W]) and begin / end of the
// event table under it.  The work is grouping S rows by a key of W words: an open-addressed SET OF ROWS with a power-of-two number of
// slots, at least 2 S.  A slot that is claimed holds a row of its class, and every row it ever holds has the same words, so any of them
// serves for the comparison; the words decide, the hash only finds the home slot.
//   k_cls_insert_thread  W <= 8: one thread per row.  The row's words are hashed to 64 bits (a sum of mixed words, so that the wave form
//                        adds up the same value), the row probes from its home slot: an empty slot is claimed with a compare-and-swap,
//                        an occupied one is decided by comparing the words, a slot of another class is stepped over (counted: info[3]).
//                        W <= 2 (KEYED): the one or two words are the key, the slots hold the keys themselves (0 = empty, no row is
//                        without a colour) and smallest[slot] the class's smallest row: no second read of any row.  W > 2: the slots
//                        hold rows, and a later row of the class lowers the slot with atomicMin, so the slot IS the smallest row; all
//                        ones is empty.  Every row remembers its slot.  EVERY PROBE LOOP IS COUNTED and ends within `slots` steps; a
//                        row that found neither its class nor an empty slot raises a flag and the build returns an error text.
//                        HOT KEY: the core class holds nearly every row.  Lanes compare their words with the row below, the lanes that
//                        differ lead a run (ballot), only a leader probes, its followers take its slot by shuffle; the leader's row is
//                        the run's smallest, and it issues atomicMin only after a plain read showed a larger row there.
//   k_cls_insert_wave    W > 8: one wave per row, lane j holds words j, j + 64, ..; the hash is summed and the comparison voted across
//                        the wave, lane 0 issues the atomics.
//   k_cls_flags          flag[r] = r is the smallest row of its slot; one exclusive scan over the flags gives the class ids, already
//   scan, k_cls_number   ascending by first; class[r] = id[smallest row of r's slot].  The total is the number of classes P.
//   k_cls_rows           one thread per row: first[p] at the first row; segments, length, edges and occurrences of the row into the sums
//                        of p = class[r], runs of one class in neighbouring lanes summed by a segmented scan over the wave and added
//                        once by the run's leader, as tpc_components.hip folds its sums.
//   k_cls_presence       presence[p] = the words of row first[p]
//   k_cls_sets           one thread per class: n = popcount of its words; classes, segments and edges of [n] (bins in LDS while C + 1 <=
//                        1024 of them fit, flushed once per block), and the largest segments[p], test first, then atomicMax
// Integers, commutative sums and a smallest row: the result is exact and depends neither on the schedule nor on the hash.
// Memory: kept until the next segment, colour or class build 4 B / row (class), per class 4 B (first), 32 B of sums and 4 W B of
// presence, and 24 B x (C + 1) of sets; during the call 4 B / row of slots remembered, 4 B / row of flags, 4 B per slot (12 B while
// W <= 2) and the scan's scratch.  None of it exists in a context that never asks for classes.  What does not fit the free device
// memory is refused with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint64_t CLS_MAX_ROWS = ((uint64_t)1 << 31) - 1;   // a row, a slot and a class id are 32 bits each, all ones is none
constexpr uint32_t CLS_NONE = 0xFFFFFFFFu;
constexpr uint32_t CLS_THREAD_WORDS = 8;                      // up to here one thread reads a row, beyond one wave does
constexpr uint32_t CLS_FLAG_GAVE_UP = 1u, CLS_FLAG_ROW = 2u;
constexpr int CLS_SUMS = 4;                                   // planes of sums: segments, length, edges, occurrences
constexpr uint32_t CLS_LDS_BINS = 1024;                       // bins of the sets a block keeps in LDS: 3 x 8 B x 1024 = 24 KiB

__device__ __forceinline__ uint32_t cls_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ unsigned long long cls_mix(unsigned long long x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// what word w of a row adds to the row's hash: a sum over the words, whoever adds them up
__device__ __forceinline__ unsigned long long cls_word(uint32_t w, uint32_t bits) { return cls_mix(((unsigned long long)(w + 1) << 32) | bits); }

__device__ __forceinline__ unsigned long long cls_wave_sum(unsigned long long v)
{
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// KEYED: the slot of `key` (never 0), claimed if need be; CLS_NONE after `slots` steps.  met: the slots of other classes stepped over.
__device__ __forceinline__ uint32_t cls_place_key(unsigned long long key, unsigned long long *key_of, uint64_t slots, unsigned long long home, unsigned long long &met)
{
    uint64_t at = home & (slots - 1);
    for (uint64_t probes = 0; probes < slots; probes++) {
        unsigned long long seen = __hip_atomic_load(&key_of[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == 0) seen = atomicCAS(&key_of[at], 0ull, key);
        if (seen == 0 || seen == key) return (uint32_t)at;
        met++;
        at = (at + 1) & (slots - 1);
    }
    return CLS_NONE;
}

// the smallest row of a slot: test first, the core class's rows come in nearly ascending
__device__ __forceinline__ void cls_lower(uint32_t *smallest, uint32_t r)
{
    if (r < cls_load(smallest)) atomicMin(smallest, r);
}

// Rows in the slots, one lane: the slot of row r's class, claimed if need be and lowered to r; CLS_NONE after `slots` steps.
__device__ __forceinline__ uint32_t cls_place_row(uint32_t r, const uint32_t *__restrict__ presence, uint32_t words, uint64_t n_rows, uint32_t *row_of, uint64_t slots,
                                                  unsigned long long home, unsigned long long &met)
{
    uint64_t at = home & (slots - 1);
    const uint32_t *mine = presence + (uint64_t)r * words;
    for (uint64_t probes = 0; probes < slots; probes++) {
        uint32_t seen = cls_load(&row_of[at]);
        if (seen == CLS_NONE) seen = atomicCAS(&row_of[at], CLS_NONE, r);
        if (seen == CLS_NONE || seen == r) return (uint32_t)at;
        bool same = seen < n_rows;
        for (uint32_t w = 0; same && w < words; w++) same = presence[(uint64_t)seen * words + w] == mine[w];
        if (same) {
            if (r < seen) atomicMin(&row_of[at], r);   // (seen may be stale and too large: the atomic decides)
            return (uint32_t)at;
        }
        met++;
        at = (at + 1) & (slots - 1);
    }
    return CLS_NONE;
}

// key_of: KEYED, [slots], 0 = empty.  rows: KEYED smallest[slots], else the slots themselves; all ones = empty either way.  A whole wave
// runs every iteration (the stride is a multiple of 64), lanes past the last row take part in the shuffles and ballots and nothing else.
template <bool KEYED>
__global__ void k_cls_insert_thread(const uint32_t *__restrict__ presence, uint32_t words, uint64_t n_rows, unsigned long long mask, unsigned long long *key_of, uint32_t *rows,
                                    uint64_t slots, uint32_t *__restrict__ slot_of, unsigned long long *__restrict__ met_total, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long met = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r - lane < n_rows; r += stride) {
        bool live = r < n_rows, as_below = false;
        unsigned long long key = 0, sum = 0;
        if (live) {
            const uint32_t *mine = presence + r * words;
            as_below = r > 0;
            for (uint32_t w = 0; w < words; w++) {
                const uint32_t bits = mine[w];
                sum += cls_word(w, bits);
                if (KEYED) key |= (unsigned long long)bits << (32 * (w & 1u));
                else if (r > 0) as_below = as_below && bits == presence[(r - 1) * words + w];
            }
            if (KEYED && key == 0) { atomicOr(flags, CLS_FLAG_ROW); live = false; }   // (cannot happen: every row has an occurrence)
        }
        if (KEYED) {
            const unsigned long long key_below = __shfl_up(key, 1);
            as_below = key_below == key;   // (a lane that is not live holds 0, a live one never does)
        }
        const bool head = !live || lane == 0 || !as_below;
        const unsigned long long heads = __ballot(head);
        const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
        uint32_t at = CLS_NONE;
        if (head && live) {
            const unsigned long long home = cls_mix(sum) & mask;
            if (KEYED) {
                at = cls_place_key(key, key_of, slots, home, met);
                if (at != CLS_NONE) cls_lower(&rows[at], (uint32_t)r);   // the leader's row is the run's smallest
            } else at = cls_place_row((uint32_t)r, presence, words, n_rows, rows, slots, home, met);
        }
        at = __shfl(at, start);
        if (live) {
            slot_of[r] = at;
            if (at == CLS_NONE) atomicOr(flags, CLS_FLAG_GAVE_UP);
        }
    }
    met = cls_wave_sum(met);
    if (lane == 0 && met) atomicAdd(met_total, met);
}

// one wave per row: the row is uniform over the wave, and so is every branch around a shuffle or a vote
template <bool KEYED>
__global__ void k_cls_insert_wave(const uint32_t *__restrict__ presence, uint32_t words, uint64_t n_rows, unsigned long long mask, unsigned long long *key_of, uint32_t *rows,
                                  uint64_t slots, uint32_t *__restrict__ slot_of, unsigned long long *__restrict__ met_total, uint32_t *__restrict__ flags)
{
    const uint32_t lane = threadIdx.x & 63u, waves = blockDim.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * waves;
    unsigned long long met = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * waves + (threadIdx.x >> 6); r < n_rows; r += stride) {
        const uint32_t *mine = presence + r * words;
        unsigned long long sum = 0;
        for (uint32_t w = lane; w < words; w += 64) sum += cls_word(w, mine[w]);
        const unsigned long long home = cls_mix(cls_wave_sum(sum)) & mask;
        uint32_t at = CLS_NONE;
        if (KEYED) {
            if (lane == 0) {
                const unsigned long long key = mine[0] | (words > 1 ? (unsigned long long)mine[1] << 32 : 0ull);
                if (key == 0) atomicOr(flags, CLS_FLAG_ROW);
                else {
                    at = cls_place_key(key, key_of, slots, home, met);
                    if (at != CLS_NONE) cls_lower(&rows[at], (uint32_t)r);
                    else atomicOr(flags, CLS_FLAG_GAVE_UP);
                }
                slot_of[r] = at;
            }
            continue;
        }
        uint64_t slot = home & (slots - 1);
        for (uint64_t probes = 0; probes < slots; probes++) {
            uint32_t seen = CLS_NONE;
            if (lane == 0) {
                seen = cls_load(&rows[slot]);
                if (seen == CLS_NONE) seen = atomicCAS(&rows[slot], CLS_NONE, (uint32_t)r);
            }
            seen = __shfl(seen, 0);
            if (seen == CLS_NONE || seen == (uint32_t)r) { at = (uint32_t)slot; break; }
            bool differs = seen >= n_rows;
            if (!differs)
                for (uint32_t w = lane; w < words; w += 64) differs = differs || presence[(uint64_t)seen * words + w] != mine[w];
            if (!__any(differs)) {
                if (lane == 0 && (uint32_t)r < seen) atomicMin(&rows[slot], (uint32_t)r);
                at = (uint32_t)slot;
                break;
            }
            if (lane == 0) met++;
            slot = (slot + 1) & (slots - 1);
        }
        if (lane == 0) {
            slot_of[r] = at;
            if (at == CLS_NONE) atomicOr(flags, CLS_FLAG_GAVE_UP);
        }
    }
    met = cls_wave_sum(met);
    if (lane == 0 && met) atomicAdd(met_total, met);
}

// flag: n_rows + 1 entries, the scan's last element is the number of classes.  smallest: of every slot (W > 2: the slots themselves)
__global__ void k_cls_flags(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ smallest, uint64_t slots, uint64_t n_rows, uint32_t *__restrict__ flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rows; r += stride) {
        const uint32_t s = r < n_rows ? slot_of[r] : CLS_NONE;
        flag[r] = s < slots && smallest[s] == (uint32_t)r ? 1u : 0u;
    }
}

// id: the exclusive scan of the flags
__global__ void k_cls_number(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ smallest, uint64_t slots, const uint32_t *__restrict__ id, uint64_t n_rows,
                             uint32_t *__restrict__ class_of)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        const uint32_t s = slot_of[r], m = s < slots ? smallest[s] : CLS_NONE;
        class_of[r] = m < n_rows ? id[m] : CLS_NONE;
    }
}

// the sum of v over the lanes start .. lane of this lane's run (start: the run's first lane)
__device__ __forceinline__ unsigned long long cls_run_sum(unsigned long long v, uint32_t lane, uint32_t start)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long below = __shfl_up(v, d);
        if (lane >= start + d) v += below;
    }
    return v;
}

// col_rows: the colour table's [4][n_rows] (first event, occurrences, ..).  id: [n_rows + 1], row r is its class's first when id steps
// behind it.  sums: [CLS_SUMS][n_classes].  A whole wave runs every iteration, as in k_cls_insert_thread.
__global__ void k_cls_rows(const uint32_t *__restrict__ class_of, const uint32_t *__restrict__ id, uint64_t n_rows, const uint32_t *__restrict__ col_rows,
                           const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint64_t n_events, uint32_t k, uint32_t *__restrict__ first,
                           unsigned long long *__restrict__ sums, uint64_t n_classes, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r - lane < n_rows; r += stride) {
        bool active = r < n_rows;
        uint32_t p = CLS_NONE;
        unsigned long long weight = 0, occurrences = 0;
        if (active) {
            p = class_of[r];
            const uint32_t e0 = col_rows[r];
            active = p < n_classes && e0 < n_events;
            if (!active) { atomicOr(flags, CLS_FLAG_ROW); p = CLS_NONE; }
            else {
                weight = (unsigned long long)end[e0] - begin[e0];
                occurrences = col_rows[n_rows + r];
                if (id[r + 1] != id[r]) first[p] = (uint32_t)r;
            }
        }
        const uint32_t p_below = __shfl_up(p, 1);
        const bool head = lane == 0 || p_below != p;   // (the lanes that are not active are runs of their own: they hold all ones)
        const unsigned long long heads = __ballot(head), actives = __ballot(active);
        const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
        const unsigned long long run = col_run(lane, heads, actives);
        const uint32_t last = run ? 63u - (uint32_t)__clzll((long long)run) : lane;   // of a leader: the last lane of its run
        const unsigned long long weight_run = __shfl(cls_run_sum(weight, lane, start), last), occ_run = __shfl(cls_run_sum(occurrences, lane, start), last);
        if (head && active) {
            const unsigned long long n = (unsigned long long)__popcll(run);
            atomicAdd(&sums[p], n);
            atomicAdd(&sums[n_classes + p], weight_run + n * k);   // length = weight + k per segment
            atomicAdd(&sums[2 * n_classes + p], weight_run);
            atomicAdd(&sums[3 * n_classes + p], occ_run);
        }
    }
}

__global__ void k_cls_presence(const uint32_t *__restrict__ first, uint64_t n_classes, const uint32_t *__restrict__ col_presence, uint32_t words, uint64_t n_rows,
                               uint32_t *__restrict__ presence, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, total = n_classes * words;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint64_t p = i / words;
        const uint32_t r = first[p];
        if (r < n_rows) presence[i] = col_presence[(uint64_t)r * words + (i - p * words)];
        else atomicOr(flags, CLS_FLAG_ROW);
    }
}

// sets: [0, C] classes, [C + 1, 2C + 1] segments, [2C + 2, 3C + 2] edges.  LDS: 3 x (C + 1) 64-bit bins of dynamic shared memory, or none.
template <bool LDS>
__global__ void k_cls_sets(const uint32_t *__restrict__ presence, uint32_t words, const unsigned long long *__restrict__ sums, uint64_t n_classes, uint32_t n_colors,
                           unsigned long long *__restrict__ sets, unsigned long long *__restrict__ largest)
{
    extern __shared__ unsigned long long s_bins[];
    const uint32_t bins = n_colors + 1;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < 3 * bins; i += blockDim.x) s_bins[i] = 0;
        __syncthreads();
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_classes; p += stride) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < words; w++) n += (uint32_t)__popc(presence[p * words + w]);
        const unsigned long long segments = sums[p], edges = sums[2 * n_classes + p];
        if (segments > __hip_atomic_load(largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(largest, segments);
        if (n > n_colors) continue;  // (cannot happen: every colour is below n_colors)
        if (LDS) { atomicAdd(&s_bins[n], 1ull); atomicAdd(&s_bins[bins + n], segments); atomicAdd(&s_bins[2 * bins + n], edges); }
        else { atomicAdd(&sets[n], 1ull); atomicAdd(&sets[bins + n], segments); atomicAdd(&sets[2 * bins + n], edges); }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 3 * bins; i += blockDim.x) if (s_bins[i]) atomicAdd(&sets[i], s_bins[i]);
    }
}

int cls_fetch_check(tpc_ctx *c, const char *what, uint64_t total, uint64_t at, uint64_t n, bool missing)
{
    if ((n && missing) || at > total || n > total - at)
        return fail(c, -1, "segment classes: bad %s range (%llu %ss at %llu of %llu)", what, (unsigned long long)n, what, (unsigned long long)at, (unsigned long long)total);
    return 0;
}

// the test options hold for one build: whichever way it returns, the next one runs on its own
struct ClsOptions {
    tpc_ctx *c;
    int slots_log2, hash_bits, grid, wide;
    explicit ClsOptions(tpc_ctx *c_) : c(c_), slots_log2(c_->opt_classes_slots_log2), hash_bits(c_->opt_classes_hash_bits), grid(c_->opt_classes_grid), wide(c_->opt_classes_wide) {}
    ~ClsOptions() { c->opt_classes_slots_log2 = 0; c->opt_classes_hash_bits = -1; c->opt_classes_grid = 0; c->opt_classes_wide = 0; }
};

}  // namespace

extern "C" {

int tpc_segments_classes_build(tpc_ctx *c)
{
    if (!c) return -1;
    classes_drop(c);
    const ClsOptions opt(c);
    if (int rc = stage_needs_segments(c, "classes", "group")) return rc;
    if (!c->col.valid) return fail(c, -1, "segment classes: build the colour table first (tpc_segments_colors_build)");
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments;
    const uint32_t words = c->col.words, n_colors = c->col.n_colors, bins = n_colors + 1;
    if (n_rows > CLS_MAX_ROWS) return fail(c, -1, "segment classes: %llu segments, a row holds at most %llu", (unsigned long long)n_rows, (unsigned long long)CLS_MAX_ROWS);
    if (c->col.n_rows != n_rows) return fail(c, -10, "segment classes: the colour table holds %llu rows, the build counted %llu segments", (unsigned long long)c->col.n_rows, (unsigned long long)n_rows);
    if (opt.slots_log2 < 0 || opt.slots_log2 > 31) return fail(c, -1, "segment classes: option test_classes_slots_log2 = %d is not in 0 .. 31", opt.slots_log2);
    if (opt.hash_bits < -1 || opt.hash_bits > 64) return fail(c, -1, "segment classes: option test_classes_hash_bits = %d is not in 0 .. 64", opt.hash_bits);
    if (opt.wide < 0 || opt.wide > 2) return fail(c, -1, "segment classes: option test_classes_wide = %d is not one of 0, 1, 2", opt.wide);
    HIPCHK(c, hipSetDevice(c->device));
    const bool keyed = words <= 2, wave = opt.wide == 1 || (opt.wide == 0 && words > CLS_THREAD_WORDS);
    const unsigned long long mask = opt.hash_bits < 0 || opt.hash_bits >= 64 ? ~0ull : (1ull << opt.hash_bits) - 1;
    // at least 2 S slots; a slot is 32 bits with all ones for none, so 2^31 of them at the most (S < 2^31 classes still fit)
    uint64_t slots = 64;
    if (opt.slots_log2) slots = (uint64_t)1 << opt.slots_log2;
    else while (slots < 2 * n_rows && slots < ((uint64_t)1 << 31)) slots <<= 1;
    auto grid = [&](uint64_t n) { return dim3(opt.grid > 0 ? std::min<unsigned>(col_grid(n), (unsigned)opt.grid) : col_grid(n)); };

    // sizes in 64 bits, summed before the first allocation; what is kept per class has its bound: one class per row
    const uint64_t row_bytes = n_rows * 4 + 16, flag_bytes = (n_rows + 1) * 4, slot_bytes = slots * (keyed ? 12 : 4) + 16, sets_bytes = (uint64_t)bins * 24;
    const uint64_t per_class = 4 + CLS_SUMS * 8 + (uint64_t)words * 4, kept_bound = n_rows * per_class + 48;
    size_t scan_bytes = 0;
    uint32_t *slot_of = nullptr, *flag = nullptr, *flags = nullptr, *slot_rows = nullptr;
    unsigned long long *key_of = nullptr;
    void *scan_tmp = nullptr;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, flag, flag, 0u, n_rows + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess)
        return fail(c, -10, "segment classes: the scan could not be sized");
    const uint64_t need = 2 * row_bytes + flag_bytes + slot_bytes + sets_bytes + kept_bound + scan_bytes + 16 + 64;
    if (int rc = stage_fits(c, "classes", need, "%llu of them %llu slots, up to %llu what %u presence words per class take", (unsigned long long)slot_bytes, (unsigned long long)slots,
                            (unsigned long long)kept_bound, words))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) classes_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->cls.class_of, row_bytes) != hipSuccess || dev_malloc(c, (void **)&c->cls.sets, sets_bytes) != hipSuccess || !temps.get(c, &slot_of, row_bytes) ||
        !temps.get(c, &flag, flag_bytes) || !temps.get(c, &slot_rows, slots * 4 + 16) || (keyed && !temps.get(c, &key_of, slots * 8)) || !temps.get(c, &scan_tmp, scan_bytes + 16) ||
        !temps.get(c, &flags, 64))
        return done(fail(c, -10, "segment classes: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    // 64 bytes of scalars: flags[0], then the probes that met another class, then the largest class
    unsigned long long *met = (unsigned long long *)(flags + 2), *largest = met + 1;
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(flags, 0, 64, s) == hipSuccess && hipMemsetAsync(slot_rows, 0xFF, slots * 4, s) == hipSuccess &&
              (!keyed || hipMemsetAsync(key_of, 0, slots * 8, s) == hipSuccess) && hipMemsetAsync(c->cls.sets, 0, sets_bytes, s) == hipSuccess;
    uint32_t n_classes = 0, raised = 0;
    unsigned long long met_host = 0, largest_host = 0;
    if (ok) {
        Timed t(c, TPC_K_CLASSES);   // the whole stage on the stream, the wait for the class count included (as TPC_K_COMPONENTS)
        if (n_rows) {
            // (a wave per row: four rows per workgroup of 256)
            if (wave && keyed) hipLaunchKernelGGL(k_cls_insert_wave<true>, grid(n_rows * 64), dim3(256), 0, s, c->col.presence, words, n_rows, mask, key_of, slot_rows, slots, slot_of, met, flags);
            else if (wave) hipLaunchKernelGGL(k_cls_insert_wave<false>, grid(n_rows * 64), dim3(256), 0, s, c->col.presence, words, n_rows, mask, key_of, slot_rows, slots, slot_of, met, flags);
            else if (keyed) hipLaunchKernelGGL(k_cls_insert_thread<true>, grid(n_rows), dim3(256), 0, s, c->col.presence, words, n_rows, mask, key_of, slot_rows, slots, slot_of, met, flags);
            else hipLaunchKernelGGL(k_cls_insert_thread<false>, grid(n_rows), dim3(256), 0, s, c->col.presence, words, n_rows, mask, key_of, slot_rows, slots, slot_of, met, flags);
        }
        hipLaunchKernelGGL(k_cls_flags, grid(n_rows + 1), dim3(256), 0, s, slot_of, slot_rows, slots, n_rows, flag);
        ok = rocprim::exclusive_scan(scan_tmp, scan_bytes, flag, flag, 0u, n_rows + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        if (ok && n_rows) hipLaunchKernelGGL(k_cls_number, grid(n_rows), dim3(256), 0, s, slot_of, slot_rows, slots, flag, n_rows, c->cls.class_of);
        // the number of classes decides the size of what is kept: the one wait in the middle
        ok = ok && hipMemcpyAsync(&n_classes, flag + n_rows, sizeof n_classes, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess && hipMemcpyAsync(&met_host, met, sizeof met_host, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "classes", ok)) return done(rc);
        if (raised & CLS_FLAG_ROW) return done(fail(c, -10, "segment classes: a row of the colour table holds no colour"));
        if (raised & CLS_FLAG_GAVE_UP)
            return done(fail(c, -10, "segment classes: gave up after %llu probes: the set of %llu slots is too small for the classes of %llu segments (option test_classes_slots_log2 = %d)",
                             (unsigned long long)slots, (unsigned long long)slots, (unsigned long long)n_rows, opt.slots_log2));
        if (n_classes > n_rows || (n_rows && !n_classes)) return done(fail(c, -10, "segment classes: %u classes of %llu segments", n_classes, (unsigned long long)n_rows));
        const uint64_t first_bytes = (uint64_t)n_classes * 4 + 16, sums_bytes = (uint64_t)n_classes * CLS_SUMS * 8 + 16, presence_bytes = (uint64_t)n_classes * words * 4 + 16;
        if (dev_malloc(c, (void **)&c->cls.first, first_bytes) != hipSuccess || dev_malloc(c, (void **)&c->cls.sums, sums_bytes) != hipSuccess ||
            dev_malloc(c, (void **)&c->cls.presence, presence_bytes) != hipSuccess)
            return done(fail(c, -10, "segment classes: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->cls.first, 0xFF, first_bytes, s) == hipSuccess && hipMemsetAsync(c->cls.sums, 0, sums_bytes, s) == hipSuccess &&
             hipMemsetAsync(c->cls.presence, 0, presence_bytes, s) == hipSuccess;
        if (ok && n_rows) {
            hipLaunchKernelGGL(k_cls_rows, grid(n_rows), dim3(256), 0, s, c->cls.class_of, flag, n_rows, c->col.rows, c->seg.ev[0], c->seg.ev[1], n_events, (uint32_t)c->seg.k, c->cls.first,
                               c->cls.sums, (uint64_t)n_classes, flags);
            hipLaunchKernelGGL(k_cls_presence, grid((uint64_t)n_classes * words), dim3(256), 0, s, c->cls.first, (uint64_t)n_classes, c->col.presence, words, n_rows, c->cls.presence, flags);
            if (bins <= CLS_LDS_BINS)
                hipLaunchKernelGGL(k_cls_sets<true>, dim3(std::min(grid(n_classes).x, 1024u)), dim3(256), (size_t)bins * 24, s, c->cls.presence, words, c->cls.sums, (uint64_t)n_classes, n_colors,
                                   c->cls.sets, largest);
            else
                hipLaunchKernelGGL(k_cls_sets<false>, grid(n_classes), dim3(256), 0, s, c->cls.presence, words, c->cls.sums, (uint64_t)n_classes, n_colors, c->cls.sets, largest);
        }
        ok = ok && hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&largest_host, largest, sizeof largest_host, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->cls.peak_bytes = need - kept_bound + first_bytes + sums_bytes + presence_bytes;
    }
    if (int rc = stage_wait(c, "classes", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment classes: a row lies in no class"));
    c->cls.n_classes = n_classes; c->cls.n_rows = n_rows; c->cls.largest = largest_host; c->cls.met = met_host; c->cls.words = words; c->cls.n_colors = n_colors;
    c->cls.valid = true;
    return 0;
}

int tpc_segments_classes_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->cls.valid) return fail(c, -1, "segment classes: tpc_segments_classes_build first");
    if (!info) return fail(c, -1, "segment classes: info required");
    info[0] = c->cls.n_classes; info[1] = c->cls.n_rows; info[2] = c->cls.largest; info[3] = c->cls.met; info[4] = c->cls.peak_bytes;
    return 0;
}

int tpc_segments_classes_fetch_members(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *class_host)
{
    if (!c) return -1;
    if (!c->cls.valid) return fail(c, -1, "segment classes: tpc_segments_classes_build first");
    return fetch_planes(c, "classes", "row", c->cls.class_of, c->cls.n_rows, r0, n, { class_host });
}

int tpc_segments_classes_fetch_rows(tpc_ctx *c, uint64_t p0, uint64_t n, uint32_t *first_host, uint64_t *segments_host, uint64_t *length_host, uint64_t *edges_host,
                                    uint64_t *occurrences_host)
{
    if (!c) return -1;
    if (!c->cls.valid) return fail(c, -1, "segment classes: tpc_segments_classes_build first");
    uint64_t *const dst[CLS_SUMS] = { segments_host, length_host, edges_host, occurrences_host };
    bool missing = !first_host;
    for (uint64_t *d : dst) missing = missing || !d;
    if (int rc = cls_fetch_check(c, "class", c->cls.n_classes, p0, n, missing)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!n) return 0;
    HIPCHK(c, hipMemcpy(first_host, c->cls.first + p0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < CLS_SUMS; i++) HIPCHK(c, hipMemcpy(dst[i], c->cls.sums + (uint64_t)i * c->cls.n_classes + p0, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_classes_fetch_presence(tpc_ctx *c, uint64_t p0, uint64_t n, uint32_t *words_host)
{
    if (!c) return -1;
    if (!c->cls.valid) return fail(c, -1, "segment classes: tpc_segments_classes_build first");
    if (int rc = cls_fetch_check(c, "class", c->cls.n_classes, p0, n, !words_host)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(words_host, c->cls.presence + p0 * c->cls.words, n * c->cls.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_classes_fetch_sets(tpc_ctx *c, uint64_t *classes_host, uint64_t *segments_host, uint64_t *edges_host)
{
    if (!c) return -1;
    if (!c->cls.valid) return fail(c, -1, "segment classes: tpc_segments_classes_build first");
    if (!classes_host || !segments_host || !edges_host) return fail(c, -1, "segment classes: all three arrays of the sets are required");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bins = (size_t)c->cls.n_colors + 1;
    HIPCHK(c, hipMemcpy(classes_host, c->cls.sets, bins * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(segments_host, c->cls.sets + bins, bins * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(edges_host, c->cls.sets + 2 * bins, bins * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
