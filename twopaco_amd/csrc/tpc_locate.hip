// tpc_locate.hip -- the edge index of the compacted graph and the location of a query text in it: is a sequence that was no input
// in the graph, where, and in which colours.  Kernels and the C-ABI of the tpc_segments_edges_* and tpc_segments_locate_* groups of
// include/twopaco_hip.h, which states the definition (row span, edge index, smallest g, hit, run, per-record sums).  No counterpart
// in the reference.
//
// Input of the index: the event table of the last tpc_segments_build_* and the text T it was built over.  n = k + 1.
//   SegRows        rank[e] of a first event is its row (tpc_segrows.h)
//   k_loc_span     one thread per first event: g0[row] = rec_start[sequence] + begin, checked against the record, and the bits
//                  [g0, g0 + end - begin) of a mask over T.  Spans of different rows are disjoint, so a word inside a span is
//                  stored whole and only the two edge words of a span need atomicOr.
//   the sort       rocprim::radix_sort_pairs of (g0, row) by g0: the row of a position is then one binary search.
//   k_loc_tile<COUNT>   the sketch's tile shape over T (256 threads, 32 positions per thread, words + halo through LDS, long-lived
//                  workgroups striding over the tiles, the hash of tpc_edgehash.h): counts the masked positions with a valid window
//                  (the table is sized by them: the one wait in the middle) and the masked positions without one (skipped).
//   k_loc_tile<INSERT>  the same walk inserts every such position into an open-addressed table in HBM, linear probing from
//                  hash & (slots - 1).  A slot is 16 B: word 0 = tag:24 | g:40 (tag = the hash's top 24 bits), word 1 = the row, all
//                  ones = empty.  atomicCAS from empty claims a slot (an ENTRY).  On an equal tag the LETTERS of the two windows
//                  are compared, 32 per load, both strands: the same key takes atomicMin on word 0 -- the tags are equal, so the
//                  minimum is the smaller g -- and counts as a DUPLICATE; another key probes on.  Slots only ever go from empty to
//                  one key and keep that key, so every insert of a key walks the same slots and ends in the same one: entries,
//                  duplicates and the surviving g do not depend on the schedule.  The probe loop is bounded by the slot count and
//                  its longest walk is kept; an insert that finds no slot is counted and the build refused.
//   k_loc_rows     AFTER all inserts, one thread per slot finds the row of the slot's final g (binary search in the sorted g0: spans are
//                  disjoint, so the last span that starts at or before g holds it) and stores word 1.  No reader runs before this kernel has ended -- a locate is a later call on the
//                  same stream -- so no reader sees a (g, row) pair that never belonged together, and no insert ever reads a row.
// Locate: Q's packed words and N mask are uploaded as temporaries of the call, padded as tpc_seq_upload pads T.
//   k_loc_tile<PROBE>   the same walk over Q: per position roll, probe, compare the letters against T at the slot's g, write
//                  hit[p] (64 bits: all ones invalid, all ones - 1 absent, else rev << 63 | g) and row[p] (all ones / all ones - 1
//                  likewise).  The hash constants come from device memory, the tile counter is 32 bits, the runtime loops are not
//                  unrolled and n's bounds are stated: what the compiler hoists out of four nested loops then fits the scalar
//                  registers (no SGPR spill; with the constants by value and the sums folded here it spilled 42).
//   k_loc_fold     one thread folds 32 consecutive positions of hit[] / row[]: windows, found and forward of the record it is in
//                  (one binary search when it leaves the record it knew), and the run of hits in one row, flushed when the row or
//                  the record changes by walking the set bits of the row's presence words: shared[record][colour] += run length.
//                  A kernel of its own: it streams 12 B per position, and the probe kernel keeps none of its pointers live.
//   k_loc_heads    one thread per position evaluates the continue rule against p - 1 and p + 1: head | tail << 1
//   the scan       exclusive over positions + 1 head flags: the slot of every run and their number (the second wait)
//   k_loc_place    a head writes q_first, row, rev, off_first into slot scan[p], a tail q_last into slot scan[p + 1] - 1
//   k_loc_close    one thread per run: length = q_last - q_first + 1 and runs[record of q_first] += 1
// Memory: kept until the next segment build, edge build or (checked by text_uploads) text upload 16 B / slot and 8 B / row; of a
// locate 12 B / position, 20 B / run, 32 B / record and 8 B x colours / record.  During the build also the mask (4 B / 32
// positions of T), the row index, 24 B / row of sort buffers; during a locate the query text and 8 B / position of flags.
#include "tpc_segrows.h"
#include "tpc_edgehash.h"

namespace {

constexpr unsigned long long LOC_EMPTY = ~0ull;
constexpr unsigned long long LOC_G_MASK = (1ull << 40) - 1;
constexpr unsigned long long LOC_INVALID = ~0ull, LOC_ABSENT = ~0ull - 1;
constexpr uint32_t LOC_ROW_INVALID = 0xFFFFFFFFu, LOC_ROW_ABSENT = 0xFFFFFFFEu;
constexpr unsigned long long LOC_NO_SPAN = 1ull << 40;   // the sort key of a row without a span: behind every position
constexpr int LOC_WG_PER_CU = 6;
enum { LOC_COUNT = 0, LOC_INSERT = 1, LOC_PROBE = 2 };
// counters[]: 0 entries (COUNT: valid masked positions), 1 duplicates, 2 skipped, 3 longest probe, 4 inserts without a slot, 5 events outside their record / slots without a row
enum { LC_ENTRIES = 0, LC_DUPLICATES = 1, LC_SKIPPED = 2, LC_PROBE = 3, LC_FULL = 4, LC_BAD = 5, LC_WORDS = 8 };

struct LocSlot {
    unsigned long long key;
    uint32_t row, unused;
};

__global__ void k_loc_span(const uint32_t *__restrict__ first, const uint32_t *__restrict__ rank, uint64_t n_events, uint64_t n_rows, const uint32_t *__restrict__ begin,
                           const uint32_t *__restrict__ end, const uint32_t *__restrict__ seq_begin, uint32_t n_rec, const uint64_t *__restrict__ rec_start,
                           const uint64_t *__restrict__ rec_len, uint64_t n_text, uint32_t *__restrict__ span, uint64_t span_words, uint64_t *__restrict__ g0_of,
                           unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals, unsigned long long *__restrict__ counters)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        if (!((first[e >> 5] >> (e & 31)) & 1u)) continue;
        const uint32_t row = rank[e];
        if (row >= n_rows) { atomicAdd(&counters[LC_BAD], 1ull); continue; }
        const uint32_t lo = col_seq_end(seq_begin, n_rec, (uint32_t)e);
        const uint32_t b = begin[e], en = end[e];
        bool ok = lo >= 1 && lo <= n_rec && en >= b;
        uint64_t g0 = 0;
        if (ok) {
            const uint64_t start = rec_start[lo - 1], len = rec_len[lo - 1];
            ok = en <= len && start <= n_text && len <= n_text - start;
            g0 = start + b;
        }
        const uint64_t n = ok ? (uint64_t)en - b : 0;
        ok = ok && ((g0 + n + 31) >> 5) <= span_words;
        g0_of[row] = ok ? g0 : 0;
        keys[row] = ok && n ? g0 : LOC_NO_SPAN;
        vals[row] = row;
        if (!ok) { atomicAdd(&counters[LC_BAD], 1ull); continue; }
        if (!n) continue;
        const uint64_t last = g0 + n - 1, w0 = g0 >> 5, w1 = last >> 5;
        const uint32_t head = ~0u << (g0 & 31), tail = ~0u >> (31 - (last & 31));
        if (w0 == w1) { atomicOr(&span[w0], head & tail); continue; }
        atomicOr(&span[w0], head);
        for (uint64_t w = w0 + 1; w < w1; w++) span[w] = ~0u;
        atomicOr(&span[w1], tail);
    }
}

// Are the windows a[ga, ga + n) and b[gb, gb + n) one edge?  0: no; 1: equal letter for letter; 2: a is the reverse complement of b.
// Neither window holds an 'N'; both texts are padded, so the word behind a window's last exists.
__device__ __forceinline__ int loc_same(const uint64_t *__restrict__ a, uint64_t ga, const uint64_t *__restrict__ b, uint64_t gb, int n)
{
    // both strands in one pass over a's words: word w of b's reverse complement is the reversed word that ends n - 32 w letters in
    const int full = n >> 5, rem = n & 31;
    bool fwd = true, rev = true;
#pragma nounroll
    for (int w = 0; w < full && (fwd || rev); w++) {
        const uint64_t x = tpc_text_word(a, ga + 32 * w);
        fwd = fwd && x == tpc_text_word(b, gb + 32 * w);
        rev = rev && x == tpc_revcomp_word(tpc_text_word(b, gb + n - 32 * w - 32));
    }
    if (rem && (fwd || rev)) {
        const uint64_t m = (1ull << (2 * rem)) - 1, x = tpc_text_word(a, ga + 32 * full) & m;
        fwd = fwd && x == (tpc_text_word(b, gb + 32 * full) & m);
        rev = rev && x == (tpc_revcomp_word(tpc_text_word(b, gb)) >> (64 - 2 * rem));
    }
    return fwd ? 1 : rev ? 2 : 0;
}

struct LocFold {
    // the record this thread last found and what it saw of it
    int64_t rec = -1;
    uint64_t rec_end = 0;
    unsigned long long windows = 0, found = 0, forward = 0;
    // the run of hits in one row
    uint32_t run_row = LOC_ROW_INVALID;
    unsigned long long run_len = 0;
};

struct LocQuery {
    const uint64_t *t_bases;      // T
    uint64_t n_text, n_rows, positions;
    const uint64_t *rec_start, *rec_len;   // Q's records
    uint32_t n_rec;
    const uint32_t *presence;     // the colour table's, or none
    uint32_t words, n_colors;
    unsigned long long *hit;
    uint32_t *row;
    unsigned long long *recs, *shared;
};

__device__ __forceinline__ void loc_flush_run(LocFold &f, const LocQuery &q)
{
    if (f.run_len && f.rec >= 0 && q.presence && f.run_row < q.n_rows) {
        for (uint32_t w = 0; w < q.words; w++) {
            uint32_t bits = q.presence[(uint64_t)f.run_row * q.words + w];
            while (bits) {
                const uint32_t col = w * 32 + (uint32_t)__ffs((int)bits) - 1;
                bits &= bits - 1;
                if (col < q.n_colors) atomicAdd(&q.shared[(uint64_t)f.rec * q.n_colors + col], f.run_len);
            }
        }
    }
    f.run_len = 0;
    f.run_row = LOC_ROW_INVALID;
}

__device__ __forceinline__ void loc_flush(LocFold &f, const LocQuery &q)
{
    loc_flush_run(f, q);
    if (f.rec >= 0) {
        if (f.windows) atomicAdd(&q.recs[f.rec], f.windows);
        if (f.found) atomicAdd(&q.recs[(uint64_t)q.n_rec + f.rec], f.found);
        if (f.forward) atomicAdd(&q.recs[2 * (uint64_t)q.n_rec + f.rec], f.forward);
    }
    f.windows = f.found = f.forward = 0;
}

// the record that holds position p, or -1; end = where what this answer says stops holding
__device__ __forceinline__ int64_t loc_record(const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, uint32_t n_rec, uint64_t p, uint64_t &end)
{
    uint32_t lo = 0, hi = n_rec;   // how many records start at or before p
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (rec_start[mid] <= p) lo = mid + 1; else hi = mid; }
    end = p + 1;
    if (!lo) return -1;
    const uint64_t stop = rec_start[lo - 1] + rec_len[lo - 1];
    if (p >= stop) return -1;
    end = stop;
    return (int64_t)lo - 1;
}

template <int MODE>
__global__ void __launch_bounds__(TPC_TILE_THREADS)
k_loc_tile(const uint64_t *__restrict__ tab, int n, const uint64_t *__restrict__ bases, const uint32_t *__restrict__ nmask, uint64_t n_text, uint32_t n_tiles, const uint32_t *__restrict__ span,
           LocSlot *__restrict__ slots, uint64_t slot_mask, uint64_t hash_mask, unsigned long long *__restrict__ counters, LocQuery q)
{
    __shared__ uint64_t s_b[TPC_TILE_WORDS];
    __shared__ uint32_t s_n[TPC_TILE_WORDS];
    __shared__ uint64_t s_t[16];
    __builtin_assume(n >= 1 && n / 32 + 2 <= TPC_XW_MAX);   // (the host refuses what the halo does not admit; said here, loop guards over n need no scalar registers)
    const int tid = threadIdx.x;
    if (tid < 16) s_t[tid] = tab[tid];   // h, hn, hc, hcr of SketchTab, from device memory: 32 scalar registers less than by value
    const int xw = n / 32 + 2;  // the last thread's last window ends (31 + n) / 32 words behind its own
    unsigned long long entries = 0, duplicates = 0, skipped = 0, longest = 0, full = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (a text below 2^40 positions: below 2^27 tiles)
        const uint64_t wfirst = (uint64_t)tile * TPC_TILE_THREADS;
        const uint64_t wbase = wfirst - 1;
        __syncthreads();  // (the previous tile's readers are done; first round: the constants are staged)
        tpc_stage_tile(s_b, s_n, bases, nmask, wfirst, xw);
        __syncthreads();
        const uint64_t g0 = (wfirst + tid) * TPC_RUN;
        if (MODE != LOC_PROBE && g0 >= n_text) continue;
        const uint32_t marked = MODE == LOC_PROBE ? 0u : span[wfirst + tid];
        if (MODE != LOC_PROBE && !marked) continue;
        if (MODE == LOC_PROBE && g0 >= q.positions) continue;
        uint64_t F, R;
        int ncnt;
        tpc_edge_eat<true>(s_t, s_b, s_n, g0, wbase, n, F, R, ncnt);
        for (int s = 0; s < TPC_RUN; s++) {
            const uint64_t g = g0 + s;
            if (MODE == LOC_PROBE && g >= q.positions) break;
            const bool wanted = MODE == LOC_PROBE || ((marked >> s) & 1u);
            if (wanted && ncnt != 0) {
                skipped++;
                if (MODE == LOC_PROBE) { q.hit[g] = LOC_INVALID; q.row[g] = LOC_ROW_INVALID; }
            }
            if (wanted && ncnt == 0 && MODE == LOC_COUNT) entries++;
            if (wanted && ncnt == 0 && MODE != LOC_COUNT) {
                const uint64_t x = tpc_edge_hash(F, R) & hash_mask;
                const unsigned long long tag = x & ~LOC_G_MASK, mine = tag | g;
                uint64_t i = x & slot_mask, steps = 0;
                unsigned long long hit = LOC_ABSENT;
                uint32_t hit_row = LOC_ROW_ABSENT;
                bool placed = false;
                for (; steps <= slot_mask; steps++, i = (i + 1) & slot_mask) {
                    unsigned long long cur = *reinterpret_cast<volatile unsigned long long *>(&slots[i].key);
                    if (cur == LOC_EMPTY) {
                        if (MODE == LOC_PROBE) break;    // absent
                        cur = atomicCAS(&slots[i].key, LOC_EMPTY, mine);
                        if (cur == LOC_EMPTY) { entries++; placed = true; break; }
                    }
                    if ((cur & ~LOC_G_MASK) != tag) continue;
                    const uint64_t there = cur & LOC_G_MASK;
                    if (there + (uint64_t)n > (MODE == LOC_PROBE ? q.n_text : n_text)) continue;   // (no such slot after a good build)
                    if (MODE == LOC_INSERT) {
                        if (!loc_same(bases, g, bases, there, n)) continue;
                        atomicMin(&slots[i].key, mine);
                        duplicates++;
                        placed = true;
                        break;
                    }
                    const int same = loc_same(bases, g, q.t_bases, there, n);
                    if (!same) continue;
                    hit = (same == 2 ? 1ull << 63 : 0ull) | there;
                    hit_row = slots[i].row;
                    break;
                }
                if (steps > longest) longest = steps;
                if (MODE == LOC_INSERT && !placed) full++;
                if (MODE == LOC_PROBE) { q.hit[g] = hit; q.row[g] = hit_row; }
            }
            tpc_edge_roll(s_t, s_b, s_n, g, wbase, n, F, R, ncnt);
        }
    }
    if (MODE == LOC_PROBE) return;
    // every thread is here: one sum per wave
    for (int off = 32; off > 0; off >>= 1) {
        entries += __shfl_down(entries, off, 64);
        duplicates += __shfl_down(duplicates, off, 64);
        skipped += __shfl_down(skipped, off, 64);
        full += __shfl_down(full, off, 64);
        const unsigned long long other = __shfl_down(longest, off, 64);
        if (other > longest) longest = other;
    }
    if ((tid & 63) == 0) {
        if (entries) atomicAdd(&counters[LC_ENTRIES], entries);
        if (duplicates) atomicAdd(&counters[LC_DUPLICATES], duplicates);
        if (skipped && MODE == LOC_COUNT) atomicAdd(&counters[LC_SKIPPED], skipped);
        if (full) atomicAdd(&counters[LC_FULL], full);
        if (longest) atomicMax(&counters[LC_PROBE], longest);
    }
}

// The sums of a locate: one thread folds TPC_RUN consecutive positions of hit[] / row[] -- windows, found and forward of the record
// it is in (one binary search when it leaves the record it knew) and the run of hits in one row, flushed when the row or the record
// changes by walking the set bits of the row's presence words.
__global__ void k_loc_fold(LocQuery q)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * TPC_RUN;
    for (uint64_t p0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * TPC_RUN; p0 < q.positions; p0 += stride) {
        LocFold fold;
        for (uint64_t p = p0; p < p0 + TPC_RUN && p < q.positions; p++) {
            const unsigned long long hit = q.hit[p];
            if (hit == LOC_INVALID) continue;
            if (fold.rec < 0 || p >= fold.rec_end) {
                loc_flush(fold, q);
                fold.rec = loc_record(q.rec_start, q.rec_len, q.n_rec, p, fold.rec_end);
            }
            fold.windows++;
            if (hit == LOC_ABSENT) continue;
            const uint32_t hit_row = q.row[p];
            fold.found++;
            fold.forward += !(hit >> 63);
            if (hit_row != fold.run_row) { loc_flush_run(fold, q); fold.run_row = hit_row; }
            fold.run_len++;
        }
        loc_flush(fold, q);
    }
}

// sorted_g0[0 .. n_spans) ascend, sorted_row[] their rows
__global__ void k_loc_rows(LocSlot *__restrict__ slots, uint64_t n_slots, const unsigned long long *__restrict__ sorted_g0, const uint32_t *__restrict__ sorted_row,
                           uint64_t n_rows, unsigned long long *__restrict__ counters)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const unsigned long long key = slots[i].key;
        if (key == LOC_EMPTY) continue;
        const unsigned long long g = key & LOC_G_MASK;
        uint64_t lo = 0, hi = n_rows;   // how many spans start at or before g
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (sorted_g0[mid] <= g) lo = mid + 1; else hi = mid; }
        const uint32_t row = lo ? sorted_row[lo - 1] : LOC_ROW_INVALID;
        if (row < n_rows) slots[i].row = row;
        else atomicAdd(&counters[LC_BAD], 1ull);
    }
}

__device__ __forceinline__ bool loc_is_hit(unsigned long long h) { return h != LOC_INVALID && h != LOC_ABSENT; }

// does the hit at p continue the one at p - 1?
__device__ __forceinline__ bool loc_continues(const unsigned long long *__restrict__ hit, const uint32_t *__restrict__ row, uint64_t p)
{
    if (p == 0) return false;
    const unsigned long long h = hit[p], before = hit[p - 1];
    if (!loc_is_hit(h) || !loc_is_hit(before) || row[p] != row[p - 1] || (h >> 63) != (before >> 63)) return false;
    const unsigned long long g = h & LOC_G_MASK, g_before = before & LOC_G_MASK;
    return (h >> 63) ? g + 1 == g_before : g == g_before + 1;   // (one row: the offsets differ as the positions do)
}

// flags[p] = head | tail << 1; heads[p] = the head bit, heads[positions] = 0: the scan's last element is the run count
__global__ void k_loc_heads(const unsigned long long *__restrict__ hit, const uint32_t *__restrict__ row, uint64_t positions, uint32_t *__restrict__ flags,
                            uint32_t *__restrict__ heads)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= positions; p += stride) {
        uint32_t head = 0, tail = 0;
        if (p < positions) {
            if (loc_is_hit(hit[p])) {
                head = loc_continues(hit, row, p) ? 0u : 1u;
                tail = (p + 1 < positions && loc_continues(hit, row, p + 1)) ? 0u : 1u;
            }
            flags[p] = head | tail << 1;
        }
        heads[p] = head;
    }
}

// runs: [0, B) q_first, [B, 2B) q_last (k_loc_close makes it the length), [2B, 3B) row, [3B, 4B) rev, [4B, 5B) off_first
__global__ void k_loc_place(const unsigned long long *__restrict__ hit, const uint32_t *__restrict__ row, uint64_t positions, const uint32_t *__restrict__ flags,
                            const uint32_t *__restrict__ slot, const uint64_t *__restrict__ g0_of, uint64_t n_rows, uint32_t *__restrict__ runs, uint64_t n_runs)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < positions; p += stride) {
        const uint32_t f = flags[p];
        if (!f) continue;
        if (f & 1u) {
            const uint64_t b = slot[p];
            const unsigned long long h = hit[p], g = h & LOC_G_MASK;
            const uint32_t r = row[p];
            if (b < n_runs) {
                runs[b] = (uint32_t)p;
                runs[2 * n_runs + b] = r;
                runs[3 * n_runs + b] = (uint32_t)(h >> 63);
                runs[4 * n_runs + b] = r < n_rows && g >= g0_of[r] ? (uint32_t)(g - g0_of[r]) : 0xFFFFFFFFu;
            }
        }
        if (f & 2u) {
            const uint64_t b = (uint64_t)slot[p + 1] - 1;  // (a tail has its head at or before it: slot[p + 1] >= 1)
            if (slot[p + 1] >= 1 && b < n_runs) runs[n_runs + b] = (uint32_t)p;
        }
    }
}

__global__ void k_loc_close(uint32_t *__restrict__ runs, uint64_t n_runs, const uint64_t *__restrict__ rec_start, const uint64_t *__restrict__ rec_len, uint32_t n_rec,
                            unsigned long long *__restrict__ recs)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n_runs; b += stride) {
        const uint32_t q_first = runs[b], q_last = runs[n_runs + b];
        runs[n_runs + b] = q_last >= q_first ? q_last - q_first + 1 : 0u;
        uint64_t end;
        const int64_t rec = loc_record(rec_start, rec_len, n_rec, q_first, end);
        if (rec >= 0) atomicAdd(&recs[3 * (uint64_t)n_rec + rec], 1ull);
    }
}

int loc_text_ok(tpc_ctx *c, const char *noun)
{
    if (c->text_windowed) return fail(c, -1, "segment %s: this context holds only its window of the text", noun);
    if (!c->bases || !c->nmask || c->bases != c->seg.text_bases || c->n_text != c->seg.text_n || c->text_uploads != c->seg.text_uploads)
        return fail(c, -1, "segment %s: the text of tpc_seq_upload the table was built over is no longer resident", noun);
    return 0;
}

uint64_t loc_grid(tpc_ctx *c, uint64_t n_tiles)
{
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n_cu <= 0) { (void)hipGetLastError(); n_cu = 256; }
    return std::max<uint64_t>(1, std::min<uint64_t>(n_tiles, c->opt_locate_grid > 0 ? (uint64_t)c->opt_locate_grid : (uint64_t)n_cu * LOC_WG_PER_CU));
}

int edg_needs(tpc_ctx *c, const char *noun)
{
    if (!c->edg.valid) return fail(c, -1, "segment %s: tpc_segments_edges_build first", noun);
    return 0;
}

int loc_needs(tpc_ctx *c)
{
    if (!c->loc.valid) return fail(c, -1, "segment locate: tpc_segments_locate first");
    return 0;
}

}  // namespace

extern "C" {

int tpc_segments_edges_build(tpc_ctx *c)
{
    if (!c) return -1;
    edges_drop(c);
    if (int rc = stage_needs_segments(c, "edges", "index")) return rc;
    if (int rc = loc_text_ok(c, "edges")) return rc;
    const int k = c->seg.k, n = k + 1;
    if (n / 32 + 2 > TPC_XW_MAX)
        return fail(c, -1, "segment edges: k=%d is too large: a window of k + 1 letters must fit the %d halo words of a tile (k <= %d)", k, TPC_XW_MAX, (TPC_XW_MAX - 1) * 32 - 2);
    if (c->n_text >= (1ull << 40)) return fail(c, -1, "segment edges: a text of %llu positions, a slot holds positions below 2^40", (unsigned long long)c->n_text);
    if (c->opt_edges_slots_log2 < 0 || c->opt_edges_slots_log2 > 40) return fail(c, -1, "segment edges: option test_edges_slots_log2 = %d is not in 0 .. 40", c->opt_edges_slots_log2);
    if (c->opt_edges_hash_bits < 0 || c->opt_edges_hash_bits > 64) return fail(c, -1, "segment edges: option test_edges_hash_bits = %d is not in 0 .. 64", c->opt_edges_hash_bits);
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n_rec = c->seg.n_rec;
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != c->seg.events) return fail(c, -1, "segment edges: the stream holds events of more sequences than the %u given", n_rec);

    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments, span_words = c->n_words_alloc;
    // sizes in 64 bits, summed before the first allocation; the table is sized by the count in the middle and checked again there
    const uint64_t span_bytes = span_words * 4, g0_bytes = n_rows * 8 + 16, keys_bytes = n_rows * 8 + 16, vals_bytes = n_rows * 4 + 16, counter_bytes = LC_WORDS * 8;
    unsigned long long *keys = nullptr, *sorted = nullptr, *counters = nullptr;
    uint32_t *vals = nullptr, *sorted_vals = nullptr, *span = nullptr;
    uint64_t *d_tab = nullptr;   // the hash constants, read by the tile kernels from device memory
    size_t sort_bytes = 0;
    SegRows idx;
    if (!idx.size(c) || rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, sorted, vals, sorted_vals, n_rows, 0, 41, c->stream) != hipSuccess)
        return fail(c, -10, "segment edges: the scan and the sort could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, sort_bytes);   // one scratch for the scan and the sort
    const uint64_t need = span_bytes + g0_bytes + 2 * keys_bytes + 2 * vals_bytes + counter_bytes + sizeof(SketchTab) + idx.bytes();
    if (int rc = stage_fits(c, "edges", need, "%llu of them the span mask over %llu positions, %llu the spans of %llu rows and their sort", (unsigned long long)span_bytes,
                            (unsigned long long)c->n_text, (unsigned long long)(g0_bytes + 2 * keys_bytes + 2 * vals_bytes), (unsigned long long)n_rows))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) edges_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->edg.g0, g0_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &span, span_bytes + 16) || !temps.get(c, &keys, keys_bytes) ||
        !temps.get(c, &sorted, keys_bytes) || !temps.get(c, &vals, vals_bytes) || !temps.get(c, &sorted_vals, vals_bytes) || !temps.get(c, &counters, counter_bytes) || !temps.get(c, &d_tab, sizeof(SketchTab)))
        return done(fail(c, -10, "segment edges: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    hipStream_t s = c->stream;
    const SketchTab tab = tpc_edge_tab(n);
    const uint64_t hash_mask = c->opt_edges_hash_bits > 0 && c->opt_edges_hash_bits < 64 ? (1ull << c->opt_edges_hash_bits) - 1 : ~0ull;
    const uint64_t grid = loc_grid(c, c->n_tiles);
    const LocQuery none{};
    unsigned long long host[LC_WORDS] = {};
    bool ok = hipMemsetAsync(span, 0, span_bytes + 16, s) == hipSuccess && hipMemsetAsync(counters, 0, counter_bytes, s) == hipSuccess &&
              hipMemsetAsync(c->edg.g0, 0, g0_bytes, s) == hipSuccess && hipMemsetAsync(keys, 0xFF, keys_bytes, s) == hipSuccess && idx.fill(s) &&
              hipMemcpyAsync(d_tab, &tab, sizeof tab, hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok) {
        Timed t(c, TPC_K_LOCATE);   // the whole build on the stream, the wait for the count included
        ok = idx.enqueue(c);
        if (ok && n_events)
            hipLaunchKernelGGL(k_loc_span, dim3(col_grid(n_events)), dim3(256), 0, s, c->seg.first, idx.rank, n_events, n_rows, c->seg.ev[0], c->seg.ev[1], c->seg.ev[2], n_rec,
                               c->seg.rec, c->seg.rec + n_rec, c->n_text, span, span_words, c->edg.g0, keys, vals, counters);
        if (ok && n_rows) ok = rocprim::radix_sort_pairs(idx.scan_tmp, sort_bytes, keys, sorted, vals, sorted_vals, n_rows, 0, 41, s) == hipSuccess;
        if (ok && c->n_text >= (uint64_t)n)
            hipLaunchKernelGGL(k_loc_tile<LOC_COUNT>, dim3((uint32_t)grid), dim3(TPC_TILE_THREADS), 0, s, d_tab, n, c->bases, c->nmask, c->n_text, (uint32_t)c->n_tiles, span, (LocSlot *)nullptr,
                               (uint64_t)0, hash_mask, counters, none);
        ok = ok && idx.total(s) && hipMemcpyAsync(host, counters, counter_bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "edges", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment edges: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (host[LC_BAD]) return done(fail(c, -10, "segment edges: %llu first events lie outside their sequence", host[LC_BAD]));
        const uint64_t keys_in = host[LC_ENTRIES], skipped = host[LC_SKIPPED];
        if (keys_in > c->n_text) return done(fail(c, -10, "segment edges: %llu edges over a text of %llu positions", (unsigned long long)keys_in, (unsigned long long)c->n_text));
        int log2 = c->opt_edges_slots_log2;
        if (!log2) { log2 = 4; while (log2 < 41 && (1ull << log2) < 2 * keys_in) log2++; }   // a load factor of at most 0.5
        const uint64_t n_slots = 1ull << log2, slot_bytes = n_slots * sizeof(LocSlot);
        if (int rc = stage_fits(c, "edges", slot_bytes, "the table of 2^%d slots for %llu edges", log2, (unsigned long long)keys_in)) return done(rc);
        if (dev_malloc(c, &c->edg.slots, slot_bytes) != hipSuccess) return done(fail(c, -10, "segment edges: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        LocSlot *slots = (LocSlot *)c->edg.slots;
        ok = hipMemsetAsync(slots, 0xFF, slot_bytes, s) == hipSuccess && hipMemsetAsync(counters, 0, counter_bytes, s) == hipSuccess;
        if (ok && keys_in) {
            hipLaunchKernelGGL(k_loc_tile<LOC_INSERT>, dim3((uint32_t)grid), dim3(TPC_TILE_THREADS), 0, s, d_tab, n, c->bases, c->nmask, c->n_text, (uint32_t)c->n_tiles, span, slots, n_slots - 1,
                               hash_mask, counters, none);
            hipLaunchKernelGGL(k_loc_rows, dim3(col_grid(n_slots)), dim3(256), 0, s, slots, n_slots, sorted, sorted_vals, n_rows, counters);
        }
        ok = ok && hipMemcpyAsync(host, counters, counter_bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "edges", ok)) return done(rc);
        if (host[LC_FULL])
            return done(fail(c, -1, "segment edges: the table of 2^%d slots is full, %llu of %llu edges found no slot", log2, host[LC_FULL], (unsigned long long)keys_in));
        if (host[LC_BAD]) return done(fail(c, -10, "segment edges: %llu slots hold a position outside every span", host[LC_BAD]));
        if (host[LC_ENTRIES] + host[LC_DUPLICATES] != keys_in)
            return done(fail(c, -10, "segment edges: %llu entries and %llu duplicates of %llu edges", host[LC_ENTRIES], host[LC_DUPLICATES], (unsigned long long)keys_in));
        c->edg.n_slots = n_slots; c->edg.n_rows = n_rows; c->edg.entries = host[LC_ENTRIES]; c->edg.duplicates = host[LC_DUPLICATES]; c->edg.skipped = skipped;
        c->edg.longest_probe = host[LC_PROBE]; c->edg.peak_bytes = need + slot_bytes; c->edg.hash_mask = hash_mask; c->edg.text_uploads = c->text_uploads;
    }
    if (!ok) return done(stage_wait(c, "edges", false));   // the fills could not be enqueued: nothing was built
    c->edg.valid = true;
    return 0;
}

int tpc_segments_edges_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = edg_needs(c, "edges")) return rc;
    if (!info) return fail(c, -1, "segment edges: info required");
    info[0] = c->edg.entries; info[1] = c->edg.duplicates; info[2] = c->edg.skipped; info[3] = c->edg.n_slots; info[4] = c->edg.longest_probe; info[5] = c->edg.peak_bytes;
    return 0;
}

int tpc_segments_locate(tpc_ctx *c, const uint64_t *q_bases, const uint32_t *q_nmask, uint64_t n_q_text, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec)
{
    if (!c) return -1;
    locate_drop(c);
    if (int rc = edg_needs(c, "locate")) return rc;
    if (int rc = stage_needs_segments(c, "locate", "look up")) return rc;
    if (int rc = loc_text_ok(c, "locate")) return rc;
    if (c->edg.text_uploads != c->text_uploads) return fail(c, -1, "segment locate: the text of tpc_seq_upload the table was built over is no longer resident");
    if (!q_bases || !q_nmask || n_q_text < 2) return fail(c, -1, "segment locate: a packed query text is required");
    if (!((q_nmask[0] & 1u) && ((q_nmask[(n_q_text - 1) >> 5] >> ((n_q_text - 1) & 31)) & 1u))) return fail(c, -1, "segment locate: the query text must start and end with the N separator");
    if (n_rec && (!rec_start || !rec_len)) return fail(c, -1, "segment locate: the query's records are required");
    for (uint32_t r = 0; r < n_rec; r++) {
        if (rec_start[r] > n_q_text || rec_len[r] > n_q_text - rec_start[r]) return fail(c, -1, "segment locate: query record %u lies outside the query text", r);
        if (r && rec_start[r] < rec_start[r - 1] + rec_len[r - 1]) return fail(c, -1, "segment locate: the query's records must ascend and not overlap");
    }
    const int n = c->seg.k + 1;
    const uint64_t positions = n_q_text >= (uint64_t)n ? n_q_text - n + 1 : 0;
    if (positions >= 0xFFFFFFFEull) return fail(c, -1, "segment locate: %llu positions, a run holds positions below 2^32 - 2: cut the query into batches", (unsigned long long)positions);
    HIPCHK(c, hipSetDevice(c->device));
    const bool colored = c->col.valid && c->col.n_rows == c->edg.n_rows && c->col.presence;
    const uint32_t n_colors = colored ? c->col.n_colors : 0u;
    const uint64_t nw = (n_q_text + 31) / 32, tiles = (nw + TPC_TILE_THREADS - 1) / TPC_TILE_THREADS;
    const uint64_t alloc = ((n_q_text / TPC_RUN + 512) / 512) * 512 + TPC_XW_MAX + 2;   // as tpc_seq_upload pads T
    // sizes in 64 bits, summed before the first allocation; the runs are not counted yet: at most one per position
    const uint64_t text_bytes = alloc * 12, rec_bytes = 2 * (uint64_t)n_rec * 8 + 16, hit_bytes = positions * 8 + 16, row_bytes = positions * 4 + 16;
    const uint64_t flag_bytes = (positions + 1) * 4 + 16, recs_bytes = 4 * (uint64_t)n_rec * 8 + 16, runs_bound = positions * 20 + 16;
    if (n_colors && (uint64_t)n_rec > (~0ull >> 4) / n_colors) return fail(c, -20, "segment locate: %u records of %u colours do not fit the free device memory", n_rec, n_colors);
    const uint64_t shared_bytes = colored ? (uint64_t)n_rec * n_colors * 8 + 16 : 0;
    size_t scan_bytes = 0;
    uint32_t *flags = nullptr, *heads = nullptr;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, heads, heads, 0u, positions + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess)
        return fail(c, -10, "segment locate: the scan could not be sized");
    const uint64_t need = text_bytes + rec_bytes + hit_bytes + row_bytes + 2 * flag_bytes + recs_bytes + runs_bound + shared_bytes + scan_bytes + sizeof(SketchTab) + 16;
    if (int rc = stage_fits(c, "locate", need, "%llu of them the hits, rows, flags and runs of %llu positions, %llu the sums of %u records in %u colours",
                            (unsigned long long)(hit_bytes + row_bytes + 2 * flag_bytes + runs_bound), (unsigned long long)positions, (unsigned long long)(recs_bytes + shared_bytes), n_rec,
                            n_colors))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) locate_drop(c);
        return code;
    };
    uint64_t *d_bases = nullptr, *d_rec = nullptr, *d_tab = nullptr;
    uint32_t *d_nmask = nullptr;
    void *scan_tmp = nullptr;
    if (dev_malloc(c, (void **)&c->loc.hit, hit_bytes) != hipSuccess || dev_malloc(c, (void **)&c->loc.row, row_bytes) != hipSuccess ||
        dev_malloc(c, (void **)&c->loc.recs, recs_bytes) != hipSuccess || (colored && dev_malloc(c, (void **)&c->loc.shared, shared_bytes) != hipSuccess) ||
        !temps.get(c, &d_bases, alloc * 8) || !temps.get(c, &d_nmask, alloc * 4) || !temps.get(c, &d_rec, rec_bytes) || !temps.get(c, &d_tab, sizeof(SketchTab)) || !temps.get(c, &flags, flag_bytes) ||
        !temps.get(c, &heads, flag_bytes) || !temps.get(c, &scan_tmp, scan_bytes + 16))
        return done(fail(c, -10, "segment locate: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    hipStream_t s = c->stream;
    uint32_t last_word = 0;
    const SketchTab tab = tpc_edge_tab(n);
    bool ok = hipMemcpyAsync(d_tab, &tab, sizeof tab, hipMemcpyHostToDevice, s) == hipSuccess && hipMemsetAsync(d_bases, 0, alloc * 8, s) == hipSuccess && hipMemsetAsync(d_nmask, 0xFF, alloc * 4, s) == hipSuccess &&   // padding = N
              hipMemcpyAsync(d_bases, q_bases, nw * 8, hipMemcpyHostToDevice, s) == hipSuccess && hipMemcpyAsync(d_nmask, q_nmask, nw * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
              hipMemsetAsync(c->loc.recs, 0, recs_bytes, s) == hipSuccess && (!colored || hipMemsetAsync(c->loc.shared, 0, shared_bytes, s) == hipSuccess);
    if (ok && (n_q_text & 31)) {   // the bits of the last word past the text are N
        last_word = q_nmask[nw - 1] | (~0u << (n_q_text & 31));
        ok = hipMemcpyAsync(d_nmask + (nw - 1), &last_word, sizeof last_word, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    if (ok && n_rec)
        ok = hipMemcpyAsync(d_rec, rec_start, (size_t)n_rec * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
             hipMemcpyAsync(d_rec + n_rec, rec_len, (size_t)n_rec * 8, hipMemcpyHostToDevice, s) == hipSuccess;
    LocQuery q{};
    q.t_bases = c->bases; q.n_text = c->n_text; q.n_rows = c->edg.n_rows; q.positions = positions;
    q.rec_start = d_rec; q.rec_len = d_rec + n_rec; q.n_rec = n_rec;
    q.presence = colored ? c->col.presence : nullptr; q.words = colored ? c->col.words : 0u; q.n_colors = n_colors;
    q.hit = c->loc.hit; q.row = c->loc.row; q.recs = c->loc.recs; q.shared = c->loc.shared;
    uint32_t n_runs = 0;
    if (ok) {
        Timed t(c, TPC_K_LOCATE);   // the whole call on the stream, the wait for the run count included
        if (positions)
            hipLaunchKernelGGL(k_loc_tile<LOC_PROBE>, dim3((uint32_t)loc_grid(c, tiles)), dim3(TPC_TILE_THREADS), 0, s, d_tab, n, d_bases, d_nmask, n_q_text, (uint32_t)tiles,
                               (const uint32_t *)nullptr, (LocSlot *)c->edg.slots, c->edg.n_slots - 1, c->edg.hash_mask, (unsigned long long *)nullptr, q);
        if (positions) hipLaunchKernelGGL(k_loc_fold, dim3(col_grid((positions + TPC_RUN - 1) / TPC_RUN)), dim3(256), 0, s, q);
        hipLaunchKernelGGL(k_loc_heads, dim3(col_grid(positions + 1)), dim3(256), 0, s, c->loc.hit, c->loc.row, positions, flags, heads);
        ok = rocprim::exclusive_scan(scan_tmp, scan_bytes, heads, heads, 0u, positions + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        ok = ok && hipMemcpyAsync(&n_runs, heads + positions, sizeof n_runs, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "locate", ok)) return done(rc);
        if (n_runs > positions) return done(fail(c, -10, "segment locate: %u runs over %llu positions", n_runs, (unsigned long long)positions));
        const uint64_t runs_bytes = (uint64_t)n_runs * 20 + 16;
        if (dev_malloc(c, (void **)&c->loc.runs, runs_bytes) != hipSuccess) return done(fail(c, -10, "segment locate: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->loc.runs, 0xFF, runs_bytes, s) == hipSuccess;
        if (ok && n_runs) {
            hipLaunchKernelGGL(k_loc_place, dim3(col_grid(positions)), dim3(256), 0, s, c->loc.hit, c->loc.row, positions, flags, heads, c->edg.g0, c->edg.n_rows, c->loc.runs,
                               (uint64_t)n_runs);
            hipLaunchKernelGGL(k_loc_close, dim3(col_grid(n_runs)), dim3(256), 0, s, c->loc.runs, (uint64_t)n_runs, q.rec_start, q.rec_len, n_rec, c->loc.recs);
        }
        c->loc.peak_bytes = need - runs_bound + runs_bytes;
    }
    if (int rc = stage_wait(c, "locate", ok)) return done(rc);
    std::vector<unsigned long long> sums(2 * (size_t)n_rec);
    if (n_rec) HIPCHK(c, hipMemcpy(sums.data(), c->loc.recs, sums.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < n_rec; r++) { c->loc.windows += sums[r]; c->loc.found += sums[(size_t)n_rec + r]; }
    c->loc.positions = positions; c->loc.n_runs = n_runs; c->loc.n_rec = n_rec; c->loc.n_colors = n_colors;
    c->loc.valid = true;
    return 0;
}

int tpc_segments_locate_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (int rc = loc_needs(c)) return rc;
    if (!info) return fail(c, -1, "segment locate: info required");
    info[0] = c->loc.positions; info[1] = c->loc.windows; info[2] = c->loc.found; info[3] = c->loc.n_runs; info[4] = c->loc.n_colors; info[5] = c->loc.peak_bytes;
    return 0;
}

int tpc_segments_locate_fetch_hits(tpc_ctx *c, uint64_t p0, uint64_t n, uint64_t *hit_host, uint32_t *row_host)
{
    if (!c) return -1;
    if (int rc = loc_needs(c)) return rc;
    if ((n && (!hit_host || !row_host)) || p0 > c->loc.positions || n > c->loc.positions - p0)
        return fail(c, -1, "segment locate: bad position range (%llu positions at %llu of %llu)", (unsigned long long)n, (unsigned long long)p0, (unsigned long long)c->loc.positions);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) {
        HIPCHK(c, hipMemcpy(hit_host, c->loc.hit + p0, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(row_host, c->loc.row + p0, n * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

int tpc_segments_locate_fetch_runs(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *q_first, uint32_t *length, uint32_t *row, uint32_t *rev, uint32_t *off_first)
{
    if (!c) return -1;
    if (int rc = loc_needs(c)) return rc;
    return fetch_planes(c, "locate", "run", c->loc.runs, c->loc.n_runs, r0, n, { q_first, length, row, rev, off_first });
}

int tpc_segments_locate_fetch_records(tpc_ctx *c, uint64_t s0, uint64_t n, uint64_t *windows, uint64_t *found, uint64_t *forward, uint64_t *runs)
{
    if (!c) return -1;
    if (int rc = loc_needs(c)) return rc;
    const uint64_t n_rec = c->loc.n_rec;
    if ((n && (!windows || !found || !forward || !runs)) || s0 > n_rec || n > n_rec - s0)
        return fail(c, -1, "segment locate: bad record range (%llu records at %llu of %llu)", (unsigned long long)n, (unsigned long long)s0, (unsigned long long)n_rec);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t *dst[4] = {windows, found, forward, runs};
    for (int i = 0; i < 4 && n; i++) HIPCHK(c, hipMemcpy(dst[i], c->loc.recs + (size_t)i * n_rec + s0, n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_locate_fetch_shared(tpc_ctx *c, uint64_t s0, uint64_t n, uint64_t *counts_host)
{
    if (!c) return -1;
    if (int rc = loc_needs(c)) return rc;
    if (!c->loc.shared) return fail(c, -1, "segment locate: no colour table was valid at the time of the locate, there are no shared counts");
    const uint64_t n_rec = c->loc.n_rec;
    if ((n && !counts_host) || s0 > n_rec || n > n_rec - s0)
        return fail(c, -1, "segment locate: bad record range (%llu records at %llu of %llu)", (unsigned long long)n, (unsigned long long)s0, (unsigned long long)n_rec);
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(counts_host, c->loc.shared + s0 * c->loc.n_colors, n * c->loc.n_colors * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
