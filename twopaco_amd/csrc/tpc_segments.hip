// tpc_segments.hip -- the segment table of the compacted graph, built on the device from the junction stream.
//
// Replaces, for graphdump's gfa1 / gfa2 / fasta formats, the serial part of the reference's walk
// (reference src/graphdump/graphdump.cpp:44-113 the segment naming, :398-480 the loop over the junction records;
// restated in twopaco_amd/host/junctiondump.cpp: SegmentNamer::Name, WalkSegments).  The walk reads the stream one
// record at a time because (1) a segment is printed in full at the FIRST sight, in file order, of |name| and (2) segments
// whose deciding character is 'N' take fresh names 2^34, 2^34 + 1, ... in file order.  Here both are a minimum / a scan:
//   k_seg_flags   one thread per 12-byte slot: is it a separator (position OR id field holds the separator value,
//                 junctionapi.h:91), does it close an event (it and the slot before are records: consecutive records
//                 of one sequence).  Exclusive scans give every slot its sequence id (separators before it; 32 bits,
//                 wrapping as the reader's counter does) and every event its index e in file order.
//   k_seg_name    one thread per slot: the walk's checks for the pair (previous record, this record) -- the first failing
//                 pair in file order is kept by an atomicMin over (slot << 2 | kind) -- and name[e] by the reference's
//                 rule; the deciding character is one scattered read of the packed text (bases / nmask word).  A set
//                 nmask bit means "not ACGT"; the sorted list amb[] of text positions holding a valid letter other than
//                 N tells an 'N' (fresh name) from such a letter (MakeUpChar gives -1: the name is -1), by binary search.
//                 An exclusive scan over the 'N' flags numbers the fresh names.
//   k_seg_min     table[|name[e]|] = min(e) with atomicMin on 32-bit entries; 'N'-named events get 2^34 + their rank.
//   k_seg_first   first[e] = 'N'-named or table[|name[e]|] == e, bit-packed by wave ballot; counts the bits.
//   k_seg_events  one thread per slot, from the two scans alone (slot i closes an event when e_of steps behind it, is a separator
//                 when seq_of does): begin[e] / end[e] = the position fields of the event's two records, and
//                 seq_event_begin[s] = events before the s-th separator (the events of sequence s are [seq_event_begin[s],
//                 seq_event_begin[s + 1])) -- the EVENT TABLE, what a formatter needs of the stream beside name[] and first[].
// Memory (B = bytes): stream 12 B / slot (the caller's), scans 8 B / slot, name 8 B + begin 4 B + end 4 B + 'N' rank 4 B + first
// 1 bit per event, seq_event_begin 4 B per input sequence, table 4 B x (largest |name| + 1) <= 32 B x (largest |id| + 1), ids being below 2^31 (an event with a larger one is
// the walk's "A vertex id is too large": it gets the name 0 and does not size the table).  Streams of 2^32 - 1 slots or more are refused (32-bit event
// indices), and so is a table that does not fit the free device memory: an error text, never a fault.
#include "../../include/twopaco_hip.h"
#include "tpc_device.h"
#include "tpc_internal.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdio>

namespace {

constexpr uint64_t SEG_ID_LIMIT = 1ull << 31;    // MAX_JUNCTION_ID, graphdump.cpp:44
constexpr int64_t SEG_FRESH = (int64_t)1 << 34;  // first fresh name, graphdump.cpp:60

__device__ __forceinline__ bool seg_is_sep(const uint32_t *__restrict__ slots, uint64_t i)
{
    const uint32_t *p = slots + i * 3;
    return p[0] == 0xFFFFFFFFu || (p[1] == 0xFFFFFFFFu && p[2] == 0x7FFFFFFFu);
}

__device__ __forceinline__ int64_t seg_id(const uint32_t *__restrict__ slots, uint64_t i)
{
    const uint32_t *p = slots + i * 3;
    return (int64_t)((uint64_t)p[1] | ((uint64_t)p[2] << 32));
}

__device__ __forceinline__ uint64_t seg_mag(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// n + 1 entries each: the scans' last elements are the totals
__global__ void k_seg_flags(const uint32_t *__restrict__ slots, uint64_t n, uint32_t *__restrict__ sep, uint32_t *__restrict__ ev)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) {
        const bool s = i < n && seg_is_sep(slots, i);
        sep[i] = s ? 1u : 0u;
        ev[i] = (i < n && i > 0 && !s && !seg_is_sep(slots, i - 1)) ? 1u : 0u;
    }
}

__device__ __forceinline__ bool seg_in_list(const uint64_t *__restrict__ a, uint64_t n, uint64_t v)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo < n && a[lo] == v;
}

// scal[0] = min over failing pairs of (slot << 2 | kind), scal[1] = largest |name| of an event that is not 'N'-named
__global__ void k_seg_name(const uint32_t *__restrict__ slots, uint64_t n, int k, const uint32_t *__restrict__ seq_of, const uint32_t *__restrict__ e_of,
                           const uint64_t *__restrict__ bases, const uint32_t *__restrict__ nmask, const uint64_t *__restrict__ rec_start,
                           const uint64_t *__restrict__ rec_len, uint32_t n_rec, const uint64_t *__restrict__ amb, uint64_t n_amb,
                           int64_t *__restrict__ name, uint32_t *__restrict__ nflag, uint64_t n_events, unsigned long long *__restrict__ scal)
{
    __shared__ unsigned long long s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    unsigned long long my_max = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (seg_is_sep(slots, i)) continue;
        if (i == 0) continue;  // first record, sequence 0
        if (seg_is_sep(slots, i - 1)) {
            // first record of the stream with a sequence id other than 0, or a sequence id stepping by more than one
            if (i == 1 || seg_is_sep(slots, i - 2)) atomicMin(&scal[0], (unsigned long long)(i << 2 | TPC_SEG_CORRUPTED));
            continue;
        }
        const uint64_t e = e_of[i];
        if (e >= n_events) continue;  // (cannot happen: e_of is the scan of the event flags)
        const uint32_t seq = seq_of[i];
        const uint32_t lp = slots[(i - 1) * 3], rp = slots[i * 3];
        const uint64_t len = seq < n_rec ? rec_len[seq] : 0;  // more sequences in the stream than in the text: empty
        int64_t nm = 0;
        uint32_t fresh = 0;
        if (rp <= lp || (uint64_t)rp + (uint64_t)k > len) {
            atomicMin(&scal[0], (unsigned long long)(i << 2 | TPC_SEG_CORRUPTED));
        } else {
            const int64_t lid = seg_id(slots, i - 1), rid = seg_id(slots, i);
            const uint64_t l = seg_mag(lid), r = seg_mag(rid);
            if (l >= SEG_ID_LIMIT || r >= SEG_ID_LIMIT) {
                atomicMin(&scal[0], (unsigned long long)(i << 2 | TPC_SEG_ID_TOO_LARGE));
            } else {
                const bool forward = l < r || (l == r && l > 0);
                const int64_t start = forward ? lid : -rid;
                // lp + k < rp + k <= len and rp - 1 >= lp >= 0: both inside the sequence
                const uint64_t g = rec_start[seq] + (forward ? (uint64_t)lp + (uint64_t)k : (uint64_t)rp - 1);
                const bool not_acgt = (nmask[g >> 5] >> (g & 31)) & 1u;
                uint32_t code = (uint32_t)(bases[g >> 5] >> (2 * (g & 31))) & 3u;
                if (not_acgt) {
                    // the complement of anything but ACGT is 'N'; read forward, a letter other than N has no code
                    if (forward && n_amb && seg_in_list(amb, n_amb, g)) nm = -1; else fresh = 1;
                } else {
                    if (!forward) code = 3u - code;
                    const int64_t v = (int64_t)code | (start < 0 ? (int64_t)(4ull | (seg_mag(start) << 3)) : (int64_t)((uint64_t)start << 3));
                    nm = start != lid ? -v : v;  // graphdump.cpp:88-91: reverse, but not between two ids of 0 (start = -0 is the left id)
                }
                if (!fresh) my_max = max(my_max, (unsigned long long)seg_mag(nm));
            }
        }
        name[e] = nm;
        nflag[e] = fresh;
    }
    if (my_max) atomicMax(&s_max, my_max);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&scal[1], s_max);
}

__global__ void k_seg_min(int64_t *__restrict__ name, const uint32_t *__restrict__ nflag, const uint32_t *__restrict__ nrank, uint64_t n_events,
                          uint32_t *__restrict__ table, uint64_t n_table)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_events; e += stride) {
        if (nflag[e]) { name[e] = SEG_FRESH + (int64_t)nrank[e]; continue; }
        const uint64_t m = seg_mag(name[e]);
        if (m < n_table) atomicMin(&table[m], (uint32_t)e);
    }
}

// one wave per 64 events: the ballot is two words of first[] (its allocation is a whole number of 64-bit pairs)
__global__ void k_seg_first(const int64_t *__restrict__ name, uint64_t n_events, const uint32_t *__restrict__ table, uint64_t n_table,
                            uint32_t *__restrict__ first, unsigned long long *__restrict__ n_first)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;  // a multiple of 64: every lane of a wave leaves the loop together
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e - lane < n_events; e += stride) {
        bool f = false;
        if (e < n_events) {
            const int64_t nm = name[e];
            const uint64_t m = seg_mag(nm);
            f = nm >= SEG_FRESH || (m < n_table && table[m] == (uint32_t)e);
        }
        const unsigned long long b = __ballot(f);
        if (lane == 0) {
            first[e >> 5] = (uint32_t)b;
            first[(e >> 5) + 1] = (uint32_t)(b >> 32);
            mine += (unsigned long long)__popcll(b);
        }
    }
    if (mine) atomicAdd(n_first, mine);
}

// The event table.  seq_of / e_of: the exclusive scans (n + 1 entries).  The events of one sequence are consecutive, so the
// separator that ends sequence s gives seq_event_begin[s + 1]; entries behind the last separator hold the event count.
__global__ void k_seg_events(const uint32_t *__restrict__ slots, uint64_t n, const uint32_t *__restrict__ seq_of, const uint32_t *__restrict__ e_of,
                             uint32_t *__restrict__ begin, uint32_t *__restrict__ end, uint64_t n_events, uint32_t *__restrict__ seq_begin, uint32_t n_rec)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t n_sep = seq_of[n];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n || i <= n_rec; i += stride) {
        if (i <= n_rec && (i == 0 || i > n_sep)) seq_begin[i] = i == 0 ? 0u : (uint32_t)n_events;
        if (i >= n) continue;
        const uint32_t e = e_of[i], s = seq_of[i];
        if (e_of[i + 1] != e && i > 0 && e < n_events) {  // slot i closes event e
            begin[e] = slots[(i - 1) * 3];
            end[e] = slots[i * 3];
        }
        if (seq_of[i + 1] != s && s < n_rec) seq_begin[s + 1] = e;  // the (s + 1)-th separator: e events lie before it
    }
}

int seg_scan32(hipStream_t s, uint32_t *data, uint64_t n, void *&tmp, size_t &tmp_cap)
{
    size_t need = 0;
    if (rocprim::exclusive_scan(nullptr, need, data, data, 0u, n, rocprim::plus<uint32_t>(), s) != hipSuccess) return -2;
    if (need > tmp_cap) {
        if (tmp) (void)hipFree(tmp);
        tmp = nullptr; tmp_cap = 0;
        if (hipMalloc(&tmp, need) != hipSuccess) return -3;
        tmp_cap = need;
    }
    return rocprim::exclusive_scan(tmp, need, data, data, 0u, n, rocprim::plus<uint32_t>(), s) == hipSuccess ? 0 : -2;
}

unsigned seg_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

bool seg_fits(size_t bytes)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    return bytes + ((size_t)64 << 20) <= free_b;
}

}  // namespace

// slots: n_slots x 12 bytes on the device.  *name_out / *first_out: device arrays of res->events entries / (events + 63) / 64 * 2
// words, the caller's to free; both null when the stream has no event.  ev_out[0] / ev_out[1]: begin[] / end[] (res->events
// entries each, null without events), ev_out[2]: seq_event_begin[] (n_rec + 1 entries, never null); the caller's to free too.  0, or < 0 with a text in err (TPC_SEG_ERR_TEXT bytes).
int tpc_launch_segments(hipStream_t s, const uint32_t *slots, uint64_t n_slots, int k, const uint64_t *bases, const uint32_t *nmask,
                        const uint64_t *d_rec_start, const uint64_t *d_rec_len, uint32_t n_rec, const uint64_t *d_amb, uint64_t n_amb,
                        int64_t **name_out, uint32_t **first_out, uint32_t **ev_out, TpcSegResult *res, char *err)
{
    *name_out = nullptr; *first_out = nullptr;
    ev_out[0] = ev_out[1] = ev_out[2] = nullptr;
    *res = TpcSegResult{};
    err[0] = 0;
    if (n_slots >= 0xFFFFFFFFull) { snprintf(err, TPC_SEG_ERR_TEXT, "segment table: %llu slots, event indices are 32 bits (fewer than 2^32 - 1 slots)", (unsigned long long)n_slots); return -20; }
    uint32_t *seq_of = nullptr, *e_of = nullptr, *nflag = nullptr, *table = nullptr, *first = nullptr, *begin = nullptr, *end = nullptr, *seq_begin = nullptr;
    int64_t *name = nullptr;
    unsigned long long *scal = nullptr;
    void *tmp = nullptr;
    size_t tmp_cap = 0;
    int rc = 0;
    unsigned long long h[3] = { ~0ull, 0ull, 0ull };  // first error, largest |name|, first bits set
    uint32_t n_events = 0, n_named = 0;
    auto done = [&](int code) {
        for (void *p : { (void *)seq_of, (void *)e_of, (void *)nflag, (void *)table, (void *)scal, tmp }) if (p) (void)hipFree(p);
        if (code) { for (void *p : { (void *)name, (void *)first, (void *)begin, (void *)end, (void *)seq_begin }) if (p) (void)hipFree(p); }
        return code;
    };
    const size_t scan_bytes = (size_t)(n_slots + 1) * sizeof(uint32_t);
    if (!seg_fits(2 * scan_bytes)) { snprintf(err, TPC_SEG_ERR_TEXT, "segment table: %zu bytes of scan scratch do not fit the free device memory", 2 * scan_bytes); return -20; }
    if (hipMalloc((void **)&seq_of, scan_bytes) != hipSuccess || hipMalloc((void **)&e_of, scan_bytes) != hipSuccess ||
        hipMalloc((void **)&scal, sizeof h) != hipSuccess) return done(-10);
    hipLaunchKernelGGL(k_seg_flags, dim3(seg_grid(n_slots + 1)), dim3(256), 0, s, slots, n_slots, seq_of, e_of);
    if ((rc = seg_scan32(s, seq_of, n_slots + 1, tmp, tmp_cap)) || (rc = seg_scan32(s, e_of, n_slots + 1, tmp, tmp_cap))) return done(rc);
    if (hipMemcpyAsync(&n_events, e_of + n_slots, sizeof n_events, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(scal, h, sizeof h, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(-10);
    const uint64_t first_words = ((uint64_t)n_events + 63) / 64 * 2;
    const size_t ev_bytes = (size_t)n_events * 16 + ((size_t)n_events + 1) * 4 + first_words * 4 + ((size_t)n_rec + 1) * 4;
    if (!seg_fits(ev_bytes)) {
        snprintf(err, TPC_SEG_ERR_TEXT, "segment table: %zu bytes for %u events and %u sequences do not fit the free device memory", ev_bytes, n_events, n_rec);
        return done(-20);
    }
    if (hipMalloc((void **)&nflag, ((size_t)n_events + 1) * 4) != hipSuccess || hipMalloc((void **)&seq_begin, ((size_t)n_rec + 1) * 4) != hipSuccess) return done(-10);
    if (n_events && (hipMalloc((void **)&name, (size_t)n_events * 8) != hipSuccess || hipMalloc((void **)&first, first_words * 4) != hipSuccess ||
                     hipMalloc((void **)&begin, (size_t)n_events * 4) != hipSuccess || hipMalloc((void **)&end, (size_t)n_events * 4) != hipSuccess)) return done(-10);
    if (hipMemsetAsync(nflag + n_events, 0, 4, s) != hipSuccess || (first && hipMemsetAsync(first, 0, first_words * 4, s) != hipSuccess)) return done(-10);
    if (n_slots)
        hipLaunchKernelGGL(k_seg_name, dim3(seg_grid(n_slots)), dim3(256), 0, s, slots, n_slots, k, seq_of, e_of, bases, nmask, d_rec_start, d_rec_len, n_rec,
                           d_amb, n_amb, name, nflag, (uint64_t)n_events, scal);
    // before e_of is reused for the 'N' ranks below
    hipLaunchKernelGGL(k_seg_events, dim3(seg_grid(std::max<uint64_t>(n_slots, (uint64_t)n_rec + 1))), dim3(256), 0, s, slots, n_slots, seq_of, e_of, begin, end,
                       (uint64_t)n_events, seq_begin, n_rec);
    if (hipMemcpyAsync(h, scal, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(-10);
    res->events = n_events;
    res->err_slot = 0; res->err_kind = TPC_SEG_OK;
    if (h[0] != ~0ull) { res->err_slot = h[0] >> 2; res->err_kind = (int)(h[0] & 3); }
    if (n_events) {  // also after an error: only the events that fail their own checks (name 0) are not what the rule gives
        // nflag is read by k_seg_min as the flag AND as the rank: scan a copy (e_of's first n_events + 1 entries are free now)
        uint32_t *nrank = e_of;
        if (hipMemcpyAsync(nrank, nflag, ((size_t)n_events + 1) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return done(-10);
        if ((rc = seg_scan32(s, nrank, (uint64_t)n_events + 1, tmp, tmp_cap))) return done(rc);
        if (hipMemcpyAsync(&n_named, nrank + n_events, sizeof n_named, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(-10);
        const uint64_t n_table = h[1] + 1;  // |name| < 8 * (largest |id| + 1) <= 2^34
        const size_t table_bytes = (size_t)n_table * sizeof(uint32_t);
        if (!seg_fits(table_bytes)) {
            snprintf(err, TPC_SEG_ERR_TEXT, "segment table: the first-sight table of %zu bytes (largest segment name %llu) does not fit the free device memory", table_bytes, h[1]);
            return done(-20);
        }
        if (hipMalloc((void **)&table, table_bytes) != hipSuccess) return done(-10);
        if (hipMemsetAsync(table, 0xFF, table_bytes, s) != hipSuccess) return done(-10);
        hipLaunchKernelGGL(k_seg_min, dim3(seg_grid(n_events)), dim3(256), 0, s, name, nflag, nrank, (uint64_t)n_events, table, n_table);
        hipLaunchKernelGGL(k_seg_first, dim3(seg_grid(n_events)), dim3(256), 0, s, name, (uint64_t)n_events, table, n_table, first, scal + 2);
        if (hipMemcpyAsync(h, scal, sizeof h, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(-10);
        res->segments = h[2];
        res->named = n_named;
        res->table_bytes = table_bytes;
    }
    if (hipGetLastError() != hipSuccess) return done(-10);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) res->peak_bytes = total_b - free_b;
    *name_out = name; *first_out = first;
    ev_out[0] = begin; ev_out[1] = end; ev_out[2] = seq_begin;
    return done(0);
}
