// tpc_segtext.hip -- the text of the compacted graph (gfa1 / gfa2 / fasta) rendered on the device from the event table of
// tpc_segments.hip and the packed letters of tpc_seq_upload.
//
// The text is, byte for byte, what the sinks of twopaco_amd/host/graphformat.h (Gfa1Sink, Gfa2Sink, FastaSink fed by
// FormatChunk) write for the table, in file order; the header lines stay on the host.  Event e of sequence s, size = end + k -
// begin, owns in this order: the segment line when first[e] (S, or ">id" and the body wrapped at 80 letters), the occurrence
// line (C / F), the link line (L / E) when e is not the first event of s and the event before it is not named 0 (the sinks'
// prevId_ != 0: 0 is the walk's "no segment yet"), and the path line (P / O) of s when e is its last.
//   k_text_size     one thread per event: off[e] = bytes of its lines but the path line -- widths are computed (digit counts of
//                   64-bit values), nothing is printed -- and piece[e] = bytes of its piece of the path line (digits of |name|,
//                   the strand, one separator or terminator byte).  Sizes and bytes come from ONE template (emit_lines) run
//                   with a counting or a storing emitter, so they cannot disagree.
//   scan            piece[] exclusive, 64 bits (rocPRIM)
//   k_text_addpath  one thread per sequence: the path line (head + the sequence's pieces + tail) is added to its last event
//   scan            off[] exclusive: off[e] = where event e begins in the whole text, off[n_events] = the text's size
//   k_text_render   a byte window [byte0, byte0 + n) of the text into a device buffer.  Work is cut by OUTPUT BYTES: a workgroup
//                   owns one tile of TPC_TEXT_TILE bytes, finds the events that meet it by binary search in off[], builds the
//                   tile in LDS and stores it with 16-byte vector stores, lane i at base + 16 i.  Three phases fill a tile:
//                   (1) short lines, one thread per event, every byte clipped against the tile (the cost is that of the
//                   event's names and numbers: a body is skipped by adding its length); (2) body letters and (3) path-line
//                   bytes, one thread per BYTE of the tile: the byte finds its event in off[], its letter in the 2-bit text
//                   (forward: a set nmask bit is 'N' unless the position is in the sorted ambiguity list, whose letter is then
//                   amb_letter[]; reverse, name <= 0: read backwards, complemented, anything but ACGT is 'N') or its piece in
//                   piece[] by binary search.  So a 100-Mbp body or a path line of a million events is spread over as many
//                   workgroups as it has tiles, and no thread's work grows with the length of a body or of a path.  A window
//                   may begin or end anywhere: inside a number, a body or a path line.
// Memory: 16 B per event (off[], piece[]) beside the table; a window buffer is the caller's.  Stores are plain C++.
#include "../../include/twopaco_hip.h"
#include "tpc_device.h"
#include "tpc_internal.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdio>

namespace {

__device__ const uint64_t TEXT_P10[20] = {
    1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull, 100000000000ull,
    1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
    1000000000000000000ull, 10000000000000000000ull };

__device__ __forceinline__ uint32_t text_digits(uint64_t v)
{
    uint32_t d = 1;
    while (d < 20 && v >= TEXT_P10[d]) d++;
    return d;
}

__device__ __forceinline__ char text_digit(uint64_t v, uint32_t d, uint32_t i) { return (char)('0' + (v / TEXT_P10[d - 1 - i]) % 10); }

__device__ __forceinline__ uint64_t text_mag(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

// the last index i in [lo, hi] with a[i] <= v (a ascends, a[lo] <= v)
template <typename T> __device__ __forceinline__ uint64_t text_last_le(const T *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if ((uint64_t)a[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the sequence that holds event e: the last s with seq_begin[s] <= e (sequences without events share their entry with the next)
__device__ __forceinline__ uint32_t text_seq_of(const TpcTextPlan &T, uint64_t e) { return (uint32_t)text_last_le(T.seq_begin, 0, T.n_rec, e); }

struct TextEvent {
    int64_t nm, prev_nm;
    uint64_t m, size, prev_size;
    uint32_t b, en, s;
    bool first, link, last;
};

__device__ __forceinline__ void text_load(const TpcTextPlan &T, uint64_t e, TextEvent &ev)
{
    ev.nm = T.name[e]; ev.m = text_mag(ev.nm);
    ev.b = T.begin[e]; ev.en = T.end[e];
    ev.size = (uint64_t)ev.en + (uint64_t)T.k - ev.b;
    ev.first = (T.first[e >> 5] >> (e & 31)) & 1u;
    ev.s = text_seq_of(T, e);
    ev.link = false;
    ev.last = e + 1 == T.seq_begin[ev.s + 1];
    ev.prev_nm = 0; ev.prev_size = 0;
    if (e > T.seq_begin[ev.s]) {
        // GfaSink::Segment prints the link only `if (prevId_ != 0)`: a name of 0 is the walk's "no segment yet"
        ev.prev_nm = T.name[e - 1]; ev.prev_size = (uint64_t)T.end[e - 1] + (uint64_t)T.k - T.begin[e - 1];
        ev.link = ev.prev_nm != 0;
    }
}

__device__ __forceinline__ uint64_t text_body_bytes(int format, uint64_t size) { return format == TPC_TEXT_FASTA ? size + (size + 79) / 80 : size; }

// widths only
struct CountEmitter {
    uint64_t pos = 0, body_at = 0;
    __device__ void ch(char) { pos++; }
    __device__ void num(uint64_t v) { pos += text_digits(v); }
    __device__ void str(const char *, uint64_t n) { pos += n; }
    __device__ void body(uint64_t n) { body_at = pos; pos += n; }
};

// bytes into the tile [t0, t1) held in LDS, everything outside dropped
struct TileEmitter {
    uint64_t pos, t0, t1;
    uint8_t *tile;
    __device__ void ch(char c) { if (pos >= t0 && pos < t1) tile[pos - t0] = (uint8_t)c; pos++; }
    __device__ void num(uint64_t v)
    {
        const uint32_t d = text_digits(v);
        if (pos + d <= t0 || pos >= t1) { pos += d; return; }
        for (uint32_t i = 0; i < d; i++) ch(text_digit(v, d, i));
    }
    __device__ void str(const char *p, uint64_t n)
    {
        if (pos + n <= t0 || pos >= t1) { pos += n; return; }
        for (uint64_t i = 0; i < n; i++) ch(p[i]);
    }
    __device__ void body(uint64_t n) { pos += n; }
};

// Gfa2Sink::At
template <class Em> __device__ __forceinline__ void text_at(Em &em, uint64_t pos, uint64_t length)
{
    em.num(pos);
    if (pos == length) em.ch('$');
}

// the lines of one event but the path line: Gfa1Sink / Gfa2Sink / FastaSink, SegmentLine + Occurrence + Link
template <class Em> __device__ void emit_lines(const TpcTextPlan &T, const TextEvent &ev, Em &em)
{
    const uint64_t k = (uint64_t)T.k;
    const char strand = ev.nm >= 0 ? '+' : '-';
    if (T.format == TPC_TEXT_FASTA) {
        if (!ev.first) return;
        em.ch('>'); em.num(ev.m); em.ch('\n');
        em.body(text_body_bytes(T.format, ev.size));
        return;
    }
    const char *sn = T.seq_names + T.seq_name_off[ev.s];
    const uint64_t snl = T.seq_name_off[ev.s + 1] - T.seq_name_off[ev.s];
    if (T.format == TPC_TEXT_GFA1) {
        if (ev.first) { em.ch('S'); em.ch('\t'); em.num(ev.m); em.ch('\t'); em.body(ev.size); em.ch('\n'); }
        em.ch('C'); em.ch('\t'); em.num(ev.m); em.ch('\t'); em.ch(strand); em.ch('\t'); em.str(sn, snl); em.ch('\t'); em.ch('+'); em.ch('\t'); em.num(ev.en); em.ch('\n');
        if (ev.link) {
            em.ch('L'); em.ch('\t'); em.num(text_mag(ev.prev_nm)); em.ch('\t'); em.ch(ev.prev_nm >= 0 ? '+' : '-'); em.ch('\t'); em.num(ev.m); em.ch('\t'); em.ch(strand);
            em.ch('\t'); em.num(k); em.ch('M'); em.ch('\n');
        }
        return;
    }
    const uint64_t total = T.rec_len[ev.s];
    if (ev.first) { em.ch('S'); em.ch('\t'); em.num(ev.m); em.ch('\t'); em.num(ev.size); em.ch('\t'); em.body(ev.size); em.ch('\n'); }
    em.ch('F'); em.ch('\t'); em.num(ev.m); em.ch('\t'); em.str(sn, snl); em.ch(strand); em.ch('\t'); em.ch('0'); em.ch('\t'); em.num(ev.size); em.ch('$'); em.ch('\t');
    text_at(em, ev.b, total); em.ch('\t'); text_at(em, (uint64_t)ev.en + k, total); em.ch('\t'); em.num(k); em.ch('M'); em.ch('\n');
    if (ev.link) {
        const int64_t a = ev.prev_nm, b = ev.nm;
        const uint64_t as = ev.prev_size, bs = ev.size;
        const uint64_t a0 = a > 0 ? as - k : 0, a1 = a > 0 ? as : k;  // the overlapping k-mer on each segment
        const uint64_t b0 = b > 0 ? 0 : bs - k, b1 = b > 0 ? k : bs;
        em.ch('E'); em.ch('\t'); em.num(text_mag(a)); em.ch(a >= 0 ? '+' : '-'); em.ch('\t'); em.num(ev.m); em.ch(strand); em.ch('\t');
        text_at(em, a0, as); em.ch('\t'); text_at(em, a1, as); em.ch('\t'); text_at(em, b0, bs); em.ch('\t'); text_at(em, b1, bs); em.ch('\t'); em.num(k); em.ch('M'); em.ch('\n');
    }
}

// "P\t" name "\t" ... "*\n"  /  "O\t" name "p\t" ... : bytes of the head and of the tail (the last piece's own byte is '\t' / '\n')
__device__ __forceinline__ uint64_t text_path_head(int format, uint64_t name_len) { return format == TPC_TEXT_GFA1 ? 3 + name_len : 4 + name_len; }
__device__ __forceinline__ uint64_t text_path_tail(int format) { return format == TPC_TEXT_GFA1 ? 2 : 0; }

__global__ void k_text_size(TpcTextPlan T)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= T.n_events; e += stride) {
        uint64_t lines = 0, piece = 0;
        if (e < T.n_events) {
            TextEvent ev;
            text_load(T, e, ev);
            CountEmitter em;
            emit_lines(T, ev, em);
            lines = em.pos;
            if (T.format != TPC_TEXT_FASTA) piece = text_digits(ev.m) + 2;
        }
        T.off[e] = lines;
        T.piece[e] = piece;
    }
}

// after the scan of piece[]
__global__ void k_text_addpath(TpcTextPlan T)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.n_rec; s += stride) {
        const uint64_t e0 = T.seq_begin[s], e1 = T.seq_begin[s + 1];
        if (e1 <= e0) continue;
        const uint64_t name_len = T.seq_name_off[s + 1] - T.seq_name_off[s];
        T.off[e1 - 1] += text_path_head(T.format, name_len) + (T.piece[e1] - T.piece[e0]) + text_path_tail(T.format);
    }
}

// letter i (0 .. size) of the body of an event, as SegmentBody gives it
__device__ __forceinline__ char text_letter(const TpcTextPlan &T, int64_t nm, uint32_t b, uint64_t size, uint32_t s, uint64_t i)
{
    const bool forward = nm > 0;
    const uint64_t g = T.rec_start[s] + b + (forward ? i : size - 1 - i);
    const uint32_t code = (uint32_t)(T.bases[g >> 5] >> (2 * (g & 31))) & 3u;
    if ((T.nmask[g >> 5] >> (g & 31)) & 1u) {
        if (forward && T.n_amb) {
            uint64_t lo = 0, hi = T.n_amb;
            while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (T.amb[mid] < g) lo = mid + 1; else hi = mid; }
            if (lo < T.n_amb && T.amb[lo] == g) return (char)T.amb_letter[lo];
        }
        return 'N';
    }
    return forward ? "ACGT"[code] : "TGCA"[code];
}

// byte q of the path line of sequence s, whose events are [e0, e1)
__device__ char text_path_byte(const TpcTextPlan &T, uint32_t s, uint64_t e0, uint64_t e1, uint64_t q)
{
    const bool gfa1 = T.format == TPC_TEXT_GFA1;
    const char *sn = T.seq_names + T.seq_name_off[s];
    const uint64_t snl = T.seq_name_off[s + 1] - T.seq_name_off[s];
    if (q == 0) return gfa1 ? 'P' : 'O';
    if (q == 1) return '\t';
    if (q < 2 + snl) return sn[q - 2];
    const uint64_t head = text_path_head(T.format, snl);
    if (q < head) return (!gfa1 && q == 2 + snl) ? 'p' : '\t';
    q -= head;
    const uint64_t pieces = T.piece[e1] - T.piece[e0];
    if (q >= pieces) return q == pieces ? '*' : '\n';
    const uint64_t target = T.piece[e0] + q;
    const uint64_t f = text_last_le(T.piece, e0, e1 - 1, target);  // every piece has 3 bytes or more: no ties
    const uint64_t i = target - T.piece[f];
    const int64_t nm = T.name[f];
    const uint64_t m = text_mag(nm);
    const uint32_t d = text_digits(m);
    if (i < d) return text_digit(m, d, (uint32_t)i);
    if (i == d) return nm >= 0 ? '+' : '-';
    if (f + 1 == e1) return gfa1 ? '\t' : '\n';
    return gfa1 ? ',' : ' ';
}

// one workgroup per tile of the window [w0, w1); out holds whole tiles
__global__ void __launch_bounds__(256) k_text_render(TpcTextPlan T, uint64_t w0, uint64_t w1, uint8_t *__restrict__ out)
{
    __shared__ uint4 tile4[TPC_TEXT_TILE / 16];
    uint8_t *tile = reinterpret_cast<uint8_t *>(tile4);
    const uint64_t t0 = w0 + (uint64_t)blockIdx.x * TPC_TEXT_TILE;
    if (t0 >= w1) return;
    const uint64_t t1 = w1 - t0 < (uint64_t)TPC_TEXT_TILE ? w1 : t0 + (uint64_t)TPC_TEXT_TILE;
    // the events that meet the tile: [ea, eb); off[ea] <= t0 < off[ea + 1] and off[eb] >= t1 (off[n_events] is the total >= w1)
    const uint64_t ea = text_last_le(T.off, 0, T.n_events, t0);
    uint64_t eb = ea + 1;
    {
        uint64_t lo = ea + 1, hi = T.n_events;
        while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (T.off[mid] < t1) lo = mid + 1; else hi = mid; }
        eb = lo;
    }
    // (1) short lines
    for (uint64_t e = ea + threadIdx.x; e < eb; e += blockDim.x) {
        const uint64_t at = T.off[e];
        if (T.off[e + 1] == at) continue;  // fasta: an event seen before has no text
        TextEvent ev;
        text_load(T, e, ev);
        TileEmitter em{at, t0, t1, tile};
        emit_lines(T, ev, em);
    }
    // (2) + (3) bodies and path lines, by byte
    for (uint32_t j = threadIdx.x; j < (uint32_t)(t1 - t0); j += blockDim.x) {
        const uint64_t p = t0 + j;
        const uint64_t e = text_last_le(T.off, ea, eb - 1, p);
        const uint64_t r = p - T.off[e];
        const int64_t nm = T.name[e];
        const uint32_t b = T.begin[e], en = T.end[e];
        const uint64_t size = (uint64_t)en + (uint64_t)T.k - b;
        const bool first = (T.first[e >> 5] >> (e & 31)) & 1u;
        uint64_t body_end = 0;
        if (first) {
            const uint32_t dm = text_digits(text_mag(nm));
            const uint64_t body_at = T.format == TPC_TEXT_GFA1 ? 3 + dm : T.format == TPC_TEXT_GFA2 ? 4 + dm + text_digits(size) : 2 + dm;
            body_end = body_at + text_body_bytes(T.format, size);
            if (r < body_at) continue;
            if (r < body_end) {
                uint64_t i = r - body_at;
                char c = '\n';
                if (T.format == TPC_TEXT_FASTA) {
                    const uint64_t line = i / 81, col = i % 81;
                    i = col == 80 ? size : line * 80 + col;
                }
                if (i < size) c = text_letter(T, nm, b, size, text_seq_of(T, e), i);
                tile[j] = (uint8_t)c;
                continue;
            }
        }
        if (T.format == TPC_TEXT_FASTA) continue;
        const uint32_t s = text_seq_of(T, e);
        const uint64_t e1 = T.seq_begin[s + 1];
        if (e + 1 != e1) continue;
        TextEvent ev;
        text_load(T, e, ev);
        CountEmitter em;
        emit_lines(T, ev, em);
        if (r < em.pos) continue;
        tile[j] = (uint8_t)text_path_byte(T, s, T.seq_begin[s], e1, r - em.pos);
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (t0 - w0));  // a multiple of the tile size from an aligned base
    for (uint32_t i = threadIdx.x; i < (uint32_t)((t1 - t0 + 15) / 16); i += blockDim.x) dst[i] = tile4[i];
}

int text_scan64(hipStream_t s, uint64_t *data, uint64_t n, void *&tmp, size_t &tmp_cap)
{
    size_t need = 0;
    if (rocprim::exclusive_scan(nullptr, need, data, data, (uint64_t)0, n, rocprim::plus<uint64_t>(), s) != hipSuccess) return -2;
    if (need > tmp_cap) {
        if (tmp) (void)hipFree(tmp);
        tmp = nullptr; tmp_cap = 0;
        if (hipMalloc(&tmp, need) != hipSuccess) return -3;
        tmp_cap = need;
    }
    return rocprim::exclusive_scan(tmp, need, data, data, (uint64_t)0, n, rocprim::plus<uint64_t>(), s) == hipSuccess ? 0 : -2;
}

unsigned text_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192)); }

}  // namespace

int tpc_launch_segtext_plan(hipStream_t s, TpcTextPlan &plan, uint64_t *total_bytes, char *err)
{
    err[0] = 0;
    *total_bytes = 0;
    plan.off = nullptr; plan.piece = nullptr;
    const size_t bytes = ((size_t)plan.n_events + 1) * 8;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return -10; }
    // the two arrays, the scans' scratch (a fraction of one array) and the margin the segment table keeps
    if (2 * bytes + bytes / 8 + ((size_t)64 << 20) > free_b) {
        snprintf(err, TPC_SEG_ERR_TEXT, "graph text: %zu bytes of offsets for %llu events do not fit the free device memory", 2 * bytes, (unsigned long long)plan.n_events);
        return -20;
    }
    void *tmp = nullptr;
    size_t tmp_cap = 0;
    int rc = 0;
    auto done = [&](int code) {
        if (tmp) (void)hipFree(tmp);
        if (code) { if (plan.off) (void)hipFree(plan.off); if (plan.piece) (void)hipFree(plan.piece); plan.off = plan.piece = nullptr; }
        return code;
    };
    if (hipMalloc((void **)&plan.off, bytes) != hipSuccess || hipMalloc((void **)&plan.piece, bytes) != hipSuccess) return done(-10);
    hipLaunchKernelGGL(k_text_size, dim3(text_grid(plan.n_events + 1)), dim3(256), 0, s, plan);
    if ((rc = text_scan64(s, plan.piece, plan.n_events + 1, tmp, tmp_cap))) return done(rc);
    if (plan.format != TPC_TEXT_FASTA && plan.n_rec) hipLaunchKernelGGL(k_text_addpath, dim3(text_grid(plan.n_rec)), dim3(256), 0, s, plan);
    if ((rc = text_scan64(s, plan.off, plan.n_events + 1, tmp, tmp_cap))) return done(rc);
    if (hipMemcpyAsync(total_bytes, plan.off + plan.n_events, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return done(-10);
    if (hipGetLastError() != hipSuccess) return done(-10);
    return done(0);
}

void tpc_launch_segtext_render(hipStream_t s, const TpcTextPlan &plan, uint64_t byte0, uint64_t n_bytes, uint8_t *out)
{
    if (!n_bytes) return;
    const uint64_t tiles = (n_bytes + TPC_TEXT_TILE - 1) / TPC_TEXT_TILE;
    hipLaunchKernelGGL(k_text_render, dim3((unsigned)tiles), dim3(256), 0, s, plan, byte0, byte0 + n_bytes, out);
}
