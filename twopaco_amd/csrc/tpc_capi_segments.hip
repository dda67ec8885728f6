// tpc_capi_segments.hip -- C-ABI of the segment table (tpc_segments_*): the worker it replaces is graphdump's serial walk,
// reference src/graphdump/graphdump.cpp:44-113 (segment naming) and :398-480 (the loop over the junction records).
// Kernels and their memory bound: tpc_segments.hip.  The text of the graph from that table (tpc_segments_text_*): tpc_segtext.hip.
#include "tpc_ctx.h"

#include <cerrno>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <sys/stat.h>
#include <unistd.h>

namespace {

void text_plan_drop(tpc_ctx *c)
{
    for (void *p : { (void *)c->text_plan.off, (void *)c->text_plan.piece, c->text_names, (void *)c->text_win }) if (p) (void)hipFree(p);
    c->text_plan = TpcTextPlan{};
    c->text_names = nullptr;
    c->text_win = nullptr; c->text_win_cap = 0;
    c->text_valid = false;
    c->text_total = 0;
    c->text_ms = 0;
}

// WHO DROPS WHOM, written once: dropping a table drops what was built over it.
//   segments <- colours <- distances        (the matrices were summed over the colour table)
//   segments <- links   <- bubbles          (the bubbles were found over the link table)
//   colours, links      <- components       (joined by the link rows, summed over the colour rows)
//   colours, links      <- superbubbles     (searched over the link rows' arcs, presence ORed over the colour rows)
//   colours             <- classes          (the colour rows grouped by their presence words)
//   colours             <- tracks           (the colour rows projected onto the sequences' events)
//   superbubbles        <- variants         (the sequences walked through the superbubble rows and their member lists)
//   segments <- anchors                     (paired and chained over the event table alone)
//   segments <- edges   <- locate           (the index holds positions of the build's text and rows; a locate holds hits in that index)
//   segments <- the graph text's plan
void free_all(std::initializer_list<const void *> ps) { for (const void *p : ps) if (p) (void)hipFree(const_cast<void *>(p)); }

}  // namespace

namespace tpch {

void distances_drop(tpc_ctx *c) { free_all({c->dst.mat}); c->dst = {}; }
void classes_drop(tpc_ctx *c) { free_all({c->cls.class_of, c->cls.first, c->cls.sums, c->cls.presence, c->cls.sets}); c->cls = {}; }
void tracks_drop(tpc_ctx *c) { free_all({c->trk.rows, c->trk.sums}); c->trk = {}; }
void components_drop(tpc_ctx *c) { free_all({c->cmp.component, c->cmp.root, c->cmp.sums, c->cmp.presence}); c->cmp = {}; }
void variants_drop(tpc_ctx *c)
{
    free_all({c->var.trv, c->var.trv_mask, c->var.all, c->var.all64, c->var.presence, c->var.site_off, c->var.ref_allele, c->var.site64, c->var.hist});
    c->var = {};
}
void superbubbles_drop(tpc_ctx *c)
{
    variants_drop(c);
    free_all({c->sbb.off, c->sbb.heads, c->sbb.exit_of, c->sbb.u32, c->sbb.u64, c->sbb.presence, c->sbb.member_off, c->sbb.members});
    c->sbb = {};
}
void locate_drop(tpc_ctx *c) { free_all({c->loc.hit, c->loc.row, c->loc.runs, c->loc.recs, c->loc.shared}); c->loc = {}; }
void edges_drop(tpc_ctx *c) { locate_drop(c); free_all({c->edg.slots, c->edg.g0}); c->edg = {}; }
void anchors_drop(tpc_ctx *c) { free_all({c->anc.mate, c->anc.rows, c->anc.sums}); c->anc = {}; }
void bubbles_drop(tpc_ctx *c) { free_all({c->bub.rows, c->bub.sides, c->bub.hist}); c->bub = {}; }
void colors_drop(tpc_ctx *c) { distances_drop(c); components_drop(c); superbubbles_drop(c); classes_drop(c); tracks_drop(c); free_all({c->col.rows, c->col.presence, c->col.hist}); c->col = {}; }
void links_drop(tpc_ctx *c) { bubbles_drop(c); components_drop(c); superbubbles_drop(c); free_all({c->lnk.rows, c->lnk.first}); c->lnk = {}; }

}  // namespace tpch

namespace {

void segments_drop(tpc_ctx *c)
{
    text_plan_drop(c);
    colors_drop(c);
    links_drop(c);
    anchors_drop(c);
    edges_drop(c);
    free_all({c->seg.name, c->seg.first, c->seg.ev[0], c->seg.ev[1], c->seg.ev[2], c->seg.rec, c->seg.amb});
    c->seg = {};
}

int segments_build(tpc_ctx *c, const uint32_t *d_slots, uint64_t n_slots, int k, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec,
                   const uint64_t *amb_pos, uint64_t n_amb)
{
    segments_drop(c);
    if (k < 0) return fail(c, -1, "segment table: k must not be negative");
    if (!c->bases || !c->nmask || c->text_windowed) return fail(c, -1, "segment table: tpc_seq_upload the whole text first");
    if (n_rec && (!rec_start || !rec_len)) return fail(c, -1, "segment table: records required");
    if (n_amb && !amb_pos) return fail(c, -1, "segment table: ambiguity positions required");
    // everything the kernels index the text with is checked here: a sequence lies inside the text, the list is ascending
    for (uint32_t r = 0; r < n_rec; r++)
        if (rec_start[r] > c->n_text || rec_len[r] > c->n_text - rec_start[r]) return fail(c, -1, "segment table: sequence %u lies outside the uploaded text", r);
    for (uint64_t i = 1; i < n_amb; i++)
        if (amb_pos[i - 1] >= amb_pos[i]) return fail(c, -1, "segment table: ambiguity positions must ascend");
    uint64_t *d_rec = nullptr, *d_amb = nullptr;
    int rc = 0;
    if (hipMalloc((void **)&d_rec, (2 * (size_t)n_rec + 1) * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&d_amb, (n_amb + 1) * sizeof(uint64_t)) != hipSuccess) rc = -10;
    if (rc == 0 && n_rec && (hipMemcpyAsync(d_rec, rec_start, (size_t)n_rec * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                             hipMemcpyAsync(d_rec + n_rec, rec_len, (size_t)n_rec * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess)) rc = -10;
    if (rc == 0 && n_amb && hipMemcpyAsync(d_amb, amb_pos, n_amb * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = -10;
    TpcSegResult res{};
    char text[TPC_SEG_ERR_TEXT] = "";
    if (rc == 0) {
        Timed t(c, TPC_K_SEGMENTS);
        rc = tpc_launch_segments(c->stream, d_slots, n_slots, k, c->bases, c->nmask, d_rec, d_rec + n_rec, n_rec, d_amb, n_amb, &c->seg.name, &c->seg.first, c->seg.ev, &res, text);
    }
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc || e != hipSuccess) { for (void *p : { (void *)d_rec, (void *)d_amb }) if (p) (void)hipFree(p); }
    else { c->seg.rec = d_rec; c->seg.amb = d_amb; }  // the graph text reads them (tpc_segments_text_plan)
    if (rc) return text[0] ? fail(c, rc, "%s", text) : fail(c, rc, "segment table failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    HIPCHK(c, e);
    c->seg.events = res.events; c->seg.segments = res.segments; c->seg.named = res.named; c->seg.table_bytes = res.table_bytes;
    c->seg.slots = n_slots; c->seg.peak_bytes = res.peak_bytes; c->seg.n_rec = n_rec;
    c->seg.err_slot = res.err_slot; c->seg.err_kind = res.err_kind;
    c->seg.n_amb = n_amb; c->seg.k = k;
    c->seg.text_bases = c->bases; c->seg.text_n = c->n_text; c->seg.text_uploads = c->text_uploads;
    c->seg.valid = true;
    return 0;
}

// one render, timed into the sum behind TPC_K_SEGTEXT (the caller has synchronised ev1 before it reads the sum)
struct TextTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok() { return (e0 || hipEventCreate(&e0) == hipSuccess) && (e1 || hipEventCreate(&e1) == hipSuccess); }
    void add(tpc_ctx *c) { float ms = 0; if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) c->text_ms += ms; }
    ~TextTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

size_t text_tiles(uint64_t n) { return (size_t)((n + TPC_TEXT_TILE - 1) / TPC_TEXT_TILE * TPC_TEXT_TILE); }

bool text_ready(tpc_ctx *c) { return c && c->seg.valid && c->text_valid && c->bases == c->seg.text_bases && c->n_text == c->seg.text_n && c->text_uploads == c->seg.text_uploads && !c->text_windowed; }

}  // namespace

extern "C" {

int tpc_segments_build_host(tpc_ctx *c, const void *stream_host, uint64_t n_bytes, int k, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec,
                            const uint64_t *amb_pos, uint64_t n_amb)
{
    if (!c || (n_bytes && !stream_host)) return fail(c, -1, "segment table: stream required");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n_slots = n_bytes / 12;  // trailing bytes that do not fill a slot end the stream (junctionapi.h:83-89)
    uint32_t *d_slots = nullptr;
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    if (n_slots * 12 + ((size_t)64 << 20) > free_b) return fail(c, -20, "segment table: the stream of %llu bytes does not fit the free device memory", (unsigned long long)(n_slots * 12));
    HIPCHK(c, hipMalloc((void **)&d_slots, n_slots * 12 + 64));
    int rc = 0;
    if (n_slots && hipMemcpyAsync(d_slots, stream_host, n_slots * 12, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(c, -10, "segment table: stream upload failed");
    if (rc == 0) rc = segments_build(c, d_slots, n_slots, k, rec_start, rec_len, n_rec, amb_pos, n_amb);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d_slots);
    return rc;
}

int tpc_segments_build_resident(tpc_ctx *c, int k, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec, const uint64_t *amb_pos, uint64_t n_amb)
{
    if (!c) return -1;
    if (!c->stream_buf && c->stream_bytes) return fail(c, -1, "segment table: tpc_emit_stream first");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->stream_buf) {  // an empty stream was never allocated: one slot of scratch stands in for it
        uint32_t *d_slots = nullptr;
        HIPCHK(c, hipMalloc((void **)&d_slots, 64));
        const int rc = segments_build(c, d_slots, 0, k, rec_start, rec_len, n_rec, amb_pos, n_amb);
        (void)hipFree(d_slots);
        return rc;
    }
    return segments_build(c, c->stream_buf, c->stream_bytes / 12, k, rec_start, rec_len, n_rec, amb_pos, n_amb);
}

int tpc_segments_counts(const tpc_ctx *c, uint64_t *counts)
{
    if (!c || !counts || !c->seg.valid) return -1;
    counts[0] = c->seg.events; counts[1] = c->seg.segments; counts[2] = c->seg.named; counts[3] = c->seg.table_bytes; counts[4] = c->seg.slots;
    counts[5] = c->seg.peak_bytes;
    return 0;
}

int tpc_segments_error(const tpc_ctx *c, uint64_t *slot, int *kind)
{
    if (!c || !c->seg.valid) return -1;
    if (slot) *slot = c->seg.err_slot;
    if (kind) *kind = c->seg.err_kind;
    return 0;
}

int tpc_segments_fetch_names(tpc_ctx *c, uint64_t e0, uint64_t n, int64_t *name_host)
{
    if (!c || !c->seg.valid || (n && !name_host) || e0 > c->seg.events || n > c->seg.events - e0) return fail(c, -1, "segment table: bad name range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(name_host, c->seg.name + e0, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_fetch_first(tpc_ctx *c, uint64_t word0, uint64_t n_words, uint32_t *first_host)
{
    const uint64_t words = c ? (c->seg.events + 31) / 32 : 0;
    if (!c || !c->seg.valid || (n_words && !first_host) || word0 > words || n_words > words - word0) return fail(c, -1, "segment table: bad first-bit range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n_words) HIPCHK(c, hipMemcpy(first_host, c->seg.first + word0, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_fetch_events(tpc_ctx *c, uint64_t e0, uint64_t n, uint32_t *begin_host, uint32_t *end_host)
{
    if (!c || !c->seg.valid || (n && (!begin_host || !end_host)) || e0 > c->seg.events || n > c->seg.events - e0) return fail(c, -1, "segment table: bad event range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) {
        HIPCHK(c, hipMemcpy(begin_host, c->seg.ev[0] + e0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(end_host, c->seg.ev[1] + e0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

int tpc_segments_fetch_sequences(tpc_ctx *c, uint64_t s0, uint64_t n, uint32_t *first_event_host)
{
    const uint64_t entries = c ? (uint64_t)c->seg.n_rec + 1 : 0;
    if (!c || !c->seg.valid || (n && !first_event_host) || s0 > entries || n > entries - s0) return fail(c, -1, "segment table: bad sequence range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(first_event_host, c->seg.ev[2] + s0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_text_plan(tpc_ctx *c, int format, const char *seq_names, const uint64_t *seq_name_off, const uint8_t *amb_letter, uint64_t *total_bytes)
{
    if (!c) return -1;
    if (!total_bytes) return fail(c, -1, "graph text: total_bytes required");
    *total_bytes = 0;
    text_plan_drop(c);
    if (!c->seg.valid) return fail(c, -1, "graph text: build the segment table first (tpc_segments_build_host / _resident)");
    if (c->seg.err_kind != TPC_SEG_OK)
        return fail(c, -1, "graph text: the segment table holds the walk's error %d at slot %llu, there is no text to render", c->seg.err_kind, (unsigned long long)c->seg.err_slot);
    if (format != TPC_TEXT_GFA1 && format != TPC_TEXT_GFA2 && format != TPC_TEXT_FASTA) return fail(c, -1, "graph text: format %d is none of gfa1 (1), gfa2 (2), fasta (3)", format);
    if (!c->bases || !c->nmask || c->text_windowed || c->bases != c->seg.text_bases || c->n_text != c->seg.text_n || c->text_uploads != c->seg.text_uploads)
        return fail(c, -1, "graph text: the text of tpc_seq_upload the table was built over is no longer resident");
    const uint32_t n_rec = c->seg.n_rec;
    if (!seq_name_off || (seq_name_off[n_rec] && !seq_names)) return fail(c, -1, "graph text: sequence names required");
    if (seq_name_off[0] != 0) return fail(c, -1, "graph text: the names' offsets must begin at 0");
    for (uint32_t r = 0; r < n_rec; r++)
        if (seq_name_off[r] > seq_name_off[r + 1]) return fail(c, -1, "graph text: the names' offsets must ascend");
    if (c->seg.n_amb && !amb_letter) return fail(c, -1, "graph text: the letters of the %llu ambiguity positions are required", (unsigned long long)c->seg.n_amb);
    HIPCHK(c, hipSetDevice(c->device));
    // the table's own consistency: every event belongs to one of the n_rec sequences
    uint32_t last = 0;
    HIPCHK(c, hipMemcpy(&last, c->seg.ev[2] + n_rec, sizeof last, hipMemcpyDeviceToHost));
    if (last != c->seg.events) return fail(c, -1, "graph text: the stream holds events of more sequences than the %u given", n_rec);
    // names' blob | offsets | letters in one allocation
    const uint64_t blob = seq_name_off[n_rec];
    const size_t off_at = (size_t)((blob + 7) / 8 * 8), let_at = off_at + ((size_t)n_rec + 1) * 8, bytes = let_at + (size_t)c->seg.n_amb + 8;
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    if (bytes + ((size_t)64 << 20) > free_b) return fail(c, -20, "graph text: %zu bytes of sequence names and letters do not fit the free device memory", bytes);
    HIPCHK(c, hipMalloc(&c->text_names, bytes));
    uint8_t *base = (uint8_t *)c->text_names;
    if (blob) HIPCHK(c, hipMemcpyAsync(base, seq_names, blob, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + off_at, seq_name_off, ((size_t)n_rec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (c->seg.n_amb) HIPCHK(c, hipMemcpyAsync(base + let_at, amb_letter, c->seg.n_amb, hipMemcpyHostToDevice, c->stream));
    TpcTextPlan &T = c->text_plan;
    T.format = format; T.k = c->seg.k;
    T.n_events = c->seg.events; T.n_rec = n_rec;
    T.name = c->seg.name; T.first = c->seg.first; T.begin = c->seg.ev[0]; T.end = c->seg.ev[1]; T.seq_begin = c->seg.ev[2];
    T.rec_start = c->seg.rec; T.rec_len = c->seg.rec + n_rec;
    T.bases = c->bases; T.nmask = c->nmask;
    T.amb = c->seg.amb; T.amb_letter = base + let_at; T.n_amb = c->seg.n_amb;
    T.seq_names = (const char *)base; T.seq_name_off = (const uint64_t *)(base + off_at);
    char text[TPC_SEG_ERR_TEXT] = "";
    TextTimer timer;
    if (!timer.ok()) { text_plan_drop(c); return fail(c, -10, "graph text: hipEventCreate failed"); }
    (void)hipEventRecord(timer.e0, c->stream);
    const int rc = tpc_launch_segtext_plan(c->stream, T, &c->text_total, text);
    (void)hipEventRecord(timer.e1, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc || e != hipSuccess) {
        text_plan_drop(c);
        return text[0] ? fail(c, rc, "%s", text) : fail(c, rc ? rc : -10, "graph text: the size pass failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    }
    c->text_ms = 0;
    timer.add(c);
    size_t fb = 0, tb = 0;
    if (hipMemGetInfo(&fb, &tb) == hipSuccess) c->seg.peak_bytes = std::max<uint64_t>(c->seg.peak_bytes, tb - fb);
    c->text_valid = true;
    *total_bytes = c->text_total;
    return 0;
}

int tpc_segments_text_fetch(tpc_ctx *c, uint64_t byte0, uint64_t n_bytes, void *dst_host)
{
    if (!c) return -1;
    if (!text_ready(c)) return fail(c, -1, "graph text: tpc_segments_text_plan first");
    if ((n_bytes && !dst_host) || byte0 > c->text_total || n_bytes > c->text_total - byte0)
        return fail(c, -1, "graph text: bad byte range (%llu bytes at %llu of a text of %llu)", (unsigned long long)n_bytes, (unsigned long long)byte0, (unsigned long long)c->text_total);
    if (!n_bytes) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t window = std::min<uint64_t>(n_bytes, (uint64_t)256 << 20);
    if (text_tiles(window) > c->text_win_cap) {  // the window buffer is kept between calls (many small windows: no allocation each)
        if (c->text_win) (void)hipFree(c->text_win);
        c->text_win = nullptr; c->text_win_cap = 0;
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        if (text_tiles(window) + ((size_t)64 << 20) > free_b) return fail(c, -20, "graph text: a window of %zu bytes does not fit the free device memory", text_tiles(window));
        HIPCHK(c, hipMalloc((void **)&c->text_win, text_tiles(window)));
        c->text_win_cap = text_tiles(window);
    }
    uint8_t *d = c->text_win;
    hipEvent_t e0 = c->ev0[TPC_K_SEGTEXT], e1 = c->ev1[TPC_K_SEGTEXT];
    for (uint64_t done = 0; done < n_bytes; done += window) {
        const uint64_t n = std::min(window, n_bytes - done);
        (void)hipEventRecord(e0, c->stream);
        tpc_launch_segtext_render(c->stream, c->text_plan, byte0 + done, n, d);
        (void)hipEventRecord(e1, c->stream);
        if (hipMemcpyAsync((uint8_t *)dst_host + done, d, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
            hipGetLastError() != hipSuccess)
            return fail(c, -10, "graph text: rendering a window failed: %s", hipGetErrorString(hipGetLastError()));
        float ms = 0;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) c->text_ms += ms;
    }
    return 0;
}

int tpc_segments_text_write(tpc_ctx *c, int fd, uint64_t file_offset, uint64_t window_bytes, uint64_t *written)
{
    if (!c) return -1;
    if (written) *written = 0;
    if (!text_ready(c)) return fail(c, -1, "graph text: tpc_segments_text_plan first");
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0) return fail(c, -1, "graph text: bad file descriptor %d", fd);
    const bool regular = S_ISREG(st.st_mode);
    const uint64_t total = c->text_total;
    c->text_write_us = c->text_wait_us = c->text_window_bytes = 0;
    if (!total) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    auto us_since = [](std::chrono::steady_clock::time_point t0) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count(); };
    uint64_t window = window_bytes ? window_bytes : (uint64_t)64 << 20;
    window = text_tiles(std::max<uint64_t>(1, std::min<uint64_t>(std::min(window, total), (uint64_t)1 << 30)));
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // the library's choice shrinks to what is free; a size the caller asked for is taken as it is or refused
    while (!window_bytes && window > ((uint64_t)1 << 20) && 2 * window + ((size_t)64 << 20) > free_b) window = text_tiles(window / 2);
    if (2 * window + ((size_t)64 << 20) > free_b) return fail(c, -20, "graph text: two windows of %llu bytes do not fit the free device memory", (unsigned long long)window);

    uint8_t *dev[2] = {nullptr, nullptr};
    void *pin[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    hipEvent_t rendered[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    TextTimer timer[2];
    std::string why;
    bool hip_ok = hipStreamCreate(&copy) == hipSuccess && timer[0].ok() && timer[1].ok();
    for (int i = 0; i < 2 && hip_ok; i++)
        hip_ok = hipMalloc((void **)&dev[i], window) == hipSuccess && hipHostMalloc(&pin[i], window, hipHostMallocDefault) == hipSuccess &&
                 hipEventCreateWithFlags(&rendered[i], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&copied[i], hipEventDisableTiming) == hipSuccess;

    // the helper thread: windows in order, one at a time; busy[b] = buffer b is handed over and not written yet
    std::mutex lock;
    std::condition_variable changed;
    struct Job { int buf; uint64_t at, n; };
    std::vector<Job> queue;
    size_t taken = 0;
    bool busy[2] = {false, false}, closing = false;
    std::string io_error;
    uint64_t wrote = 0;
    int64_t write_us = 0;
    c->text_window_bytes = (int64_t)window;
    std::thread writer([&]() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> hold(lock);
                changed.wait(hold, [&]() { return taken < queue.size() || closing; });
                if (taken == queue.size()) return;
                j = queue[taken++];
                if (!io_error.empty()) {  // after an error nothing more is written: the buffers are only given back
                    busy[j.buf] = false;
                    hold.unlock();
                    changed.notify_all();
                    continue;
                }
            }
            std::string err;
            const char *p = (const char *)pin[j.buf];
            const auto t0 = std::chrono::steady_clock::now();
            for (uint64_t done = 0; done < j.n && err.empty();) {
                const ssize_t w = regular ? ::pwrite(fd, p + done, j.n - done, (off_t)(file_offset + j.at + done)) : ::write(fd, p + done, j.n - done);
                if (w < 0 && errno == EINTR) continue;
                if (w < 0) err = std::string("graph text: writing failed: ") + strerror(errno);
                else if (w == 0) err = "graph text: writing failed: no byte was taken";
                else done += (uint64_t)w;
            }
            {
                std::unique_lock<std::mutex> hold(lock);
                write_us += us_since(t0);
                if (err.empty()) wrote += j.n; else if (io_error.empty()) io_error = err;
                busy[j.buf] = false;
            }
            changed.notify_all();
        }
    });

    const uint64_t windows = (total + window - 1) / window;
    auto issue = [&](uint64_t i) {  // render window i on the context's stream, copy it on the other
        const int b = (int)(i & 1);
        const uint64_t at = i * window, n = std::min(window, total - at);
        {
            std::unique_lock<std::mutex> hold(lock);  // the pinned buffer must have been written out (window i - 2)
            changed.wait(hold, [&]() { return !busy[b]; });
            if (!io_error.empty()) return false;
        }
        // (the device buffer is free: window i - 2's copy was synchronised before it was handed to the writer)
        if (hipEventRecord(timer[b].e0, c->stream) != hipSuccess) return false;
        tpc_launch_segtext_render(c->stream, c->text_plan, at, n, dev[b]);
        if (hipEventRecord(timer[b].e1, c->stream) != hipSuccess || hipEventRecord(rendered[b], c->stream) != hipSuccess ||
            hipStreamWaitEvent(copy, rendered[b], 0) != hipSuccess || hipMemcpyAsync(pin[b], dev[b], n, hipMemcpyDeviceToHost, copy) != hipSuccess ||
            hipEventRecord(copied[b], copy) != hipSuccess) return false;
        return true;
    };
    if (hip_ok) hip_ok = issue(0);
    for (uint64_t i = 0; hip_ok && i < windows; i++) {
        const int b = (int)(i & 1);
        if (i + 1 < windows && !issue(i + 1)) { hip_ok = false; break; }  // window i + 1 renders while window i copies
        const auto t0 = std::chrono::steady_clock::now();
        if (hipEventSynchronize(copied[b]) != hipSuccess) { hip_ok = false; break; }
        c->text_wait_us += us_since(t0);
        timer[b].add(c);
        {
            std::unique_lock<std::mutex> hold(lock);
            if (!io_error.empty()) break;
            busy[b] = true;
            queue.push_back(Job{b, i * window, std::min(window, total - i * window)});
        }
        changed.notify_all();
    }
    {
        std::unique_lock<std::mutex> hold(lock);
        closing = true;
    }
    changed.notify_all();
    writer.join();
    c->text_write_us = write_us;
    const hipError_t last = hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    if (copy) { (void)hipStreamSynchronize(copy); (void)hipStreamDestroy(copy); }
    for (int i = 0; i < 2; i++) {
        if (dev[i]) (void)hipFree(dev[i]);
        if (pin[i]) (void)hipHostFree(pin[i]);
        if (rendered[i]) (void)hipEventDestroy(rendered[i]);
        if (copied[i]) (void)hipEventDestroy(copied[i]);
    }
    if (written) *written = wrote;
    if (!io_error.empty()) return fail(c, -30, "%s", io_error.c_str());
    if (!hip_ok || wrote != total) return fail(c, -10, "graph text: rendering or copying a window failed: %s", hipGetErrorString(last));
    return 0;
}

}  // extern "C"
