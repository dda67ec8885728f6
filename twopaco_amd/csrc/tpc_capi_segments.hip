// tpc_capi_segments.hip -- C-ABI of the segment table (tpc_segments_*): the worker it replaces is graphdump's serial walk,
// reference src/graphdump/graphdump.cpp:44-113 (segment naming) and :398-480 (the loop over the junction records).
// Kernels and their memory bound: tpc_segments.hip.
#include "tpc_ctx.h"

namespace {

int segments_build(tpc_ctx *c, const uint32_t *d_slots, uint64_t n_slots, int k, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec,
                   const uint64_t *amb_pos, uint64_t n_amb)
{
    c->seg_valid = false;
    for (void *p : { (void *)c->seg_name, (void *)c->seg_first, (void *)c->seg_ev[0], (void *)c->seg_ev[1], (void *)c->seg_ev[2] }) if (p) (void)hipFree(p);
    c->seg_name = nullptr; c->seg_first = nullptr;
    c->seg_ev[0] = c->seg_ev[1] = c->seg_ev[2] = nullptr;
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
        rc = tpc_launch_segments(c->stream, d_slots, n_slots, k, c->bases, c->nmask, d_rec, d_rec + n_rec, n_rec, d_amb, n_amb, &c->seg_name, &c->seg_first, c->seg_ev, &res, text);
    }
    const hipError_t e = hipStreamSynchronize(c->stream);
    for (void *p : { (void *)d_rec, (void *)d_amb }) if (p) (void)hipFree(p);
    if (rc) return text[0] ? fail(c, rc, "%s", text) : fail(c, rc, "segment table failed (%d): %s", rc, hipGetErrorString(hipGetLastError()));
    HIPCHK(c, e);
    c->seg_events = res.events; c->seg_segments = res.segments; c->seg_named = res.named; c->seg_table_bytes = res.table_bytes;
    c->seg_slots = n_slots; c->seg_peak_bytes = res.peak_bytes; c->seg_n_rec = n_rec;
    c->seg_err_slot = res.err_slot; c->seg_err_kind = res.err_kind;
    c->seg_valid = true;
    return 0;
}

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
    if (!c || !counts || !c->seg_valid) return -1;
    counts[0] = c->seg_events; counts[1] = c->seg_segments; counts[2] = c->seg_named; counts[3] = c->seg_table_bytes; counts[4] = c->seg_slots;
    counts[5] = c->seg_peak_bytes;
    return 0;
}

int tpc_segments_error(const tpc_ctx *c, uint64_t *slot, int *kind)
{
    if (!c || !c->seg_valid) return -1;
    if (slot) *slot = c->seg_err_slot;
    if (kind) *kind = c->seg_err_kind;
    return 0;
}

int tpc_segments_fetch_names(tpc_ctx *c, uint64_t e0, uint64_t n, int64_t *name_host)
{
    if (!c || !c->seg_valid || (n && !name_host) || e0 > c->seg_events || n > c->seg_events - e0) return fail(c, -1, "segment table: bad name range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(name_host, c->seg_name + e0, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_fetch_first(tpc_ctx *c, uint64_t word0, uint64_t n_words, uint32_t *first_host)
{
    const uint64_t words = c ? (c->seg_events + 31) / 32 : 0;
    if (!c || !c->seg_valid || (n_words && !first_host) || word0 > words || n_words > words - word0) return fail(c, -1, "segment table: bad first-bit range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n_words) HIPCHK(c, hipMemcpy(first_host, c->seg_first + word0, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_fetch_events(tpc_ctx *c, uint64_t e0, uint64_t n, uint32_t *begin_host, uint32_t *end_host)
{
    if (!c || !c->seg_valid || (n && (!begin_host || !end_host)) || e0 > c->seg_events || n > c->seg_events - e0) return fail(c, -1, "segment table: bad event range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) {
        HIPCHK(c, hipMemcpy(begin_host, c->seg_ev[0] + e0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(end_host, c->seg_ev[1] + e0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

int tpc_segments_fetch_sequences(tpc_ctx *c, uint64_t s0, uint64_t n, uint32_t *first_event_host)
{
    const uint64_t entries = c ? (uint64_t)c->seg_n_rec + 1 : 0;
    if (!c || !c->seg_valid || (n && !first_event_host) || s0 > entries || n > entries - s0) return fail(c, -1, "segment table: bad sequence range");
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(first_event_host, c->seg_ev[2] + s0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
