// tpc_stage.h -- what the stages over the segment table (tpc_colors.hip, tpc_links.hip, tpc_bubbles.hip, tpc_distances.hip, tpc_components.hip, tpc_superbubbles.hip, tpc_anchors.hip, tpc_locate.hip, tpc_classes.hip, tpc_tracks.hip, tpc_variants.hip) share
// on the host side.  `noun` is the stage's name in its error texts: "colours", "links", "bubbles", "distances", "components", "superbubbles", "anchors", "edges", "locate", "classes", "tracks", "variants".  Every including unit
// gets its own copy (anonymous namespace), as of tpc_segrows.h: the library exports none of it.
#pragma once
#include "tpc_ctx.h"

namespace {

// The segment table a stage reads: built, and by a walk that ended well.  verb: what the stage would have done with the segments.
inline int stage_needs_segments(tpc_ctx *c, const char *noun, const char *verb)
{
    if (!c->seg.valid) return fail(c, -1, "segment %s: build the segment table first (tpc_segments_build_host / _resident)", noun);
    if (c->seg.err_kind != TPC_SEG_OK)
        return fail(c, -1, "segment %s: the segment table holds the walk's error %d at slot %llu, there are no segments to %s", noun, c->seg.err_kind,
                    (unsigned long long)c->seg.err_slot, verb);
    return 0;
}

// The free-memory refusal: `need` bytes, summed before the first allocation, and 64 MiB beside them must fit the free device memory.
// detail: what the large terms of the sum are, inside the parentheses of the text.  0, or the error code with the text set.
__attribute__((format(printf, 4, 5))) inline int stage_fits(tpc_ctx *c, const char *noun, uint64_t need, const char *detail, ...)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // after a whole run in this context the first pass's partition buffers are still held: they are given back before this is refused
    if (need + ((uint64_t)64 << 20) > free_b && release_partition_buffers(c)) HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    if (need + ((uint64_t)64 << 20) <= free_b) return 0;
    char text[256];
    va_list ap;
    va_start(ap, detail);
    vsnprintf(text, sizeof text, detail, ap);
    va_end(ap);
    return fail(c, -20, "segment %s: %llu bytes (%s) do not fit the free device memory", noun, (unsigned long long)need, text);
}

// The device temporaries of one stage call: freed when the call returns, whichever way.
struct StageTemps {
    std::vector<void *> held;
    template <typename T>
    bool get(tpc_ctx *c, T **p, size_t bytes)
    {
        if (dev_malloc(c, (void **)p, bytes) != hipSuccess) return false;
        held.push_back(*p);
        return true;
    }
    ~StageTemps() { for (void *p : held) (void)hipFree(p); }
};

// The wait at the end of what a stage enqueued (ok: everything could be enqueued).  0, or the error code with the text set.
inline int stage_wait(tpc_ctx *c, const char *noun, bool ok)
{
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (!ok || e != hipSuccess || hipGetLastError() != hipSuccess) return fail(c, -10, "segment %s: the kernels failed: %s", noun, hipGetErrorString(e));
    return 0;
}

// The planar fetch: `planes` holds dst.size() planes of n_rows uint32 each, rows [r0, r0 + n) of every plane go to the host arrays of
// dst in order.  what: "row" or "side", the unit of the range in the error text.
inline int fetch_planes(tpc_ctx *c, const char *noun, const char *what, const uint32_t *planes, uint64_t n_rows, uint64_t r0, uint64_t n, std::initializer_list<uint32_t *> dst)
{
    bool missing = false;
    for (uint32_t *d : dst) missing = missing || !d;
    if ((n && missing) || r0 > n_rows || n > n_rows - r0)
        return fail(c, -1, "segment %s: bad %s range (%llu %ss at %llu of %llu)", noun, what, (unsigned long long)n, what, (unsigned long long)r0, (unsigned long long)n_rows);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t plane = 0;
    for (uint32_t *d : dst) {
        if (n) HIPCHK(c, hipMemcpy(d, planes + plane * n_rows + r0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        plane++;
    }
    return 0;
}

}  // namespace
