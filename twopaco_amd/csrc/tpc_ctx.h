// tpc_ctx.h -- the context behind the C-ABI (struct tpc_ctx) and the helpers its translation units share:
//   tpc_capi.hip          context, options, parameters, text, the first pass (tpc_pass1_*), filter / mask transfers, timers
//   tpc_capi_pass2.hip    second pass, junction keys, ids, junction stream (tpc_pass2_*, tpc_junction*, tpc_emit*)
//   tpc_capi_shard.hip    the filter cut by address over ranks (tpc_shard_*), mask unions
//   tpc_capi_combine.hip  the filter replicated through set-bit lists (tpc_combine_*)
//   tpc_capi_segments.hip the segment table of the compacted graph and its text (tpc_segments_*)
//   tpc_colors.hip        the segment colour table (tpc_segments_colors_*), kernels and entry points
//   tpc_links.hip         the link table of the compacted graph (tpc_segments_links_*), kernels and entry points
//   tpc_bubbles.hip       the simple bubbles of the compacted graph (tpc_segments_bubbles_*), kernels and entry points
//   tpc_distances.hip     the genome distance matrices over the colour table (tpc_segments_distances_*), kernels and entry points
//   tpc_components.hip    the connected components over the link and colour tables (tpc_segments_components_*), kernels and entry points
//   tpc_superbubbles.hip  the bounded superbubbles over the link and colour tables (tpc_segments_superbubbles_*), kernels and entry points
//   tpc_anchors.hip       the anchor blocks against a reference colour (tpc_segments_anchors_*), kernels and entry points
//   tpc_locate.hip        the edge index and the location of a query text in it (tpc_segments_edges_*, tpc_segments_locate_*), kernels and entry points
//   tpc_edgehash.h        the two-strand rolling hash of an edge, shared by tpc_sketch.hip and tpc_locate.hip
//   tpc_classes.hip       the colour classes over the colour table (tpc_segments_classes_*), kernels and entry points
//   tpc_tracks.hip        the presence tracks: the colour rows projected onto the sequences' coordinates (tpc_segments_tracks_*), kernels and entry points
//   tpc_variants.hip      the variants: the sequences walked through the superbubbles, grouped into alleles (tpc_segments_variants_*), kernels and entry points
//   tpc_stage.h           what the eight stages above share on the host side: preconditions, the free-memory refusal, temporaries, the planar fetch
//   tpc_segrows.h         the row of every event, rebuilt by the colour, link, bubble and component stages: its owner and the device helpers over it
//   tpc_sketch.hip        the distinct-edge sketch behind `-f auto` (tpc_distinct_sketch), kernel and entry point
// No CPU fallback anywhere: every entry point needs a HIP device.
#pragma once
#include "../../include/twopaco_hip.h"
#include "tpc_internal.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <map>

struct tpc_ctx {
    __attribute__((always_inline)) tpc_ctx() = default;  // into tpc_ctx_create, its one caller: the library exports no constructor
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // parameters
    bool have_params = false;
    TpcHashParams P{};
    uint64_t tab_host[TPC_TAB_WORDS + TPC_QSEED_WORDS]{};  // the character tables, then k_q_hash2's seed rows (tpc_set_params)
    uint64_t *tab = nullptr;
    int C = 1;
    // text
    uint64_t *bases = nullptr;
    uint32_t *nmask = nullptr;
    uint64_t n_text = 0, n_words = 0, n_words_alloc = 0, n_tiles = 0;
    uint64_t text_uploads = 0;  // tpc_seq_upload calls so far
    // periodic-window masks of the text (tpc_internal.h:TpcLaunch): [8][n_words_alloc] = per_qs, the six bit planes of the copy distance, per_i (at 7 * n_words_alloc); built at the first
    // partitioned pass after an upload / a change of k (ensure_periodic), option "periodic_skip" (default on)
    uint32_t *periodic = nullptr;
    bool periodic_valid = false;
    bool periodic_any_q = false, periodic_any_i = false;  // some position copies its verdict / drops its insert (else the masks are never read)
    int opt_periodic = 1;
    bool opt_shard_periodic = false;  // option shard_periodic_skip: the tpc_shard_hash kernels skip too, the host calls tpc_shard_periodic_copy
    // sharded contexts may hold only the words of the tiles they hash (+ halo): bases / nmask then point text_w0 words BEFORE
    // the allocations, so that kernels keep indexing by global word
    uint64_t *bases_alloc = nullptr;
    uint32_t *nmask_alloc = nullptr;
    int opt_text_window = 0;
    bool text_windowed = false;
    uint64_t text_w0 = 0, text_w1 = 0;
    // filter + masks
    uint32_t *filter = nullptr;
    uint64_t filter_words = 0;
    uint32_t *rmask = nullptr, *mask = nullptr;
    bool mask_dirty = false;   // run-wide mask holds more than one round
    int rounds_done = 0;
    // marks of the current round / final list
    uint64_t *marks = nullptr;
    uint64_t marks_cap = 0, n_marks = 0;
    bool marks_valid = false;  // marks[] is the compaction of rmask
    bool rmask_sums_valid = false;  // block_sums / rmask_sums_n are those of the current rmask (left by the partitioned query's count)
    uint64_t rmask_sums_n = 0;
    uint64_t *block_sums = nullptr;
    uint64_t *scan_blocks = nullptr;  // scan2 per-chunk counts / offsets
    // exact filter table
    void *table = nullptr;
    uint64_t table_cap = 0, table_alloc = 0;
    // junction keys
    uint64_t *keys = nullptr;
    uint64_t n_keys = 0, keys_cap = 0;
    bool finalized = false;
    std::vector<uint64_t> keys_host;
    uint32_t *idtab = nullptr;
    uint64_t idtab_cap = 0;
    size_t idtab_bytes = 0;
    void *sort_scratch = nullptr;
    size_t sort_scratch_bytes = 0;
    // emit
    int64_t *emit_id = nullptr;
    uint64_t emit_cap = 0, n_emit = 0;
    // junction stream (bytes of the output file)
    uint32_t *stream_buf = nullptr;
    uint64_t stream_cap = 0, stream_bytes = 0;
    // per-rank formatting (tpc_emit_stream_partial -> tpc_emit_stream_part): kept between the two calls
    uint64_t *sp_rec = nullptr, *sp_vscan = nullptr, *sp_cnt = nullptr, *sp_lo = nullptr;
    uint32_t *sp_flags = nullptr;
    uint32_t sp_n_rec = 0;
    // The tables of the compacted graph, one group each.  A group's drop (tpc_capi_segments.hip: segments_drop ... anchors_drop) frees
    // its pointers, assigns {} and drops what was built over it.
    // segment table (tpc_segments_*, tpc_capi_segments.hip): name[e], first[] bit-packed and the event table, of the last build
    struct Segments {
        int64_t *name = nullptr;
        uint32_t *first = nullptr;
        uint32_t *ev[3] = {nullptr, nullptr, nullptr};  // the event table: begin[e], end[e], seq_event_begin[0 .. n_rec]
        uint32_t n_rec = 0;
        uint64_t events = 0, segments = 0, named = 0, table_bytes = 0, slots = 0, peak_bytes = 0;
        uint64_t err_slot = 0;
        int err_kind = 0;
        bool valid = false;
        // ... kept for the graph text (tpc_segments_text_*, tpc_segtext.hip): the build's sequence records and ambiguity positions, and
        // the text they index
        uint64_t *rec = nullptr, *amb = nullptr;   // device: rec_start[n_rec] then rec_len[n_rec]; amb_pos[n_amb]
        uint64_t n_amb = 0, text_n = 0, text_uploads = 0;
        const void *text_bases = nullptr;
        int k = 0;
    } seg;
    // the plan of the last tpc_segments_text_plan
    TpcTextPlan text_plan;
    void *text_names = nullptr;       // device: the names' blob, then (8-aligned) its offsets, then amb_letter
    uint8_t *text_win = nullptr;      // device: the window buffer of tpc_segments_text_fetch, whole tiles
    size_t text_win_cap = 0;
    bool text_valid = false;
    uint64_t text_total = 0;
    double text_ms = 0;               // TPC_K_SEGTEXT: kernels since the last plan
    int64_t text_write_us = 0, text_wait_us = 0, text_window_bytes = 0;  // of the last tpc_segments_text_write (tpc_get_stat)
    // segment colour table (tpc_segments_colors_*, tpc_colors.hip) of the last tpc_segments_colors_build
    struct Colors {
        uint32_t *rows = nullptr;            // device, [4][n_rows]: first event, occurrences, forward, n_colors
        uint32_t *presence = nullptr;        // device, [n_rows][words]
        unsigned long long *hist = nullptr;  // device, [2][n_colors + 1]: segments, bases
        uint64_t n_rows = 0;
        uint32_t n_colors = 0, words = 0;
        bool valid = false;
    } col;
    // link table (tpc_segments_links_*, tpc_links.hip) of the last tpc_segments_links_build
    struct Links {
        uint32_t *rows = nullptr;            // device, [3][n_rows]: first event, count, same
        uint32_t *first = nullptr;           // device, [(seg.events + 31) / 32]: link_first bits
        uint64_t n_rows = 0, occurrences = 0, slots = 0, peak_bytes = 0;
        bool valid = false;
    } lnk;
    int opt_links_slots_log2 = 0;            // option test_links_slots_log2 (tests only): slots of the link set, 0 = by the occurrences
    // simple bubbles (tpc_segments_bubbles_*, tpc_bubbles.hip) of the last tpc_segments_bubbles_build
    struct Bubbles {
        uint32_t *rows = nullptr;            // device, [4][n_rows]: source, arm_a, arm_b, sink
        uint32_t *sides = nullptr;           // device, [3][n_sides]: degree, smallest and largest neighbour
        unsigned long long *hist = nullptr;  // device, [6]: sides of degree 0, 1, 2, 3, 4, 5 or more
        uint64_t n_rows = 0, n_sides = 0, arcs = 0, peak_bytes = 0;
        bool valid = false;
    } bub;
    // genome distance matrices (tpc_segments_distances_*, tpc_distances.hip) of the last tpc_segments_distances_build
    struct Distances {
        unsigned long long *mat = nullptr;   // device, [2][n_colors][n_colors]: segments, edges
        uint64_t n_colors = 0, n_rows = 0, planes = 0, peak_bytes = 0;
        bool valid = false;
    } dst;
    // connected components (tpc_segments_components_*, tpc_components.hip) of the last tpc_segments_components_build
    struct Components {
        uint32_t *component = nullptr;       // device, [n_rows]: the component id of every row
        uint32_t *root = nullptr;            // device, [n_comp]: the smallest row of every component
        unsigned long long *sums = nullptr;  // device, [5][n_comp]: segments, links, length, edges, occurrences
        uint32_t *presence = nullptr;        // device, [n_comp][words]
        uint64_t n_comp = 0, n_rows = 0, largest = 0, peak_bytes = 0;
        uint32_t words = 0;
        bool valid = false;
    } cmp;
    // superbubbles (tpc_segments_superbubbles_*, tpc_superbubbles.hip) of the last tpc_segments_superbubbles_build
    struct Superbubbles {
        uint32_t *off = nullptr;             // device, [n_sides + 1]: the CSR offsets of the sides' arcs
        uint32_t *heads = nullptr;           // device, [n_arcs]: the heads, ascending within a side
        uint32_t *exit_of = nullptr;         // device, [n_sides]: the exit of the superbubble a side is the entrance of, all ones for none
        uint32_t *u32 = nullptr;             // device, [5][n_rows]: entrance, exit, inside, arcs, n_colors
        unsigned long long *u64 = nullptr;   // device, [3][n_rows]: paths, min_edges, max_edges
        uint32_t *presence = nullptr;        // device, [n_rows][words]
        uint32_t *member_off = nullptr;      // device, [n_rows + 1]
        uint32_t *members = nullptr;         // device, [n_members]: the inside sides of every row, ascending
        uint64_t n_rows = 0, n_sides = 0, n_members = 0, n_arcs = 0, unmirrored = 0, peak_bytes = 0;
        uint32_t words = 0, max_inside = 0;
        bool valid = false;
    } sbb;
    // anchor blocks (tpc_segments_anchors_*, tpc_anchors.hip) of the last tpc_segments_anchors_build
    struct Anchors {
        uint32_t *mate = nullptr;            // device, [n_events]: the mate of every anchor, all ones for none
        uint32_t *rows = nullptr;            // device, [4][n_blocks]: query_first, query_last, ref_first, ref_last
        unsigned long long *sums = nullptr;  // device, [4][n_colors]: blocks, anchors, edges, reverse_edges; then ref_edges
        uint64_t n_blocks = 0, n_anchors = 0, n_events = 0, ref_edges = 0, peak_bytes = 0;
        uint32_t n_colors = 0, ref_color = 0;
        bool valid = false;
    } anc;
    // edge index (tpc_segments_edges_*, tpc_locate.hip) of the last tpc_segments_edges_build: canonical (k+1)-mer -> (g, row)
    struct Edges {
        void *slots = nullptr;               // device, [n_slots] x 16 B: {tag:24 | g:40, row:32, unused:32}, all ones = empty
        uint64_t *g0 = nullptr;              // device, [n_rows]: the global position of every row's span
        uint64_t n_slots = 0, n_rows = 0, entries = 0, duplicates = 0, skipped = 0, longest_probe = 0, peak_bytes = 0, hash_mask = 0;
        uint64_t text_uploads = 0;
        bool valid = false;
    } edg;
    // the last tpc_segments_locate (tpc_locate.hip): per position, per run, per query record
    struct Locate {
        unsigned long long *hit = nullptr;   // device, [positions]
        uint32_t *row = nullptr;             // device, [positions]
        uint32_t *runs = nullptr;            // device, [5][n_runs]: q_first, length, row, rev, off_first
        unsigned long long *recs = nullptr;  // device, [4][n_rec]: windows, found, forward, runs
        unsigned long long *shared = nullptr;  // device, [n_rec][n_colors], or none
        uint64_t positions = 0, windows = 0, found = 0, n_runs = 0, n_rec = 0, peak_bytes = 0;
        uint32_t n_colors = 0;
        bool valid = false;
    } loc;
    // colour classes (tpc_segments_classes_*, tpc_classes.hip) of the last tpc_segments_classes_build
    struct Classes {
        uint32_t *class_of = nullptr;        // device, [n_rows]: the class id of every row
        uint32_t *first = nullptr;           // device, [n_classes]: the smallest row of every class
        unsigned long long *sums = nullptr;  // device, [4][n_classes]: segments, length, edges, occurrences
        uint32_t *presence = nullptr;        // device, [n_classes][words]
        unsigned long long *sets = nullptr;  // device, [3][n_colors + 1]: classes, segments, edges by number of colours
        uint64_t n_classes = 0, n_rows = 0, largest = 0, met = 0, peak_bytes = 0;
        uint32_t words = 0, n_colors = 0;
        bool valid = false;
    } cls;
    // options test_classes_* (tests only), each for the next tpc_segments_classes_build alone
    int opt_classes_slots_log2 = 0;          // slots of the class set, 0 = by the rows
    int opt_classes_hash_bits = -1;          // low bits of the row's hash that are kept, -1 = all 64
    int opt_classes_grid = 0;                // at most this many workgroups per kernel, 0 = by the rows
    int opt_classes_wide = 0;                // 1 = a wave per row, 2 = a thread per row, 0 = by the words
    // presence tracks (tpc_segments_tracks_*, tpc_tracks.hip) of the last tpc_segments_tracks_build
    struct Tracks {
        uint32_t *rows = nullptr;            // device, [3][n_intervals]: first_event, last_event, row
        unsigned long long *sums = nullptr;  // device, [4][n_colors]: intervals, edges, core_edges, private_edges; then [2][n_colors + 1]: depth_intervals, depth_edges
        uint64_t n_intervals = 0, selected = 0, peak_bytes = 0;
        uint32_t n_colors = 0, only = 0;
        bool valid = false;
    } trk;
    // variants (tpc_segments_variants_*, tpc_variants.hip) of the last tpc_segments_variants_build
    struct Variants {
        uint32_t *trv = nullptr;             // device, [5][n_trav]: start, last, d, row, edges
        unsigned long long *trv_mask = nullptr;  // device, [n_trav]
        uint32_t *all = nullptr;             // device, [5][n_all]: row, sides, edges, first, n_colors
        unsigned long long *all64 = nullptr; // device, [2][n_all]: mask, traversals
        uint32_t *presence = nullptr;        // device, [n_all][words]
        uint32_t *site_off = nullptr;        // device, [n_sbb + 1]: the first allele of every superbubble row
        uint32_t *ref_allele = nullptr;      // device, [n_sbb]: all ones for none
        unsigned long long *site64 = nullptr;  // device, [2][n_sbb]: traversals, ref_traversals
        unsigned long long *hist = nullptr;  // device, [hist_bins]: the sites by their number of alleles
        uint64_t n_trav = 0, n_all = 0, n_sbb = 0, sites = 0, strays = 0, hist_bins = 0, peak_bytes = 0;
        uint32_t n_colors = 0, words = 0, ref = 0;
        bool valid = false;
    } var;
    int opt_variants_grid = 0;               // option test_variants_grid (tests only), for the next tpc_segments_variants_build alone: at most this many workgroups per kernel, 0 = by the events
    int opt_tracks_grid = 0;                 // option test_tracks_grid (tests only), for the next tpc_segments_tracks_build alone: at most this many workgroups per kernel, 0 = by the events
    int opt_edges_slots_log2 = 0;            // option test_edges_slots_log2 (tests only): slots of the edge index, 0 = by the edges
    int opt_edges_hash_bits = 0;             // option test_edges_hash_bits (tests only): bits of the edge's hash that are kept, 0 = all 64
    int opt_locate_grid = 0;                 // option test_locate_grid (tests only): at most this many workgroups of the tile kernels, 0 = by the CUs
    int opt_components_step_limit = 0;       // option test_components_step_limit (tests only): steps of a find and retries of a hook, 0 = segments + 1
    int opt_distances_chunk_words = 0;       // option test_distances_chunk_words (tests only): column words a block stages at once, 0 = the kernel's own
    // scalars
    unsigned long long *counters = nullptr;  // device, 8 words
    unsigned long long *route_scratch = nullptr;  // device, 128 words: tpc_shard_route's per-owner counts and cursors
    uint64_t *sh_off = nullptr;  // device, [regions + 1]: offsets of the level-1 regions in a packed buffer (compacted exchange)
    size_t sh_off_bytes = 0;
    // options
    int opt_test_first = 0;
    int opt_insert_mode = 0;   // 0 auto, 1 direct atomicOr, 2 partitioned (LDS write-combining)
    int opt_slice_bits = 20;
    // partitioned insert
    bool filter_zero_pending = false;  // filter_reset requested, not yet materialised
    static constexpr int NPBUF = 19;  // 0 buf1, 1 cnt1, 2 buf2, 3 cnt2, 4 ovf, 5 ovf_cur, 6 surv, 7 surv_cur, 8 off2, 9 buf3, 10 cnt3, 11 off3; sharded contexts: 12 / 13 the insert's APPLY-side overflow list + cursor, 14 / 15 the query's hash-side list, 16 / 17 its apply-side list (sh_ovf); 18 the group boundaries of the 6-byte query (tpc_qpart6.h)
    void *pbuf[NPBUF] = {};   // shared by insert and query
    size_t pbytes[NPBUF] = {};
    std::vector<uint64_t> off2_uploaded, off3_uploaded;   // region offset tables currently in pbuf[8] / pbuf[11]
    int opt_part_levels = 0;   // 0 auto (three levels when L - slice_bits > 18), 2, 3
    int opt_shard_tight = 1;   // sharded passes: level-1 regions at the expected fill + 6 sigma (they travel whole); 0 = the one-GPU slack of 1.3 x
    // what the last insert / query actually ran (tpc_get_stat)
    int stat_path[2] = {0, 0};       // 1 direct kernel, 2 / 3 partitioned with that many levels (+10: partitioned, then completed by the direct kernel)
    int64_t stat_batches[2] = {0, 0};
    mutable int stat_kernel[5] = {0, 0, 0, 0, 0};  // hash kernel of the last insert / query, the query's verification kernel, the form and the seeding of k_q_hash2 (TpcLaunch::stat_kernel)
    mutable int stat_split[2] = {0, 0};  // kernel (0 rolling, 4 closed form) and launches of the last tpc_pass1_split_hist (TpcLaunch::stat_split)
    int stat_fmt[2] = {0, 0};        // entry format of the last partitioned insert (level 2: 0 = 32-bit, 3 = planar 24-bit) / query (0 = 8-byte, 6 = planar 48-bit)
    int64_t stat_filter2_retries = 0;  // exact-filter passes repeated with the full-size table (last tpc_pass2_filter)
    int64_t stat_aggregate_retries = 0;  // ... by the last tpc_pass2_aggregate_records
    int stat_filter2_counted = 0;        // the last exact-filter launch counted occurrences (k_filter2 / k_filter2_rec <C, true>)
    int opt_verify_marks = 1;  // the partitioned query's marks: 1 = write-combined lists (k_mark_split / k_mark_apply), 0 = device atomics in the verification kernel
    int stat_mark_path = 0;    // the marks of the last query's mask: 1 = through the lists, 0 = device atomics or the direct kernel ("query_mark_path")
    int64_t stat_mark_fallback = 0;  // entries of the last query's lists that found a ring or region full and were ORed straight into the mask ("query_mark_fallback")
    int64_t opt_part_min_tiles = 256;  // never cut batches smaller than this many 512-word tiles
    int64_t opt_part_budget = 0;  // bytes of partition buffers per batch; 0 = automatic (part_budget())
    int opt_query_mode = 0;    // 0 auto, 1 direct loads, 2 partitioned
    // deferred apply (insert and query of a round both in one tile batch): the insert stops after its level-2 binning and the
    // query's lookup kernel builds every filter slice itself (k_apply_lookup), so the filter is written once and never read back
    int opt_fuse = 1;
    bool pending_apply = false;   // the filter in HBM does not hold the last insert yet
    bool pending_fresh = false;
    bool pending_shard = false;   // ... and that insert was a sharded one (tpc_shard_apply*): its overflow entries wait in the pass' apply-side list
    TpcPartPlan pending_pl;
    void *ikeep[2] = {nullptr, nullptr};  // the insert's level-2 regions and counts while an apply is pending
    size_t ikeep_bytes[2] = {0, 0};
    uint64_t *ikeep_ovf = nullptr;        // ... and its overflow entries (the query reuses the overflow list), [0, n) as
    uint64_t ikeep_ovf_cap = 0;           //     produced, [cap, cap + n) grouped by slice for the fused kernel
    uint64_t pending_novf = 0;
    uint32_t *iovf_cnt = nullptr;         // [2 x slices] count and cursor of the grouping
    uint64_t *iovf_off = nullptr;         // [slices + 1]
    uint32_t iovf_slices = 0;
    int64_t stat_fused = 0;
    int64_t stat_query_overflow = 0;  // entries the last partitioned query batch handed to its overflow list
    int64_t stat_insert_overflow = 0; // ... and the last partitioned insert batch
    int64_t stat_pbuf_releases = 0;  // times the partition buffers were given back to let a second-pass allocation through
    // address-sharded filter (tpc_shard_*)
    uint32_t sh_rank = 0, sh_world = 1;
    TpcPartPlan sh_ipl;
    TpcQPlan sh_qpl;
    bool sh_have[2] = {false, false};
    uint64_t sh_per[2] = {0, 0}, sh_batches[2] = {0, 0};
    uint64_t sh_nsurv = 0;
    bool sh_defer = false;   // the insert plan at hand may leave its apply to the query's lookup (one batch, room for its level-2 regions)
    // Overflow lists of a sharded pass, two per pass (round 4): the hash kernels append to the PRODUCED list (tpc_shard_overflow_get
    // reads it), tpc_shard_overflow_set writes the gathered entries into the APPLIED list, which the apply side extends (level-2
    // losses) and consumes (k_part_ovf / k_q_ovf).  With one list per pass a hash running under the previous batch's exchange
    // (tpc_shard_hash_begin) would append to the list that exchange is about to overwrite.
    bool sh_ovf_set[2] = {false, false};   // tpc_shard_overflow_set was called since the last apply of the pass
    hipStream_t stream2 = nullptr;         // tpc_shard_hash_begin: the hash of a pass beside the main stream's work
    bool sh_async[2] = {false, false};     // a hash of the pass is in flight on stream2
    unsigned long long sh_ov_host[2][2] = {{0, 0}, {0, 0}};
    // combined exchange (tpc_combine_*, tpc_combine.hip): option replicate_filter keeps the WHOLE filter on every rank of a sharded
    // context (sh_world > 1); tpc_pass1_insert / tpc_pass1_query then run the one-GPU passes over this rank's chunk of the tiles
    int opt_replicate = 0;
    bool qb_valid = false;               // tpc_pass1_query_begin enqueued the first batch's hash and binning of the query of [qb_lo, qb_hi]
    uint64_t qb_lo = 0, qb_hi = 0;       //   (anything that reallocates or writes a partition buffer, or changes the text, clears it)
    TpcQPlan qb_pl;                      // ... under this plan (geometry, tiles per batch, buffers): the query reuses it, never plans again
    int64_t stat_q_plan[3] = {0, 0, 0};  // tiles per batch, b1, b2 of the last partitioned query
    int stat_q_begun = 0;                // the last query's first batch was the one tpc_pass1_query_begin binned
    bool pending_lists = false;          // the pending (deferred) insert lives in imported set-bit lists (cmb_ls), not in level-2 regions
    TpcListSrc cmb_ls;                   // ... these (payload and directories are the caller's device buffers)
    TpcPartPlan cmb_geo;                 // slice geometry of the last deferred insert (tpc_combine_export / _merge / _import agree on it)
    bool cmb_have_geo = false;
    uint64_t *cmb_base = nullptr;        // device, [64]: first unit of every source block
    unsigned long long *cmb_cur = nullptr;  // device, [65]: units claimed per destination block, overflow flag
    // timing
    hipEvent_t ev0[TPC_K_COUNT]{}, ev1[TPC_K_COUNT]{};
    bool ev_used[TPC_K_COUNT]{};
    // debug switches, read from the environment once per context (not on every pass)
    bool dbg_ovf = false, dbg_phases = false, dbg_timing = false, no_lean = false;
    uint64_t reserve_text_bytes = 0;  // tpc_reserve ran before the upload: bytes the text will need, kept out of the buffer budget
};

namespace tpch {

int fail(tpc_ctx *c, int code, const char *fmt, ...);
TpcLaunch make_launch(const tpc_ctx *c);
TpcLaunch make_launch_periodic(const tpc_ctx *c);  // + the periodic-window masks (the hash kernels of tpc_pass1_insert / tpc_pass1_query only)
void ensure_periodic(tpc_ctx *c);
uint64_t rotln_host(uint64_t x, int L, int r);
hipError_t dev_malloc(tpc_ctx *c, void **p, size_t bytes);  // hipMalloc; gives the partition buffers back and tries again when it does not fit
int read_counter(tpc_ctx *c, int i, uint64_t *out);
int materialize_reset(tpc_ctx *c);      // a pending tpc_filter_reset becomes a real zero fill
int flush_pending_apply(tpc_ctx *c);    // the deferred apply of the last insert, for anything that reads the filter other than the fused lookup
double range_mass(const tpc_ctx *c, uint64_t lo, uint64_t hi);
bool ensure_pbuf(tpc_ctx *c, int i, size_t need);
bool release_partition_buffers(tpc_ctx *c);
uint64_t filter_words_for(int L, uint32_t world);
int64_t part_budget(const tpc_ctx *c);
uint64_t next_batches(uint64_t b);
uint64_t text_tiles512(const tpc_ctx *c);
bool replicated(const tpc_ctx *c);      // option replicate_filter on a rank of a sharded context
void pass_tiles(const tpc_ctx *c, uint64_t &t_begin, uint64_t &t_end);
uint64_t pass_tile_count(const tpc_ctx *c);
size_t qpart_need(const TpcQPlan &pl, int i);
bool part_hash_supported(const tpc_ctx *c);
bool plan_query(const tpc_ctx *c, uint64_t lo, uint64_t hi, bool gated, TpcQPlan &pl);
int compact_mask(tpc_ctx *c, const uint32_t *m);
void stream_part_release(tpc_ctx *c);   // tpc_capi_pass2.hip
void colors_drop(tpc_ctx *c);           // these twelve and segments_drop: tpc_capi_segments.hip, where who drops whom is written once
void links_drop(tpc_ctx *c);
void bubbles_drop(tpc_ctx *c);
void distances_drop(tpc_ctx *c);
void components_drop(tpc_ctx *c);
void superbubbles_drop(tpc_ctx *c);
void anchors_drop(tpc_ctx *c);
void edges_drop(tpc_ctx *c);
void locate_drop(tpc_ctx *c);
void classes_drop(tpc_ctx *c);
void tracks_drop(tpc_ctx *c);
void variants_drop(tpc_ctx *c);

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) return tpch::fail(c, -10, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int TPC_DISTANCES_TILE = 32;  // tpc_distances.hip: colours on each side of the tile one workgroup of its Gram kernel owns (tpc_get_stat "distances_tile")

struct Timed {
    tpc_ctx *c;
    int which;
    Timed(tpc_ctx *c_, int w) : c(c_), which(w) { (void)hipEventRecord(c->ev0[w], c->stream); }
    ~Timed() { (void)hipEventRecord(c->ev1[which], c->stream); c->ev_used[which] = true; }
};

template <typename T>
int ensure(tpc_ctx *c, T *&p, uint64_t &cap, uint64_t need)
{
    if (need <= cap && p) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    uint64_t n = need + need / 8 + 16;
    HIPCHK(c, dev_malloc(c, (void **)&p, n * sizeof(T)));
    cap = n;
    return 0;
}

}  // namespace tpch

using namespace tpch;
