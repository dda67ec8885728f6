/*
 * twopaco_hip.h -- C-ABI of the MI355X junction-enumeration library (libtwopaco_hip.so).
 *
 * This is the drop-in boundary for TwoPaCo's two-pass junction enumeration.  The reference
 * has no FFI: its operator boundary is the C++ factory TwoPaCo::CreateEnumerator
 * (reference src/graphconstructor/vertexenumerator.h:37-46) whose constructor
 * (vertexenumerator.h:122-466) runs the worker classes below on CPU threads.  Each entry
 * point here replaces one of those workers / data structures; twopaco_amd/host/ keeps the
 * CreateEnumerator signature and calls only this ABI.  Reference paths are relative to
 * /root/reference/src ; VE.h = graphconstructor/vertexenumerator.h.
 *
 * Conventions: plain C, opaque context, int status (0 = ok, <0 = error, text via
 * tpc_last_error).  The caller owns every host buffer; the library owns device memory
 * until tpc_ctx_destroy.  One host thread per context; calls are synchronous with respect
 * to their outputs.  Device pointers (the *_dev entry points) are raw HIP device addresses.
 *
 * Text model.  The reference streams each FASTA record as 'N' + bases + 'N' in overlapping
 * Tasks (VE.h:1108-1226).  The library works on the equivalent global text
 *     T = N rec0 N rec1 N ... rec(S-1) N
 * indexed by a global position g (uint64): base g is the 2-bit code (A0 C1 G2 T3,
 * dnachar.cpp:18-33) at bits 2*(g%32) of bases[g/32] -- the CompressedString layout
 * (compressedstring.h:188-195) -- and bit g%32 of nmask[g/32] is set when T[g] is 'N'
 * (any non-ACGT character, VE.h:1174, and the separators).  A "vertex position" g is the
 * k-mer window T[g..g+k); its sequence coordinate is g - rec_start.
 */
#ifndef TWOPACO_HIP_H_
#define TWOPACO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tpc_ctx tpc_ctx;

#define TPC_MAX_Q 64                   /* hash functions: 1..16 on the rolling kernels (direct and partitioned), 17..64 on closed-form direct kernels */
#define TPC_INVALID_VERTEX INT64_MAX   /* graphconstructor/common.cpp:5                  */

/* Kernel ids for tpc_kernel_ms (hipEvent-timed duration of the last launch of each). */
enum {
    TPC_K_FILTER_RESET = 0, /* ConcurrentBitVector ctor zeroing, concurrentbitvector.cpp:11-24 */
    TPC_K_INSERT = 1,       /* FilterFillerWorker, VE.h:995-1105                               */
    TPC_K_QUERY = 2,        /* CandidateCheckingWorker, VE.h:586-704                           */
    TPC_K_COMPACT = 3,      /* candidate mask -> position list (replaces candidate_<r>.tmp)    */
    TPC_K_FILTER2 = 4,      /* CandidateFinalFilteringWorker, VE.h:708-829                     */
    TPC_K_SCAN2 = 5,        /* TrueBifurcations, VE.h:1228-1256                                */
    TPC_K_SORT = 6,         /* BifurcationStorage::Init sort, bifurcationstorage.h:65          */
    TPC_K_EMIT = 7,         /* EdgeConstructionWorker id lookup, VE.h:927-958                  */
    TPC_K_SPLIT = 8,        /* InitialFilterFillerWorker, VE.h:503-583                         */
    TPC_K_SHARD_HASH = 9,   /* tpc_shard_hash: level 1 of a sharded pass                       */
    TPC_K_SHARD_APPLY = 10, /* tpc_shard_apply: levels 2-3 of a sharded pass                   */
    TPC_K_STREAM = 11,      /* tpc_emit_stream: FlushEdgeResults + JunctionPositionWriter bytes  */
    TPC_K_FUSED = 12,       /* deferred apply: k_q_split + k_apply_lookup (inside TPC_K_QUERY), or the apply alone when it was flushed */
    TPC_K_LOOKUP = 13,      /* the k_apply_lookup launch of TPC_K_FUSED alone (the one kernel insert and query share: its time is split by bytes) */
    TPC_K_COMBINE = 14,     /* tpc_combine_export / tpc_combine_merge: k_slice_combine                                        */
    TPC_K_SEGMENTS = 15,    /* tpc_segments_build_*: names and first-sight bits of the compacted graph's segments, graphdump.cpp:44-113, 398-480 */
    TPC_K_SEGTEXT = 16,     /* tpc_segments_text_*: the graph text rendered from the event table (host/graphformat.h's sinks); summed over the
                               kernels since the last tpc_segments_text_plan (the plan's own included)                                    */
    TPC_K_SKETCH = 17,      /* tpc_distinct_sketch: HyperLogLog registers of the distinct canonical (k+1)-mers (no counterpart in the reference) */
    TPC_K_COLORS = 18,      /* tpc_segments_colors_build: rows, counts and presence bits of the segment colour table (no counterpart in the reference) */
    TPC_K_LINKS = 19,       /* tpc_segments_links_build: the device hash set of the distinct links, their counts and first bits (no counterpart in the reference) */
    TPC_K_BUBBLES = 20,     /* tpc_segments_bubbles_build: arcs, degrees, the simple bubbles and the degree histogram (no counterpart in the reference) */
    TPC_K_DISTANCES = 21,   /* tpc_segments_distances_build: bit columns, weight planes and the two colour x colour matrices (no counterpart in the reference) */
    TPC_K_COMPONENTS = 22,  /* tpc_segments_components_build: the union-find over the link rows, the numbering and the per-component sums (no counterpart in the reference) */
    TPC_K_SUPERBUBBLES = 23, /* tpc_segments_superbubbles_build: the adjacency lists, the bounded search per entrance and the report (no counterpart in the reference) */
    TPC_K_ANCHORS = 24,     /* tpc_segments_anchors_build: the keys, their sort, mates, heads and tails, the blocks and the per-colour sums (no counterpart in the reference) */
    TPC_K_LOCATE = 25,      /* tpc_segments_edges_build / tpc_segments_locate, whichever ran last: the stage on the stream from its first kernel to its last (no counterpart in the reference) */
    TPC_K_CLASSES = 26,     /* tpc_segments_classes_build: the set of rows keyed by their presence words, the numbering and the per-class sums (no counterpart in the reference) */
    TPC_K_TRACKS = 27,      /* tpc_segments_tracks_build: the row of every event, the heads, their scan, the intervals and the sums (no counterpart in the reference) */
    TPC_K_VARIANTS = 28,    /* tpc_segments_variants_build: the walks, their scan, the sorts by row and mask, the alleles, presence and sites (no counterpart in the reference) */
    TPC_K_COUNT = 29
};

/* Context on HIP device `device`.  Fails (non-zero) when no GPU / device is present:
 * there is no CPU fallback behind this ABI. */
int tpc_ctx_create(int device, tpc_ctx **out);
void tpc_ctx_destroy(tpc_ctx *ctx);
const char *tpc_last_error(const tpc_ctx *ctx);

/* Optional: make the runtime load every kernel code object now (an attribute query of one kernel per translation unit,
 * ~30 ms in all) instead of at the first real launch.  Neither call needs a stream or touches context state, so a one-shot
 * caller (the CLI) runs tpc_warmup on a second host thread while it allocates the filter and uploads the text; tpc_preload
 * is the same for a device that has no context yet. */
int tpc_preload(int device);
int tpc_warmup(tpc_ctx *ctx);
/* Optional: allocate the partition buffers of the first pass now, for a text of at most n_text_max positions (after
 * tpc_set_params, before tpc_seq_upload), instead of inside the first tpc_pass1_insert.  A one-shot caller (the CLI) knows
 * an upper bound of the text length from its input files' sizes and lets this run beside parsing: device allocations of
 * tens of GiB take tens of milliseconds (the reference allocates its filter up front too, vertexenumerator.h:258-259). */
int tpc_reserve(tpc_ctx *ctx, uint64_t n_text_max);

/* Hash parameters: vertex length k, filter bits L (filter has 2^L bits), q functions and
 * their character tables seed_table[q][5] (A,C,G,T,N) -- the only entries of
 * CharacterHash::hashvalues the path ever reads (characterhash.h:41-59).  Replaces
 * VertexRollingHashSeed (vertexrollinghash.h:13-52). */
int tpc_set_params(tpc_ctx *ctx, int k, int L, int q, const uint64_t *seed_table);

/* Parse-once replacement for DistributeTasks (VE.h:1108-1226): upload the packed global
 * text.  bases has ceil(n_text/32) uint64 words, nmask ceil(n_text/32) uint32 words;
 * T[0] and T[n_text-1] must be 'N'. */
int tpc_seq_upload(tpc_ctx *ctx, const uint64_t *bases, const uint32_t *nmask, uint64_t n_text);

/* Start a new enumeration over the uploaded text: forgets the junction keys, masks and round
 * state of the previous run (the reference builds a fresh VertexEnumerator per run, VE.h:122). */
int tpc_run_begin(tpc_ctx *ctx);

/* HyperLogLog registers (p = 14: 16384 one-byte registers) of the distinct canonical (k+1)-mers of the uploaded text: the edges
 * tpc_pass1_insert puts into the filter, i.e. the one quantity the right filter size depends on (host/filterplan.h turns the
 * registers into a count and the count into L and rounds; `twopaco -f auto`).  The reference has no counterpart: its README
 * leaves the filter size to a rule of thumb.  Needs tpc_seq_upload only -- no tpc_set_params, L being what the caller is about
 * to decide -- and works after tpc_set_params and after a run as well; it changes nothing a pass reads.  Every call starts from
 * zeroed registers.  With n = k + 1 and h[0..3] = the first four outputs of splitmix64 started at state 0x5457504143 (state +=
 * 0x9E3779B97F4A7C15, then the finaliser tpc_mix64 of csrc/tpc_device.h), every window w = T[g .. g + n) that holds no 'N'
 * (separators included) contributes
 *     F = XOR over t of rotl64(h[w_t], (n - 1 - t) mod 64)        R = XOR over t of rotl64(h[3 - w_t], t mod 64)  (F of the reverse complement)
 *     x = mix64(min(F, R));  idx = x >> 50;  v = x << 14;  rank = 51 if v == 0, else clz64(v) + 1;  reg[idx] = max(reg[idx], rank)
 * Windows with an 'N' contribute nothing (the at most two A/T dummy edges the insert adds beside an 'N' run are not counted).
 * *n_windows (may be NULL) = the number of contributing windows.  A text shorter than n gives all-zero registers and 0.  max is
 * order independent: the result is bit-exact.  k + 1 must fit a tile's halo (k <= 670); a larger k is refused with an error text. */
int tpc_distinct_sketch(tpc_ctx *ctx, int k, uint8_t *registers_host /* [16384] */, uint64_t *n_windows /* may be NULL */);

/* ConcurrentBitVector(2^L) construction = zero fill (concurrentbitvector.cpp:11-24, VE.h:257). */
int tpc_filter_reset(tpc_ctx *ctx);

/* First-pass insert, FilterFillerWorker (VE.h:995-1105): every canonical (k+1)-mer edge of
 * every N-free vertex (A/T dummy edges beside N), gated by the round's vertex-hash range
 * [lo,hi] inclusive (VE.h:1063-1073).  n_kmers (may be NULL) receives the number of vertex
 * positions hashed. */
int tpc_pass1_insert(tpc_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t *n_kmers);

/* Split pass histogram, InitialFilterFillerWorker (VE.h:503-583): uses (and overwrites) the
 * filter as scratch; bins_host receives 2^24 counters (VE.h:471).  records: global start
 * and length of every dispatched record (len >= k), n_rec of them. */
int tpc_pass1_split_hist(tpc_ctx *ctx, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec,
                         uint32_t *bins_host);

/* First-pass query, CandidateCheckingWorker (VE.h:586-704): sets this round's candidate
 * mask (bit g) and returns the number of marks ("Candidate marks count", VE.h:387). */
int tpc_pass1_query(tpc_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t *n_marks);
/* The part of the query that does not read the filter -- level-1 hash and level-2 binning of the first tile batch (the reference's
 * CandidateCheckingWorker computes its hashes before it touches the filter too, VE.h:633-640) -- enqueued on the context's stream; the
 * call returns without waiting.  The tpc_pass1_query of the same range that follows continues from there.  Between the two the caller
 * may move the round's insert between ranks (tpc_combine_merge / _import): the lists travel while the probes are being binned.  Optional. */
int tpc_pass1_query_begin(tpc_ctx *ctx, uint64_t lo, uint64_t hi);

/* Second-pass exact filter over this round's marks, CandidateFinalFilteringWorker
 * (VE.h:708-829) + TrueBifurcations (VE.h:1228-1256): appends the round's junction keys,
 * ORs the round mask into the run-wide mask (MergeOr, VE.h:909-913). Counters as logged at
 * VE.h:384-386. */
int tpc_pass2_filter(tpc_ctx *ctx, uint64_t abundance, uint64_t *n_true, uint64_t *n_false, uint64_t *table_size);

/* The same filter with its table sharded by key hash over `world` ranks (multi-GPU runs whose candidate marks stay on the rank
 * that hashed them, twopaco_amd/dist.py): tpc_pass2_marks compacts this round's mask into the ordered list of marked positions
 * (*n_marks of them, kept for the output pass); tpc_pass2_mark_owners copies that list to pos_dev and writes the rank that owns
 * each position's canonical key -- every occurrence of a k-mer, on either strand, goes to one owner; the host layer routes the
 * positions (tpc_shard_route / tpc_shard_permute64, a variable all-to-all of 8 bytes per marked position) and
 * tpc_pass2_filter_positions runs the exact filter over the positions a rank received: complete (prev, next) sets and counts per
 * key, hence the reference's verdict; it appends this rank's junction keys (to be all-gathered:
 * tpc_junction_keys_export / _import) and merges the round mask as tpc_pass2_filter does.  Needs the whole text on the rank. */
int tpc_pass2_marks(tpc_ctx *ctx, uint64_t *n_marks);
int tpc_pass2_mark_owners(tpc_ctx *ctx, uint32_t world, uint64_t *pos_dev, int32_t *owner_dev);
int tpc_pass2_filter_positions(tpc_ctx *ctx, const uint64_t *pos_dev, uint64_t n, uint64_t abundance, uint64_t *n_true, uint64_t *n_false,
                               uint64_t *table_size);
/* Text-free variant of the above: what travels is a record of key_words + 1 uint64 per marked position -- the canonical key and
 * prev | next << 3 as its strand sees them (candidateoccurence.h:25-50) -- so the owner needs none of the text and every rank
 * can keep just its chunk (option text_window).  tpc_pass2_mark_records writes the records of this rank's marks and their
 * owners, the host layer routes the rows (tpc_shard_route + tpc_shard_permute_rows, variable all-to-all),
 * tpc_pass2_filter_records is the exact filter over the received records. */
int tpc_pass2_mark_records(tpc_ctx *ctx, uint32_t world, uint64_t *records_dev, int32_t *owner_dev);
int tpc_pass2_filter_records(tpc_ctx *ctx, const uint64_t *records_dev, uint64_t n, uint64_t abundance, uint64_t *n_true, uint64_t *n_false,
                             uint64_t *table_size);
/* Combine before routing, second pass: tpc_pass2_aggregate_records runs the exact filter over this rank's OWN marks first (into its
 * table: CandidateFinalFilteringWorker's map per rank, VE.h:708-829) and writes one record per DISTINCT key -- the key and, in the last
 * word, bit 63 | the letter sets of prev / next, "seen at least twice" and the occurrence count its marks add up to -- with the key's
 * owner; *n_records of them (<= the rank's marks: size the buffers for those).  On many-genome inputs a key is marked dozens of times, so
 * far fewer rows travel (M2 at two ranks: 22 M marks -> ~1 M records per rank).  The rows are routed as before and
 * tpc_pass2_filter_aggregated merges what a rank received: sets OR-ed, counts added, the reference's verdict (isBif, abundance cut) on
 * the sums.  Occurrences are counted whenever `abundance` is a real cut (< 2^40) -- pass the same value to both calls on every rank.
 * tpc_pass2_filter_records takes aggregated and per-position records alike (under a cut below 2^40 it counts, as the aggregated call does);
 * what differs is how the table is sized. */
int tpc_pass2_aggregate_records(tpc_ctx *ctx, uint32_t world, uint64_t abundance, uint64_t *records_dev, int32_t *owner_dev, uint64_t *n_records);
int tpc_pass2_filter_aggregated(tpc_ctx *ctx, const uint64_t *records_dev, uint64_t n, uint64_t abundance, uint64_t *n_true, uint64_t *n_false,
                                uint64_t *table_size);
int tpc_shard_permute_rows(tpc_ctx *ctx, const uint64_t *src_dev, const uint32_t *perm_dev, uint64_t n, int row_words, uint64_t *dst_dev);

/* BifurcationStorage::Init (bifurcationstorage.h:27-66): sort all junction keys in
 * CompressedString::Less order (compressedstring.h:93-104) and build the id index. */
int tpc_junctions_finalize(tpc_ctx *ctx, uint64_t *n_junctions);

/* Capacity in 64-bit words of one key: CalculateNeededCapacity (candidateoccurence.h:129-133). */
int tpc_key_words(const tpc_ctx *ctx);

/* Sorted junction keys, n_junctions x key_words uint64 (what bifurcations.bin holds, sorted). */
int tpc_junction_keys(tpc_ctx *ctx, uint64_t *keys_host);

/* Junction keys appended so far by tpc_pass2_filter, unsorted (the content of the reference's
 * bifurcations.bin scratch file, VE.h:219,1228-1256): *n receives their number; keys_host (may be
 * NULL to query n only) receives n x key_words words.  tpc_junction_keys_set replaces the set --
 * the multi-GPU driver uses the pair to union the per-rank sets before tpc_junctions_finalize. */
int tpc_junction_keys_raw(tpc_ctx *ctx, uint64_t *keys_host, uint64_t *n);
int tpc_junction_keys_set(tpc_ctx *ctx, const uint64_t *keys_host, uint64_t n);
/* The same pair on DEVICE buffers, so that the union of the per-rank key sets can be all-gathered without
 * touching the host: _export copies min(n, cap_keys) keys to dst_dev and reports n; _import replaces
 * (append = 0) or extends (append = 1) the set with n keys from src_dev. */
int tpc_junction_keys_export(tpc_ctx *ctx, uint64_t *dst_dev, uint64_t cap_keys, uint64_t *n);
int tpc_junction_keys_import(tpc_ctx *ctx, const uint64_t *src_dev, uint64_t n, int append);

/* BifurcationStorage::GetId (bifurcationstorage.h:100-127) for one k-mer given as k ASCII
 * characters: +(rank+1), -(rank+1) or TPC_INVALID_VERTEX.  Host-side binary search over the
 * downloaded keys (VertexEnumerator::GetId is a cold query API, VE.h:99-102). */
int64_t tpc_get_id(tpc_ctx *ctx, const char *kmer);

/* Output pass id lookup, EdgeConstructionWorker (VE.h:927-940): for every marked N-free
 * position of the run-wide mask, in increasing g, its junction id (or TPC_INVALID_VERTEX for
 * a Bloom false positive).  Results stay in device memory; n_marked = list length, n_valid =
 * entries with a real id. */
int tpc_emit(tpc_ctx *ctx, uint64_t *n_marked, uint64_t *n_valid);
/* Copy the emit lists to the host: g_host[n_marked], id_host[n_marked]. */
int tpc_emit_fetch(tpc_ctx *ctx, uint64_t *g_host, int64_t *id_host);

/* The (position, id) lists tpc_emit left on the device, out to / in from device buffers: a multi-GPU host whose ranks each looked up
 * the ids of their own marked positions gathers the lists (in rank order = position order) on the rank that formats the
 * output and installs them there before tpc_emit_stream. */
int tpc_emit_export(tpc_ctx *ctx, uint64_t *g_dev, int64_t *id_dev);
int tpc_emit_import(tpc_ctx *ctx, const uint64_t *g_dev, const int64_t *id_dev, uint64_t n);

/* The output file's bytes, built on the device after tpc_emit: FlushEdgeResults (VE.h:837-854) +
 * JunctionPositionWriter::WriteJunction (junctionapi.h:118-132).  12-byte little-endian records
 * (u32 position in its sequence, i64 id) in (sequence, position) order; the first / last k-mer of
 * every sequence of >= k bases without a junction id gets a stub id n_junctions + 42, + 43, ...
 * (VE.h:419, 942-948); one separator (0xFFFFFFFF, INT64_MAX) per sequence-id step before the first
 * record of a sequence (junctionapi.h:120-123).  rec_start / rec_len: global text position and
 * length of EVERY input sequence (n_rec of them, short ones included: they consume an id).
 * n_bytes = stream length, n_records = records without separators ("True marks count", VE.h:451).
 * tpc_emit_stream_fetch copies [offset, offset + nbytes) to the host and may be called from several
 * threads at once (each into its own buffer; pinned buffers from tpc_host_alloc copy fastest). */
int tpc_emit_stream(tpc_ctx *ctx, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec, uint64_t *n_bytes, uint64_t *n_records);
int tpc_emit_stream_fetch(tpc_ctx *ctx, uint64_t offset, uint64_t nbytes, void *dst_host);

/* The junction stream cut over the ranks of a multi-GPU run (each holds the marks and ids of its own chunk of the text after
 * tpc_emit): every rank formats and writes its own byte range of the file, nobody gathers (position, id) lists.  The
 * reference's ordered flush (FlushEdgeResults, VE.h:837-854; JunctionPositionWriter, junctionapi.h:118-126) becomes an
 * exclusive scan over per-sequence counts.  Every slot of the stream belongs to a text position (a record to its k-mer, a
 * stub to the end k-mer it stands for, the separator between sequences j and j + 1 to the character in front of j + 1), so
 * the slots of a chunk [chunk_lo, chunk_hi) are contiguous in the file.
 *   tpc_shard_chunk          this rank's chunk of text positions (the tiles it hashes; the last rank's end is UINT64_MAX)
 *   tpc_emit_stream_partial  per sequence: cnt_host[r] = real-id records among THIS rank's marks, flags_host[r] bit 0 / 1 =
 *                            this rank holds the first / last k-mer of the sequence with a real id
 *   (the host adds the ranks up: gflags = OR of the flags | 4 for sequences of >= k bases; per sequence n = sum of cnt + stubs,
 *    e_scan / s_scan = exclusive scans of n / stubs over the sequences (n_rec + 1 entries); before[r] = cnt of the ranks before
 *    this one; r_last = last sequence of >= k bases; slot0 = slots of the ranks before this one)
 *   tpc_emit_stream_part     formats this rank's n_slots slots (12 bytes each) into the stream buffer; fetch with
 *                            tpc_emit_stream_fetch (offsets relative to the rank's first byte) */
int tpc_shard_chunk(const tpc_ctx *ctx, uint64_t *chunk_lo, uint64_t *chunk_hi);
int tpc_emit_stream_partial(tpc_ctx *ctx, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec, uint64_t *cnt_host, uint32_t *flags_host);
int tpc_emit_stream_part(tpc_ctx *ctx, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec, const uint32_t *gflags_host,
                         const uint64_t *e_scan_host, const uint64_t *s_scan_host, const uint64_t *before_host, uint32_t r_last,
                         uint64_t chunk_lo, uint64_t chunk_hi, uint64_t slot0, uint64_t n_slots, uint64_t *n_bytes);
int tpc_host_alloc(void **ptr, uint64_t bytes);
void tpc_host_free(void *ptr);

/* One rank (world == 1, e.g. the sharded protocol exercised on a single device): the survivors of the last tpc_shard_apply(QUERY)
 * are verified against hash functions 1..q-1 and marked in place -- every survivor is home and every probe address is owned here,
 * so none of the routing calls below is needed (reference: CandidateCheckingWorker's remaining probes, vertexenumerator.h:640-660). */
int tpc_shard_verify_local(tpc_ctx *ctx);

/* Periodic windows under sharding.  A position whose k + 2 characters repeat those of the position 1 .. 63 before it (homopolymers,
 * microsatellites, telomeres) would send the same probes and the same insert as that position (CandidateCheckingWorker / FilterFillerWorker see
 * the same window: vertexenumerator.h:633-674, 1035-1092); the one-GPU passes skip such positions and copy the verdict afterwards.  A host
 * of the sharded calls opts in with tpc_set_option(ctx, "shard_periodic_skip", 1) before tpc_shard_plan -- tpc_shard_hash then skips them
 * too -- and MUST call tpc_shard_periodic_copy once per round, after the marks of the round's last query batch (tpc_shard_finish /
 * tpc_shard_mark / tpc_shard_verify_local) and before anything reads the round mask (mask union, tpc_pass2_marks).  The source of a copy
 * lies in the same 512-word tile, i.e. on the same rank.  Without the option nothing is skipped and the call does nothing.
 * The call is k_periodic_copy alone over whatever the round mask holds: mark(i) = mark(i - distance(i)) at every copying position, in
 * ascending order, every other position unchanged -- on a one-rank context with the option set, after tpc_mask_import, it can be driven
 * with any marks (tests/test_gpu_periodic.py). */
int tpc_shard_periodic_copy(tpc_ctx *ctx);
/* Read-out of the periodic-window masks (tests): builds them for this text and k if they are not built, as the first partitioned pass
 * would, and copies to the host the bits of the copying positions (qs_host, tpc_mask_words words), the six bit planes of their copy
 * distance 1 .. 63 (planes_host, plane b at b * tpc_mask_words) and the bits of the positions whose insert is dropped (ins_host); bit b of
 * word w = position 32 w + b, as in the round mask.  All zero when the text has no such position, when option periodic_skip is 0, and on
 * a sharded context that did not opt in.  Changes nothing a pass would not have changed. */
int tpc_periodic_download(tpc_ctx *ctx, uint32_t *qs_host, uint32_t *planes_host, uint32_t *ins_host);

/* ---- address-sharded filter (multi-GPU) -------------------------------------------------
 * The Bloom filter (ConcurrentBitVector bitVector, VE.h:257) is cut over `world` ranks (a power of
 * two) by bit address: the partitioned passes route every address to the workgroup that owns its
 * filter slice, and rank r owns the slices of the level-1 buckets b1 with b1 % world == r.  Rank r
 * hashes the r-th contiguous chunk of the text's tiles (and, with option text_window, holds only that
 * chunk + halo); the level-1 regions are what travels (one equal-split all_to_all per pass and batch).  The library does no communication:
 * the caller (twopaco_amd/dist.py over torch.distributed, or MPI/RCCL in a C++ host) moves the
 * DEVICE buffers named below between the calls.  All ranks must make the same calls with the
 * same lo/hi.  tpc_pass1_insert / tpc_pass1_query refuse to run on a sharded context.
 *
 *   tpc_shard_config   rank/world; reallocates the filter to the 2^L/world-bit shard
 *   tpc_shard_plan     geometry of one pass (TPC_SHARD_INSERT / TPC_SHARD_QUERY), geom[16]:
 *                        [0] batches  [1] tiles (of 16384 positions) per rank and batch
 *                        [2] bytes of one destination block of the region buffer
 *                        [3] bytes of one destination block of the count buffer
 *                        [4] survivor capacity (entries)  [5] overflow capacity (entries)
 *                        [6] bytes per overflow entry  [7] slice_bits  [8] b1  [9] b2
 *                        [10] slice permutation multiplier  [11] its inverse  [12] b3 (0: two levels; filters beyond
 *                        2^38 bits take a third level on the owner: the exchange stays at level 1)
 *                      send and receive buffers hold `world` blocks each
 *   tpc_shard_hash     level 1 of the pass over this rank's tiles of `batch` into send_regions /
 *                      send_counts (block d = entries for rank d); the query also marks the
 *                      N-adjacent vertices of those tiles; *n_overflow = entries that did not fit
 *                      a region (>= 2^62: the overflow list itself overflowed -> unsupported skew)
 *   tpc_shard_overflow_get / _set   the overflow list of the pass (full addresses, any owner):
 *                      ranks all-gather their lists and set the concatenation before _apply
 *   tpc_shard_apply    levels 2-3 over the received blocks: insert ORs the owned slices; query
 *                      tests the first probe of every received edge and keeps the hits as the
 *                      survivor list (*n_survivors; ids relative to the batch)
 *   tpc_shard_pack / tpc_shard_apply_packed   exact-size exchange instead of the equal blocks: the regions have a fixed
 *                      capacity and are ~3/4 full, so after tpc_shard_hash the used prefix of every region is packed
 *                      (block d of packed_dev = the entries for rank d, bytes_per_dest_host[d] bytes, a multiple of 128);
 *                      the host layer moves the count blocks as before (equal all_to_all) and the packed blocks with a
 *                      variable all_to_all, source blocks back to back in rank order, and tpc_shard_apply_packed places
 *                      every received region by a scan of the received counts.  packed_dev holds up to world blocks of
 *                      geom[2] bytes (as the region buffer)
 *   tpc_shard_survivors       copy the survivor ids to a device buffer
 *   tpc_shard_survivor_sources   the rank that hashed each survivor's position (it rides in the id): survivors go BACK to
 *                             that rank (route + variable all_to_all) and are verified there, where their text is -- a
 *                             rank then needs only its own chunk of the packed text (tpc_set_option "text_window")
 *   tpc_shard_verify_addrs    for hash functions fn .. fn+fn_count-1: owner rank and shard-local bit
 *                             address of every survivor id in sid_dev (entry i*fn_count + j)
 *   tpc_shard_probe           answer probes against this rank's shard (hit_dev[i] = 0/1)
 *   tpc_shard_mark            set the candidate mark of every id in sid_dev (all q probes hit)
 *   tpc_shard_route           owner-major send order for `n` probes: perm_dev[i] = slot of item i, counts_host[r] =
 *                             items for rank r (the grouping a host language would do with a sort; world <= 64).  An owner
 *                             outside [0, world) is an error ("counted x of n items"): perm_dev is then not written
 *   tpc_shard_permute64       dst[perm[i]] = src[i] (the addresses into send order)
 *   tpc_shard_select          the ids of sid_dev whose fn_count answers are all 1; hit_dev holds the answers in SEND
 *                             order (owners answer in the order they were asked), sid_out_dev / *n_out the kept ids
 *   tpc_mask_export / tpc_mask_merge   round mask to / OR of `count` masks from a device buffer:
 *                             the union over ranks is the mask tpc_pass1_query would produce
 *   tpc_mask_export_padded / tpc_mask_or_blocks / tpc_mask_import   the same union as an OR all-reduce by word
 *                             ranges: export padded to world x chunk words, all_to_all of the chunks, fold the
 *                             `count` received chunks, all_gather the folded chunks, import (2 (W-1)/W mask sizes
 *                             per rank on the wire instead of W) */
#define TPC_SHARD_INSERT 0
#define TPC_SHARD_QUERY 1
int tpc_shard_config(tpc_ctx *ctx, uint32_t rank, uint32_t world);
int tpc_shard_plan(tpc_ctx *ctx, int pass, uint64_t lo, uint64_t hi, uint64_t *geom);
int tpc_shard_hash(tpc_ctx *ctx, int pass, uint64_t batch, uint64_t lo, uint64_t hi, void *send_regions_dev, void *send_counts_dev,
                   uint64_t *n_overflow);
/* Overlap of hashing and exchange (round 4).  The level-1 hash of a pass reads the text and writes the caller's send
 * buffers, the pass' produced overflow list and (query) the round mask -- nothing the exchange or the apply of another batch, or of the
 * other pass, touches: the query's hash does not depend on the round's insert at all (reference: CandidateCheckingWorker hashes the same
 * windows FilterFillerWorker did, vertexenumerator.h:633-674 / 1035-1083).
 *   tpc_shard_plan_both   plans insert and query of a round together: shared buffers sized for the larger need, both plans valid
 *   tpc_shard_hash_begin  enqueues the hash of (pass, batch) on the context's second stream and returns at once; the send buffers
 *                         must not be the ones an exchange still reads (double buffering is the caller's); one hash in flight per pass
 *   tpc_shard_hash_end    waits for it; *n_overflow as tpc_shard_hash
 * The overflow lists are two per pass: hashes append to the produced list (tpc_shard_overflow_get), tpc_shard_overflow_set fills the
 * applied one, so a hash running under batch b's exchange cannot disturb the entries batch b's apply is about to consume. */
int tpc_shard_plan_both(tpc_ctx *ctx, uint64_t lo, uint64_t hi, uint64_t *geom_insert /* [16] */, uint64_t *geom_query /* [16] */);
int tpc_shard_hash_begin(tpc_ctx *ctx, int pass, uint64_t batch, uint64_t lo, uint64_t hi, void *send_regions_dev, void *send_counts_dev);
int tpc_shard_hash_end(tpc_ctx *ctx, int pass, uint64_t *n_overflow);
int tpc_shard_overflow_get(tpc_ctx *ctx, int pass, void *dst_dev, uint64_t n);
int tpc_shard_overflow_set(tpc_ctx *ctx, int pass, const void *src_dev, uint64_t n);
int tpc_shard_apply(tpc_ctx *ctx, int pass, uint64_t batch, const void *recv_regions_dev, const void *recv_counts_dev, uint64_t *n_survivors);
int tpc_shard_pack(tpc_ctx *ctx, int pass, const void *send_regions_dev, const void *send_counts_dev, void *packed_dev, uint64_t *bytes_per_dest_host);
int tpc_shard_apply_packed(tpc_ctx *ctx, int pass, uint64_t batch, const void *recv_packed_dev, const void *recv_counts_dev, uint64_t *n_survivors);
/* tpc_shard_apply with this rank's own block read in place: block `rank` of the receive buffers is never touched (the host layer need not
 * copy it), the entries this rank hashed for its own slices are taken from the send buffers tpc_shard_hash filled -- same block index,
 * same layout.  world == 1: the receive buffers may be null.  Option "shard_tight_regions" (default 1) sizes the level-1 regions of the
 * sharded passes at their expected fill + 6 sigma (+ the gate's share in a multi-round pass) instead of the one-GPU 1.3 x: the equal
 * blocks then carry a few per cent of slack and the packing pass (tpc_shard_pack: a read and a write of every entry) can be skipped. */
int tpc_shard_apply_inplace(tpc_ctx *ctx, int pass, uint64_t batch, const void *recv_regions_dev, const void *recv_counts_dev,
                            const void *send_regions_dev, const void *send_counts_dev, uint64_t *n_survivors);
int tpc_shard_survivors(tpc_ctx *ctx, uint64_t *sid_dev);
/* The verification's bookkeeping in fused form (what the calls above do in three or four steps each; same protocol, same results):
 *   tpc_shard_survivors_home  the survivors of the last tpc_shard_apply grouped by the rank that hashed their position, into send_dev
 *                             (n entries, the n tpc_shard_apply returned); counts_host[r] = survivors for rank r (variable all_to_all
 *                             of 8 bytes each); tmp_dev: n uint64 of scratch, unused when world == 1
 *   tpc_shard_verify_send     shard-local bit addresses of hash functions fn .. fn+fn_count-1 of every survivor id in sid_dev, already in
 *                             owner-major send order: send_dev[n * fn_count], perm_dev[i * fn_count + j] = slot of survivor i's j-th
 *                             probe, counts_host[r] = probes for rank r; tmp_dev: n * fn_count uint64 of scratch.  world == 1: the
 *                             natural order is the send order; tmp_dev and perm_dev are not used (pass perm_dev = NULL on)
 *   tpc_shard_finish          last round of a batch: the candidate mark of every survivor whose fn_count answers (hit_dev, in send
 *                             order; perm_dev NULL = natural order) are all 1 -- tpc_shard_select + tpc_shard_mark without the list
 *                             in between; *n_marked = how many passed (survivors, not bits: an id given twice counts twice).
 *                             tpc_shard_select takes perm_dev = NULL the same way.
 *   Alignment: with perm_dev = NULL and fn_count = 4, tpc_shard_select and tpc_shard_finish read the four answers of a survivor as
 *   one 32-bit word, so hit_dev must then be 4-byte aligned (any device allocation is; a pointer INTO a buffer of answers must be
 *   taken at a multiple of four), and the answers must be the bytes 0 and 1 that tpc_shard_probe writes. */
int tpc_shard_survivors_home(tpc_ctx *ctx, uint64_t *tmp_dev, uint64_t *send_dev, uint64_t *counts_host);
int tpc_shard_verify_send(tpc_ctx *ctx, int fn, int fn_count, const uint64_t *sid_dev, uint64_t n, uint64_t *tmp_dev, uint64_t *send_dev, uint32_t *perm_dev,
                          uint64_t *counts_host);
int tpc_shard_finish(tpc_ctx *ctx, const uint64_t *sid_dev, uint64_t n, int fn_count, const uint8_t *hit_dev, const uint32_t *perm_dev, uint64_t *n_marked);
int tpc_shard_survivor_sources(tpc_ctx *ctx, const uint64_t *sid_dev, uint64_t n, int32_t *source_dev);
int tpc_shard_verify_addrs(tpc_ctx *ctx, int fn, int fn_count, const uint64_t *sid_dev, uint64_t n, uint64_t *addr_dev, int32_t *owner_dev);
int tpc_shard_probe(tpc_ctx *ctx, const uint64_t *addr_dev, uint64_t n, uint8_t *hit_dev);
int tpc_shard_mark(tpc_ctx *ctx, const uint64_t *sid_dev, uint64_t n);
int tpc_shard_route(tpc_ctx *ctx, const int32_t *owner_dev, uint64_t n, uint32_t *perm_dev, uint64_t *counts_host);
int tpc_shard_permute64(tpc_ctx *ctx, const uint64_t *src_dev, const uint32_t *perm_dev, uint64_t n, uint64_t *dst_dev);
int tpc_shard_select(tpc_ctx *ctx, const uint64_t *sid_dev, uint64_t n, int fn_count, const uint8_t *hit_dev, const uint32_t *perm_dev,
                     uint64_t *sid_out_dev, uint64_t *n_out);
int tpc_mask_export(tpc_ctx *ctx, uint32_t *dst_dev);
int tpc_mask_merge(tpc_ctx *ctx, const uint32_t *src_dev, uint32_t count);
int tpc_mask_export_padded(tpc_ctx *ctx, uint32_t *dst_dev, uint64_t total_words);
int tpc_mask_or_blocks(tpc_ctx *ctx, const uint32_t *blocks_dev, uint32_t count, uint64_t words, uint32_t *out_dev);
int tpc_mask_import(tpc_ctx *ctx, const uint32_t *src_dev);

/* ---- combined exchange: the filter REPLICATED through set-bit lists (multi-GPU, round 6) --------------------------------------
 * The reference's threads share one ConcurrentBitVector for free (fetch_or, concurrentbitvector.cpp:31-45; MergeOr :115-122).  Routing
 * every hash hit to the rank that owns its slice (tpc_shard_* above) moves 4 bytes per insert address and 8 per query probe; but an
 * insert matters only the first time a bit is set, and a rank's write-combining passes OR its inserts into LDS slices anyway.  Here
 * every rank keeps the WHOLE filter (option "replicate_filter" = 1 before tpc_shard_config / tpc_set_params; sensible while 2^L / 8
 * bytes fit one GPU beside the partition buffers) and hashes only its chunk of the text:
 *   tpc_filter_reset, tpc_pass1_insert   the one-GPU insert over this rank's chunk of the tiles (tpc_shard_chunk); with one tile
 *                          batch its apply is deferred: the entries wait in their level-2 regions
 *   tpc_combine_info       info[0] = 1: they do, lists can be exported ([1] slices, [2] 2^16-bit windows per slice, [3] upper bound of
 *                          a destination block in 16-byte units for `n_dest` destinations, [4] slice_bits, [5] b1, [6] b2, [7] directory
 *                          entries per destination block); info[0] = 0: the insert was applied to this rank's dense filter (several
 *                          batches, three levels, no memory): OR-reduce the filters instead (tpc_filter_copy_out / tpc_mask_or_blocks /
 *                          tpc_filter_copy_in: an all_to_all of word ranges, a fold, an all_gather)
 *   tpc_combine_export     every slice built in LDS from the rank's own entries; its SET BITS leave as 16-bit offsets per
 *                          2^16-bit window (csrc/tpc_lists.h): block d of payload_dev (cap_units 16-byte units each) = the slices of
 *                          the level-1 buckets b1 % n_dest == d in the order [b1 / n_dest][b2]; dir_dev[d][slice][window] =
 *                          first unit << 24 | entries; units_host[d] = units used.  2 bytes per DISTINCT set bit of the chunk
 *   (exchange, the host's: an all-gather of the exports, blocks and directories; or a reduce-scatter -- block d and its directory to rank d)
 *   tpc_combine_merge      reduce-scatter only: the owner ORs the n_src = world received blocks (source s at unit src_base_host[s], its
 *                          directory at dir_dev + s * stride, stride = info[7]) slice by slice and emits the merged lists of ITS slices
 *                          (one block, directory [slice][window]); the sum of the received units always suffices as capacity
 *   (all-gather of the merged blocks and their directories)
 *   tpc_combine_import     the lists every slice is to be built from: n_src blocks (block s at unit src_base_host[s], its directory at
 *                          dir_dev + s * dir_stride).  n_owner = W > 0 (all-gathered blocks): block s lists only the slices of the
 *                          level-1 buckets b1 % W == s % W, keyed [b1 / W][b2] -- the W merged blocks of tpc_combine_merge (n_src = W),
 *                          or all W x W blocks of the ranks' exports, rank-major (n_src = W * W, no reduce-scatter); n_owner = 0: every
 *                          block lists every slice (exports with n_dest = 1).  The insert is then pending again: the buffers must stay
 *                          untouched until the query ran
 *   tpc_pass1_query        the one-GPU query over this rank's chunk; its first lookup builds every slice from the lists, writes it to
 *                          the rank's filter and tests the chunk's probes in LDS: no probe, no survivor, no answer crosses a link.
 *                          The round mask then holds the marks of this rank's positions (as after tpc_shard_finish: second pass sharded
 *                          by key hash, tpc_pass2_marks ...)
 *   tpc_combine_choose     the bytes model both hosts print and follow: bytes a rank receives per round for (1) all-gather of exports,
 *                          (2) reduce-scatter + all-gather of merged lists, (3) dense OR all-reduce, from the mean export size; returns
 *                          the cheapest.  No context: pure arithmetic. */
int tpc_combine_info(tpc_ctx *ctx, uint32_t n_dest, uint64_t *info /* [8] */);
int tpc_combine_export(tpc_ctx *ctx, uint32_t n_dest, uint16_t *payload_dev, uint64_t cap_units, uint64_t *dir_dev, uint64_t *units_host);
int tpc_combine_merge(tpc_ctx *ctx, uint32_t n_src, const uint16_t *payload_dev, const uint64_t *src_base_host, const uint64_t *dir_dev, uint16_t *out_payload_dev,
                      uint64_t out_cap_units, uint64_t *out_dir_dev, uint64_t *units_host);
int tpc_combine_import(tpc_ctx *ctx, uint32_t n_src, uint32_t n_owner, const uint16_t *payload_dev, const uint64_t *src_base_host, const uint64_t *dir_dev, uint64_t dir_stride);
int tpc_combine_choose(uint32_t world, int L, uint64_t mean_export_units, double *bytes /* [3] */);
/* Words [word0, word0 + n_words) of the filter to / from a device buffer (the dense form of the exchange; a pending insert is applied first). */
int tpc_filter_copy_out(tpc_ctx *ctx, uint64_t word0, uint64_t n_words, uint32_t *dst_dev);
int tpc_filter_copy_in(tpc_ctx *ctx, uint64_t word0, uint64_t n_words, const uint32_t *src_dev);

/* ---- segment table of the compacted graph (graphdump's walk on the device) ----------------------------------------------------
 * graphdump's gfa1 / gfa2 / fasta formats walk the junction stream one record at a time: every pair of consecutive records of one
 * sequence is a segment occurrence (an EVENT), named by its end junctions and one character of the text, and printed in full
 * at the first sight of its name (graphdump.cpp:44-113 the naming, :398-480 the walk).  The walk is serial because of "first
 * sight" and because segments whose deciding character is 'N' get fresh names 2^34, 2^34 + 1, ... in file order; both are a
 * minimum / a scan over all events.  This group builds, for a stream of n_bytes / 12 slots (the bytes of de_bruijn.bin: a
 * slot is a separator when its position OR its id field holds the separator value, junctionapi.h:91; trailing bytes that do
 * not fill a slot are ignored), one entry per event e in file order:
 *   name[e]   signed segment name, SegmentNamer::Name of twopaco_amd/host/junctiondump.cpp (graphdump.cpp:44-113)
 *   first[e]  bit e % 32 of word e / 32: e is the smallest event index with this |name| (exact: a direct-addressed table of
 *             32-bit event indices filled with atomicMin; 'N'-named events are always first)
 *   begin[e], end[e]   the position fields of the event's left and right record (32 bits each)
 *   seq_event_begin[s], s = 0 .. n_rec   the number of events whose sequence id (the count of separator slots before the event)
 *             is < s: the events of sequence s are [seq_event_begin[s], seq_event_begin[s + 1]), entries behind the last
 *             separator hold the event count.  Together with name[] and first[] this EVENT TABLE is all a formatter needs of
 *             the stream (twopaco_amd/host/graphformat.h)
 * and the walk's first error in file order.  The text comes from tpc_seq_upload (tpc_set_params is not needed: a context used only
 * for this holds no filter and no partition buffers); rec_start / rec_len are those of EVERY input sequence, as for tpc_emit_stream;
 * amb_pos (n_amb entries, ascending, may be NULL when n_amb = 0) lists the global text positions that hold a valid letter other
 * than A C G T N: the packed text cannot tell them from 'N', the namer can (graphdump.cpp:75-92: such a letter after the left
 * junction of a forward segment gives the name -1, an 'N' there a fresh name).
 * Memory: the stream (12 B / slot), 8 B / slot of scan scratch, 21 B / event, 4 B / input sequence, and the table of 4 x (largest |name| + 1) bytes,
 * at most 32 x (largest |id| + 1).  A stream of 2^32 - 1 slots or more, or one whose buffers do not fit the free device memory,
 * is refused with an error text (never a fault).
 *   tpc_segments_build_host      from the stream's bytes in host memory (what graphdump reads from the file)
 *   tpc_segments_build_resident  from the stream tpc_emit_stream left on the device in this context; same table
 *   tpc_segments_counts          counts[0] events, [1] distinct segments (first bits set), [2] 'N'-named events, [3] bytes of the
 *                                first-sight table, [4] slots, [5] peak bytes of device memory in use during the build
 *   tpc_segments_error           the first failing pair of consecutive records in file order (what the serial walk would have
 *                                thrown): *slot = slot index of the pair's second record (of the first record of the stream when its
 *                                sequence id is not 0), *kind = 0 none, 1 "The input is corrupted", 2 "A vertex id is too large,
 *                                cannot generate GFA" (|id| >= 2^31 in an event; inside one pair the corruption checks come first).
 *                                The table is built all the same: an event that fails its own checks gets the name 0, every
 *                                other entry is what the rule gives (sequence ids being the count of separators before a slot);
 *                                begin[] / end[] of such an event are unspecified
 *   tpc_segments_fetch_names / _first   name[e0 .. e0 + n) / words [word0, word0 + n_words) of first[] to the host
 *   tpc_segments_fetch_events           begin[e0 .. e0 + n) and end[e0 .. e0 + n) to the host
 *   tpc_segments_fetch_sequences        seq_event_begin[s0 .. s0 + n), s0 + n <= n_rec + 1, to the host
 * A range outside the table is refused with an error text. */
#define TPC_SEG_OK 0
#define TPC_SEG_CORRUPTED 1
#define TPC_SEG_ID_TOO_LARGE 2
int tpc_segments_build_host(tpc_ctx *ctx, const void *stream_host, uint64_t n_bytes, int k, const uint64_t *rec_start, const uint64_t *rec_len,
                            uint32_t n_rec, const uint64_t *amb_pos, uint64_t n_amb);
int tpc_segments_build_resident(tpc_ctx *ctx, int k, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec, const uint64_t *amb_pos,
                                uint64_t n_amb);
int tpc_segments_counts(const tpc_ctx *ctx, uint64_t *counts /* [6] */);
int tpc_segments_error(const tpc_ctx *ctx, uint64_t *slot, int *kind);
int tpc_segments_fetch_names(tpc_ctx *ctx, uint64_t e0, uint64_t n, int64_t *name_host);
int tpc_segments_fetch_first(tpc_ctx *ctx, uint64_t word0, uint64_t n_words, uint32_t *first_host);
int tpc_segments_fetch_events(tpc_ctx *ctx, uint64_t e0, uint64_t n, uint32_t *begin_host, uint32_t *end_host);
int tpc_segments_fetch_sequences(tpc_ctx *ctx, uint64_t s0, uint64_t n, uint32_t *first_event_host);

/* The TEXT of the compacted graph, rendered on the device from the event table of the last build and the letters of
 * tpc_seq_upload (csrc/tpc_segtext.hip): byte for byte what the sinks of twopaco_amd/host/graphformat.h (Gfa1Sink, Gfa2Sink,
 * FastaSink fed by FormatChunk) write for the table, in file order.  The header lines (HeaderLines) are the caller's.
 *   tpc_segments_text_plan   sizes and offsets of every event's lines (a size pass and two 64-bit exclusive scans); *total_bytes =
 *                            the size of the whole text.  Needs a built table whose tpc_segments_error kind is TPC_SEG_OK and the
 *                            text of tpc_seq_upload still resident; refused otherwise, and for a format outside 1..3.
 *                            seq_names / seq_name_off: the names of the n_rec input sequences as one byte blob, name s =
 *                            [seq_name_off[s], seq_name_off[s + 1]) (the caller adds the "s0_" prefix when asked; the kernels only
 *                            copy).  amb_letter[i]: the letter at amb_pos[i] of the build, as the parser upper-cases it (R, Y, K, ...;
 *                            may be NULL when the build had n_amb = 0): a forward body prints it, a reversed one prints 'N'.
 *                            Adds 16 B per event, which count toward counts[5] of tpc_segments_counts; a new build or a new
 *                            plan drops the old plan.
 *   tpc_segments_text_fetch  renders the byte window [byte0, byte0 + n_bytes) of the text and copies it to dst_host.  A window may
 *                            begin or end anywhere (inside a number, a body, a path line); a range outside [0, total) is refused.
 *   tpc_segments_text_write  the whole text to the file descriptor fd: two device windows and two pinned host buffers of
 *                            window_bytes (0 = the library's choice), window i + 1 rendered while window i is copied and a helper
 *                            thread writes it -- with pwrite at file_offset + the bytes so far on a regular file, with write, in
 *                            order, otherwise (a pipe; file_offset is then ignored).  Short writes and EINTR are handled; an I/O
 *                            error ends the call with its text.  *written = bytes written (the caller truncates a file to
 *                            file_offset + *written).
 * Nothing here faults when device memory is short: the call is refused with an error text. */
#define TPC_TEXT_GFA1 1
#define TPC_TEXT_GFA2 2
#define TPC_TEXT_FASTA 3
int tpc_segments_text_plan(tpc_ctx *ctx, int format, const char *seq_names, const uint64_t *seq_name_off /* [n_rec + 1] */,
                           const uint8_t *amb_letter /* [n_amb], may be NULL when n_amb = 0 */, uint64_t *total_bytes);
int tpc_segments_text_fetch(tpc_ctx *ctx, uint64_t byte0, uint64_t n_bytes, void *dst_host);
int tpc_segments_text_write(tpc_ctx *ctx, int fd, uint64_t file_offset, uint64_t window_bytes /* 0 = library's choice */, uint64_t *written);

/* The SEGMENT COLOUR TABLE (csrc/tpc_colors.hip): for every segment of the compacted graph, which colours hold it and how often.
 * No counterpart in the reference; its gfa1 defines the table (an S line with a body is a row, a C line one occurrence of a row in
 * a sequence), and ComputeColors of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The
 * caller maps every input sequence to a colour, color_of_seq[s] in [0, n_colors) for s < n_rec of the build (one colour per file,
 * per sequence, or any other map).  One ROW per segment, that is per event whose first bit is set, in event order -- the order of
 * the body-carrying S lines of gfa1; every 'N'-named event (names >= 2^34) is a row of its own.  For row r with first event e0:
 *   first_event[r]  e0 (name = |name[e0]| and length = end[e0] - begin[e0] + k come from the fetches of the group above)
 *   occurrences[r]  events e with |name[e]| == |name[e0]|
 *   forward[r]      those of them with name[e] > 0
 *   presence[r]     W = ceil(n_colors / 32) words, bit c % 32 of word c / 32 set iff such an event lies in a sequence of colour c
 *   n_colors[r]     popcount of presence[r]
 * and the histogram: segments[n] rows with n_colors == n and bases[n] the 64-bit sum of their lengths, n = 0 .. n_colors (bin 0
 * stays empty).  Separate from the build and opt-in: a context that never calls it holds none of this, and tpc_segments_counts
 * reports what it reported before.
 *   tpc_segments_colors_build           over the table of the last tpc_segments_build_*.  Refused with an error text: no table, a
 *                                       table whose tpc_segments_error kind is not TPC_SEG_OK, n_colors == 0 or above 2^31, a colour >= n_colors,
 *                                       buffers beyond the free device memory.  Memory: 16 B + 4 W B per row and 16 B per histogram
 *                                       bin, kept until the next segment build or colour build; during the call also the first-sight
 *                                       table again (counts[3]), 4 B / event and 4 B / sequence.  Kernel time: TPC_K_COLORS.
 *   tpc_segments_colors_info            info[0] rows, [1] colours, [2] W
 *   tpc_segments_colors_fetch_rows      first_event / occurrences / forward / n_colors of rows [r0, r0 + n) to the host
 *   tpc_segments_colors_fetch_presence  the n x W presence words of rows [r0, r0 + n), row-major
 *   tpc_segments_colors_fetch_hist      segments[0 .. n_colors] and bases[0 .. n_colors]
 * A range outside the table is refused with an error text. */
int tpc_segments_colors_build(tpc_ctx *ctx, const uint32_t *color_of_seq /* [n_rec] */, uint32_t n_colors);
int tpc_segments_colors_info(tpc_ctx *ctx, uint64_t *info /* [3] */);
int tpc_segments_colors_fetch_rows(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *first_event_host, uint32_t *occurrences_host, uint32_t *forward_host,
                                   uint32_t *n_colors_host);
int tpc_segments_colors_fetch_presence(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *words_host /* [n x W] */);
int tpc_segments_colors_fetch_hist(tpc_ctx *ctx, uint64_t *segments_host /* [n_colors + 1] */, uint64_t *bases_host /* [n_colors + 1] */);

/* The LINK TABLE of the compacted graph (csrc/tpc_links.hip): every distinct link between two segments once.  No counterpart in the
 * reference, whose gfa1 prints one L line per occurrence; ComputeLinks of twopaco_amd/host/graphformat.h is the serial statement the
 * kernels are tested against.  The definition, over the event table of the last tpc_segments_build_*:
 *   LINK OCCURRENCE  every event e that is not the first event of its sequence closes an occurrence (name[e - 1], name[e]) -- exactly
 *                    where GfaSink::Segment calls Link, that is one L line of gfa1.
 *   LINK CLASS       occurrences (a, b) and (c, d) are the same link when (c, d) == (a, b) or (c, d) == (-b, -a): the same bidirected
 *                    edge, walked on the other strand.
 *   ROWS             one per class, in the order of the classes' first occurrences in event order.  For row r:
 *     first_event[r]   the event e of the first occurrence; the row is SPELLED as that occurrence, from = name[e - 1], to = name[e]
 *     count[r]         the occurrences of the class
 *     same[r]          those of them spelled exactly as the row (the rest are spelled (-to, -from))
 *   FIRST BITS       link_first: one bit per event, laid out as first[] is (bit e % 32 of word e / 32), set when e closes the first
 *                    occurrence of its class.
 *   'N'-named segments (names >= 2^34) are segments like any other: a link that touches one is simply unique.  A class that is its
 *   own reverse (a+ a-) cannot occur with odd k; it is one class all the same, with same == count.
 * Separate from the build and opt-in: a context that never calls it holds none of this, and tpc_segments_counts reports what it
 * reported before.  It is independent of the colour table: both may be built over one segment table, in either order.
 *   tpc_segments_links_build        over the table of the last tpc_segments_build_*: a device hash set of the classes (open addressing,
 *                                   the smallest power of two >= 2 x occurrences slots, at least 1024, 20 B each during the call).
 *                                   Refused with an error text: no table, a table whose tpc_segments_error kind is not TPC_SEG_OK,
 *                                   more than 2^31 segments, buffers beyond the free device memory, a set that fills up (only with
 *                                   the option test_links_slots_log2); the context stays usable.  Kept until the next segment build
 *                                   or link build: 12 B per row and one bit per event.  Kernel time: TPC_K_LINKS.
 *   tpc_segments_links_info         info[0] rows, [1] occurrences, [2] slots, [3] the stage's device bytes at their peak
 *   tpc_segments_links_fetch_rows   first_event / count / same of rows [r0, r0 + n) to the host
 *   tpc_segments_links_fetch_first  words [word0, word0 + n_words) of link_first, (events + 31) / 32 words in all
 * A range outside the table is refused with an error text. */
int tpc_segments_links_build(tpc_ctx *ctx);
int tpc_segments_links_info(tpc_ctx *ctx, uint64_t *info /* [4] */);
int tpc_segments_links_fetch_rows(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *first_event_host, uint32_t *count_host, uint32_t *same_host);
int tpc_segments_links_fetch_first(tpc_ctx *ctx, uint64_t word0, uint64_t n_words, uint32_t *bits_host);

/* The SIMPLE BUBBLES of the compacted graph (csrc/tpc_bubbles.hip): where the genomes differ.  Two segments leave one side of a
 * segment, touch nothing else, and meet again at one side of another segment: a substitution, a short insertion or a short deletion
 * between genomes; the colour rows of the two arms say which genomes carry which allele.  No counterpart in the reference;
 * ComputeBubbles of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The definition, over the
 * link table of the last tpc_segments_links_build:
 *   ROW              a segment, in the order of gfa1's S lines with a body: the rows of the colour table.
 *   SIDE             an oriented segment, code = row * 2 + (1 when the strand is '-'), in 32 bits; rev(code) = code ^ 1.  2^31 segments
 *                    or more are refused: the code of all ones is kept for "no side" (the lo of a side of degree 0).
 *   ARCS             a link row spelled (from, to) gives the arc from -> to and the arc rev(to) -> rev(from).  When the two are one arc
 *                    (a+ a-, its own reverse) it counts ONCE.  A self-loop a+ a+ gives two different arcs, a+ -> a+ and a- -> a-.
 *   OUT SET, DEGREE  out(u): the heads of the arcs that leave side u.  The link table holds every class once, so no arc arrives twice.
 *                    deg(u) = |out(u)|.  The in-neighbours of v are the rev of out(rev(v)).
 *   SIMPLE BUBBLE at side s, when all of these hold:
 *                      out(s) = {a, b}, two members;
 *                      deg(rev(a)) == 1 and deg(rev(b)) == 1: s is the only way in to each arm;
 *                      deg(a) == 1, deg(b) == 1 and out(a) == out(b) == {t};
 *                      deg(rev(t)) == 2;
 *                      the rows of s, a, b, t are four different rows (no hairpin, no inversion read as a bubble, no arm that is a
 *                      self-loop).
 *   CANONICAL ORIENTATION  every bubble is found twice, at s and at rev(t) with the arms rev(a), rev(b) and the sink rev(s).  It is
 *                    reported ONCE, in the orientation whose source code is the smaller.
 *   ARM ORDER        arm_a is the arm with the smaller code in the reported orientation.
 *   ROW ORDER        bubble rows ascend by source code; a side is the source of at most one bubble, so the order is total.
 *   NOT BUBBLES      three or more alleles at one place (deg(s) >= 3), nested bubbles and longer superbubbles are not simple bubbles
 *                    and are not reported: that is the definition.
 *   SIDE ARRAYS      deg[u], lo[u] = the smallest and hi[u] = the largest member of out(u), for every side u; with deg[u] == 0 lo is all
 *                    ones and hi is 0.  The definition reads only sides of degree 1 (lo is the neighbour) and 2 (lo, hi are the two).
 *   HISTOGRAM        hist[d] = the sides of degree d for d = 0 .. 4, hist[5] = those of degree 5 or more; hist[0] are the dead ends.
 * Separate from the build and opt-in: a context that never calls it holds none of this; tpc_segments_counts, the colour outputs and the
 * link outputs are what they were, in any order of the three builds.
 *   tpc_segments_bubbles_build       over the link table of the last tpc_segments_links_build.  Refused with an error text: no segment
 *                                    table, a table whose tpc_segments_error kind is not TPC_SEG_OK, no link table, 2^31 segments
 *                                    or more, buffers beyond the free device memory; the context stays usable.  Kept until the next
 *                                    segment, link or bubble build: 16 B per bubble, 12 B per side and 48 B of histogram.  TPC_K_BUBBLES
 *                                    times the stage on the stream from its first kernel to its last, the host's one wait for the
 *                                    bubble count and the allocation of the rows included, as TPC_K_LINKS times the link stage.
 *   tpc_segments_bubbles_info        info[0] bubbles, [1] sides (2 x segments), [2] arcs, [3] the stage's device bytes at their peak
 *   tpc_segments_bubbles_fetch_rows  source / arm_a / arm_b / sink (side codes) of bubbles [b0, b0 + n) to the host
 *   tpc_segments_bubbles_fetch_sides deg / lo / hi of sides [c0, c0 + n) to the host
 *   tpc_segments_bubbles_fetch_hist  the six bins
 * A range outside a table is refused with an error text. */
int tpc_segments_bubbles_build(tpc_ctx *ctx);
int tpc_segments_bubbles_info(tpc_ctx *ctx, uint64_t *info /* [4]: bubbles, sides, arcs, peak device bytes */);
int tpc_segments_bubbles_fetch_rows(tpc_ctx *ctx, uint64_t b0, uint64_t n, uint32_t *source, uint32_t *arm_a, uint32_t *arm_b, uint32_t *sink);
int tpc_segments_bubbles_fetch_sides(tpc_ctx *ctx, uint64_t c0, uint64_t n, uint32_t *deg, uint32_t *lo, uint32_t *hi);
int tpc_segments_bubbles_fetch_hist(tpc_ctx *ctx, uint64_t *hist /* [6] */);

/* The GENOME DISTANCE MATRICES (csrc/tpc_distances.hip): how much every colour shares with every other one.  No counterpart in the
 * reference; ComputeDistances of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The
 * definition, over the colour table of the last tpc_segments_colors_build (rows r < S, colours c < C):
 *   ROW              whatever the colour table calls a row: a segment, in the order of gfa1's S lines with a body.  That includes the
 *                    'N'-named rows (names >= 2^34, every one a row of its own) and the rows the reference names -1 for ambiguous
 *                    letters; the stage counts them as the colour table holds them and claims nothing more about them.
 *   WEIGHT           weight[r] = end[e0] - begin[e0] for the row's first event e0: the row's length minus k, the number of
 *                    (k+1)-mers (EDGES) the segment spells.  Edges, not bases: neighbouring segments overlap by k bases, so summed
 *                    lengths would count the junction k-mers twice, while every edge of the compacted graph lies in exactly one
 *                    segment.  32 bits per row, 64 bits when summed.
 *   segments[i][j]   the rows whose presence holds both colour i and colour j.
 *   edges[i][j]      the sum of weight over those rows.
 *   SHAPE            both C x C, uint64, symmetric, stored in full, row-major.  The diagonal holds a colour's own totals; a colour
 *                    that no sequence has is a zero row and a zero column.
 *   EXACT            integers and a commutative sum: the result does not depend on the schedule.  No floating point on the device;
 *                    a reader gets the Jaccard similarity of two colours as edges[i][j] / (edges[i][i] + edges[j][j] - edges[i][j]).
 * Separate from the builds and opt-in: a context that never calls it holds none of this; tpc_segments_counts, the colour outputs,
 * the link outputs and the bubble outputs are what they were, in any order of the builds.
 *   tpc_segments_distances_build  over the colour table of the last tpc_segments_colors_build.  Refused with an error text: no
 *                                 segment table, a table whose tpc_segments_error kind is not TPC_SEG_OK, no colour table (a new
 *                                 segment build drops it), more than 2^24 colours (16 B x C^2 must not wrap; no device holds it), matrices or bit columns beyond the free device memory; the context stays
 *                                 usable.  Kept until the next segment, colour or distance build: 16 B x C^2.  During the call also
 *                                 8 B x C x ceil(S / 64) of colour-major bit columns and 256 B x ceil(S / 64) of weight bit planes.
 *                                 TPC_K_DISTANCES times the stage on the stream from its first kernel to its last.
 *   tpc_segments_distances_info   info[0] colours, [1] rows, [2] weight bit planes used (the bit width of the largest weight),
 *                                 [3] the stage's device bytes at their peak
 *   tpc_segments_distances_fetch  rows [i0, i0 + n_rows) of both matrices to the host, n_rows x C values each
 * A range outside the matrix is refused with an error text. */
int tpc_segments_distances_build(tpc_ctx *ctx);
int tpc_segments_distances_info(tpc_ctx *ctx, uint64_t *info /* [4]: colours, rows, planes used, peak device bytes */);
int tpc_segments_distances_fetch(tpc_ctx *ctx, uint64_t i0, uint64_t n_rows, uint64_t *segments_host /* [n_rows x C] */, uint64_t *edges_host /* [n_rows x C] */);

/* The CONNECTED COMPONENTS of the compacted graph (csrc/tpc_components.hip): which pieces hang together.  No counterpart in the
 * reference; ComputeComponents of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The
 * definition, over the link table of the last tpc_segments_links_build and the colour table of the last tpc_segments_colors_build,
 * both over one segment table:
 *   ROW              a segment.  The rows are the colour table's, in the order of gfa1's S lines with a body.
 *   JOINED           the rows of `from` and `to` of a link row are joined.  Strands do not matter.  A self-loop and a link that is its
 *                    own reverse join a row to itself.  'N'-named segments are segments like any other.
 *   COMPONENT        a class of the transitive closure of JOINED.  A segment that no link touches is a component of one.  Its ROOT
 *                    is its smallest row.
 *   COMPONENT ID     components are numbered from 0, ascending by root: the order in which gfa1 first prints a segment of each.
 *   PER ROW          component[r].
 *   PER COMPONENT p  root[p]; segments[p]; links[p], the link rows whose ends lie in it (every link row lies in exactly one);
 *                    length[p], the sum of its segments' lengths in bases; edges[p], the sum of their weights, end - begin of the
 *                    row's first event, the weight of the distance matrices (length - k per segment); occurrences[p], the sum of the
 *                    colour rows' occurrences; presence[p], the OR of the colour rows' presence words; n_colors[p], its popcount.
 *                    The sums are 64-bit.
 *   CONSEQUENCES     every input sequence with an event lies in exactly one component, because consecutive segments of a sequence
 *                    are linked; with one colour per sequence presence[p] therefore says which contigs make up component p.  The sum
 *                    of segments[p] is the number of rows and the sum of links[p] the number of link rows.
 *   EXACT            integers, commutative sums and ORs, and a root that is the smallest row whatever the order of the atomics: the
 *                    result does not depend on the schedule.
 * Separate from the builds and opt-in: a context that never calls it holds none of this; tpc_segments_counts and the colour, link,
 * bubble and distance outputs are what they were, in any order of the builds.
 *   tpc_segments_components_build          a lock-free union-find over parent[S] (one thread per link row hooks the larger root under
 *                                          the smaller with a compare-and-swap), one flatten pass, a scan for the ids, then the sums.
 *                                          Every loop is counted: a find ends within S steps and a link retries at most S times;
 *                                          reaching the bound (only with the option test_components_step_limit) is an error text
 *                                          ("segment components: gave up ...").  Also refused with an error text: no segment table,
 *                                          a table whose tpc_segments_error kind is not TPC_SEG_OK, no link table, no colour table,
 *                                          2^31 segments or more, buffers beyond the free device memory; the context stays usable.
 *                                          Kept until the next segment, link, colour or component build: 4 B per row, per component
 *                                          4 B of root, 40 B of sums and 4 W B of presence.  During the call 12 B per row of parent,
 *                                          label and flags and the row index of the link stage.  TPC_K_COMPONENTS times the stage on
 *                                          the stream from its first kernel to its last, the host's one wait for the component count
 *                                          included, as TPC_K_BUBBLES times the bubble stage.
 *   tpc_segments_components_info           info[0] components, [1] rows, [2] the segments of the largest component, [3] the stage's
 *                                          device bytes at their peak
 *   tpc_segments_components_fetch_members  component[r] of rows [r0, r0 + n) to the host
 *   tpc_segments_components_fetch_rows     root / segments / links / length / edges / occurrences of components [p0, p0 + n)
 *   tpc_segments_components_fetch_presence the n x W presence words of components [p0, p0 + n), row-major (n_colors is their popcount)
 * A range outside a table is refused with an error text. */
int tpc_segments_components_build(tpc_ctx *ctx);
int tpc_segments_components_info(tpc_ctx *ctx, uint64_t *info /* [4]: components, rows, segments of the largest component, peak device bytes */);
int tpc_segments_components_fetch_members(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *component_host);
int tpc_segments_components_fetch_rows(tpc_ctx *ctx, uint64_t p0, uint64_t n, uint32_t *root_host, uint64_t *segments_host, uint64_t *links_host,
                                       uint64_t *length_host, uint64_t *edges_host, uint64_t *occurrences_host);
int tpc_segments_components_fetch_presence(tpc_ctx *ctx, uint64_t p0, uint64_t n, uint32_t *words_host /* [n x W] */);

/* The SUPERBUBBLES of the compacted graph (csrc/tpc_superbubbles.hip), after Onodera, Sadakane and Shibuya 2013 and bounded to 64
 * sides: where the genomes differ, beyond the two-allele case of the simple bubbles above.  No counterpart in the reference.  The
 * definition, over the link table of the last tpc_segments_links_build and the colour table of the last tpc_segments_colors_build,
 * both over one segment table:
 *   ROW, SIDE, ARC   as of the tpc_segments_bubbles_* group: code = row * 2 + minus, rev(code) = code ^ 1, a link row gives the arcs
 *                    from -> to and rev(to) -> rev(from), out(u) is the set of heads of the arcs that leave u, deg(u) its size.
 *                    in(v) = { rev(w) : w in out(rev(v)) }.
 *   U(s, t)          for sides s != t, the set of sides reachable from s along arcs without leaving t: s and t are included, a path
 *                    may end at t but not continue through it.
 *   SUPERBUBBLE      (s, t) with ENTRANCE s, EXIT t and INSIDE U \ {s, t} when all of the following hold:
 *                    1. deg(s) >= 2 and t is in U.
 *                    2. MATCHING.  U equals the set of sides from which t is reachable along arcs without entering s.  Equivalently, where 3 holds:
 *                       every side of U other than t has all its out-neighbours in U and at least one; every side of U other than s has
 *                       all its in-neighbours in U.
 *                    3. ACYCLIC.  The arcs with both ends in U form no cycle.  This includes no arc t -> s and no self-loop.
 *                    4. ONE STRAND PER SEGMENT.  No two sides of U have the same row.  This excludes hairpins and inversions read as
 *                       bubbles, as the "four different rows" of the simple bubbles does.
 *                    5. MINIMAL.  No side t' of the inside makes (s, t') satisfy 1-4.
 *                    6. BOUNDED.  |inside| <= max_inside, a parameter with default 62 and allowed range 2 .. 62, so a superbubble is at
 *                       most 64 sides and one 64-bit mask covers it.
 *                    A side is the entrance of at most one superbubble; exit(s) is that superbubble's exit, or none.  Nested
 *                    superbubbles are each reported at their own entrance.
 *   REPORTED         (s, t) when exit(s) = t and either code(s) < code(rev(t)) or exit(rev(t)) != rev(s): a structure found from both
 *                    ends appears once, under the smaller entrance; one found from one end only still appears.  Rows ascend by
 *                    entrance code.
 *   PER ROW          entrance, exit; inside, the number of sides of the inside; arcs, the arcs with both ends in U; paths, the distinct
 *                    arc paths from s to t (64 bits: at most 2^60 are possible); min_edges and max_edges, the smallest and largest sum
 *                    over an s-t path of the weights of its inside segments, the weight being that of the distance matrices and the
 *                    components, length - k (64 bits; an indel shows as min != max); presence, the OR of the inside rows' colour
 *                    words, and n_colors, its popcount; its MEMBERS, the inside sides in ascending code.
 *   EXACT            integers with commutative or order-free results: the arrays do not depend on the schedule.
 * Separate from the builds and opt-in: a context that never calls it holds none of this, and the segment, colour, link, bubble,
 * distance and component outputs are what they were, in any order of the builds.
 *   tpc_segments_superbubbles_build            the adjacency lists (CSR over sides, every list ascending), one bounded search per side of
 *                                              degree 2 or more, the reporting rule, and one more walk per reported row for its
 *                                              numbers.  Refused with an error text: no segment table, a table whose tpc_segments_error
 *                                              kind is not TPC_SEG_OK, no link table, no colour table, max_inside outside 2 .. 62, 2^31
 *                                              segments or more, 2^31 links or more, buffers beyond the free device memory; the context
 *                                              stays usable.  Kept until the next segment, link, colour or superbubble build.
 *                                              TPC_K_SUPERBUBBLES times the stage on the stream from its first kernel to its last, the
 *                                              host's one wait for the row and member counts included.
 *   tpc_segments_superbubbles_info             info[0] superbubbles, [1] sides, [2] members in total, [3] entrances without a mirror
 *                                              (exit(s) = t but exit(rev(t)) != rev(s)), [4] the stage's device bytes at their peak,
 *                                              [5] arcs, [6] max_inside of the build
 *   tpc_segments_superbubbles_fetch_adjacency  the CSR offsets [sides + 1] and the heads [arcs]
 *   tpc_segments_superbubbles_fetch_exits      exit[] of sides [c0, c0 + n), all ones standing for none
 *   tpc_segments_superbubbles_fetch_rows       the planes of rows [b0, b0 + n)
 *   tpc_segments_superbubbles_fetch_members    the member offsets [superbubbles + 1] and the member sides [members]
 *   tpc_segments_superbubbles_fetch_presence   the n x W presence words of rows [b0, b0 + n), row-major
 * A range outside a table is refused with an error text. */
int tpc_segments_superbubbles_build(tpc_ctx *ctx, uint32_t max_inside);
int tpc_segments_superbubbles_info(tpc_ctx *ctx, uint64_t *info /* [7] */);
int tpc_segments_superbubbles_fetch_adjacency(tpc_ctx *ctx, uint32_t *offsets_host /* [sides + 1] */, uint32_t *heads_host /* [arcs] */);
int tpc_segments_superbubbles_fetch_exits(tpc_ctx *ctx, uint64_t c0, uint64_t n, uint32_t *exit_host);
int tpc_segments_superbubbles_fetch_rows(tpc_ctx *ctx, uint64_t b0, uint64_t n, uint32_t *entrance_host, uint32_t *exit_host, uint32_t *inside_host, uint32_t *arcs_host,
                                         uint32_t *n_colors_host, uint64_t *paths_host, uint64_t *min_edges_host, uint64_t *max_edges_host);
int tpc_segments_superbubbles_fetch_members(tpc_ctx *ctx, uint32_t *offsets_host /* [superbubbles + 1] */, uint32_t *sides_host /* [members] */);
int tpc_segments_superbubbles_fetch_presence(tpc_ctx *ctx, uint64_t b0, uint64_t n, uint32_t *words_host /* [n x W] */);

/* The ANCHOR BLOCKS of the compacted graph (csrc/tpc_anchors.hip): where the sequence that a colour shares with a reference colour
 * lies in both, in which order, on which strand, and where the match breaks -- a dot plot, a synteny view, a set of liftover
 * anchors.  A block is an exact match, or an exact reverse-complement match, between two intervals in which every (k+1)-mer is unique
 * on both sides: the kind of object MUMmer's maximal unique matches are, read off the graph.  No counterpart in the reference;
 * ComputeAnchors of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The definition, over the
 * event table of the last tpc_segments_build_*:
 *   EVENT, ROW, COLOUR  those of the colour table: an event is one occurrence of a segment, a row one segment in first-sight order,
 *                    the caller gives color_of_seq[s].  R is the reference colour.
 *   COUNT            count[r][c] is the number of events of row r that lie in sequences of colour c.
 *   ANCHOR           an event e of row r in colour c != R is an anchor when count[r][R] == 1 and count[r][c] == 1.
 *   MATE             mate[e] of an anchor is the one event of r in colour R.  Events of colour R have no mate, non-anchors have none.
 *   REVERSE          the anchor is reverse when name[e] and name[mate[e]] have different signs.
 *   'N'-named segments (names >= 2^34) are rows of their own, so they are never anchors.
 *   CONTINUES        an anchor e continues e - 1 when all of these hold: both events lie in the same sequence; e - 1 is an anchor with
 *                    the same reverse flag; mate[e] == mate[e - 1] + 1 when forward, mate[e] == mate[e - 1] - 1 when reverse; both
 *                    mates lie in the same reference sequence.  (Consecutive events of one sequence share their junction:
 *                    end[e - 1] == begin[e].)
 *   BLOCK            a maximal run query_first .. query_last of anchors in which each one continues the one before it.  Its reference
 *                    events ref_first .. ref_last ascend: forward they are mate[query_first] .. mate[query_last], reverse they are
 *                    mate[query_last] .. mate[query_first].  Query interval [begin[query_first], end[query_last] + k), reference
 *                    interval [begin[ref_first], end[ref_last] + k): both have the same length.  anchors = query_last - query_first
 *                    + 1, edges = end[query_last] - begin[query_first].  Blocks are reported ascending by query_first.
 *   PER COLOUR c != R  blocks[c], anchors[c], edges[c] and reverse_edges[c], the edges of the reverse blocks; colour R's entries are 0.
 *                    The edge sums are 64-bit.
 *   REF EDGES        the sum of end - begin over all events of colour R.
 *   SELF-REVERSE-COMPLEMENT segments are treated like any other: their strand is what the names say.
 *   EXACT            integers with commutative sums: the arrays do not depend on the schedule.
 * Separate from the builds and opt-in: a context that never calls it holds none of this, tpc_segments_counts reports what it
 * reported before, and the other tables are what they were, in any order of the builds.
 *   tpc_segments_anchors_build         one key row << bits | colour per event, one radix sort over the key bits in use, the runs of
 *                                      equal keys give count == 1 on both sides and the mates, one thread per event evaluates the
 *                                      continue rule, one scan numbers the blocks.  Refused with an error text: no segment table, a
 *                                      table whose tpc_segments_error kind is not TPC_SEG_OK, n_colors == 0, a colour >= n_colors,
 *                                      ref_color >= n_colors, buffers beyond the free device memory; the context stays usable.  Kept
 *                                      until the next segment build or anchor build: 4 B per event of mates, 16 B per block, 32 B per
 *                                      colour.  TPC_K_ANCHORS times the stage on the stream from its first kernel to its last, the
 *                                      host's one wait for the block count included.
 *   tpc_segments_anchors_info          info[0] blocks, [1] anchors, [2] colours, [3] the reference colour, [4] ref_edges, [5] the
 *                                      stage's device bytes at their peak
 *   tpc_segments_anchors_fetch_mates   mate[] of events [e0, e0 + n), 0xFFFFFFFF standing for none
 *   tpc_segments_anchors_fetch_rows    query_first / query_last / ref_first / ref_last of blocks [b0, b0 + n)
 *   tpc_segments_anchors_fetch_shared  the four per-colour sums, n_colors entries each
 * A range outside a table is refused with an error text. */
int tpc_segments_anchors_build(tpc_ctx *ctx, const uint32_t *color_of_seq /* [n_rec] */, uint32_t n_colors, uint32_t ref_color);
int tpc_segments_anchors_info(tpc_ctx *ctx, uint64_t *info /* [6] */);
int tpc_segments_anchors_fetch_mates(tpc_ctx *ctx, uint64_t e0, uint64_t n, uint32_t *mate_host);
int tpc_segments_anchors_fetch_rows(tpc_ctx *ctx, uint64_t b0, uint64_t n, uint32_t *query_first, uint32_t *query_last, uint32_t *ref_first, uint32_t *ref_last);
int tpc_segments_anchors_fetch_shared(tpc_ctx *ctx, uint64_t *blocks, uint64_t *anchors, uint64_t *edges, uint64_t *reverse_edges /* [n_colors] each */);

/* The EDGE INDEX of the compacted graph and LOCATE (csrc/tpc_locate.hip): is a sequence that was no input in the graph, where, and
 * in which colours.  No counterpart in the reference.  Definitions; host/graphformat.h states them serially.
 *   n = k + 1.  T is the text of tpc_seq_upload that the last segment build read.  A WINDOW W_T(g) = T[g, g + n) is VALID when the
 *   N mask holds none of its positions (letters other than ACGT are N, as in the packed text).  canon(w) = the smaller of w and its
 *   reverse complement.
 *   ROWS             the colour table's: the events whose first bit is set, in event order; e0(r) = the first event of row r.  The
 *                    SPAN of r is the global positions g0(r) + j, 0 <= j < end[e0] - begin[e0], g0(r) = rec_start[seq(e0)] + begin[e0],
 *                    the sequence of an event from seq_event_begin.
 *   EDGE INDEX I     one entry for every position g of some row's span with W_T(g) valid: key canon(W_T(g)), value (g, row).  Where
 *                    several positions share a key the SMALLEST g is the entry and the others are DUPLICATES; span positions with an
 *                    invalid window are SKIPPED.  The result is exact and does not depend on the schedule.
 *   QUERY TEXT Q     packed exactly like T (N rec0 N rec1 N ...), with its own rec_start / rec_len, ascending.  Each position p with
 *                    p + n <= |Q| is INVALID (W_Q(p) holds an N), ABSENT (canon(W_Q(p)) is no key of I) or a HIT (g, row, rev):
 *                    rev = 0 when W_Q(p) == W_T(g) letter for letter (a palindromic window counts as forward), 1 when it is the
 *                    reverse complement.  off = g - g0(row).  The LETTERS decide: the hash only finds the slot.
 *   RUN              the hit at p CONTINUES the one at p - 1 when both are hits of one row with one rev and off[p] == off[p - 1] + 1
 *                    (forward) or - 1 (reverse).  A run is a maximal chain; runs are numbered by ascending p.  A separator is an N,
 *                    so no run crosses records.  Per run: q_first, length (windows), row, rev, off_first.  A run of L windows says that
 *                    the query letters [p, p + L + k) are the row's span letters [off, off + L + k) in text orientation (reverse: the
 *                    reverse complement of [off_first - L + 1, off_first + 1 + k)).
 *   PER RECORD       64-bit sums windows (valid), found, forward (hits with rev = 0), runs and, when a colour table is valid at the
 *                    time of the call, shared[rec][c]: the hits whose row has colour c in its presence.
 * Device encoding: hit[p] is 64 bits, all ones = invalid, all ones - 1 = absent, else rev << 63 | g (g < 2^40); row[p] is 32 bits, all
 * ones / all ones - 1 likewise.  Run arrays are 32 bits each: a query text of 2^32 - 2 positions or more is refused (cut it into batches).
 *   tpc_segments_edges_build           marks the spans in a bit mask over T, counts and then inserts the masked valid positions with the
 *                                      tile kernel of tpc_distinct_sketch's shape into an open-addressed table of 16-byte slots
 *                                      {tag:24 | g:40, row:32} at a load factor of at most 0.5 (atomicCAS claims, equal letters take
 *                                      atomicMin), and writes every slot's row in a pass of its own after all inserts.  Refused: no
 *                                      segment table or a failed walk, a text that is not the build's or a windowed one, k + 1 beyond
 *                                      the tile halo (k > 670), a text of 2^40 positions or more, a forced table that is full, buffers
 *                                      beyond the free device memory.  Kept until the next segment build, edge build or text upload.
 *                                      Options (tests): test_edges_slots_log2 forces the table size, test_edges_hash_bits keeps that
 *                                      many bits of the hash (keys then share tag and home slot), test_locate_grid bounds the
 *                                      workgroups of the tile kernels.
 *   tpc_segments_edges_info            info[0] entries, [1] duplicates, [2] skipped, [3] slots, [4] the longest probe (slots stepped
 *                                      over by one insert), [5] the stage's device memory at its peak
 *   tpc_segments_locate                uploads Q (q_bases / q_nmask of (n_q_text + 31) / 32 words, as tpc_seq_upload takes T) and its
 *                                      records as temporaries, rolls, probes and compares every position, folds the per-record and
 *                                      per-colour sums, numbers the runs with one scan.  Uses the colour table that is valid at the
 *                                      time of the call; none: no shared counts.  TPC_K_LOCATE times the last edge build or locate.
 *   tpc_segments_locate_info           info[0] positions (|Q| - n + 1, or 0), [1] windows, [2] found, [3] runs, [4] colours used (0 =
 *                                      none), [5] the call's device memory at its peak
 *   tpc_segments_locate_fetch_hits     hit[] / row[] of positions [p0, p0 + n)
 *   tpc_segments_locate_fetch_runs     the five run arrays of runs [r0, r0 + n)
 *   tpc_segments_locate_fetch_records  the four sums of records [s0, s0 + n)
 *   tpc_segments_locate_fetch_shared   shared[s][c] of records [s0, s0 + n), n x colours counts; refused without a colour table
 * Ranges outside a table are refused with an error text. */
int tpc_segments_edges_build(tpc_ctx *ctx);
int tpc_segments_edges_info(tpc_ctx *ctx, uint64_t *info /* [6] */);
int tpc_segments_locate(tpc_ctx *ctx, const uint64_t *q_bases, const uint32_t *q_nmask, uint64_t n_q_text, const uint64_t *rec_start, const uint64_t *rec_len, uint32_t n_rec);
int tpc_segments_locate_info(tpc_ctx *ctx, uint64_t *info /* [6] */);
int tpc_segments_locate_fetch_hits(tpc_ctx *ctx, uint64_t p0, uint64_t n, uint64_t *hit_host, uint32_t *row_host);
int tpc_segments_locate_fetch_runs(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *q_first, uint32_t *length, uint32_t *row, uint32_t *rev, uint32_t *off_first);
int tpc_segments_locate_fetch_records(tpc_ctx *ctx, uint64_t s0, uint64_t n, uint64_t *windows, uint64_t *found, uint64_t *forward, uint64_t *runs);
int tpc_segments_locate_fetch_shared(tpc_ctx *ctx, uint64_t s0, uint64_t n, uint64_t *counts_host /* [n x colours] */);

/* The COLOUR CLASSES of the compacted graph (csrc/tpc_classes.hip): the distinct sets of colours that segments have -- which genomes
 * share sequence that nobody else has, and how much.  No counterpart in the reference; ComputeClasses of
 * twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The definition, over the colour table of the
 * last tpc_segments_colors_build:
 *   ROW              a row of the colour table, 'N'-named segments included.
 *   CLASS            the rows whose presence words are all equal.  Its FIRST is its smallest row.
 *   CLASS ID         classes are numbered from 0, ascending by first: the order in which gfa1 first prints a segment of each.
 *   PER ROW          class[r].
 *   PER CLASS p      first[p]; segments[p]; length[p], the sum of the segments' lengths in bases; edges[p], the sum of end - begin of
 *                    each row's first event, the weight of the distance matrices (length - k per segment); occurrences[p], the sum of
 *                    the colour rows' occurrences; presence[p], the W words every row of the class holds; n_colors[p], their popcount.
 *                    The sums are 64-bit.
 *   PER n THAT OCCURS  the number of classes with n_colors == n, and the sums of their segments and edges (the sets).
 *   CONSEQUENCES     the segments[p] sum to the rows; the segments of the classes with n_colors == n sum to the colour table's
 *                    histogram bin n; segments[i][j] and edges[i][j] of the distance matrices are the sums of segments[p] and edges[p]
 *                    over the classes that hold both colours; no class is empty, because every row has an occurrence.
 *   EXACT            integers, commutative sums and a smallest row: the result depends neither on the schedule nor on the hash.
 * Separate from the builds and opt-in: a context that never calls it holds none of this; tpc_segments_counts and the colour, link,
 * bubble, distance, component and other outputs are what they were, in any order of the builds.
 *   tpc_segments_classes_build           an open-addressed set of rows with a power-of-two number of slots, at least 2 S: a row hashes
 *                                        its W words to 64 bits, claims an empty slot with a compare-and-swap or is decided against the
 *                                        words of the row a slot holds, and steps over the slots of other classes (the words decide,
 *                                        the hash only finds the home slot).  One thread per row while W <= 8, one wave per row beyond;
 *                                        while W <= 2 the words are the key and no row is read twice.  The smallest row per slot, one
 *                                        flag per row that is it, one scan for the ids, then the sums, folded per wave.  Every probe
 *                                        loop is counted and ends within `slots` steps; a set too small for the classes (only with the
 *                                        option test_classes_slots_log2) is an error text ("segment classes: gave up ...") from kernels
 *                                        that end normally.  Also refused with an error text: no segment table, a table whose
 *                                        tpc_segments_error kind is not TPC_SEG_OK, no colour table, 2^31 segments or more, buffers
 *                                        beyond the free device memory; the context stays usable.  Kept until the next segment, colour
 *                                        or class build: 4 B per row, per class 4 B of first, 32 B of sums and 4 W B of presence, and
 *                                        24 B x (colours + 1) of sets.  During the call 8 B per row of remembered slots and flags and
 *                                        4 B per slot (12 B while W <= 2).  TPC_K_CLASSES times the stage on the stream from its first
 *                                        kernel to its last, the host's one wait for the class count included, as TPC_K_COMPONENTS
 *                                        times the component stage.  Options (tests, each for the next build only; see
 *                                        tpc_set_option): test_classes_slots_log2, test_classes_hash_bits, test_classes_grid,
 *                                        test_classes_wide.
 *   tpc_segments_classes_info            info[0] classes, [1] rows, [2] the segments of the largest class, [3] the probes that met a
 *                                        slot of another class (depends on the schedule: it shows that the chain path ran), [4] the
 *                                        stage's device bytes at their peak
 *   tpc_segments_classes_fetch_members   class[r] of rows [r0, r0 + n) to the host
 *   tpc_segments_classes_fetch_rows      first / segments / length / edges / occurrences of classes [p0, p0 + n)
 *   tpc_segments_classes_fetch_presence  the n x W presence words of classes [p0, p0 + n), row-major (n_colors is their popcount)
 *   tpc_segments_classes_fetch_sets      classes / segments / edges by number of colours, colours + 1 entries each (0 where no class has n)
 * A range outside a table is refused with an error text. */
int tpc_segments_classes_build(tpc_ctx *ctx);
int tpc_segments_classes_info(tpc_ctx *ctx, uint64_t *info /* [5]: classes, rows, segments of the largest class, probes past another class, peak device bytes */);
int tpc_segments_classes_fetch_members(tpc_ctx *ctx, uint64_t r0, uint64_t n, uint32_t *class_host);
int tpc_segments_classes_fetch_rows(tpc_ctx *ctx, uint64_t p0, uint64_t n, uint32_t *first_host, uint64_t *segments_host, uint64_t *length_host, uint64_t *edges_host,
                                    uint64_t *occurrences_host);
int tpc_segments_classes_fetch_presence(tpc_ctx *ctx, uint64_t p0, uint64_t n, uint32_t *words_host /* [n x W] */);
int tpc_segments_classes_fetch_sets(tpc_ctx *ctx, uint64_t *classes_host, uint64_t *segments_host, uint64_t *edges_host /* [n_colors + 1] each */);

/* The PRESENCE TRACKS of the input sequences (csrc/tpc_tracks.hip): for every stretch of every sequence, which colours share it -- the
 * colour rows projected onto the sequences' coordinates, neighbouring occurrences of equal presence merged into one interval.  No
 * counterpart in the reference; ComputeTracks of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested
 * against.  The definition, over the event table of the last tpc_segments_build_* and the colour table of the last
 * tpc_segments_colors_build:
 *   EVENT, ROW, COLOUR, PRESENCE, N_COLORS  those of the colour table.  row(e) is the row of event e, seq(e) its sequence,
 *                    colour(e) = color_of_seq[seq(e)].
 *   SELECTED         with only == 0xFFFFFFFF every event is selected; otherwise the events with colour(e) == only.
 *   CONTINUES        a selected event e continues e - 1 when seq(e) == seq(e - 1) and the W presence words of row(e) and row(e - 1)
 *                    are all equal.  The words decide: equal n_colors is not enough, equal rows is a shortcut.
 *   SHARED JUNCTIONS consecutive events of one sequence share their junction: end[e - 1] == begin[e].
 *   INTERVAL         a maximal run first .. last of selected events in which each continues the one before it.  It stands for the
 *                    (k+1)-mers that start at positions [begin[first], end[last]) of its sequence, in bases
 *                    [begin[first], end[last] + k).  events = last - first + 1, edges = end[last] - begin[first]; its presence and
 *                    n_colors are those of row(first).  Intervals are reported ascending by first.
 *   TILING           the intervals of one sequence tile [begin[its first event], end[its last event]) with no gap and no overlap.  Two
 *                    sequences never share an interval, even with the same colour and the same presence at the border.  A sequence
 *                    without events has no interval.  'N'-named segments are rows of their own, as everywhere else.
 *   PER COLOUR c     64-bit sums over the intervals whose sequence has colour c: intervals[c]; edges[c]; core_edges[c], the edges of
 *                    the intervals with n_colors == C; private_edges[c], those with n_colors == 1.  With only == c the other colours'
 *                    entries are 0.  With one colour in all, core and private coincide.
 *   PER DEPTH n      0 .. C: depth_intervals[n] and depth_edges[n] over all reported intervals.
 *   CONSEQUENCES     edges[c] equals the sum of end - begin over the events of colour c: ref_edges of the anchor table with ref = c.
 *                    The per-depth edges sum to the per-colour edges.  With only == c the rows are exactly the rows of the
 *                    all-colours table whose sequence has colour c, in the same order.
 *   EXACT            integers and commutative sums: nothing depends on the schedule.
 * Separate from the builds and opt-in: a context that never calls it holds none of this; tpc_segments_counts and every other stage's
 * arrays are what they were, in any order of the builds.
 *   tpc_segments_tracks_build        the row of every event (as the colour stage finds it), then per event its sequence, its colour,
 *                                    whether it is selected and whether it is a head (does not continue): one thread per event while
 *                                    W <= 8, one wave per event beyond; one exclusive scan over the heads numbers the intervals (its
 *                                    total is the host's one wait); a head writes first_event and row, a tail last_event; the sums by
 *                                    one thread per interval, neighbouring lanes of one colour folded into one vector atomic per
 *                                    sum by the run's leader and those of one n_colors likewise, the bins in LDS while there are at
 *                                    most 512 colours.  color_of_seq [n_rec] and n_colors: THAT THIS IS THE MAP THE
 *                                    COLOUR TABLE WAS BUILT WITH IS THE CALLER'S PROMISE; only the colour count can be checked.
 *                                    Refused with an error text that begins "segment tracks:", the context staying usable: no segment
 *                                    table, a table whose tpc_segments_error kind is not TPC_SEG_OK, no colour table or one of another
 *                                    colour count, a colour >= n_colors, only_color >= n_colors and not 0xFFFFFFFF, buffers beyond the
 *                                    free device memory.  Kept until the next segment, colour or track build: 12 B per interval and
 *                                    48 B per colour (+ 16 B); during the call 12 B per event, 4 B per name of the first-sight table,
 *                                    4 B per sequence and the scan's scratch.  TPC_K_TRACKS times the stage on the stream from its
 *                                    first kernel to its last, the wait for the interval count included.  Option (tests, the next
 *                                    build only; see tpc_set_option): test_tracks_grid.
 *   tpc_segments_tracks_info         info[0] intervals, [1] selected events, [2] colours, [3] only (0xFFFFFFFF: all), [4] the stage's
 *                                    device bytes at their peak
 *   tpc_segments_tracks_fetch_rows   first_event / last_event / row of intervals [i0, i0 + n)
 *   tpc_segments_tracks_fetch_colors intervals / edges / core_edges / private_edges per colour, n_colors entries each
 *   tpc_segments_tracks_fetch_depth  intervals / edges per number of colours, n_colors + 1 entries each (0 where no interval has n)
 * A range outside the table is refused with an error text. */
int tpc_segments_tracks_build(tpc_ctx *ctx, const uint32_t *color_of_seq /* [n_rec] */, uint32_t n_colors, uint32_t only_color /* 0xFFFFFFFF: all */);
int tpc_segments_tracks_info(tpc_ctx *ctx, uint64_t *info /* [5]: intervals, selected events, colours, only, peak device bytes */);
int tpc_segments_tracks_fetch_rows(tpc_ctx *ctx, uint64_t i0, uint64_t n, uint32_t *first_event, uint32_t *last_event, uint32_t *row);
int tpc_segments_tracks_fetch_colors(tpc_ctx *ctx, uint64_t *intervals, uint64_t *edges, uint64_t *core_edges, uint64_t *private_edges /* [n_colors] each */);
int tpc_segments_tracks_fetch_depth(tpc_ctx *ctx, uint64_t *intervals, uint64_t *edges /* [n_colors + 1] each */);

/* The VARIANTS (csrc/tpc_variants.hip): which allele every genome carries through every superbubble.  No counterpart in the reference;
 * ComputeVariants of twopaco_amd/host/graphformat.h is the serial statement the kernels are tested against.  The definition, over the
 * event table of the last tpc_segments_build_*, its colour table, its link table and the superbubble table built with max_inside M:
 *   EVENT, ROW, SIDE, COLOUR  row(e), side(e) = row(e) * 2 + (name[e] < 0), rev(side) = side ^ 1, seq(e) and colour(e) =
 *                    color_of_seq[seq(e)] as in the groups above.  Superbubble row b has entrance[b], exit[b] and its members, the inside
 *                    sides in ascending code.
 *   WALK             for an event e and a direction d: d = + (0) visits e, e + 1, .. reading side(x); d = - (1) visits e, e - 1, ..
 *                    reading rev(side(x)), the same sequence read on its other strand.  A walk never leaves the events of seq(e).
 *   TRAVERSAL        a walk (e, d) is a traversal of row b when its first side read is entrance[b], every following side is a member of
 *                    b until the side read is exit[b] -- that event is its `last` -- and it reaches last before its sequence ends.  A
 *                    walk that runs out of sequence is not a traversal (a contig end inside the superbubble).  A walk that reads a side
 *                    that is neither a member nor the exit is not one either and is counted in STRAYS (0 by the matching property).  By
 *                    acyclicity a traversal reads at most inside[b] members: every walk is bounded by M + 1 steps.  Every event starts
 *                    at most two traversals: + for the row whose entrance is side(e), - for the row whose entrance is rev(side(e)); a
 *                    side is the entrance of at most one row.  Traversals are numbered in the order (e, d), + before -.  Per
 *                    traversal: start, last, d, row, mask (bit i set when member i of the row's member list was read) and edges =
 *                    |begin[hi] - end[lo]| with lo, hi the smaller and larger of start and last: the sum of the weights of the members
 *                    read, 0 for a walk straight from entrance to exit.
 *   ALLELE           two traversals of one row are the same allele iff their masks are equal (in an acyclic set of arcs the vertices of
 *                    a path determine the path).  Per allele: row, mask, sides = popcount(mask), edges (equal for all its
 *                    traversals), traversals (64-bit), first (its smallest traversal), presence (W words: the colours with such a
 *                    traversal) and n_colors.  Alleles are numbered ascending by (row, first).
 *   SITE             a superbubble row with at least one traversal: its alleles are allele_offset[b] .. allele_offset[b + 1], its
 *                    traversals their sum.  The histogram counts the sites by their number of alleles.  alleles[b] <= paths[b].
 *   REFERENCE        with ref_color != 0xFFFFFFFF: ref_allele[b] is the allele (its number among all alleles) of the smallest traversal
 *                    of b whose colour(start) == ref_color, all ones without one; ref_traversals[b] counts such traversals.
 *   EXACT            integers, minima, ORs and commutative sums: nothing depends on the schedule.
 * Separate from the builds and opt-in: a context that never calls it holds none of this; every other stage's arrays are what they
 * were, in any order of the builds.
 *   tpc_segments_variants_build      the side of every event, a map from entrance to row, one thread per (event, direction) that walks
 *                                    at most M + 1 steps inside its sequence's events and finds each member's bit by a binary search
 *                                    in the row's members; one scan compacts the traversals in order; two stable radix sorts order
 *                                    them by (row, mask), so that an allele is a run, its first traversal the run's head and its
 *                                    count the run's length; one more sort numbers the alleles by (row, first); presence by atomicOr,
 *                                    the reference by atomicMin and atomicAdd per site.  No loop is unbounded.  color_of_seq [n_rec]
 *                                    and n_colors must be those of the colour build (the caller's promise; the count is checked).
 *                                    Refused with an error text that begins "segment variants:", the context staying usable: no
 *                                    segment, colour, link or superbubble table, a segment table that holds the walk's error, a colour
 *                                    >= n_colors, ref_color >= n_colors and not 0xFFFFFFFF, 2^31 events or more (two walks per event
 *                                    are numbered in 32 bits, which also covers 2^32 - 1 events), buffers beyond the free device
 *                                    memory.  Kept until the next segment, colour, link, superbubble or variant build: 28 B per
 *                                    traversal, 36 B + 4 W B per allele, 24 B per superbubble row; during the call 44 B per event
 *                                    and 52 B per traversal more.  TPC_K_VARIANTS times the stage on the stream from its first
 *                                    kernel to its last, its three waits for the counts included.  Option (tests, the next build
 *                                    only; see tpc_set_option): test_variants_grid.
 *   tpc_segments_variants_info       info[0] sites, [1] alleles, [2] traversals, [3] strays, [4] the stage's device bytes at their
 *                                    peak, [5] colours, [6] ref_color (0xFFFFFFFF: none), [7] histogram bins (the most alleles of a
 *                                    site + 1), [8] superbubble rows
 *   tpc_segments_variants_fetch_traversals  start / last / d / row / edges / mask of traversals [t0, t0 + n)
 *   tpc_segments_variants_fetch_alleles     row / sides / edges / first / n_colors / mask / traversals of alleles [a0, a0 + n)
 *   tpc_segments_variants_fetch_presence    the W = ceil(colours / 32) presence words of alleles [a0, a0 + n)
 *   tpc_segments_variants_fetch_sites       of superbubble rows [b0, b0 + n): allele_offset (n + 1 entries), traversals, ref_allele,
 *                                           ref_traversals
 *   tpc_segments_variants_fetch_hist        sites by number of alleles, info[7] entries
 * A range outside the table is refused with an error text. */
int tpc_segments_variants_build(tpc_ctx *ctx, const uint32_t *color_of_seq /* [n_rec] */, uint32_t n_colors, uint32_t ref_color /* 0xFFFFFFFF: none */);
int tpc_segments_variants_info(tpc_ctx *ctx, uint64_t *info /* [9] */);
int tpc_segments_variants_fetch_traversals(tpc_ctx *ctx, uint64_t t0, uint64_t n, uint32_t *start, uint32_t *last, uint32_t *dir, uint32_t *row, uint32_t *edges, uint64_t *mask);
int tpc_segments_variants_fetch_alleles(tpc_ctx *ctx, uint64_t a0, uint64_t n, uint32_t *row, uint32_t *sides, uint32_t *edges, uint32_t *first, uint32_t *n_colors, uint64_t *mask,
                                        uint64_t *traversals);
int tpc_segments_variants_fetch_presence(tpc_ctx *ctx, uint64_t a0, uint64_t n, uint32_t *words_host /* [n x W] */);
int tpc_segments_variants_fetch_sites(tpc_ctx *ctx, uint64_t b0, uint64_t n, uint32_t *allele_offset /* [n + 1] */, uint64_t *traversals, uint32_t *ref_allele, uint64_t *ref_traversals);
int tpc_segments_variants_fetch_hist(tpc_ctx *ctx, uint64_t *sites_host /* [info[7]] */);

/* ---- parity taps (debug; used by tests/) ---------------------------------------------- */
uint64_t tpc_filter_words(const tpc_ctx *ctx);               /* 2^L/32 + 1, concurrentbitvector.cpp:12 (sharded: 2^L/32/world) */
int tpc_filter_download(tpc_ctx *ctx, uint32_t *words_host); /* tpc_filter_words words       */
/* Restore a downloaded filter (the reference's commented-out ReloadBloomFilter, VE.h:29,113-121): a
 * checkpoint of the most expensive state of a run; the next tpc_pass1_query uses these bits. */
int tpc_filter_upload(tpc_ctx *ctx, const uint32_t *words_host);
uint64_t tpc_mask_words(const tpc_ctx *ctx);                 /* n_text/32 + 1                 */
int tpc_mask_download(tpc_ctx *ctx, int run_wide, uint32_t *words_host);
/* Vertex hashes of the windows at g0..g0+n-1: out[(g-g0)*2q + 2i] = pos_i, +1 = neg_i. */
int tpc_hash_dump(tpc_ctx *ctx, uint64_t g0, uint64_t n, uint64_t *out_host);

/* ---- measurement ------------------------------------------------------------------------ */
/* Duration in ms of the most recent launch(es) of kernel `which`, measured with hipEvents on
 * the stream the kernel ran on; <0 if it has not run. */
double tpc_kernel_ms(const tpc_ctx *ctx, int which);
/* Tuning knobs (results never depend on them):
 *   insert_test_first  direct insert kernel: 0 = atomicOr per address, 1 = test-then-atomicOr (VE.h:1088)
 *   insert_mode / query_mode   0 = automatic, 1 = direct scattered kernel, 2 = LDS write-combining passes
 *   slice_bits         log2 bits of a filter slice held in LDS (6..20, default 20)
 *   part_levels        0 = automatic (three binning levels when L - slice_bits > 18), 2, 3
 *   text_window        1: on a sharded context tpc_seq_upload keeps only the words of the tiles this rank hashes (chunk
 *                      rank * ceil(tiles / world) ..., + halo); such a context runs the sharded first pass only (rank 0 of the
 *                      C++ host keeps the whole text for the second pass)
 *   fuse_apply_lookup  1 (default): when the insert of a round fits one tile batch and the query is partitioned with the same
 *                      geometry, the insert stops after its level-2 binning and the lookup kernel of the query's FIRST batch builds
 *                      each filter slice itself (the filter is written once and not read back by that batch); TPC_K_INSERT then
 *                      covers hash + split only and TPC_K_FUSED the shared kernel; 0: off
 *   verify_marks       1 (default): the partitioned query's verification writes one verdict per survivor and two kernels OR the marked
 *                      positions into the candidate mask through LDS, in whole lines (k_mark_split, k_mark_apply); 0: it marks with
 *                      one device atomic per passing survivor.  TPC_VERIFY_MARKS=0 / 1 in the environment overrides the option
 *                      (measurements; read once per process).  The sharded first pass always marks with atomics
 *   qhash_pushes       process-wide, 6 (default): k_q_hash2 compacts the 3 + 3 unknown edges of a position per lane and pushes them
 *                      with every lane active; 8: the 4 + 4 candidates as predicated pushes.  TPC_QHASH_PUSHES=6 / 8 in the
 *                      environment overrides the option (measurements; read once per process)
 *   qhash_roll_scalars process-wide, 1 (default): k_q_hash2 rolls its hash with letter hashes taken from scalar registers by lane masks; 0: with
 *                      two 16-byte LDS reads per position.  TPC_QHASH_ROLL_SCALARS=0 / 1 overrides it.  A sharded context (more
 *                      than one rank) with qhash_pushes = 8 always takes the LDS reads, whatever this option says: one of its
 *                      instantiations spilled with the selects.  "query_hash_form" tells which roll ran
 *   qhash_seed_scalars process-wide, 1 (default): k_q_hash2 seeds a thread's run of 16 positions from function 0's pre-rotated letter
 *                      rows [k][5] x 16 bytes that tpc_set_params keeps in device memory: the five rows of a character are loaded at a
 *                      uniform index and XORed in under one-hot lane masks of the letter; 0: from the same rows in LDS, one 16-byte read per character at
 *                      a per-lane index.  TPC_QHASH_SEED_SCALARS=0 / 1 overrides it.  k > "query_hash_seed_maxk" (64) has no such rows and seeds by rolling
 *                      whatever the option says.  "query_hash_seed" tells which seeding ran
 *   mark_bucket_bits / mark_region_cap / mark_slice_bits   tests only, process-wide (0 = automatic): log2 positions of a bucket of the
 *                      mark lists (14..21), entries of a (workgroup, bucket) region (tiny: most entries take the atomic fallback),
 *                      log2 bits of the LDS slice k_mark_apply holds (10..20: a larger bucket is cut into sub-slices)
 *   test_sched_cap     tests only, process-wide: rounds per segment of the split kernels' round schedule (0 = what fits in LDS)
 *   test_mask_scan     tests only, process-wide: which scan of the block sums the mask compaction (tpc_pass2_marks, tpc_pass2_filter, the
 *                      partitioned query's counts) takes: 0 = by size (one workgroup up to 4096 block sums of 8192 positions each and
 *                      beyond 64 x 4096, the segmented pair of kernels between), 1 = always the single workgroup (more than 4096 sums: its
 *                      loop turns over and carries), 2 = the segmented pair whenever the segments number 1..64 (a small text: one
 *                      segment with base 0).  "mask_scan_form" tells which one the last count took
 *   test_fail_mallocs  tests only, process-wide: the next N second-pass / output allocations fail at their first attempt, as if
 *                      the device were full (they then give the partition buffers back and try again, see "pbuf_releases")
 *   test_sketch_grid   tests only, process-wide: workgroups of tpc_distinct_sketch's kernel (0 = a few per CU), so that a small text
 *                      makes every workgroup stride over several tiles
 *   test_force_anyq    tests only, process-wide: 1 = the closed-form first-pass kernels that serve q = 17..64
 *                      (csrc/tpc_pass1_anyq.hip) for every q, so that they can be checked on the goldens with q <= 16
 *   test_links_slots_log2  tests only: the next tpc_segments_links_build takes 2^n slots for its link set instead of sizing it by
 *                      the occurrences (0 = by the occurrences), so that long probe chains and a full set can be reached
 *   test_classes_slots_log2  tests only, the next tpc_segments_classes_build alone: 2^n slots (n = 1 .. 31) for its set of rows instead
 *                      of sizing it by the rows (0 = by the rows), so that long chains, a set that is exactly full and a set that is
 *                      too small ("segment classes: gave up ...", an error return from kernels that end normally) can be reached
 *   test_classes_hash_bits   tests only, the next tpc_segments_classes_build alone: only the low n bits of a row's hash are used,
 *                      n = 0 .. 64 (negative = all 64, the default), so that different keys share a home slot
 *   test_classes_grid  tests only, the next tpc_segments_classes_build alone: at most n workgroups per kernel of the stage (0 = by
 *                      the rows), so that a table of a few thousand rows makes every workgroup stride several times
 *   test_classes_wide  tests only, the next tpc_segments_classes_build alone: 1 forces the wave-per-row form at any W, 2 the
 *                      thread-per-row form (0 = by W)
 *   test_tracks_grid   tests only, the next tpc_segments_tracks_build alone: at most n workgroups per kernel of the stage (0 = by the
 *                      events), so that a table of a few thousand events makes every workgroup stride several times
 *   test_variants_grid tests only, the next tpc_segments_variants_build alone: at most n workgroups per kernel of the stage (0 = by the
 *                      events), so that a table of a few thousand events makes every workgroup stride several times
 *   test_distances_chunk_words  tests only: the next tpc_segments_distances_build stages n column words (64 rows each) per chunk
 *                      instead of its own 64 (0 = its own; more than 64 is refused), so that a table of a few hundred rows crosses
 *                      chunk borders and ends in a partial chunk
 *   test_components_step_limit  tests only: the next tpc_segments_components_build gives a find n steps and a hook n retries instead
 *                      of segments + 1 (0 = segments + 1), so that the give-up path -- an error return from kernels that end
 *                      normally -- can be reached
 *   part_budget_bytes  partition buffers per tile batch (0 = automatic: 40 GiB, or 60 % of the free device
 *                      memory when that is more; any number of batches, not only powers of two); part_min_tiles  smallest batch */
/*   replicate_filter   1 (before tpc_shard_config / tpc_set_params): a sharded context keeps the whole filter; tpc_pass1_insert / tpc_pass1_query
 *                      run over this rank's chunk of the tiles and the tpc_combine_* calls exchange set-bit lists (see there) */
int tpc_set_option(tpc_ctx *ctx, const char *name, int64_t value);
/* What the last first-pass calls ran: "insert_path" / "query_path" = 1 direct kernel, 2 or 3 = LDS
 * write-combining with that many levels (+10: it overflowed and the direct kernel completed the pass);
 * "insert_batches" / "query_batches" = tile batches; "filter2_retries" = exact-filter passes repeated
 * with the full-size table by the last exact filter (tpc_pass2_filter*), "aggregate_retries" those of the last tpc_pass2_aggregate_records;
 * "filter2_counted" = 1 when the last exact-filter launch (either call) counted occurrences (an abundance cut applies), 0 when it kept
 * only "seen twice"; "text_words" = packed words of the text held (a window with option text_window); "fused_lookups" = queries that built the filter slices themselves (deferred apply); "query_overflow_entries" = entries the last batch of the last partitioned query handed to its overflow list (full rings or regions: address skew); "distances_tile" = colours on each side of the tile one workgroup of tpc_segments_distances_build's Gram kernel owns (a constant; the tests choose their colour counts around it); "pbuf_releases" = times a second-pass or output allocation did not fit beside the first pass' partition buffers, which were then freed (the next first pass allocates them again); "round_marks" = candidate marks of the round the last
 * tpc_pass2_filter consumed (what tpc_pass1_query reports; the sharded first pass has no single call that does);
 * "device_free_bytes" / "device_total_bytes" = hipMemGetInfo of the context's device, now;
 * of the last tpc_segments_text_write: "text_write_us" = microseconds its helper thread spent inside write / pwrite, "text_wait_us" =
 * microseconds the calling thread waited for a window's render and copy to finish, "text_window_bytes" = the window size used;
 * which kernels the last first pass ran (after a "+10" path: those of the partitioned pass the direct kernel completed):
 * "insert_hash_kernel" = 0 none (the direct rolling kernel), 1 the instruction-lean hash with its seed table in LDS, 2 the same
 * without it (k too large for q), 3 the classic k_part_hash, 4 the closed form (q > 16, tpc_pass1_anyq.hip);
 * "query_hash_kernel" = 0 none (direct), 1 the lean k_q_hash2, 2 k_q_hash, 4 the closed form;
 * "split_kernel" = of the last tpc_pass1_split_hist: 0 the rolling k_split<Q> (q <= 16), 4 the closed form k_split_anyq (q > 16 or option
 * test_force_anyq); "split_phases" = the ballot launches of that call: min(q, 3) on a sparse scratch filter, q when q x text length
 * exceeds 2^L / 8 (both 0 before the first call);
 * "query_hash_form" = of the last k_q_hash2 launch (0 after another hash kernel): 1 = six compacted pushes per position (option
 * qhash_pushes), + 2 = the roll from scalar registers (option qhash_roll_scalars), + 4 = its gated instantiation (a range [lo, hi] that
 * is not the whole hash space);
 * "query_hash_seed" = 1 when the last k_q_hash2 launch seeded its runs from the uniform rows (option qhash_seed_scalars), 0 when it read
 * them from LDS or rolled (k > 64), and after another hash kernel -- a stat of its own and not a bit of "query_hash_form", whose values
 * 0..7 callers compare as they stand; "query_hash_seed_maxk" = the longest k that has such rows (a constant);
 * "query_verify_kernel" = 0 none (the direct kernels verify in place), 1 k_q_verify2 lazy, 2 k_q_verify2 eager (TPC_VERIFY_LAZY=0), 3 k_q_verify;
 * "query_mark_path" = how the last query set the marks of its mask: 1 the write-combined lists, 0 device atomics (option verify_marks, a
 * plan whose lists do not fit the level-1 buffer) or the direct kernel (also when it completed an overflowed partitioned pass);
 * "query_mark_fallback" = entries of those lists that found a ring or a region full and were ORed straight into the mask (0 on path 0);
 * "text_word_begin" / "text_word_end" = the packed words [begin, end) of the text this context holds ("text_words" is their difference);
 * "periodic_any_query" / "periodic_any_insert" = 1 when the detection-only launch of the periodic-window masks found a position that
 * copies its verdict / drops its insert (0 before the masks of this text and k were asked for, or with the option off);
 * "mask_scan_form" = process-wide, the scan of the block sums that the last mask count of any context launched: 1 the single
 * workgroup (k_scan_sums), 2 the segmented pair (k_scan_sums_seg + k_scan_sums_wide), 0 before the first count (option test_mask_scan).
 * -1: unknown name. */
int64_t tpc_get_stat(const tpc_ctx *ctx, const char *name);

#ifdef __cplusplus
}
#endif
#endif /* TWOPACO_HIP_H_ */
