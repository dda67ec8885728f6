"""ctypes bindings over libtwopaco_hip.so (device C-ABI, include/twopaco_hip.h) and
libtwopaco_host.so (C wrappers over the C++ host layer).  Plumbing only: every compute call
goes to the HIP library; if it is missing this module raises -- there is no fallback."""
import ctypes
import os

import numpy as np

from .build import lib_dir

INVALID_VERTEX = (1 << 63) - 1
DISTANCES_TILE = 32  # TPC_DISTANCES_TILE of csrc/tpc_ctx.h, what Context.stat("distances_tile") returns: colours on each side of the tile one workgroup of
                     # the Gram kernel owns; here for the tests' parametrisation, and tests/test_gpu_distances.py holds the two equal
KERNELS = {"fused": 12, "filter_reset": 0, "insert": 1, "query": 2, "compact": 3, "filter2": 4, "scan2": 5, "sort": 6, "emit": 7, "split": 8,
           "shard_hash": 9, "shard_apply": 10, "stream": 11, "lookup": 13, "combine": 14, "segments": 15, "segtext": 16, "sketch": 17, "colors": 18, "links": 19, "bubbles": 20,
           "distances": 21, "components": 22, "superbubbles": 23, "anchors": 24, "locate": 25, "classes": 26, "tracks": 27, "variants": 28}

# every symbol include/twopaco_hip.h declares
HIP_SYMBOLS = ["tpc_ctx_create", "tpc_ctx_destroy", "tpc_last_error", "tpc_set_params", "tpc_seq_upload",
               "tpc_run_begin", "tpc_filter_reset", "tpc_pass1_insert", "tpc_pass1_split_hist", "tpc_pass1_query", "tpc_pass2_filter",
               "tpc_junctions_finalize", "tpc_key_words", "tpc_junction_keys", "tpc_junction_keys_raw", "tpc_junction_keys_set", "tpc_get_id", "tpc_emit",
               "tpc_emit_fetch", "tpc_filter_words", "tpc_filter_download", "tpc_mask_words", "tpc_mask_download",
               "tpc_hash_dump", "tpc_kernel_ms", "tpc_set_option",
               "tpc_shard_config", "tpc_shard_plan", "tpc_shard_hash", "tpc_shard_overflow_get", "tpc_shard_overflow_set", "tpc_shard_apply",
               "tpc_shard_pack", "tpc_shard_apply_packed", "tpc_pass2_marks", "tpc_pass2_mark_owners", "tpc_pass2_filter_positions",
               "tpc_pass2_mark_records", "tpc_pass2_filter_records", "tpc_pass2_aggregate_records", "tpc_pass2_filter_aggregated", "tpc_shard_permute_rows", "tpc_emit_export", "tpc_emit_import",
               "tpc_shard_survivors", "tpc_shard_survivor_sources", "tpc_shard_verify_addrs", "tpc_shard_probe", "tpc_shard_mark", "tpc_mask_export", "tpc_mask_merge",
               "tpc_shard_route", "tpc_shard_permute64", "tpc_shard_select", "tpc_mask_export_padded", "tpc_mask_or_blocks", "tpc_mask_import",
               "tpc_emit_stream", "tpc_emit_stream_fetch", "tpc_host_alloc", "tpc_host_free", "tpc_get_stat", "tpc_filter_upload",
               "tpc_junction_keys_export", "tpc_junction_keys_import", "tpc_warmup", "tpc_preload", "tpc_reserve", "tpc_shard_chunk", "tpc_emit_stream_partial", "tpc_emit_stream_part",
               "tpc_shard_plan_both", "tpc_shard_hash_begin", "tpc_shard_hash_end", "tpc_shard_apply_inplace", "tpc_shard_survivors_home", "tpc_shard_verify_send", "tpc_shard_finish", "tpc_shard_verify_local", "tpc_shard_periodic_copy", "tpc_periodic_download",
               "tpc_pass1_query_begin", "tpc_combine_info", "tpc_combine_export", "tpc_combine_merge", "tpc_combine_import", "tpc_combine_choose", "tpc_filter_copy_out", "tpc_filter_copy_in",
               "tpc_segments_build_host", "tpc_segments_build_resident", "tpc_segments_counts", "tpc_segments_error", "tpc_segments_fetch_names", "tpc_segments_fetch_first",
               "tpc_segments_fetch_events", "tpc_segments_fetch_sequences", "tpc_segments_text_plan", "tpc_segments_text_fetch", "tpc_segments_text_write", "tpc_distinct_sketch",
               "tpc_segments_colors_build", "tpc_segments_colors_info", "tpc_segments_colors_fetch_rows", "tpc_segments_colors_fetch_presence", "tpc_segments_colors_fetch_hist",
               "tpc_segments_links_build", "tpc_segments_links_info", "tpc_segments_links_fetch_rows", "tpc_segments_links_fetch_first",
               "tpc_segments_bubbles_build", "tpc_segments_bubbles_info", "tpc_segments_bubbles_fetch_rows", "tpc_segments_bubbles_fetch_sides", "tpc_segments_bubbles_fetch_hist",
               "tpc_segments_distances_build", "tpc_segments_distances_info", "tpc_segments_distances_fetch",
               "tpc_segments_components_build", "tpc_segments_components_info", "tpc_segments_components_fetch_members", "tpc_segments_components_fetch_rows",
               "tpc_segments_components_fetch_presence",
               "tpc_segments_superbubbles_build", "tpc_segments_superbubbles_info", "tpc_segments_superbubbles_fetch_adjacency", "tpc_segments_superbubbles_fetch_exits",
               "tpc_segments_superbubbles_fetch_rows", "tpc_segments_superbubbles_fetch_members", "tpc_segments_superbubbles_fetch_presence",
               "tpc_segments_anchors_build", "tpc_segments_anchors_info", "tpc_segments_anchors_fetch_mates", "tpc_segments_anchors_fetch_rows",
               "tpc_segments_anchors_fetch_shared",
               "tpc_segments_edges_build", "tpc_segments_edges_info", "tpc_segments_locate", "tpc_segments_locate_info", "tpc_segments_locate_fetch_hits",
               "tpc_segments_locate_fetch_runs", "tpc_segments_locate_fetch_records", "tpc_segments_locate_fetch_shared",
               "tpc_segments_classes_build", "tpc_segments_classes_info", "tpc_segments_classes_fetch_members", "tpc_segments_classes_fetch_rows",
               "tpc_segments_classes_fetch_presence", "tpc_segments_classes_fetch_sets",
               "tpc_segments_tracks_build", "tpc_segments_tracks_info", "tpc_segments_tracks_fetch_rows", "tpc_segments_tracks_fetch_colors",
               "tpc_segments_tracks_fetch_depth",
               "tpc_segments_variants_build", "tpc_segments_variants_info", "tpc_segments_variants_fetch_traversals", "tpc_segments_variants_fetch_alleles",
               "tpc_segments_variants_fetch_presence", "tpc_segments_variants_fetch_sites", "tpc_segments_variants_fetch_hist"]
VARIANTS_NONE = 0xFFFFFFFF  # ref_color of tpc_segments_variants_build: no reference; ref_allele: no traversal of the reference
TRACKS_ALL = 0xFFFFFFFF  # only_color of tpc_segments_tracks_build: every colour
SEGMENT_ERRORS = {0: None, 1: "The input is corrupted", 2: "A vertex id is too large, cannot generate GFA"}  # TPC_SEG_*: what graphdump's serial walk throws

_hip = None
_host = None


def combine_choose(world, L, mean_export_units):
    """(mode, bytes received per rank for [all-gather of exports, reduce-scatter + all-gather, dense OR all-reduce]); mode 1..3 = the cheapest."""
    b = (ctypes.c_double * 3)()
    mode = hip().tpc_combine_choose(world, L, int(mean_export_units), b)
    return mode, [float(x) for x in b]


def _load(name):
    path = os.path.join(lib_dir(), name)
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)" % path)
    return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def hip():
    global _hip
    if _hip is None:
        L = _load("libtwopaco_hip.so")
        u64, i64, p, ci = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.tpc_ctx_create.argtypes = [ci, ctypes.POINTER(p)]
        L.tpc_ctx_destroy.argtypes = [p]
        L.tpc_last_error.restype = ctypes.c_char_p
        L.tpc_last_error.argtypes = [p]
        L.tpc_set_params.argtypes = [p, ci, ci, ci, p]
        L.tpc_seq_upload.argtypes = [p, p, p, u64]
        L.tpc_filter_reset.argtypes = [p]
        L.tpc_run_begin.argtypes = [p]
        L.tpc_pass1_insert.argtypes = [p, u64, u64, p]
        L.tpc_pass1_split_hist.argtypes = [p, p, p, ctypes.c_uint32, p]
        L.tpc_pass1_query.argtypes = [p, u64, u64, p]
        L.tpc_pass2_filter.argtypes = [p, u64, p, p, p]
        L.tpc_junctions_finalize.argtypes = [p, p]
        L.tpc_key_words.argtypes = [p]
        L.tpc_junction_keys.argtypes = [p, p]
        L.tpc_junction_keys_raw.argtypes = [p, p, p]
        L.tpc_junction_keys_set.argtypes = [p, p, u64]
        L.tpc_junction_keys_export.argtypes = [p, p, u64, p]
        L.tpc_junction_keys_import.argtypes = [p, p, u64, ci]
        L.tpc_get_id.restype = i64
        L.tpc_get_id.argtypes = [p, ctypes.c_char_p]
        L.tpc_emit.argtypes = [p, p, p]
        L.tpc_emit_fetch.argtypes = [p, p, p]
        L.tpc_filter_words.restype = u64
        L.tpc_filter_words.argtypes = [p]
        L.tpc_filter_download.argtypes = [p, p]
        L.tpc_filter_upload.argtypes = [p, p]
        L.tpc_warmup.argtypes = [p]
        L.tpc_preload.argtypes = [ctypes.c_int]
        L.tpc_reserve.argtypes = [p, u64]
        L.tpc_mask_words.restype = u64
        L.tpc_mask_words.argtypes = [p]
        L.tpc_mask_download.argtypes = [p, ci, p]
        L.tpc_hash_dump.argtypes = [p, u64, u64, p]
        L.tpc_kernel_ms.restype = ctypes.c_double
        L.tpc_kernel_ms.argtypes = [p, ci]
        L.tpc_set_option.argtypes = [p, ctypes.c_char_p, i64]
        u32 = ctypes.c_uint32
        L.tpc_shard_config.argtypes = [p, u32, u32]
        L.tpc_shard_plan.argtypes = [p, ci, u64, u64, p]
        L.tpc_shard_hash.argtypes = [p, ci, u64, u64, u64, p, p, p]
        L.tpc_shard_plan_both.argtypes = [p, u64, u64, p, p]
        L.tpc_shard_hash_begin.argtypes = [p, ci, u64, u64, u64, p, p]
        L.tpc_shard_hash_end.argtypes = [p, ci, p]
        L.tpc_shard_overflow_get.argtypes = [p, ci, p, u64]
        L.tpc_shard_overflow_set.argtypes = [p, ci, p, u64]
        L.tpc_shard_apply.argtypes = [p, ci, u64, p, p, p]
        L.tpc_pass2_marks.argtypes = [p, p]
        L.tpc_pass2_mark_owners.argtypes = [p, u32, p, p]
        L.tpc_pass2_filter_positions.argtypes = [p, p, u64, u64, p, p, p]
        L.tpc_pass2_mark_records.argtypes = [p, u32, p, p]
        L.tpc_pass2_filter_records.argtypes = [p, p, u64, u64, p, p, p]
        L.tpc_pass2_aggregate_records.argtypes = [p, u32, u64, p, p, p]
        L.tpc_pass2_filter_aggregated.argtypes = [p, p, u64, u64, p, p, p]
        L.tpc_shard_permute_rows.argtypes = [p, p, p, u64, ci, p]
        L.tpc_shard_pack.argtypes = [p, ci, p, p, p, p]
        L.tpc_shard_apply_packed.argtypes = [p, ci, u64, p, p, p]
        L.tpc_shard_apply_inplace.argtypes = [p, ci, u64, p, p, p, p, p]
        L.tpc_shard_survivors_home.argtypes = [p, p, p, p]
        L.tpc_shard_verify_send.argtypes = [p, ci, ci, p, u64, p, p, p, p]
        L.tpc_shard_finish.argtypes = [p, p, u64, ci, p, p, p]
        L.tpc_shard_verify_local.argtypes = [p]
        L.tpc_shard_periodic_copy.argtypes = [p]
        L.tpc_periodic_download.argtypes = [p, p, p, p]
        L.tpc_pass1_query_begin.argtypes = [p, u64, u64]
        L.tpc_combine_info.argtypes = [p, u32, p]
        L.tpc_combine_export.argtypes = [p, u32, p, u64, p, p]
        L.tpc_combine_merge.argtypes = [p, u32, p, p, p, p, u64, p, p]
        L.tpc_combine_import.argtypes = [p, u32, u32, p, p, p, u64]
        L.tpc_combine_choose.argtypes = [u32, ci, u64, p]
        L.tpc_filter_copy_out.argtypes = [p, u64, u64, p]
        L.tpc_filter_copy_in.argtypes = [p, u64, u64, p]
        L.tpc_shard_survivors.argtypes = [p, p]
        L.tpc_shard_verify_addrs.argtypes = [p, ci, ci, p, u64, p, p]
        L.tpc_shard_survivor_sources.argtypes = [p, p, u64, p]
        L.tpc_shard_probe.argtypes = [p, p, u64, p]
        L.tpc_shard_mark.argtypes = [p, p, u64]
        L.tpc_mask_export.argtypes = [p, p]
        L.tpc_mask_merge.argtypes = [p, p, u32]
        L.tpc_shard_route.argtypes = [p, p, u64, p, p]
        L.tpc_shard_permute64.argtypes = [p, p, p, u64, p]
        L.tpc_shard_select.argtypes = [p, p, u64, ci, p, p, p, p]
        L.tpc_mask_export_padded.argtypes = [p, p, u64]
        L.tpc_mask_or_blocks.argtypes = [p, p, u32, u64, p]
        L.tpc_mask_import.argtypes = [p, p]
        L.tpc_emit_stream.argtypes = [p, p, p, u32, p, p]
        L.tpc_emit_stream_fetch.argtypes = [p, u64, u64, p]
        L.tpc_emit_import.argtypes = [p, p, p, u64]
        L.tpc_shard_chunk.argtypes = [p, p, p]
        L.tpc_emit_stream_partial.argtypes = [p, p, p, u32, p, p]
        L.tpc_emit_stream_part.argtypes = [p, p, p, u32, p, p, p, p, u32, u64, u64, u64, u64, p]
        L.tpc_segments_build_host.argtypes = [p, p, u64, ci, p, p, u32, p, u64]
        L.tpc_segments_build_resident.argtypes = [p, ci, p, p, u32, p, u64]
        L.tpc_segments_counts.argtypes = [p, p]
        L.tpc_segments_error.argtypes = [p, p, p]
        L.tpc_segments_fetch_names.argtypes = [p, u64, u64, p]
        L.tpc_segments_fetch_first.argtypes = [p, u64, u64, p]
        L.tpc_segments_fetch_events.argtypes = [p, u64, u64, p, p]
        L.tpc_segments_fetch_sequences.argtypes = [p, u64, u64, p]
        L.tpc_segments_text_plan.argtypes = [p, ci, p, p, p, p]
        L.tpc_segments_text_fetch.argtypes = [p, u64, u64, p]
        L.tpc_segments_text_write.argtypes = [p, ci, u64, u64, p]
        L.tpc_segments_colors_build.argtypes = [p, p, u32]
        L.tpc_segments_colors_info.argtypes = [p, p]
        L.tpc_segments_colors_fetch_rows.argtypes = [p, u64, u64, p, p, p, p]
        L.tpc_segments_colors_fetch_presence.argtypes = [p, u64, u64, p]
        L.tpc_segments_colors_fetch_hist.argtypes = [p, p, p]
        L.tpc_segments_links_build.argtypes = [p]
        L.tpc_segments_links_info.argtypes = [p, p]
        L.tpc_segments_links_fetch_rows.argtypes = [p, u64, u64, p, p, p]
        L.tpc_segments_links_fetch_first.argtypes = [p, u64, u64, p]
        L.tpc_segments_bubbles_build.argtypes = [p]
        L.tpc_segments_bubbles_info.argtypes = [p, p]
        L.tpc_segments_bubbles_fetch_rows.argtypes = [p, u64, u64, p, p, p, p]
        L.tpc_segments_bubbles_fetch_sides.argtypes = [p, u64, u64, p, p, p]
        L.tpc_segments_bubbles_fetch_hist.argtypes = [p, p]
        L.tpc_segments_distances_build.argtypes = [p]
        L.tpc_segments_distances_info.argtypes = [p, p]
        L.tpc_segments_distances_fetch.argtypes = [p, u64, u64, p, p]
        L.tpc_segments_components_build.argtypes = [p]
        L.tpc_segments_components_info.argtypes = [p, p]
        L.tpc_segments_components_fetch_members.argtypes = [p, u64, u64, p]
        L.tpc_segments_components_fetch_rows.argtypes = [p, u64, u64, p, p, p, p, p, p]
        L.tpc_segments_components_fetch_presence.argtypes = [p, u64, u64, p]
        L.tpc_segments_superbubbles_build.argtypes = [p, ctypes.c_uint32]
        L.tpc_segments_superbubbles_info.argtypes = [p, p]
        L.tpc_segments_superbubbles_fetch_adjacency.argtypes = [p, p, p]
        L.tpc_segments_superbubbles_fetch_exits.argtypes = [p, u64, u64, p]
        L.tpc_segments_superbubbles_fetch_rows.argtypes = [p, u64, u64, p, p, p, p, p, p, p, p]
        L.tpc_segments_superbubbles_fetch_members.argtypes = [p, p, p]
        L.tpc_segments_superbubbles_fetch_presence.argtypes = [p, u64, u64, p]
        L.tpc_segments_anchors_build.argtypes = [p, p, ctypes.c_uint32, ctypes.c_uint32]
        L.tpc_segments_anchors_info.argtypes = [p, p]
        L.tpc_segments_anchors_fetch_mates.argtypes = [p, u64, u64, p]
        L.tpc_segments_anchors_fetch_rows.argtypes = [p, u64, u64, p, p, p, p]
        L.tpc_segments_anchors_fetch_shared.argtypes = [p, p, p, p, p]
        L.tpc_segments_edges_build.argtypes = [p]
        L.tpc_segments_edges_info.argtypes = [p, p]
        L.tpc_segments_locate.argtypes = [p, p, p, u64, p, p, ctypes.c_uint32]
        L.tpc_segments_locate_info.argtypes = [p, p]
        L.tpc_segments_locate_fetch_hits.argtypes = [p, u64, u64, p, p]
        L.tpc_segments_locate_fetch_runs.argtypes = [p, u64, u64, p, p, p, p, p]
        L.tpc_segments_locate_fetch_records.argtypes = [p, u64, u64, p, p, p, p]
        L.tpc_segments_locate_fetch_shared.argtypes = [p, u64, u64, p]
        L.tpc_segments_classes_build.argtypes = [p]
        L.tpc_segments_classes_info.argtypes = [p, p]
        L.tpc_segments_classes_fetch_members.argtypes = [p, u64, u64, p]
        L.tpc_segments_classes_fetch_rows.argtypes = [p, u64, u64, p, p, p, p, p]
        L.tpc_segments_classes_fetch_presence.argtypes = [p, u64, u64, p]
        L.tpc_segments_classes_fetch_sets.argtypes = [p, p, p, p]
        L.tpc_segments_tracks_build.argtypes = [p, p, u32, u32]
        L.tpc_segments_tracks_info.argtypes = [p, p]
        L.tpc_segments_tracks_fetch_rows.argtypes = [p, u64, u64, p, p, p]
        L.tpc_segments_tracks_fetch_colors.argtypes = [p, p, p, p, p]
        L.tpc_segments_tracks_fetch_depth.argtypes = [p, p, p]
        L.tpc_segments_variants_build.argtypes = [p, p, u32, u32]
        L.tpc_segments_variants_info.argtypes = [p, p]
        L.tpc_segments_variants_fetch_traversals.argtypes = [p, u64, u64, p, p, p, p, p, p]
        L.tpc_segments_variants_fetch_alleles.argtypes = [p, u64, u64, p, p, p, p, p, p, p]
        L.tpc_segments_variants_fetch_presence.argtypes = [p, u64, u64, p]
        L.tpc_segments_variants_fetch_sites.argtypes = [p, u64, u64, p, p, p, p]
        L.tpc_segments_variants_fetch_hist.argtypes = [p, p]
        L.tpc_distinct_sketch.argtypes = [p, ci, p, p]
        L.tpc_host_alloc.argtypes = [ctypes.POINTER(p), u64]
        L.tpc_host_free.argtypes = [p]
        L.tpc_get_stat.restype = i64
        L.tpc_get_stat.argtypes = [p, ctypes.c_char_p]
        _hip = L
    return _hip


def host():
    global _host
    if _host is None:
        hip()  # dependency of the host library
        L = _load("libtwopaco_host.so")
        u64, i64, p, ci = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        L.tpch_last_error.restype = ctypes.c_char_p
        L.tpch_free.argtypes = [p]
        L.tpch_seed_table.argtypes = [u64, ci, ci, ci, p]
        L.tpch_text_new.restype = p
        L.tpch_text_free.argtypes = [p]
        L.tpch_text_add_fasta.argtypes = [p, ctypes.POINTER(ctypes.c_char_p), ci, ci]
        L.tpch_text_add_codes.argtypes = [p, p, u64]
        for name, res in [("tpch_text_length", u64), ("tpch_text_words", u64), ("tpch_text_bases", p), ("tpch_text_nmask", p),
                          ("tpch_text_records", ctypes.c_uint32), ("tpch_text_rec_start", p), ("tpch_text_rec_length", p)]:
            getattr(L, name).restype = res
            getattr(L, name).argtypes = [p]
        L.tpch_create_enumerator.restype = p
        L.tpch_create_enumerator.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                             ctypes.c_char_p, ci, u64, ci, ci, ctypes.POINTER(p)]
        L.tpch_create_enumerator_mgpu.restype = p
        L.tpch_create_enumerator_mgpu.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                  ctypes.c_char_p, ci, u64, ci, ci, ci, ci, ci, ctypes.POINTER(p)]
        L.tpch_create_enumerator_graph.restype = p
        L.tpch_create_enumerator_graph.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                   ctypes.c_char_p, ci, u64, ci, ci, ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.POINTER(p)]
        L.tpch_create_enumerator_colors.restype = p
        L.tpch_create_enumerator_colors.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                    ctypes.c_char_p, ci, u64, ci, ci, ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.POINTER(p)]
        L.tpch_create_enumerator_links.restype = p
        L.tpch_create_enumerator_links.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                   ctypes.c_char_p, ci, u64, ci, ci, ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.c_char_p, ctypes.c_char_p,
                                                   ctypes.c_char_p, ci, ctypes.POINTER(p)]
        L.tpch_create_enumerator_distances.restype = p
        L.tpch_create_enumerator_distances.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                       ctypes.c_char_p, ci, u64, ci, ci, ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.c_char_p, ctypes.c_char_p,
                                                       ctypes.c_char_p, ci, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci, ctypes.POINTER(p)]
        L.tpch_create_enumerator_components.restype = p
        L.tpch_create_enumerator_components.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, u64, ctypes.c_char_p,
                                                        ctypes.c_char_p, ci, u64, ci, ci, ctypes.c_char_p, ctypes.c_char_p, ci, ci, ctypes.c_char_p, ctypes.c_char_p,
                                                        ctypes.c_char_p, ci, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(p)]
        L.tpch_create_enumerator_auto.restype = p
        L.tpch_create_enumerator_auto.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, u64, u64, u64, u64, ctypes.c_char_p, ctypes.c_char_p, ci, u64, ci,
                                                  ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(p)]
        L.tpch_hll_estimate.restype = ctypes.c_double
        L.tpch_hll_estimate.argtypes = [p, u64]
        L.tpch_filter_plan.argtypes = [u64, ci, u64, u64, ci, p, p]
        L.tpch_graph_format.argtypes = [ctypes.POINTER(ctypes.c_char_p), ci, u64, ctypes.c_char_p, ci, ci, u64, p, p, p, p, u64, p, ctypes.c_char_p]
        L.tpch_enumerator_free.argtypes = [p]
        L.tpch_vertices_count.restype = u64
        L.tpch_vertices_count.argtypes = [p]
        L.tpch_get_id.restype = i64
        L.tpch_get_id.argtypes = [p, ctypes.c_char_p]
        L.tpch_hash_seed.argtypes = [p, p]
        L.tpch_synth_genome.argtypes = [u64, u64, p]
        L.tpch_synth_substitute.argtypes = [p, u64, u64, u64, p]
        L.tpch_synth_n_runs.argtypes = [p, u64, u64, u64, u64]
        _host = L
    return _host


def _view(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n)


def seed_table(q, bits, seed=None):
    """q x 5 (A,C,G,T,N) character tables; seed=None draws from /dev/urandom like the reference."""
    t = np.zeros((q, 5), dtype=np.uint64)
    if host().tpch_seed_table(0 if seed is None else seed, 0 if seed is None else 1, q, bits, t.ctypes.data) != 0:
        raise RuntimeError(host().tpch_last_error().decode())
    return t


HLL_REGISTERS = 16384  # p = 14 (include/twopaco_hip.h: tpc_distinct_sketch)


def hll_estimate(registers):
    """The distinct count behind HyperLogLog registers (host/filterplan.h); no device."""
    r = np.ascontiguousarray(registers, dtype=np.uint8)
    return float(host().tpch_hll_estimate(r.ctypes.data, r.size))


def filter_plan(n_distinct, q, text_length, filter_bytes_cap, rounds=0):
    """`-f auto`'s plan (host/filterplan.h; no device): dict with L, rounds, clipped, L_fp, L_mem and false_marks (predicted false
    marks per position).  rounds = 0: the plan chooses them."""
    out = (ctypes.c_int * 5)()
    fm = ctypes.c_double(0)
    if host().tpch_filter_plan(int(n_distinct), int(q), int(text_length), int(filter_bytes_cap), int(rounds), out, ctypes.byref(fm)) != 0:
        raise RuntimeError(host().tpch_last_error().decode())
    return {"L": out[0], "rounds": out[1], "clipped": bool(out[2]), "L_fp": out[3], "L_mem": out[4], "false_marks": fm.value}


TEXT_FORMATS = {"gfa1": 1, "gfa2": 2, "fasta": 3}  # TPC_TEXT_* of include/twopaco_hip.h


def graph_format(files, k, fmt, out_path, name, first, begin, end, seq_event_begin, prefix=False, threads=16):
    """The text of the compacted graph (gfa1 / gfa2 / fasta) from an event table (include/twopaco_hip.h: the tpc_segments_*
    group) and the FASTA files, written to out_path by host/graphformat.h -- no device involved.  name: int64 per event,
    first: bool per event, begin / end: the positions of the event's two records, seq_event_begin: one entry per sequence
    and one more (the events of sequence s are [seq_event_begin[s], seq_event_begin[s + 1]))."""
    name = np.ascontiguousarray(name, dtype=np.int64)
    begin = np.ascontiguousarray(begin, dtype=np.uint32)
    end = np.ascontiguousarray(end, dtype=np.uint32)
    seqs = np.ascontiguousarray(seq_event_begin, dtype=np.uint32)
    if not (name.size == begin.size == end.size == len(first)) or seqs.size < 1:
        raise ValueError("graph_format: one entry per event in name, first, begin, end; at least one in seq_event_begin")
    bits = np.zeros((name.size + 31) // 32 * 32, dtype=np.uint8)
    bits[:name.size] = np.asarray(first, dtype=bool)
    words = np.ascontiguousarray(np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)) if name.size else np.zeros(1, dtype=np.uint32)
    arr = (ctypes.c_char_p * len(files))(*[f.encode() for f in files])
    rc = host().tpch_graph_format(arr, len(files), k, fmt.encode(), 1 if prefix else 0, threads, name.size, name.ctypes.data, words.ctypes.data,
                                  begin.ctypes.data, end.ctypes.data, seqs.size - 1, seqs.ctypes.data, os.fsencode(out_path))
    if rc != 0:
        raise RuntimeError(host().tpch_last_error().decode())


class PackedText:
    """The packed global text T = N rec0 N rec1 N ... (host/textpack.h)."""

    def __init__(self):
        self._h = host().tpch_text_new()

    def close(self):
        if self._h and host is not None:
            host().tpch_text_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    @classmethod
    def from_fasta(cls, files, threads=1):
        t = cls()
        arr = (ctypes.c_char_p * len(files))(*[f.encode() for f in files])
        if host().tpch_text_add_fasta(t._h, arr, len(files), threads) != 0:
            raise RuntimeError(host().tpch_last_error().decode())
        return t

    @classmethod
    def from_codes(cls, records):
        """records: iterable of uint8 arrays with codes 0..3 (ACGT) and 4 (N)."""
        t = cls()
        for r in records:
            r = np.ascontiguousarray(r, dtype=np.uint8)
            host().tpch_text_add_codes(t._h, r.ctypes.data, r.size)
        return t

    @property
    def length(self):
        return host().tpch_text_length(self._h)

    @property
    def bases(self):
        return _view(host().tpch_text_bases(self._h), host().tpch_text_words(self._h), np.uint64)

    @property
    def nmask(self):
        return _view(host().tpch_text_nmask(self._h), host().tpch_text_words(self._h), np.uint32)

    @property
    def rec_start(self):
        return _view(host().tpch_text_rec_start(self._h), host().tpch_text_records(self._h), np.uint64).copy()

    @property
    def rec_length(self):
        return _view(host().tpch_text_rec_length(self._h), host().tpch_text_records(self._h), np.uint64).copy()


class Context:
    """One device context of the C-ABI (include/twopaco_hip.h)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        rc = hip().tpc_ctx_create(device, ctypes.byref(self._h))
        if rc != 0:
            self._h = None
            raise RuntimeError("tpc_ctx_create failed (%d): no HIP device -- there is no CPU fallback" % rc)

    def close(self):
        if getattr(self, "_h", None) and hip is not None:
            hip().tpc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError("twopaco_hip: %s (%d)" % (hip().tpc_last_error(self._h).decode(), rc))

    def set_option(self, name, value):
        """tpc_set_option: the tuning knobs and the tests-only options of include/twopaco_hip.h, among them test_links_slots_log2,
        test_distances_chunk_words, test_components_step_limit (the step bound of the next segments_components_build, 0 = its own) and, each
        for the next segments_classes_build alone, test_classes_slots_log2 (2^n slots, 0 = by the rows), test_classes_hash_bits (the low n
        bits of the hash, 0 .. 64, negative = all), test_classes_grid (workgroups per kernel, 0 = by the rows) and test_classes_wide (1 = a
        wave per row, 2 = a thread per row, 0 = by the words)."""
        self._ck(hip().tpc_set_option(self._h, name.encode(), int(value)))

    def stat(self, name):
        return int(hip().tpc_get_stat(self._h, name.encode()))

    def set_params(self, k, L, q, table):
        table = np.ascontiguousarray(table, dtype=np.uint64)
        assert table.shape == (q, 5)
        self.k, self.L, self.q = k, L, q
        self._ck(hip().tpc_set_params(self._h, k, L, q, table.ctypes.data))

    def seq_upload(self, text):
        b, n = np.ascontiguousarray(text.bases), np.ascontiguousarray(text.nmask)
        self._ck(hip().tpc_seq_upload(self._h, b.ctypes.data, n.ctypes.data, text.length))

    def run_begin(self):
        self._ck(hip().tpc_run_begin(self._h))

    def distinct_sketch(self, k):
        """(registers uint8[16384], contributing windows): the HyperLogLog sketch of the distinct canonical (k+1)-mers of the
        uploaded text (csrc/tpc_sketch.hip).  Needs seq_upload only."""
        reg = np.zeros(HLL_REGISTERS, dtype=np.uint8)
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_distinct_sketch(self._h, int(k), reg.ctypes.data, ctypes.byref(n)))
        return reg, n.value

    def filter_reset(self):
        self._ck(hip().tpc_filter_reset(self._h))

    def pass1_insert(self, lo=0, hi=None, count=True):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_pass1_insert(self._h, lo, (1 << self.L) if hi is None else hi, ctypes.byref(n) if count else None))
        return n.value

    def pass1_split_hist(self, rec_start, rec_len):
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        bins = np.zeros(1 << 24, dtype=np.uint32)
        self._ck(hip().tpc_pass1_split_hist(self._h, rs.ctypes.data, rl.ctypes.data, rs.size, bins.ctypes.data))
        return bins

    def pass1_query(self, lo=0, hi=None):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_pass1_query(self._h, lo, (1 << self.L) if hi is None else hi, ctypes.byref(n)))
        return n.value

    def pass1_query_begin(self, lo=0, hi=None):
        self._ck(hip().tpc_pass1_query_begin(self._h, lo, (1 << self.L) if hi is None else hi))

    def pass2_filter(self, abundance=(1 << 64) - 1):
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_filter(self._h, abundance, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"true": a.value, "false": b.value, "table": c.value}

    def pass2_marks(self):
        """Compacts this round's mask; returns the number of marked positions (kept in the context for the output pass)."""
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_marks(self._h, ctypes.byref(n)))
        return n.value

    def pass2_mark_owners(self, world, pos_ptr, owner_ptr):
        self._ck(hip().tpc_pass2_mark_owners(self._h, world, pos_ptr, owner_ptr))

    def pass2_filter_positions(self, pos_ptr, n, abundance=(1 << 64) - 1):
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_filter_positions(self._h, pos_ptr, n, abundance, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"true": a.value, "false": b.value, "table": c.value}

    def pass2_mark_records(self, world, rec_ptr, owner_ptr):
        self._ck(hip().tpc_pass2_mark_records(self._h, world, rec_ptr, owner_ptr))

    def pass2_filter_records(self, rec_ptr, n, abundance=(1 << 64) - 1):
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_filter_records(self._h, rec_ptr, n, abundance, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"true": a.value, "false": b.value, "table": c.value}

    def pass2_aggregate_records(self, world, rec_ptr, owner_ptr, abundance=(1 << 64) - 1):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_aggregate_records(self._h, world, abundance, rec_ptr, owner_ptr, ctypes.byref(n)))
        return n.value

    def pass2_filter_aggregated(self, rec_ptr, n, abundance=(1 << 64) - 1):
        a, b, c = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_pass2_filter_aggregated(self._h, rec_ptr, n, abundance, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"true": a.value, "false": b.value, "table": c.value}

    def shard_permute_rows(self, src_ptr, perm_ptr, n, row_words, dst_ptr):
        self._ck(hip().tpc_shard_permute_rows(self._h, src_ptr, perm_ptr, n, row_words, dst_ptr))

    def junctions_finalize(self):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_junctions_finalize(self._h, ctypes.byref(n)))
        self.n_junctions = n.value
        return n.value

    def junction_keys(self):
        C = hip().tpc_key_words(self._h)
        keys = np.zeros((self.n_junctions, C), dtype=np.uint64)
        self._ck(hip().tpc_junction_keys(self._h, keys.ctypes.data))
        return keys

    def junction_keys_raw(self):
        """Keys appended so far (unsorted, before junctions_finalize)."""
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_junction_keys_raw(self._h, None, ctypes.byref(n)))
        keys = np.zeros((n.value, hip().tpc_key_words(self._h)), dtype=np.uint64)
        self._ck(hip().tpc_junction_keys_raw(self._h, keys.ctypes.data, ctypes.byref(n)))
        return keys

    def junction_keys_set(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self._ck(hip().tpc_junction_keys_set(self._h, keys.ctypes.data, keys.shape[0]))

    def key_words(self):
        return int(hip().tpc_key_words(self._h))

    def junction_keys_export(self, dst_ptr, cap_keys):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_junction_keys_export(self._h, dst_ptr, cap_keys, ctypes.byref(n)))
        return n.value

    def junction_keys_import(self, src_ptr, n, append):
        self._ck(hip().tpc_junction_keys_import(self._h, src_ptr, n, 1 if append else 0))

    def get_id(self, kmer):
        return hip().tpc_get_id(self._h, kmer.encode())

    def emit(self):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_emit(self._h, ctypes.byref(a), ctypes.byref(b)))
        self.n_marked, self.n_valid = a.value, b.value
        return a.value, b.value

    def emit_fetch(self):
        g = np.zeros(self.n_marked, dtype=np.uint64)
        ids = np.zeros(self.n_marked, dtype=np.int64)
        self._ck(hip().tpc_emit_fetch(self._h, g.ctypes.data, ids.ctypes.data))
        return g, ids

    def emit_stream(self, rec_start, rec_len):
        """The bytes of de_bruijn.bin (after emit()); returns (bytes, records without separators)."""
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        nb, nr = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._ck(hip().tpc_emit_stream(self._h, rs.ctypes.data, rl.ctypes.data, rs.size, ctypes.byref(nb), ctypes.byref(nr)))
        buf = np.zeros(nb.value, dtype=np.uint8)
        if hip().tpc_emit_stream_fetch(self._h, 0, nb.value, buf.ctypes.data) != 0:
            raise RuntimeError("tpc_emit_stream_fetch failed")
        return buf.tobytes(), nr.value

    def emit_import(self, g_dev_ptr, id_dev_ptr, n):
        """Installs n (position, id) pairs from device buffers (uint64 / int64, positions ascending) as the lists emit() would have left."""
        self._ck(hip().tpc_emit_import(self._h, g_dev_ptr, id_dev_ptr, n))
        self.n_marked = n

    def shard_chunk(self):
        """(chunk_lo, chunk_hi): this rank's chunk of text positions (after shard_config and seq_upload); the last rank's end is 2^64 - 1."""
        lo, hi = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if hip().tpc_shard_chunk(self._h, ctypes.byref(lo), ctypes.byref(hi)) != 0:
            raise RuntimeError("tpc_shard_chunk failed: seq_upload first")
        return lo.value, hi.value

    def emit_stream_partial(self, rec_start, rec_len):
        """Step 1 of the stream cut over ranks: (cnt uint64 [n_rec], flags uint32 [n_rec]) -- per sequence the real-id records among THIS
        context's marks, and bit 0 / 1: it holds the first / last k-mer with a real id."""
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        cnt, flags = np.zeros(rs.size, dtype=np.uint64), np.zeros(rs.size, dtype=np.uint32)
        self._ck(hip().tpc_emit_stream_partial(self._h, rs.ctypes.data, rl.ctypes.data, rs.size, cnt.ctypes.data, flags.ctypes.data))
        return cnt, flags

    def emit_stream_part(self, rec_start, rec_len, gflags, e_scan, s_scan, before, r_last, chunk_lo, chunk_hi, slot0, n_slots):
        """Step 2, after emit_stream_partial and the add-up over the ranks (include/twopaco_hip.h: tpc_emit_stream_part): the bytes of this
        rank's n_slots slots, the file's [12 slot0, 12 (slot0 + n_slots))."""
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        gf = np.ascontiguousarray(gflags, dtype=np.uint32)
        es, ss = np.ascontiguousarray(e_scan, dtype=np.uint64), np.ascontiguousarray(s_scan, dtype=np.uint64)
        bf = np.ascontiguousarray(before, dtype=np.uint64)
        if not (rl.size == gf.size == bf.size == rs.size and es.size == ss.size == rs.size + 1):
            raise ValueError("emit_stream_part: n_rec entries in rec_len, gflags, before; n_rec + 1 in e_scan, s_scan")
        nb = ctypes.c_uint64(0)
        self._ck(hip().tpc_emit_stream_part(self._h, rs.ctypes.data, rl.ctypes.data, rs.size, gf.ctypes.data, es.ctypes.data, ss.ctypes.data, bf.ctypes.data,
                                            r_last, chunk_lo, chunk_hi, slot0, n_slots, ctypes.byref(nb)))
        buf = np.zeros(nb.value, dtype=np.uint8)
        if hip().tpc_emit_stream_fetch(self._h, 0, nb.value, buf.ctypes.data) != 0:
            raise RuntimeError("tpc_emit_stream_fetch failed")
        return buf.tobytes()

    def segments_build(self, stream, k, rec_start, rec_len, ambiguous=()):
        """The segment table of graphdump's gfa1 / gfa2 / fasta walk (csrc/tpc_segments.hip) over the text of seq_upload.
        stream: the bytes of de_bruijn.bin, or None for the stream emit_stream left on the device.  ambiguous: ascending
        global text positions of the valid letters other than A C G T N.  Returns segments_counts()."""
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        amb = np.ascontiguousarray(ambiguous, dtype=np.uint64)
        if stream is None:
            self._ck(hip().tpc_segments_build_resident(self._h, k, rs.ctypes.data, rl.ctypes.data, rs.size, amb.ctypes.data, amb.size))
        else:
            buf = np.frombuffer(bytes(stream), dtype=np.uint8)
            self._ck(hip().tpc_segments_build_host(self._h, buf.ctypes.data, buf.size, k, rs.ctypes.data, rl.ctypes.data, rs.size, amb.ctypes.data, amb.size))
        return self.segments_counts()

    def segments_counts(self):
        """dict: events, segments (first bits set), n_named ('N'-named events), table_bytes, slots, peak_device_bytes."""
        c = np.zeros(6, dtype=np.uint64)
        self._ck(hip().tpc_segments_counts(self._h, c.ctypes.data))
        return dict(zip(("events", "segments", "n_named", "table_bytes", "slots", "peak_device_bytes"), (int(x) for x in c)))

    def segments_error(self):
        """(slot of the failing pair's second record, text of the serial walk's error) or None."""
        slot, kind = ctypes.c_uint64(0), ctypes.c_int(0)
        self._ck(hip().tpc_segments_error(self._h, ctypes.byref(slot), ctypes.byref(kind)))
        return None if kind.value == 0 else (slot.value, SEGMENT_ERRORS[kind.value])

    def segments_fetch(self, e0=0, n=None):
        """(name[e0 : e0 + n] as int64, first[e0 : e0 + n] as bool); n = None: to the last event."""
        events = self.segments_counts()["events"]
        n = events - e0 if n is None else n
        name = np.zeros(n, dtype=np.int64)
        self._ck(hip().tpc_segments_fetch_names(self._h, e0, n, name.ctypes.data))
        w0, w1 = e0 // 32, (e0 + n + 31) // 32
        words = np.zeros(max(w1 - w0, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_fetch_first(self._h, w0, words.size, words.ctypes.data))
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[e0 - 32 * w0:e0 - 32 * w0 + n].astype(bool)
        return name, bits

    def segments_fetch_events(self, e0=0, n=None):
        """(begin[e0 : e0 + n], end[e0 : e0 + n]) as uint32: the positions of every event's left and right record; n = None: to the last event."""
        n = self.segments_counts()["events"] - e0 if n is None else n
        begin, end = np.zeros(max(n, 0), dtype=np.uint32), np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_fetch_events(self._h, e0, n, begin.ctypes.data, end.ctypes.data))
        return begin, end

    def segments_fetch_sequences(self, s0, n):
        """seq_event_begin[s0 : s0 + n] as uint32 (the table has one entry more than the build was given sequences): the events
        of sequence s are [seq_event_begin[s], seq_event_begin[s + 1])."""
        out = np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_fetch_sequences(self._h, s0, n, out.ctypes.data))
        return out

    def segments_text_plan(self, fmt, seq_names, amb_letters=b""):
        """Sizes and offsets of the graph text (csrc/tpc_segtext.hip) of the last segments_build, whose error must be None.
        fmt: "gfa1" / "gfa2" / "fasta" (or the C-ABI's 1 / 2 / 3); seq_names: the name of every input sequence as it is to be
        printed (str or bytes); amb_letters: the letter at every ambiguous position of the build, in its order.  Returns the
        size of the whole text in bytes."""
        code = TEXT_FORMATS.get(fmt, fmt)
        names = [n.encode() if isinstance(n, str) else bytes(n) for n in seq_names]
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        off = np.zeros(len(names) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(n) for n in names], dtype=np.uint64) if names else 0
        letters = amb_letters.encode() if isinstance(amb_letters, str) else bytes(amb_letters)
        let = np.frombuffer(letters + b"\0", dtype=np.uint8)
        total = ctypes.c_uint64(0)
        self._ck(hip().tpc_segments_text_plan(self._h, int(code), blob.ctypes.data, off.ctypes.data, let.ctypes.data if letters else None, ctypes.byref(total)))
        return total.value

    def segments_text_fetch(self, byte0, n):
        """Bytes [byte0, byte0 + n) of the text of the last segments_text_plan, rendered on the device."""
        buf = np.zeros(max(n, 1), dtype=np.uint8)
        self._ck(hip().tpc_segments_text_fetch(self._h, byte0, n, buf.ctypes.data))
        return buf[:n].tobytes()

    def segments_text_write(self, fd, file_offset=0, window_bytes=0):
        """The whole text to the file descriptor fd (a regular file: at file_offset; a pipe: in order).  Returns the bytes written."""
        written = ctypes.c_uint64(0)
        self._ck(hip().tpc_segments_text_write(self._h, fd, file_offset, window_bytes, ctypes.byref(written)))
        return written.value

    def segments_colors_build(self, color_of_seq, n_colors):
        """The segment colour table (csrc/tpc_colors.hip) over the table of the last segments_build, whose error must be None:
        color_of_seq[s] in [0, n_colors) for every sequence of that build.  Returns segments_colors_info()."""
        col = np.ascontiguousarray(color_of_seq, dtype=np.uint32)
        self._ck(hip().tpc_segments_colors_build(self._h, col.ctypes.data if col.size else None, n_colors))
        return self.segments_colors_info()

    def segments_colors_info(self):
        """dict: rows (segments), colors, words (uint32 of presence per row)."""
        c = np.zeros(3, dtype=np.uint64)
        self._ck(hip().tpc_segments_colors_info(self._h, c.ctypes.data))
        return dict(zip(("rows", "colors", "words"), (int(x) for x in c)))

    def segments_colors_fetch_rows(self, r0=0, n=None):
        """(first_event, occurrences, forward, n_colors) of rows [r0, r0 + n) as uint32; n = None: to the last row."""
        n = self.segments_colors_info()["rows"] - r0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(4)]
        self._ck(hip().tpc_segments_colors_fetch_rows(self._h, r0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_colors_fetch_presence(self, r0=0, n=None):
        """The presence words of rows [r0, r0 + n) as uint32 [n, words]: bit c % 32 of word c // 32 is colour c."""
        info = self.segments_colors_info()
        n = info["rows"] - r0 if n is None else n
        out = np.zeros((max(n, 0), info["words"]), dtype=np.uint32)
        self._ck(hip().tpc_segments_colors_fetch_presence(self._h, r0, n, out.ctypes.data))
        return out

    def segments_colors_fetch_hist(self):
        """(segments, bases) as uint64 [colors + 1]: rows with that many colours and the sum of their lengths."""
        bins = self.segments_colors_info()["colors"] + 1
        seg, bases = np.zeros(bins, dtype=np.uint64), np.zeros(bins, dtype=np.uint64)
        self._ck(hip().tpc_segments_colors_fetch_hist(self._h, seg.ctypes.data, bases.ctypes.data))
        return seg, bases

    def segments_links_build(self):
        """The link table (csrc/tpc_links.hip) over the table of the last segments_build, whose error must be None.  Returns
        segments_links_info()."""
        self._ck(hip().tpc_segments_links_build(self._h))
        return self.segments_links_info()

    def segments_links_info(self):
        """dict: rows (distinct links), occurrences, slots (of the device hash set), peak_bytes (device memory of the stage)."""
        c = np.zeros(4, dtype=np.uint64)
        self._ck(hip().tpc_segments_links_info(self._h, c.ctypes.data))
        return dict(zip(("rows", "occurrences", "slots", "peak_bytes"), (int(x) for x in c)))

    def segments_links_fetch_rows(self, r0=0, n=None):
        """(first_event, count, same) of rows [r0, r0 + n) as uint32; n = None: to the last row."""
        n = self.segments_links_info()["rows"] - r0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(3)]
        self._ck(hip().tpc_segments_links_fetch_rows(self._h, r0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_links_fetch_first(self, word0=0, n_words=None):
        """Words [word0, word0 + n_words) of the link_first bits as uint32 (bit e % 32 of word e // 32); None: to the last word."""
        if n_words is None:
            n_words = (self.segments_counts()["events"] + 31) // 32 - word0
        out = np.zeros(max(n_words, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_links_fetch_first(self._h, word0, n_words, out.ctypes.data))
        return out

    def segments_bubbles_build(self):
        """The simple bubbles (csrc/tpc_bubbles.hip) over the link table of the last segments_links_build.  Returns
        segments_bubbles_info()."""
        self._ck(hip().tpc_segments_bubbles_build(self._h))
        return self.segments_bubbles_info()

    def segments_bubbles_info(self):
        """dict: bubbles, sides (2 x segments), arcs, peak_bytes (device memory of the stage)."""
        c = np.zeros(4, dtype=np.uint64)
        self._ck(hip().tpc_segments_bubbles_info(self._h, c.ctypes.data))
        return dict(zip(("bubbles", "sides", "arcs", "peak_bytes"), (int(x) for x in c)))

    def segments_bubbles_fetch_rows(self, b0=0, n=None):
        """(source, arm_a, arm_b, sink) of bubbles [b0, b0 + n) as uint32 side codes (row * 2 + 1 for '-'); n = None: to the last."""
        n = self.segments_bubbles_info()["bubbles"] - b0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(4)]
        self._ck(hip().tpc_segments_bubbles_fetch_rows(self._h, b0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_bubbles_fetch_sides(self, c0=0, n=None):
        """(deg, lo, hi) of sides [c0, c0 + n) as uint32; n = None: to the last side."""
        n = self.segments_bubbles_info()["sides"] - c0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(3)]
        self._ck(hip().tpc_segments_bubbles_fetch_sides(self._h, c0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_bubbles_fetch_hist(self):
        """uint64 [6]: the sides of degree 0, 1, 2, 3, 4 and 5 or more."""
        out = np.zeros(6, dtype=np.uint64)
        self._ck(hip().tpc_segments_bubbles_fetch_hist(self._h, out.ctypes.data))
        return out

    def segments_distances_build(self):
        """The genome distance matrices (csrc/tpc_distances.hip) over the colour table of the last segments_colors_build.  Returns
        segments_distances_info()."""
        self._ck(hip().tpc_segments_distances_build(self._h))
        return self.segments_distances_info()

    def segments_distances_info(self):
        """dict: colors, rows, planes (weight bit planes used), peak_bytes (device memory of the stage)."""
        c = np.zeros(4, dtype=np.uint64)
        self._ck(hip().tpc_segments_distances_info(self._h, c.ctypes.data))
        return dict(zip(("colors", "rows", "planes", "peak_bytes"), (int(x) for x in c)))

    def segments_distances_fetch(self, i0=0, n=None):
        """(segments, edges): rows [i0, i0 + n) of both matrices as uint64 [n, colors]; n = None: to the last row."""
        colors = self.segments_distances_info()["colors"]
        n = colors - i0 if n is None else n
        out = [np.zeros((max(n, 0), colors), dtype=np.uint64) for _ in range(2)]
        self._ck(hip().tpc_segments_distances_fetch(self._h, i0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_components_build(self):
        """The connected components (csrc/tpc_components.hip) over the link table of the last segments_links_build and the colour table
        of the last segments_colors_build.  Returns segments_components_info()."""
        self._ck(hip().tpc_segments_components_build(self._h))
        return self.segments_components_info()

    def segments_components_info(self):
        """dict: components, rows, largest (segments of the largest component), peak_bytes (device memory of the stage)."""
        c = np.zeros(4, dtype=np.uint64)
        self._ck(hip().tpc_segments_components_info(self._h, c.ctypes.data))
        return dict(zip(("components", "rows", "largest", "peak_bytes"), (int(x) for x in c)))

    def segments_components_fetch_members(self, r0=0, n=None):
        """component[r] of rows [r0, r0 + n) as uint32; n = None: to the last row."""
        n = self.segments_components_info()["rows"] - r0 if n is None else n
        out = np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_components_fetch_members(self._h, r0, n, out.ctypes.data))
        return out

    def segments_components_fetch_rows(self, p0=0, n=None):
        """(root as uint32; segments, links, length, edges, occurrences as uint64) of components [p0, p0 + n); n = None: to the last."""
        n = self.segments_components_info()["components"] - p0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32)] + [np.zeros(max(n, 0), dtype=np.uint64) for _ in range(5)]
        self._ck(hip().tpc_segments_components_fetch_rows(self._h, p0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_components_fetch_presence(self, p0=0, n=None):
        """uint32 [n, W] presence words of components [p0, p0 + n), W as of the colour table; n = None: to the last."""
        n = self.segments_components_info()["components"] - p0 if n is None else n
        out = np.zeros((max(n, 0), self.segments_colors_info()["words"]), dtype=np.uint32)
        self._ck(hip().tpc_segments_components_fetch_presence(self._h, p0, n, out.ctypes.data))
        return out

    def segments_classes_build(self):
        """The colour classes (csrc/tpc_classes.hip) over the colour table of the last segments_colors_build.  Returns
        segments_classes_info()."""
        self._ck(hip().tpc_segments_classes_build(self._h))
        return self.segments_classes_info()

    def segments_classes_info(self):
        """dict: classes, rows, largest (segments of the largest class), collisions (probes that met a slot of another class; depends on
        the schedule), peak_bytes (device memory of the stage)."""
        c = np.zeros(5, dtype=np.uint64)
        self._ck(hip().tpc_segments_classes_info(self._h, c.ctypes.data))
        return dict(zip(("classes", "rows", "largest", "collisions", "peak_bytes"), (int(x) for x in c)))

    def segments_classes_fetch_members(self, r0=0, n=None):
        """class[r] of rows [r0, r0 + n) as uint32; n = None: to the last row."""
        n = self.segments_classes_info()["rows"] - r0 if n is None else n
        out = np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_classes_fetch_members(self._h, r0, n, out.ctypes.data))
        return out

    def segments_classes_fetch_rows(self, p0=0, n=None):
        """(first as uint32; segments, length, edges, occurrences as uint64) of classes [p0, p0 + n); n = None: to the last."""
        n = self.segments_classes_info()["classes"] - p0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32)] + [np.zeros(max(n, 0), dtype=np.uint64) for _ in range(4)]
        self._ck(hip().tpc_segments_classes_fetch_rows(self._h, p0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_classes_fetch_presence(self, p0=0, n=None):
        """uint32 [n, W] presence words of classes [p0, p0 + n), W as of the colour table; n = None: to the last."""
        n = self.segments_classes_info()["classes"] - p0 if n is None else n
        out = np.zeros((max(n, 0), self.segments_colors_info()["words"]), dtype=np.uint32)
        self._ck(hip().tpc_segments_classes_fetch_presence(self._h, p0, n, out.ctypes.data))
        return out

    def segments_classes_fetch_sets(self):
        """(classes, segments, edges) as uint64 [colours + 1] each: by number of colours, 0 where no class has that many."""
        n = self.segments_colors_info()["colors"] + 1
        out = [np.zeros(n, dtype=np.uint64) for _ in range(3)]
        self._ck(hip().tpc_segments_classes_fetch_sets(self._h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_superbubbles_build(self, max_inside=62):
        """The bounded superbubbles (csrc/tpc_superbubbles.hip) over the link table of the last segments_links_build and the colour table
        of the last segments_colors_build; max_inside 2 .. 62.  Returns segments_superbubbles_info()."""
        self._ck(hip().tpc_segments_superbubbles_build(self._h, max_inside))
        return self.segments_superbubbles_info()

    def segments_superbubbles_info(self):
        """dict: superbubbles, sides, members (in total), unmirrored (entrances whose mirror is missing), peak_bytes, arcs, max_inside."""
        c = np.zeros(7, dtype=np.uint64)
        self._ck(hip().tpc_segments_superbubbles_info(self._h, c.ctypes.data))
        return dict(zip(("superbubbles", "sides", "members", "unmirrored", "peak_bytes", "arcs", "max_inside"), (int(x) for x in c)))

    def segments_superbubbles_fetch_adjacency(self):
        """(offsets uint32 [sides + 1], heads uint32 [arcs]): the arcs that leave every side, every list ascending."""
        info = self.segments_superbubbles_info()
        off, heads = np.zeros(info["sides"] + 1, dtype=np.uint32), np.zeros(info["arcs"], dtype=np.uint32)
        self._ck(hip().tpc_segments_superbubbles_fetch_adjacency(self._h, off.ctypes.data, heads.ctypes.data))
        return off, heads

    def segments_superbubbles_fetch_exits(self, c0=0, n=None):
        """exit[] of sides [c0, c0 + n) as uint32, all ones for none; n = None: to the last side."""
        n = self.segments_superbubbles_info()["sides"] - c0 if n is None else n
        out = np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_superbubbles_fetch_exits(self._h, c0, n, out.ctypes.data))
        return out

    def segments_superbubbles_fetch_rows(self, b0=0, n=None):
        """(entrance, exit, inside, arcs, n_colors as uint32; paths, min_edges, max_edges as uint64) of rows [b0, b0 + n); n = None: to the last."""
        n = self.segments_superbubbles_info()["superbubbles"] - b0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(5)] + [np.zeros(max(n, 0), dtype=np.uint64) for _ in range(3)]
        self._ck(hip().tpc_segments_superbubbles_fetch_rows(self._h, b0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_superbubbles_fetch_members(self):
        """(offsets uint32 [superbubbles + 1], sides uint32 [members]): the inside sides of every row, ascending."""
        info = self.segments_superbubbles_info()
        off, sides = np.zeros(info["superbubbles"] + 1, dtype=np.uint32), np.zeros(info["members"], dtype=np.uint32)
        self._ck(hip().tpc_segments_superbubbles_fetch_members(self._h, off.ctypes.data, sides.ctypes.data))
        return off, sides

    def segments_superbubbles_fetch_presence(self, b0=0, n=None):
        """uint32 [n, W] presence words of rows [b0, b0 + n), W as of the colour table; n = None: to the last."""
        n = self.segments_superbubbles_info()["superbubbles"] - b0 if n is None else n
        out = np.zeros((max(n, 0), self.segments_colors_info()["words"]), dtype=np.uint32)
        self._ck(hip().tpc_segments_superbubbles_fetch_presence(self._h, b0, n, out.ctypes.data))
        return out

    def segments_tracks_build(self, color_of_seq, n_colors, only=None):
        """The presence tracks (csrc/tpc_tracks.hip) over the table of the last segments_build and the colour table of the last
        segments_colors_build, which the caller promises was built with the same color_of_seq; only: one colour, None = all.  The
        option test_tracks_grid (set_option) caps the workgroups per kernel for the next build alone.  Returns segments_tracks_info()."""
        col = np.ascontiguousarray(color_of_seq, dtype=np.uint32)
        self._ck(hip().tpc_segments_tracks_build(self._h, col.ctypes.data if col.size else None, n_colors, TRACKS_ALL if only is None else only))
        return self.segments_tracks_info()

    def segments_tracks_info(self):
        """dict: intervals, selected (events), colors, only (None: all colours), peak_bytes (device memory of the stage)."""
        c = np.zeros(5, dtype=np.uint64)
        self._ck(hip().tpc_segments_tracks_info(self._h, c.ctypes.data))
        d = dict(zip(("intervals", "selected", "colors", "only", "peak_bytes"), (int(x) for x in c)))
        d["only"] = None if d["only"] == TRACKS_ALL else d["only"]
        return d

    def segments_tracks_fetch_rows(self, i0=0, n=None):
        """(first_event, last_event, row) of intervals [i0, i0 + n) as uint32; n = None: to the last interval."""
        n = self.segments_tracks_info()["intervals"] - i0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(3)]
        self._ck(hip().tpc_segments_tracks_fetch_rows(self._h, i0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_tracks_fetch_colors(self):
        """(intervals, edges, core_edges, private_edges) per colour as uint64 [colors]."""
        out = [np.zeros(self.segments_tracks_info()["colors"], dtype=np.uint64) for _ in range(4)]
        self._ck(hip().tpc_segments_tracks_fetch_colors(self._h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_tracks_fetch_depth(self):
        """(intervals, edges) per number of colours as uint64 [colors + 1], 0 where no interval has that many."""
        out = [np.zeros(self.segments_tracks_info()["colors"] + 1, dtype=np.uint64) for _ in range(2)]
        self._ck(hip().tpc_segments_tracks_fetch_depth(self._h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_variants_build(self, color_of_seq, n_colors, ref=None):
        """The variants (csrc/tpc_variants.hip) over the table of the last segments_build and the colour, link and superbubble tables
        built over it, the colour table with the same color_of_seq (the caller's promise); ref: the reference colour, None = none.
        The option test_variants_grid (set_option) caps the workgroups per kernel for the next build alone.  Returns segments_variants_info()."""
        col = np.ascontiguousarray(color_of_seq, dtype=np.uint32)
        self._ck(hip().tpc_segments_variants_build(self._h, col.ctypes.data if col.size else None, n_colors, VARIANTS_NONE if ref is None else ref))
        return self.segments_variants_info()

    def segments_variants_info(self):
        """dict: sites, alleles, traversals, strays, peak_bytes, colors, ref (None: no reference), hist_bins, superbubbles."""
        c = np.zeros(9, dtype=np.uint64)
        self._ck(hip().tpc_segments_variants_info(self._h, c.ctypes.data))
        d = dict(zip(("sites", "alleles", "traversals", "strays", "peak_bytes", "colors", "ref", "hist_bins", "superbubbles"), (int(x) for x in c)))
        d["ref"] = None if d["ref"] == VARIANTS_NONE else d["ref"]
        return d

    def segments_variants_fetch_traversals(self, t0=0, n=None):
        """(start, last, d, row, edges as uint32, mask as uint64) of traversals [t0, t0 + n); n = None: to the last one."""
        n = self.segments_variants_info()["traversals"] - t0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(5)] + [np.zeros(max(n, 0), dtype=np.uint64)]
        self._ck(hip().tpc_segments_variants_fetch_traversals(self._h, t0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_variants_fetch_alleles(self, a0=0, n=None):
        """(row, sides, edges, first, n_colors as uint32, mask, traversals as uint64) of alleles [a0, a0 + n); n = None: to the last one."""
        n = self.segments_variants_info()["alleles"] - a0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(5)] + [np.zeros(max(n, 0), dtype=np.uint64) for _ in range(2)]
        self._ck(hip().tpc_segments_variants_fetch_alleles(self._h, a0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_variants_fetch_presence(self, a0=0, n=None):
        """The presence words of alleles [a0, a0 + n) as uint32 [n, W]; n = None: to the last one."""
        info = self.segments_variants_info()
        n = info["alleles"] - a0 if n is None else n
        out = np.zeros((max(n, 0), (info["colors"] + 31) // 32), dtype=np.uint32)
        self._ck(hip().tpc_segments_variants_fetch_presence(self._h, a0, n, out.ctypes.data))
        return out

    def segments_variants_fetch_sites(self, b0=0, n=None):
        """(allele_offset uint32 [n + 1], traversals uint64, ref_allele uint32, ref_traversals uint64) of superbubble rows [b0, b0 + n)."""
        n = self.segments_variants_info()["superbubbles"] - b0 if n is None else n
        out = [np.zeros(max(n, 0) + 1, dtype=np.uint32), np.zeros(max(n, 0), dtype=np.uint64), np.zeros(max(n, 0), dtype=np.uint32), np.zeros(max(n, 0), dtype=np.uint64)]
        self._ck(hip().tpc_segments_variants_fetch_sites(self._h, b0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_variants_fetch_hist(self):
        """The sites by their number of alleles as uint64 [hist_bins]."""
        out = np.zeros(self.segments_variants_info()["hist_bins"], dtype=np.uint64)
        self._ck(hip().tpc_segments_variants_fetch_hist(self._h, out.ctypes.data))
        return out

    def segments_anchors_build(self, color_of_seq, n_colors, ref_color=0):
        """The anchor blocks (csrc/tpc_anchors.hip) of every other colour against ref_color, over the table of the last segments_build,
        whose error must be None: color_of_seq[s] in [0, n_colors) for every sequence of that build.  Returns segments_anchors_info()."""
        col = np.ascontiguousarray(color_of_seq, dtype=np.uint32)
        self._ck(hip().tpc_segments_anchors_build(self._h, col.ctypes.data if col.size else None, n_colors, ref_color))
        return self.segments_anchors_info()

    def segments_anchors_info(self):
        """dict: blocks, anchors, colors, ref_color, ref_edges, peak_bytes (device memory of the stage)."""
        c = np.zeros(6, dtype=np.uint64)
        self._ck(hip().tpc_segments_anchors_info(self._h, c.ctypes.data))
        return dict(zip(("blocks", "anchors", "colors", "ref_color", "ref_edges", "peak_bytes"), (int(x) for x in c)))

    def segments_anchors_fetch_mates(self, e0=0, n=None):
        """mate[] of events [e0, e0 + n) as uint32, all ones for none; n = None: to the last event."""
        n = self.segments_counts()["events"] - e0 if n is None else n
        out = np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_anchors_fetch_mates(self._h, e0, n, out.ctypes.data))
        return out

    def segments_anchors_fetch_rows(self, b0=0, n=None):
        """(query_first, query_last, ref_first, ref_last) of blocks [b0, b0 + n) as uint32 event indices; n = None: to the last block."""
        n = self.segments_anchors_info()["blocks"] - b0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(4)]
        self._ck(hip().tpc_segments_anchors_fetch_rows(self._h, b0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_anchors_fetch_shared(self):
        """(blocks, anchors, edges, reverse_edges) per colour as uint64 [colors]; the reference colour's entries are 0."""
        out = [np.zeros(self.segments_anchors_info()["colors"], dtype=np.uint64) for _ in range(4)]
        self._ck(hip().tpc_segments_anchors_fetch_shared(self._h, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_edges_build(self):
        """The edge index (csrc/tpc_locate.hip) over the table of the last segments_build, whose error must be None, and the text it
        was built over: canonical (k+1)-mer -> (smallest position, row).  Returns segments_edges_info()."""
        self._ck(hip().tpc_segments_edges_build(self._h))
        return self.segments_edges_info()

    def segments_edges_info(self):
        """dict: entries, duplicates, skipped, slots, longest_probe, peak_bytes."""
        c = np.zeros(6, dtype=np.uint64)
        self._ck(hip().tpc_segments_edges_info(self._h, c.ctypes.data))
        return dict(zip(("entries", "duplicates", "skipped", "slots", "longest_probe", "peak_bytes"), (int(x) for x in c)))

    def segments_locate(self, text):
        """Every window of the PackedText `text` through the edge index.  Returns segments_locate_info()."""
        bases, nmask = np.ascontiguousarray(text.bases), np.ascontiguousarray(text.nmask)
        start, length = np.ascontiguousarray(text.rec_start, dtype=np.uint64), np.ascontiguousarray(text.rec_length, dtype=np.uint64)
        self._ck(hip().tpc_segments_locate(self._h, bases.ctypes.data, nmask.ctypes.data, text.length, start.ctypes.data if start.size else None,
                                           length.ctypes.data if length.size else None, start.size))
        return self.segments_locate_info()

    def segments_locate_info(self):
        """dict: positions, windows, found, runs, colors (0 = no colour table was used), peak_bytes."""
        c = np.zeros(6, dtype=np.uint64)
        self._ck(hip().tpc_segments_locate_info(self._h, c.ctypes.data))
        return dict(zip(("positions", "windows", "found", "runs", "colors", "peak_bytes"), (int(x) for x in c)))

    def segments_locate_fetch_hits(self, p0=0, n=None):
        """(hit uint64, row uint32) of positions [p0, p0 + n): hit all ones = invalid, all ones - 1 = absent, else rev << 63 | g."""
        n = self.segments_locate_info()["positions"] - p0 if n is None else n
        hit, row = np.zeros(max(n, 0), dtype=np.uint64), np.zeros(max(n, 0), dtype=np.uint32)
        self._ck(hip().tpc_segments_locate_fetch_hits(self._h, p0, n, hit.ctypes.data, row.ctypes.data))
        return hit, row

    def segments_locate_fetch_runs(self, r0=0, n=None):
        """(q_first, length, row, rev, off_first) of runs [r0, r0 + n) as uint32; n = None: to the last run."""
        n = self.segments_locate_info()["runs"] - r0 if n is None else n
        out = [np.zeros(max(n, 0), dtype=np.uint32) for _ in range(5)]
        self._ck(hip().tpc_segments_locate_fetch_runs(self._h, r0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_locate_fetch_records(self, s0, n):
        """(windows, found, forward, runs) of query records [s0, s0 + n) as uint64."""
        out = [np.zeros(max(n, 0), dtype=np.uint64) for _ in range(4)]
        self._ck(hip().tpc_segments_locate_fetch_records(self._h, s0, n, *[a.ctypes.data for a in out]))
        return tuple(out)

    def segments_locate_fetch_shared(self, s0, n):
        """uint64 [n, colors]: the hits of query records [s0, s0 + n) whose row has the colour."""
        out = np.zeros((max(n, 0), self.segments_locate_info()["colors"]), dtype=np.uint64)
        self._ck(hip().tpc_segments_locate_fetch_shared(self._h, s0, n, out.ctypes.data))
        return out

    def filter_words(self):
        return int(hip().tpc_filter_words(self._h))

    def filter_download(self):
        w = np.zeros(hip().tpc_filter_words(self._h), dtype=np.uint32)
        self._ck(hip().tpc_filter_download(self._h, w.ctypes.data))
        return w

    def filter_upload(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint32)
        assert w.size == hip().tpc_filter_words(self._h)
        self._ck(hip().tpc_filter_upload(self._h, w.ctypes.data))

    def mask_download(self, run_wide=False):
        w = np.zeros(hip().tpc_mask_words(self._h), dtype=np.uint32)
        self._ck(hip().tpc_mask_download(self._h, 1 if run_wide else 0, w.ctypes.data))
        return w

    def hash_dump(self, g0, n):
        out = np.zeros((n, self.q, 2), dtype=np.uint64)
        self._ck(hip().tpc_hash_dump(self._h, g0, n, out.ctypes.data))
        return out

    def kernel_ms(self, name):
        return hip().tpc_kernel_ms(self._h, KERNELS[name])

    # ---- address-sharded filter: device pointers in, no communication here (see twopaco_amd/dist.py)
    def shard_config(self, rank, world):
        self._ck(hip().tpc_shard_config(self._h, rank, world))

    def shard_plan(self, which, lo=0, hi=None):
        g = np.zeros(16, dtype=np.uint64)
        self._ck(hip().tpc_shard_plan(self._h, which, lo, (1 << self.L) if hi is None else hi, g.ctypes.data))
        names = ["batches", "tiles_per_rank", "region_block_bytes", "count_block_bytes", "survivor_cap", "overflow_cap", "overflow_entry_bytes",
                 "slice_bits", "b1", "b2", "perm_mult", "perm_inv", "b3"]
        return {n: int(g[i]) for i, n in enumerate(names)}

    def shard_hash(self, which, batch, send_regions_ptr, send_counts_ptr, lo=0, hi=None):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_hash(self._h, which, batch, lo, (1 << self.L) if hi is None else hi, send_regions_ptr, send_counts_ptr, ctypes.byref(n)))
        return n.value

    def shard_overflow_get(self, which, dst_ptr, n):
        self._ck(hip().tpc_shard_overflow_get(self._h, which, dst_ptr, n))

    def shard_overflow_set(self, which, src_ptr, n):
        self._ck(hip().tpc_shard_overflow_set(self._h, which, src_ptr, n))

    def shard_apply(self, which, batch, recv_regions_ptr, recv_counts_ptr):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_apply(self._h, which, batch, recv_regions_ptr, recv_counts_ptr, ctypes.byref(n)))
        return n.value

    def shard_pack(self, which, send_regions_ptr, send_counts_ptr, packed_ptr, world):
        """Used prefixes of the level-1 regions, destination major; returns the bytes for every destination rank."""
        out = (ctypes.c_uint64 * world)()
        self._ck(hip().tpc_shard_pack(self._h, which, send_regions_ptr, send_counts_ptr, packed_ptr, out))
        return [int(x) for x in out]

    def shard_apply_packed(self, which, batch, recv_packed_ptr, recv_counts_ptr):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_apply_packed(self._h, which, batch, recv_packed_ptr, recv_counts_ptr, ctypes.byref(n)))
        return n.value

    def shard_apply_inplace(self, which, batch, recv_regions_ptr, recv_counts_ptr, send_regions_ptr, send_counts_ptr):
        """tpc_shard_apply with this rank's own block read from the send buffers (the receive buffers' block `rank` is never read)."""
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_apply_inplace(self._h, which, batch, recv_regions_ptr, recv_counts_ptr, send_regions_ptr, send_counts_ptr, ctypes.byref(n)))
        return n.value

    def shard_survivors_home(self, tmp_ptr, send_ptr, world):
        """Survivors of the last shard_apply grouped by the rank that hashed them; returns the count for every rank."""
        out = (ctypes.c_uint64 * world)()
        self._ck(hip().tpc_shard_survivors_home(self._h, tmp_ptr, send_ptr, out))
        return [int(x) for x in out]

    def shard_verify_send(self, fn, fn_count, sid_ptr, n, tmp_ptr, send_ptr, perm_ptr, world):
        """Probe addresses of functions fn.. in owner-major send order (+ the slot of every probe); returns the count for every rank."""
        out = (ctypes.c_uint64 * world)()
        self._ck(hip().tpc_shard_verify_send(self._h, fn, fn_count, sid_ptr, n, tmp_ptr, send_ptr, perm_ptr, out))
        return [int(x) for x in out]

    def shard_finish(self, sid_ptr, n, fn_count, hit_ptr, perm_ptr):
        """Marks every survivor whose fn_count answers are all 1; returns how many."""
        m = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_finish(self._h, sid_ptr, n, fn_count, hit_ptr, perm_ptr, ctypes.byref(m)))
        return m.value

    def shard_periodic_copy(self):
        """After a round's last query batch on a context with option shard_periodic_skip: positions that sent no probes take their twin's verdict."""
        self._ck(hip().tpc_shard_periodic_copy(self._h))

    def periodic_download(self):
        """The periodic-window masks of this text and k (built now if they are not), one entry per position of the mask words:
        qs (bool: the position copies its verdict), dist (uint8: from how many positions back, 0 where qs is clear), ins (bool: its insert is dropped)."""
        nw = hip().tpc_mask_words(self._h)
        qs, planes, ins = np.zeros(nw, dtype=np.uint32), np.zeros((6, nw), dtype=np.uint32), np.zeros(nw, dtype=np.uint32)
        self._ck(hip().tpc_periodic_download(self._h, qs.ctypes.data, planes.ctypes.data, ins.ctypes.data))

        def bits(w):
            return np.unpackbits(w.astype("<u4").view(np.uint8), bitorder="little")

        dist = np.zeros(nw * 32, dtype=np.uint8)
        for b in range(6):
            dist |= bits(planes[b]) << b
        return bits(qs).astype(bool), dist, bits(ins).astype(bool)

    def shard_verify_local(self):
        """One rank: verifies and marks the survivors of the last shard_apply(QUERY) where they are."""
        self._ck(hip().tpc_shard_verify_local(self._h))

    def shard_survivors(self, sid_ptr):
        self._ck(hip().tpc_shard_survivors(self._h, sid_ptr))

    def shard_survivor_sources(self, sid_ptr, n, src_ptr):
        self._ck(hip().tpc_shard_survivor_sources(self._h, sid_ptr, n, src_ptr))

    def shard_verify_addrs(self, fn, fn_count, sid_ptr, n, addr_ptr, owner_ptr):
        self._ck(hip().tpc_shard_verify_addrs(self._h, fn, fn_count, sid_ptr, n, addr_ptr, owner_ptr))

    def shard_probe(self, addr_ptr, n, hit_ptr):
        self._ck(hip().tpc_shard_probe(self._h, addr_ptr, n, hit_ptr))

    def shard_mark(self, sid_ptr, n):
        self._ck(hip().tpc_shard_mark(self._h, sid_ptr, n))

    def mask_export(self, dst_ptr):
        self._ck(hip().tpc_mask_export(self._h, dst_ptr))

    def mask_merge(self, src_ptr, count):
        self._ck(hip().tpc_mask_merge(self._h, src_ptr, count))

    def mask_words(self):
        return int(hip().tpc_mask_words(self._h))

    def shard_route(self, owner_ptr, n, perm_ptr, world):
        counts = np.zeros(64, dtype=np.uint64)
        self._ck(hip().tpc_shard_route(self._h, owner_ptr, n, perm_ptr, counts.ctypes.data))
        return [int(x) for x in counts[:world]]

    def shard_permute64(self, src_ptr, perm_ptr, n, dst_ptr):
        self._ck(hip().tpc_shard_permute64(self._h, src_ptr, perm_ptr, n, dst_ptr))

    def shard_select(self, sid_ptr, n, fn_count, hit_ptr, perm_ptr, out_ptr):
        m = ctypes.c_uint64(0)
        self._ck(hip().tpc_shard_select(self._h, sid_ptr, n, fn_count, hit_ptr, perm_ptr, out_ptr, ctypes.byref(m)))
        return m.value

    def mask_export_padded(self, dst_ptr, total_words):
        self._ck(hip().tpc_mask_export_padded(self._h, dst_ptr, total_words))

    def mask_or_blocks(self, blocks_ptr, count, words, out_ptr):
        self._ck(hip().tpc_mask_or_blocks(self._h, blocks_ptr, count, words, out_ptr))

    def mask_import(self, src_ptr):
        self._ck(hip().tpc_mask_import(self._h, src_ptr))

    # ---- combined exchange: the filter replicated through set-bit lists (include/twopaco_hip.h: tpc_combine_*)
    def combine_info(self, n_dest):
        g = np.zeros(8, dtype=np.uint64)
        self._ck(hip().tpc_combine_info(self._h, n_dest, g.ctypes.data))
        names = ["sparse", "slices", "windows", "cap_units", "slice_bits", "b1", "b2", "dir_entries_per_dest"]
        return {n: int(g[i]) for i, n in enumerate(names)}

    def combine_export(self, n_dest, payload_ptr, cap_units, dir_ptr):
        out = (ctypes.c_uint64 * n_dest)()
        self._ck(hip().tpc_combine_export(self._h, n_dest, payload_ptr, cap_units, dir_ptr, out))
        return [int(x) for x in out]

    def combine_merge(self, n_src, payload_ptr, src_base, dir_ptr, out_payload_ptr, out_cap_units, out_dir_ptr):
        base = (ctypes.c_uint64 * n_src)(*[int(x) for x in src_base])
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_combine_merge(self._h, n_src, payload_ptr, base, dir_ptr, out_payload_ptr, out_cap_units, out_dir_ptr, ctypes.byref(n)))
        return n.value

    def combine_import(self, n_src, n_owner, payload_ptr, src_base, dir_ptr, dir_stride):
        base = (ctypes.c_uint64 * n_src)(*[int(x) for x in src_base])
        self._ck(hip().tpc_combine_import(self._h, n_src, n_owner, payload_ptr, base, dir_ptr, dir_stride))

    def filter_copy_out(self, word0, n_words, dst_ptr):
        self._ck(hip().tpc_filter_copy_out(self._h, word0, n_words, dst_ptr))

    def filter_copy_in(self, word0, n_words, src_ptr):
        self._ck(hip().tpc_filter_copy_in(self._h, word0, n_words, src_ptr))


class Enumerator:
    """TwoPaCo::CreateEnumerator through the C++ host layer (host/vertexenumerator.h)."""

    def __init__(self, files, k, filter_bits, q=5, rounds=1, threads=1, abundance=(1 << 64) - 1, tmpdir=".",
                 out=None, seed=None, device=0, test_first=False, gpus=1, rccl=True, emulate_ranks=False, force_sharded=False,
                 graph=None, graph_out=None, graph_prefix=False, graph_threads=16, colors=None, colors_out=None,
                 links=False, links_out=None, graph_compact=False, distances=None, distances_out=None, distances_phylip=None,
                 components=None, components_out=None, components_members=None):
        """out: the junction stream's file, default de_bruijn.bin.  graph = gfa1 | gfa2 | fasta: `twopaco --graph` -- the
        compacted graph's text goes to graph_out (default de_bruijn.<graph>) and the junction stream is written only when
        `out` is given.  colors = file | sequence: `twopaco --colors` -- the segment colour table goes to colors_out (default
        de_bruijn.colors.tsv); combines with graph and out.  links: `twopaco --links` -- the link table goes to links_out (default
        de_bruijn.links.tsv); graph_compact: `--graph-compact`, with graph = gfa1.  Both combine with graph, colors and out.
        distances = file | sequence: `twopaco --distances` -- the genome distance table goes to distances_out (default
        de_bruijn.distances.tsv) and, when distances_phylip names a file, the PHYLIP matrix goes there; combines with all of the above and
        with filter_bits = "auto".  components = file | sequence: `twopaco --components` -- the component table goes to components_out
        (default de_bruijn.components.tsv) and, when components_members names a file, the component of every segment goes there; combines
        with graph, colors, links, graph_compact and out, not with distances (use the program for both)."""
        arr = (ctypes.c_char_p * len(files))(*[f.encode() for f in files])
        log = ctypes.c_void_p()
        if distances is None and (distances_out is not None or distances_phylip is not None):
            raise ValueError("distances_out / distances_phylip: only with distances = file | sequence")
        if components is None and (components_out is not None or components_members is not None):
            raise ValueError("components_out / components_members: only with components = file | sequence")
        if components is not None:
            if gpus > 1 or force_sharded or filter_bits == "auto" or distances is not None:
                raise ValueError("components: one GPU, a given filter size, not with distances")
            if graph is not None:
                graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            elif out is None:
                out = "de_bruijn.bin"
            links_out = ("de_bruijn.links.tsv" if links_out is None else links_out) if links else None
            if colors is not None:
                colors_out = "de_bruijn.colors.tsv" if colors_out is None else colors_out
            components_out = "de_bruijn.components.tsv" if components_out is None else components_out
            self._h = host().tpch_create_enumerator_components(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                               b"" if out is None else out.encode(), 0 if seed is None else 1, 0 if seed is None else seed,
                                                               device, 1 if test_first else 0, None if graph is None else graph.encode(),
                                                               None if graph is None else os.fsencode(graph_out), 1 if graph_prefix else 0, graph_threads,
                                                               None if colors is None else colors.encode(), None if colors is None else os.fsencode(colors_out),
                                                               None if links_out is None else os.fsencode(links_out), 1 if graph_compact else 0,
                                                               components.encode(), os.fsencode(components_out),
                                                               None if components_members is None else os.fsencode(components_members), ctypes.byref(log))
        elif distances is not None:
            if gpus > 1 or force_sharded or (filter_bits == "auto" and test_first):
                raise ValueError("distances: one GPU; filter_bits='auto' with the plain insert")
            if graph is not None:
                graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            elif out is None:
                out = "de_bruijn.bin"
            links_out = ("de_bruijn.links.tsv" if links_out is None else links_out) if links else None
            if colors is not None:
                colors_out = "de_bruijn.colors.tsv" if colors_out is None else colors_out
            distances_out = "de_bruijn.distances.tsv" if distances_out is None else distances_out
            self._h = host().tpch_create_enumerator_distances(arr, len(files), k, 0 if filter_bits == "auto" else filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                              b"" if out is None else out.encode(), 0 if seed is None else 1, 0 if seed is None else seed,
                                                              device, 1 if test_first else 0, None if graph is None else graph.encode(),
                                                              None if graph is None else os.fsencode(graph_out), 1 if graph_prefix else 0, graph_threads,
                                                              None if colors is None else colors.encode(), None if colors is None else os.fsencode(colors_out),
                                                              None if links_out is None else os.fsencode(links_out), 1 if graph_compact else 0,
                                                              distances.encode(), os.fsencode(distances_out),
                                                              None if distances_phylip is None else os.fsencode(distances_phylip), 1 if filter_bits == "auto" else 0, ctypes.byref(log))
        elif links or graph_compact:
            if filter_bits == "auto" or gpus > 1 or force_sharded:
                raise ValueError("links / graph_compact: one GPU and a given filter size")
            if graph is not None:
                graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            elif out is None:
                out = "de_bruijn.bin"
            links_out = ("de_bruijn.links.tsv" if links_out is None else links_out) if links else None
            if colors is not None:
                colors_out = "de_bruijn.colors.tsv" if colors_out is None else colors_out
            self._h = host().tpch_create_enumerator_links(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                          b"" if out is None else out.encode(), 0 if seed is None else 1, 0 if seed is None else seed,
                                                          device, 1 if test_first else 0, None if graph is None else graph.encode(),
                                                          None if graph is None else os.fsencode(graph_out), 1 if graph_prefix else 0, graph_threads,
                                                          None if colors is None else colors.encode(), None if colors is None else os.fsencode(colors_out),
                                                          None if links_out is None else os.fsencode(links_out), 1 if graph_compact else 0, ctypes.byref(log))
        elif colors is not None:
            if filter_bits == "auto" or gpus > 1 or force_sharded:
                raise ValueError("colors: one GPU and a given filter size")
            if graph is not None:
                graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            elif out is None:
                out = "de_bruijn.bin"
            colors_out = "de_bruijn.colors.tsv" if colors_out is None else colors_out
            self._h = host().tpch_create_enumerator_colors(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                           b"" if out is None else out.encode(), 0 if seed is None else 1, 0 if seed is None else seed,
                                                           device, 1 if test_first else 0, None if graph is None else graph.encode(),
                                                           None if graph is None else os.fsencode(graph_out), 1 if graph_prefix else 0, graph_threads,
                                                           colors.encode(), os.fsencode(colors_out), ctypes.byref(log))
        elif filter_bits == "auto":  # EnumeratorOptions::autoFilterSize (`twopaco -f auto`); rounds = 0: the plan chooses them too
            if gpus > 1 or force_sharded or test_first:
                raise ValueError("filter_bits='auto': one GPU, plain insert")
            if graph is not None:
                graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            elif out is None:
                out = "de_bruijn.bin"
            self._h = host().tpch_create_enumerator_auto(arr, len(files), k, q, rounds, threads, abundance, tmpdir.encode(), b"" if out is None else out.encode(),
                                                         0 if seed is None else 1, 0 if seed is None else seed, device, None if graph is None else graph.encode(),
                                                         None if graph is None else os.fsencode(graph_out), ctypes.byref(log))
        elif graph is not None:
            if gpus > 1 or force_sharded:
                raise ValueError("graph: one GPU only (every rank of a sharded run holds its own piece of the junction stream)")
            graph_out = "de_bruijn." + graph if graph_out is None else graph_out
            self._h = host().tpch_create_enumerator_graph(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                          b"" if out is None else out.encode(), 0 if seed is None else 1, 0 if seed is None else seed,
                                                          device, 1 if test_first else 0, graph.encode(), os.fsencode(graph_out),
                                                          1 if graph_prefix else 0, graph_threads, ctypes.byref(log))
            out = ""
        out = "de_bruijn.bin" if out is None else out
        if graph is not None or filter_bits == "auto" or colors is not None or links or graph_compact or distances is not None or components is not None:
            pass
        elif gpus > 1 or force_sharded:  # host/multigpu.h: the filter sharded by bit address over `gpus` ranks
            self._h = host().tpch_create_enumerator_mgpu(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                         out.encode(), 0 if seed is None else 1, 0 if seed is None else seed, device,
                                                         gpus, 1 if rccl else 0, 1 if emulate_ranks else 0, 1 if force_sharded else 0, ctypes.byref(log))
        else:
            self._h = host().tpch_create_enumerator(arr, len(files), k, filter_bits, q, rounds, threads, abundance, tmpdir.encode(),
                                                    out.encode(), 0 if seed is None else 1, 0 if seed is None else seed, device,
                                                    1 if test_first else 0, ctypes.byref(log))
        self.log = ctypes.string_at(log.value).decode() if log.value else ""
        if log.value:
            host().tpch_free(log)
        if not self._h:
            raise RuntimeError(host().tpch_last_error().decode())
        self.k, self.q = k, q

    def close(self):
        if getattr(self, "_h", None):
            host().tpch_enumerator_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def vertices_count(self):
        return host().tpch_vertices_count(self._h)

    def key_words(self):
        return int(hip().tpc_key_words(self._h))

    def junction_keys_export(self, dst_ptr, cap_keys):
        n = ctypes.c_uint64(0)
        self._ck(hip().tpc_junction_keys_export(self._h, dst_ptr, cap_keys, ctypes.byref(n)))
        return n.value

    def junction_keys_import(self, src_ptr, n, append):
        self._ck(hip().tpc_junction_keys_import(self._h, src_ptr, n, 1 if append else 0))

    def get_id(self, kmer):
        return host().tpch_get_id(self._h, kmer.encode())

    def hash_seed(self):
        t = np.zeros((self.q, 5), dtype=np.uint64)
        host().tpch_hash_seed(self._h, t.ctypes.data)
        return t
