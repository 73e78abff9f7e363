"""ctypes binding of include/krepp_amd.h (the C ABI of the MI355X `krepp dist` path).

This module is plumbing only: it loads ``krepp_amd/lib/libkrepp_amd.so`` (built by
``__graft_entry__.build()`` / ``krepp_amd/csrc/Makefile``) and fails loudly if it is
missing.  There is no Python or CPU fallback for any device entry point.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libkrepp_amd.so"

KR_OK = 0
KR_ERR_ARG, KR_ERR_IO, KR_ERR_FORMAT, KR_ERR_NO_DEVICE = -1, -2, -3, -4
KR_ERR_NOMEM, KR_ERR_CAPACITY, KR_ERR_STATE, KR_ERR_UNSUPPORTED = -5, -6, -7, -8
KR_VIEW_HOST, KR_VIEW_DEVICE = 0, 1
KR_BASES_HOST, KR_BASES_DEVICE, KR_TAP_ACCS, KR_TAP_HITS, KR_BASES_PINNED, KR_ROWS_ONLY, KR_ROWS_INDEXED = 0, 1, 2, 4, 8, 16, 32
KR_TILE_DEVICE = 64  # with KR_BASES_DEVICE / submit_fastq: long sequences of a batch in HBM are tiled by kernels
KR_TILE_ROWS = 128  # with KR_ROWS_ONLY: a batch that ends up tiled leaves the device as compact rows (and as device text) too
KR_SEEK = 256  # the batch is a `seek` batch: seek kernels instead of the dist chain (sketch indexes only)

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)


class KrLibView(C.Structure):
    _fields_ = [("inc", u64p), ("cmer", u32p), ("pse", u32p), ("rho", f64p),
                ("nkmers", C.c_uint64), ("nrows", C.c_uint32), ("nsubsets", C.c_uint32),
                ("nnodes", C.c_uint32), ("r", C.c_uint32), ("frac", C.c_uint32), ("w", C.c_uint32)]


class KrIndexView(C.Structure):
    _fields_ = [("k", C.c_uint32), ("h", C.c_uint32), ("m", C.c_uint32),
                ("ppos", u8p), ("npos", u8p), ("nlibs", C.c_uint32), ("libs", C.POINTER(KrLibView)),
                ("tree_nnodes", C.c_uint32), ("node_kind", u8p), ("wbackbone", C.c_uint32)]


class KrIndexBuffer(C.Structure):
    _fields_ = [("dptr", C.c_void_p), ("bytes", C.c_uint64)]


class KrParams(C.Structure):
    _fields_ = [("hdist_th", C.c_uint32), ("tau", C.c_uint32), ("chisq", C.c_double),
                ("dist_max", C.c_double), ("multi", C.c_uint32), ("no_filter", C.c_uint32)]


class KrResultView(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("nrecs", C.c_uint32),
                ("read_off", u32p), ("read_cnt", u32p), ("read_onmers", u32p), ("read_na", u8p),
                ("rec_key", u32p), ("rec_sel", u8p), ("rec_d", f64p), ("rec_v", f64p),
                ("rec_chisq", f64p), ("rec_hist", u32p), ("rec_hist_stride", C.c_uint64), ("nrows", C.c_uint64),
                ("rec_dix", u32p), ("dist_list", f64p), ("ndist", C.c_uint64)]


class KrSeekView(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("np", C.c_uint32), ("d", C.POINTER(C.c_double)), ("d_strand", C.POINTER(C.c_double)),
                ("hist", u32p), ("onmers", u32p)]


KR_EXTRACT_MATCHED, KR_EXTRACT_UNMATCHED = 1, 2
KR_PAIR_ANY, KR_PAIR_BOTH = 1, 2


class KrExtractView(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("nmatched", C.c_uint32), ("matched_bytes", C.c_uint64), ("unmatched_bytes", C.c_uint64),
                ("matched", C.c_void_p), ("unmatched", C.c_void_p), ("matched_len", C.c_uint64), ("unmatched_len", C.c_uint64)]


class KrHit(C.Structure):
    _fields_ = [("read", C.c_uint32), ("kpos", C.c_uint32), ("strand", C.c_uint32), ("lib", C.c_uint32),
                ("cmer_index", C.c_uint64), ("hd", C.c_uint32), ("se", C.c_uint32)]


class KrTiming(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_scan", C.c_float), ("ms_acc", C.c_float), ("ms_llh", C.c_float),
                ("ms_h2d", C.c_float), ("overflow_reads", C.c_uint32), ("stack_spills", C.c_uint32), ("lanes", C.c_uint32)]


class KrFastxBatch(C.Structure):
    _fields_ = [("bases", u8p), ("offsets", u64p), ("names", C.POINTER(C.c_char_p)),
                ("nreads", C.c_uint32), ("more", C.c_uint32)]


KR_FASTQ_OK, KR_FASTQ_NOT_CLEAN, KR_FASTQ_INCOMPLETE, KR_FASTQ_LONG, KR_FASTQ_CAPACITY = 0, 1, 2, 3, 4


class KrFastqParse(C.Structure):
    _fields_ = [("consumed", C.c_uint64), ("nbases", C.c_uint64), ("id_bytes", C.c_uint64), ("newlines", C.c_uint64),
                ("nreads", C.c_uint32), ("status", C.c_uint32), ("rejected", C.c_uint32), ("at_eof", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class KrMinimizerResult(C.Structure):
    _fields_ = [("keys", u64p), ("nkeys", C.c_uint64), ("n1", C.c_double), ("n2", C.c_double)]


class KrBuildParams(C.Structure):
    _fields_ = [("k", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("m", C.c_uint32), ("r", C.c_uint32),
                ("frac", C.c_uint32), ("num_threads", C.c_uint32), ("seed", C.c_uint32), ("ppos", u8p),
                ("gpu_minimizers", C.c_uint32), ("device", C.c_int32), ("sdust_t", C.c_uint32), ("sdust_w", C.c_uint32)]


class KrKeyGroups(C.Structure):
    _fields_ = [("keys", u64p), ("goff", u64p), ("ranks", u32p), ("inc", u64p), ("nkeys", C.c_uint64), ("npairs", C.c_uint64),
                ("nrows", C.c_uint32)]


class KrLibStats(C.Structure):
    _fields_ = [("nkmers", C.c_uint64), ("nsubsets", C.c_uint32), ("r", C.c_uint32), ("frac", C.c_uint32),
                ("mer_value", u64p), ("mer_freq", u64p), ("n_mer", C.c_uint64), ("deg_value", u64p), ("deg_freq", u64p), ("n_deg", C.c_uint64),
                ("se_count", u64p), ("se_outdeg", u64p)]


class KrIndexStats(C.Structure):
    _fields_ = [("nlibs", C.c_uint32), ("libs", C.POINTER(KrLibStats))]


KR_STATS_KEEP_COUNTS = 4


class KrColourClasses(C.Structure):
    _fields_ = [("class_of", u32p), ("rep", u64p), ("nkeys", C.c_uint64), ("nclasses", C.c_uint64)]


class KrSdustResult(C.Structure):
    _fields_ = [("intervals", u64p), ("offsets", u64p), ("ncontigs", C.c_uint32)]


class KrSelectTables(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("nrecs", C.c_uint32), ("rd_off", u32p), ("rd_cnt", u32p), ("rd_onmers", u32p),
                ("rec_key", u32p), ("rec_rep", u32p), ("rec_w0", u64p), ("rec_hist", u32p), ("rec_read", u32p),
                ("nrep", C.c_uint32), ("ndirect", C.c_uint32), ("rep_dv", f64p), ("dd_direct", u32p), ("dd_dv", f64p),
                ("problems", C.c_uint32)]


class KrSelectResult(C.Structure):
    _fields_ = [("rd_na", u8p), ("rd_rcnt", u32p), ("rd_roff", u32p), ("rec_sel", u8p), ("rec_d", f64p), ("rec_v", f64p),
                ("rec_chisq", f64p), ("rec_rep", u32p), ("row_key", u32p), ("row_d", f64p), ("row_dix", u32p), ("dist_list", f64p),
                ("nrows", C.c_uint64), ("rows_mode", C.c_uint32), ("rows_indexed", C.c_uint32), ("keep_v", C.c_uint32)]


class KrDedupTables(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("nrecs", C.c_uint32), ("rd_off", u32p), ("rd_cnt", u32p), ("rd_onmers", u32p),
                ("rec_key", u32p), ("rec_w0", u64p), ("rec_hist", u32p), ("rec_read", u32p)]


class KrDedupResult(C.Structure):
    _fields_ = [("rec_rep", u32p), ("rep_list", u32p), ("rep_dv", f64p), ("dd_direct", u32p), ("dd_dv", f64p), ("dd_oslot", u8p),
                ("dd_table", u64p), ("rep_room", C.c_uint32), ("table_room", C.c_uint32), ("places_room", C.c_uint32), ("rep_n", C.c_uint32), ("table_n", C.c_uint32),
                ("problems", C.c_uint32), ("err", C.c_uint32), ("rep_cap", C.c_uint32), ("places", C.c_uint32), ("dd_nodes", C.c_uint32),
                ("mask", C.c_uint32), ("dd_slots", C.c_uint32), ("dd_shift", C.c_uint32)]


class KrGzipPoint(C.Structure):
    """kr_gzip_point: where an ordinary gzip stream can be taken up again"""
    _fields_ = [("bit", C.c_uint64), ("inflated_off", C.c_uint64), ("member_len", C.c_uint64), ("member_crc", C.c_uint32),
                ("window_len", C.c_uint32), ("window", C.c_uint8 * 32768)]


# every symbol include/krepp_amd.h declares (tests check that the library exports them all)
EXPORTS = [
    "kr_host_index_load", "kr_host_sketch_load", "kr_format_seek", "kr_build_sketch", "kr_host_index_free", "kr_host_index_view", "kr_host_index_node_name",
    "kr_host_index_node_label", "kr_host_index_node_parent", "kr_host_index_node_blen",
    "kr_index_upload", "kr_index_free", "kr_index_export", "kr_index_import", "kr_index_device_bytes", "kr_index_slot_words", "kr_index_slot_format", "kr_index_log_g", "kr_index_occ_bitmap", "kr_index_broadcast",
    "kr_params_default", "kr_stream_create", "kr_stream_destroy", "kr_batch_submit", "kr_batch_wait",
    "kr_batch_collect", "kr_batch_collect_device", "kr_stream_text_enable", "kr_batch_submit_text", "kr_batch_collect_text",
    "kr_stream_fastq_enable", "kr_batch_submit_fastq", "kr_batch_submit_fasta", "kr_fasta_chunk_cut", "kr_fastq_chunk_cut", "kr_batch_fastq_names", "kr_debug_fastq_batch", "kr_debug_fastq_parse_ms", "kr_debug_tile_layout", "kr_debug_tile_shape", "kr_batch_hits", "kr_batch_readtaps",
    "kr_debug_front_end", "kr_debug_stream_move", "kr_debug_stream_addrs", "kr_debug_item_placement", "kr_debug_brent", "kr_debug_prefix", "kr_debug_colour_classes", "kr_llh_batch", "kr_llh_eval_indexed", "kr_batch_timing",
    "kr_place_tree_create", "kr_place_tree_create_lineage", "kr_place_tree_nnodes", "kr_place_summary_add",
    "kr_place_summary_text", "kr_place_tree_free", "kr_place_tree_kinds", "kr_place_batch", "kr_place_stream", "kr_place_stream_parsed", "kr_debug_place_ids", "kr_place_frame", "kr_place_counters",
    "kr_debug_last_d2h_bytes", "kr_debug_indexed_list", "kr_debug_select", "kr_debug_select_check", "kr_debug_select_layout", "kr_debug_dedup", "kr_debug_dedup_check", "kr_debug_dedup_layout", "kr_debug_acc_paths", "kr_debug_acc_layout", "kr_debug_scan_layout", "kr_debug_scan_stream", "kr_debug_place_fixed5", "kr_place_text_counters", "kr_place_path_counters", "kr_debug_place_layout", "kr_debug_place_paths", "kr_fastx_open", "kr_fastx_open_at", "kr_fastx_next", "kr_fastx_detach", "kr_fastx_release", "kr_fastx_close", "kr_fastx_parallel_chunks", "kr_fastx_pgz_stats", "kr_format_dist", "kr_debug_fixed5", "kr_free", "kr_host_alloc", "kr_host_free",
    "kr_build_index", "kr_minimizers_cpu", "kr_minimizers_device", "kr_minimizers_free", "kr_last_error", "kr_version",
    "kr_sdust_cpu", "kr_sdust_free",
    "kr_key_groups_cpu", "kr_key_groups_device", "kr_key_groups_free", "kr_debug_build_keys",
    "kr_colour_classes_cpu", "kr_colour_classes_device", "kr_colour_classes_free", "kr_debug_build_colours",
    "kr_index_stats_cpu", "kr_index_stats_device", "kr_index_stats_free", "kr_host_index_lib_info", "kr_format_inspect", "kr_debug_index_stats",
    "kr_debug_index_stats_ms",
    "kr_stream_seek_enable", "kr_batch_collect_seek", "kr_debug_seek_layout", "kr_debug_seek_ms",
    "kr_stream_extract_enable", "kr_stream_extract_max", "kr_batch_collect_extract", "kr_batch_collect_extract_bgzf", "kr_debug_extract_ms",
    "kr_stream_extract_defer", "kr_batch_extract_pair", "kr_fastq_pair_cut",
    "kr_stream_bgzf_enable", "kr_batch_submit_bgzf", "kr_debug_bgzf_inflate", "kr_debug_bgzf_inflate_host", "kr_debug_bgzf_ms",
    "kr_bgzf_member_size", "kr_bgzf_walk", "kr_bgzf_chunk_cut", "kr_fastx_open_at_bgzf",
    "kr_bgzf_deflate_bound", "kr_bgzf_deflate_host", "kr_bgzf_eof", "kr_debug_bgzf_deflate_stats",
    "kr_stream_bgzf_out_enable", "kr_batch_collect_text_bgzf", "kr_debug_bgzf_deflate", "kr_debug_bgzf_deflate_ms",
    "kr_bgzf_deflate_host_level", "kr_stream_bgzf_out_level", "kr_debug_bgzf_deflate_stats_level", "kr_debug_huffman_lengths",
    "kr_debug_huffman_lengths_device",
    "kr_bgzf_deflate_bound_member", "kr_bgzf_deflate_host_member", "kr_stream_bgzf_member", "kr_debug_bgzf_deflate_at",
    "kr_stream_place_bgzf", "kr_place_bgzf_counters",
    "kr_gzdev_open", "kr_gzdev_close", "kr_gzdev_read", "kr_gzdev_point", "kr_gzdev_counters", "kr_fastx_open_at_gzip",
    "kr_debug_gzdev_inflate", "kr_debug_gzdev_inflate_host", "kr_debug_gzdev_point_host",
]

# kr_debug_acc_paths: the accumulate kernel's path witnesses, in the order of CounterSlot (kr_dev_common.inc)
ACC_PATHS = ("fast_entered", "fast_false_early", "fast_compact", "fast_false_compacted", "fast_big_read", "fast_one_batch", "fast_multi_batch",
             "fast_extra_batches", "fix_dup_calls", "fix_dup_moved", "gen_entered_1", "gen_entered_2", "gen_entered_merge", "gen_fused", "gen_sparse",
             "gen_big", "gen_extra_batches", "gen_keytab_global", "gen_no_fit", "set_aside", "plane_redo")

_lib = None


class KrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"krepp_amd error {code}: {msg}")
        self.code = code


def load():
    """Load libkrepp_amd.so; raise if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP extension is required; there is no CPU fallback)")
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    lib.kr_last_error.restype = C.c_char_p
    lib.kr_version.restype = C.c_char_p
    lib.kr_host_index_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.kr_host_index_free.argtypes = [vp]
    lib.kr_host_index_free.restype = None
    lib.kr_host_index_view.argtypes = [vp, C.POINTER(KrIndexView)]
    lib.kr_host_index_node_name.argtypes = [vp, C.c_uint32]
    lib.kr_host_index_node_name.restype = C.c_char_p
    lib.kr_host_index_node_label.argtypes = [vp, C.c_uint32]
    lib.kr_host_index_node_label.restype = C.c_char_p
    lib.kr_host_index_node_parent.argtypes = [vp, C.c_uint32]
    lib.kr_host_index_node_parent.restype = C.c_uint32
    lib.kr_host_index_node_blen.argtypes = [vp, C.c_uint32]
    lib.kr_host_index_node_blen.restype = C.c_double
    lib.kr_index_upload.argtypes = [C.POINTER(KrIndexView), C.c_int, C.c_uint32, C.POINTER(vp)]
    lib.kr_index_free.argtypes = [vp]
    lib.kr_index_free.restype = None
    lib.kr_index_export.argtypes = [vp, vp, u64p, C.POINTER(KrIndexBuffer), u32p]
    lib.kr_index_import.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(KrIndexBuffer), u32p]
    lib.kr_index_device_bytes.argtypes = [vp]
    lib.kr_index_broadcast.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
    lib.kr_index_device_bytes.restype = C.c_uint64
    lib.kr_index_slot_words.argtypes = [vp]
    lib.kr_index_slot_format.argtypes = [vp]
    lib.kr_index_slot_format.restype = C.c_uint32
    lib.kr_index_log_g.argtypes = [vp]
    lib.kr_index_log_g.restype = C.c_uint32
    lib.kr_index_occ_bitmap.argtypes = [vp]
    lib.kr_index_occ_bitmap.restype = C.c_uint32
    lib.kr_debug_scan_layout.argtypes = [C.c_uint32, C.c_uint32, u32p]
    lib.kr_debug_scan_stream.argtypes = [vp, u32p]
    lib.kr_debug_stream_move.argtypes = [vp, C.c_int]
    lib.kr_debug_stream_addrs.argtypes = [vp, u64p]
    lib.kr_debug_item_placement.argtypes = [vp, u32p, u32p, C.POINTER(C.c_double)]
    lib.kr_debug_acc_paths.argtypes = [vp, u32p, C.c_uint32]
    lib.kr_debug_select.argtypes = [vp, C.POINTER(KrSelectTables), C.c_uint32, C.c_uint32, C.POINTER(KrSelectResult)]
    lib.kr_debug_select_check.argtypes = [C.POINTER(KrSelectTables), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.kr_debug_select_layout.argtypes = [u32p]
    lib.kr_debug_dedup.argtypes = [vp, C.POINTER(KrDedupTables), C.POINTER(KrDedupResult)]
    lib.kr_debug_dedup_check.argtypes = [C.POINTER(KrDedupTables), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.kr_debug_dedup_layout.argtypes = [u32p]
    lib.kr_debug_acc_layout.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    lib.kr_index_slot_words.restype = C.c_uint32
    lib.kr_params_default.argtypes = [C.POINTER(KrParams)]
    lib.kr_params_default.restype = None
    lib.kr_stream_create.argtypes = [vp, C.POINTER(KrParams), C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(vp)]
    lib.kr_stream_destroy.argtypes = [vp]
    lib.kr_stream_destroy.restype = None
    lib.kr_batch_submit.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32]
    lib.kr_debug_fixed5.argtypes = [C.c_double, C.c_char_p]
    lib.kr_debug_fixed5.restype = C.c_uint32
    lib.kr_stream_text_enable.argtypes = [vp, vp, C.c_uint64, C.c_uint64]
    lib.kr_batch_submit_text.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32]
    lib.kr_batch_collect_text.argtypes = [vp, C.POINTER(vp), u64p]
    lib.kr_batch_wait.argtypes = [vp]
    lib.kr_batch_collect.argtypes = [vp, C.POINTER(KrResultView)]
    lib.kr_batch_collect_device.argtypes = [vp, C.POINTER(KrResultView)]
    lib.kr_batch_hits.argtypes = [vp, C.POINTER(C.POINTER(KrHit)), u64p]
    lib.kr_batch_readtaps.argtypes = [vp, C.POINTER(u32p)]
    lib.kr_debug_front_end.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    lib.kr_debug_brent.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    lib.kr_debug_prefix.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64p]
    lib.kr_debug_colour_classes.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint64)]
    lib.kr_batch_timing.argtypes = [vp, C.POINTER(KrTiming)]
    lib.kr_llh_batch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp]
    lib.kr_place_tree_create.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.kr_place_tree_create_lineage.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    lib.kr_place_tree_nnodes.argtypes = [vp]
    lib.kr_place_tree_nnodes.restype = C.c_uint32
    lib.kr_place_summary_add.argtypes = [vp, vp, C.c_uint64, vp, C.POINTER(C.c_double)]
    lib.kr_place_summary_text.argtypes = [vp, vp, C.c_double, C.POINTER(vp), u64p]
    lib.kr_place_tree_free.argtypes = [vp]
    lib.kr_place_tree_free.restype = None
    lib.kr_place_tree_kinds.argtypes = [vp]
    lib.kr_place_tree_kinds.restype = u8p
    lib.kr_place_batch.argtypes = [vp, vp, vp, C.POINTER(KrResultView), vp, C.POINTER(C.c_char_p), C.POINTER(KrParams), C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    lib.kr_place_stream.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, C.POINTER(C.c_char_p), C.POINTER(KrParams), C.c_int,
                                    C.POINTER(C.c_int), C.POINTER(vp), u64p, C.POINTER(vp), u64p]
    lib.kr_place_stream_parsed.argtypes = [vp, vp, vp, vp, vp, C.POINTER(KrParams), C.c_int, C.POINTER(C.c_int), C.POINTER(vp), u64p,
                                           C.POINTER(vp), u64p]
    lib.kr_debug_place_ids.argtypes = [vp, vp, vp]
    lib.kr_place_frame.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.POINTER(vp), u64p]
    lib.kr_place_counters.argtypes = [u64p, u64p, u64p]
    lib.kr_place_counters.restype = None
    lib.kr_fastx_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.kr_fastx_open_at.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(vp)]
    lib.kr_stream_fastq_enable.argtypes = [vp, C.c_uint64]
    lib.kr_batch_submit_fastq.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(KrFastqParse)]
    lib.kr_batch_submit_fasta.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(KrFastqParse)]
    lib.kr_fasta_chunk_cut.argtypes = [vp, C.c_uint64]
    lib.kr_fasta_chunk_cut.restype = C.c_uint64
    lib.kr_fastq_chunk_cut.argtypes = [vp, C.c_uint64]
    lib.kr_fastq_chunk_cut.restype = C.c_uint64
    lib.kr_batch_fastq_names.argtypes = [vp, C.POINTER(u64p), C.POINTER(u32p)]
    lib.kr_debug_fastq_batch.argtypes = [vp, vp, vp]
    lib.kr_debug_fastq_parse_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.kr_stream_bgzf_enable.argtypes = [vp, C.c_uint64]
    lib.kr_batch_submit_bgzf.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(KrFastqParse)]
    lib.kr_debug_bgzf_inflate.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_debug_bgzf_inflate_host.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_debug_bgzf_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.kr_bgzf_member_size.argtypes = [vp, C.c_uint64]
    lib.kr_bgzf_member_size.restype = C.c_uint32
    lib.kr_bgzf_walk.argtypes = [vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.kr_bgzf_chunk_cut.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.kr_bgzf_chunk_cut.restype = C.c_uint64
    lib.kr_fastx_open_at_bgzf.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(vp)]
    lib.kr_gzdev_open.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    lib.kr_gzdev_close.argtypes = [vp]
    lib.kr_gzdev_close.restype = None
    lib.kr_gzdev_read.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_gzdev_point.argtypes = [vp, C.c_uint64, C.POINTER(KrGzipPoint)]
    lib.kr_gzdev_counters.argtypes = [vp, u64p]
    lib.kr_fastx_open_at_gzip.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(KrGzipPoint), C.POINTER(vp)]
    _gz_tabs = [C.c_uint64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64), u64p]
    lib.kr_debug_gzdev_inflate.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)] + _gz_tabs
    lib.kr_debug_gzdev_inflate_host.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)] + _gz_tabs
    lib.kr_debug_gzdev_point_host.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(KrGzipPoint)]
    lib.kr_bgzf_deflate_bound.argtypes = [C.c_uint64]
    lib.kr_bgzf_deflate_bound.restype = C.c_uint64
    lib.kr_bgzf_deflate_host.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_bgzf_eof.argtypes = [vp]
    lib.kr_bgzf_eof.restype = None
    lib.kr_debug_bgzf_deflate_stats.argtypes = [vp, C.c_uint64, u64p]
    lib.kr_stream_bgzf_out_enable.argtypes = [vp]
    lib.kr_batch_collect_text_bgzf.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.kr_debug_bgzf_deflate.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_debug_bgzf_deflate_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.kr_bgzf_deflate_host_level.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_stream_bgzf_out_level.argtypes = [vp, C.c_uint32]
    lib.kr_debug_bgzf_deflate_stats_level.argtypes = [vp, C.c_uint64, C.c_uint32, u64p]
    lib.kr_bgzf_deflate_bound_member.argtypes = [C.c_uint64, C.c_uint32]
    lib.kr_bgzf_deflate_bound_member.restype = C.c_uint64
    lib.kr_bgzf_deflate_host_member.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_stream_bgzf_member.argtypes = [vp, C.c_uint32]
    lib.kr_debug_bgzf_deflate_at.argtypes = [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.kr_stream_place_bgzf.argtypes = [vp, C.c_uint32]
    lib.kr_place_bgzf_counters.argtypes = [u64p, u64p]
    lib.kr_place_bgzf_counters.restype = None
    lib.kr_debug_huffman_lengths.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    lib.kr_debug_huffman_lengths_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_uint32)]
    lib.kr_debug_tile_layout.argtypes = [vp, u32p, u32p, vp, vp, vp, vp, vp]
    lib.kr_stream_seek_enable.argtypes = [vp, C.c_uint64, C.c_uint64]
    lib.kr_batch_collect_seek.argtypes = [vp, C.POINTER(KrSeekView)]
    lib.kr_debug_seek_layout.argtypes = [u32p]
    lib.kr_debug_seek_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.kr_stream_extract_enable.argtypes = [vp, C.c_double]
    lib.kr_stream_extract_max.argtypes = [vp, C.c_double]
    lib.kr_batch_collect_extract.argtypes = [vp, C.c_uint32, C.POINTER(KrExtractView)]
    lib.kr_batch_collect_extract_bgzf.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(KrExtractView)]
    lib.kr_debug_extract_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.kr_stream_extract_defer.argtypes = [vp, C.c_uint32]
    lib.kr_batch_extract_pair.argtypes = [vp, vp, C.c_uint32]
    lib.kr_fastq_pair_cut.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.kr_debug_tile_shape.argtypes = [C.c_uint64, C.c_uint32, u64p, u64p, u64p]
    lib.kr_fastx_next.argtypes = [vp, C.c_uint64, C.POINTER(KrFastxBatch)]
    lib.kr_fastx_detach.argtypes = [vp, C.POINTER(vp)]
    lib.kr_fastx_release.argtypes = [vp, vp]
    lib.kr_fastx_release.restype = None
    lib.kr_fastx_close.argtypes = [vp]
    lib.kr_fastx_close.restype = None
    lib.kr_format_dist.argtypes = [vp, C.POINTER(KrResultView), C.POINTER(C.c_char_p), C.POINTER(vp), u64p]
    lib.kr_free.argtypes = [vp]
    lib.kr_free.restype = None
    lib.kr_host_alloc.argtypes = [C.c_uint64]
    lib.kr_host_alloc.restype = vp
    lib.kr_host_free.argtypes = [vp]
    lib.kr_host_free.restype = None
    lib.kr_build_index.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(KrBuildParams)]
    lib.kr_minimizers_cpu.argtypes = [C.POINTER(KrBuildParams), vp, vp, C.c_uint32, C.POINTER(KrMinimizerResult)]
    lib.kr_minimizers_device.argtypes = [C.c_int, C.POINTER(KrBuildParams), vp, vp, C.c_uint32, C.POINTER(KrMinimizerResult)]
    lib.kr_minimizers_free.argtypes = [C.POINTER(KrMinimizerResult)]
    lib.kr_minimizers_free.restype = None
    _lib = lib
    return lib


def check(rc):
    if rc != KR_OK:
        raise KrError(rc, load().kr_last_error().decode(errors="replace"))


def _np(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).view(dtype).copy()


class HostIndex:
    """Index directory read into host memory (reference: TargetIndex::load_index, src/krepp.cpp:66-108)."""

    def __init__(self, index_dir, sketch=False):
        """sketch=True: `index_dir` is a `krepp sketch` file (kr_host_sketch_load), served as a one-leaf index"""
        self.lib = load()
        self.h = C.c_void_p()
        if sketch:
            self.lib.kr_host_sketch_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
            check(self.lib.kr_host_sketch_load(os.fsencode(str(index_dir)), C.byref(self.h)))
        else:
            check(self.lib.kr_host_index_load(os.fsencode(str(index_dir)), C.byref(self.h)))
        self.view = KrIndexView()
        check(self.lib.kr_host_index_view(self.h, C.byref(self.view)))

    k = property(lambda s: s.view.k)
    hh = property(lambda s: s.view.h)
    m = property(lambda s: s.view.m)
    nnodes = property(lambda s: s.view.tree_nnodes)

    def name(self, se):
        return self.lib.kr_host_index_node_name(self.h, int(se)).decode()

    def parent(self, se):
        return int(self.lib.kr_host_index_node_parent(self.h, int(se)))

    def blen(self, se):
        return float(self.lib.kr_host_index_node_blen(self.h, int(se)))

    def kinds(self):
        return _np(self.view.node_kind, self.view.tree_nnodes + 1, np.uint8)

    def positions(self):
        return _np(self.view.ppos, self.view.h, np.uint8), _np(self.view.npos, self.view.k - self.view.h, np.uint8)

    def lib_arrays(self, i=0):
        lv = self.view.libs[i]
        return dict(inc=_np(lv.inc, lv.nrows, np.uint64), cmer=_np(lv.cmer, 2 * lv.nkmers, np.uint32).reshape(-1, 2),
                    pse=_np(lv.pse, 2 * lv.nsubsets, np.uint32).reshape(-1, 2), rho=_np(lv.rho, lv.nnodes, np.float64),
                    r=lv.r, frac=lv.frac, w=lv.w, nnodes=lv.nnodes, nsubsets=lv.nsubsets)

    def upload(self, device=0):
        return DeviceIndex.from_view(self.view, device, KR_VIEW_HOST, keep=self)

    def close(self):
        if self.h:
            self.lib.kr_host_index_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_params(**kw):
    p = KrParams()
    load().kr_params_default(C.byref(p))
    for k_, v in kw.items():
        setattr(p, k_, v)
    return p


class DeviceIndex:
    """Index resident in one GPU's HBM (the read-only state IBatch borrows from Index)."""

    def __init__(self, handle, keep=None):
        self.lib = load()
        self.h = handle
        self._keep = keep

    @classmethod
    def from_view(cls, view, device=0, flags=KR_VIEW_HOST, keep=None):
        lib = load()
        h = C.c_void_p()
        check(lib.kr_index_upload(C.byref(view), int(device), int(flags), C.byref(h)))
        return cls(h, keep)

    def export(self):
        """(descriptor bytes, [(device pointer, bytes), ...]) of the flat buffers, for replication."""
        nb = C.c_uint64(0)
        n = C.c_uint32(0)
        check(self.lib.kr_index_export(self.h, None, C.byref(nb), None, C.byref(n)))
        desc = C.create_string_buffer(nb.value)
        bufs = (KrIndexBuffer * n.value)()
        check(self.lib.kr_index_export(self.h, desc, C.byref(nb), bufs, C.byref(n)))
        return desc.raw, [(b.dptr, b.bytes) for b in bufs]

    @classmethod
    def import_empty(cls, desc, device=0):
        """Allocate the buffers described by `desc` on `device`; the caller fills them."""
        lib = load()
        h = C.c_void_p()
        n = C.c_uint32(256)
        bufs = (KrIndexBuffer * 256)()
        check(lib.kr_index_import(desc, len(desc), int(device), C.byref(h), bufs, C.byref(n)))
        return cls(h), [(bufs[i].dptr, bufs[i].bytes) for i in range(n.value)]

    def broadcast(self, devices):
        """Replicas of this index on `devices`, filled by RCCL broadcast (kr_index_broadcast)."""
        n = len(devices)
        devs = (C.c_int * n)(*[int(d) for d in devices])
        outs = (C.c_void_p * n)()
        check(self.lib.kr_index_broadcast(self.h, n, devs, outs))
        return [DeviceIndex(C.c_void_p(outs[i])) for i in range(n)]

    @property
    def device_bytes(self):
        return int(self.lib.kr_index_device_bytes(self.h))

    @property
    def slot_words(self):
        return int(self.lib.kr_index_slot_words(self.h))

    @property
    def slot_format(self):
        return int(self.lib.kr_index_slot_format(self.h))

    @property
    def log_g(self):
        return int(self.lib.kr_index_log_g(self.h))

    @property
    def occ_bitmap(self):
        return bool(self.lib.kr_index_occ_bitmap(self.h))

    def stream(self, params=None, max_reads=1 << 16, max_bases=None, max_records=0):
        return Stream(self, params or default_params(), max_reads, max_bases or max_reads * 160, max_records)

    def front_end(self, bases, offsets, stride):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        rix = np.zeros((n, stride, 2), np.uint32)
        enc = np.zeros((n, stride, 2), np.uint32)
        valid = np.zeros((n, stride, 2), np.uint8)
        pas = np.zeros((n, stride, 2), np.uint8)
        check(self.lib.kr_debug_front_end(self.h, bases.ctypes.data, offsets.ctypes.data, n, stride,
                                          rix.ctypes.data, enc.ctypes.data, valid.ctypes.data, pas.ctypes.data))
        return rix, enc, valid, pas

    def brent(self, th, hist, onmers, rho):
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        onmers = np.ascontiguousarray(onmers, dtype=np.uint32)
        rho = np.ascontiguousarray(rho, dtype=np.float64)
        n = len(onmers)
        d = np.zeros(n)
        v = np.zeros(n)
        check(self.lib.kr_debug_brent(self.h, th, n, hist.ctypes.data, onmers.ctypes.data, rho.ctypes.data,
                                      d.ctypes.data, v.ctypes.data))
        return d, v

    def close(self):
        if self.h:
            self.lib.kr_index_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Result:
    """Host copy of one batch's results (see kr_result_view)."""

    def __init__(self, rv, np_planes, copy_hist):
        n, c = rv.nreads, rv.nrecs
        self.nreads, self.nrecs, self.nrows = n, c, int(rv.nrows)
        self.read_off = _np(rv.read_off, n, np.uint32)
        self.read_cnt = _np(rv.read_cnt, n, np.uint32)
        self.read_onmers = _np(rv.read_onmers, n, np.uint32)
        self.read_na = _np(rv.read_na, n, np.uint8)
        key = _np(rv.rec_key, c, np.uint32)
        keep = key != 0  # record slots are handed out in per-wave chunks; key 0 marks an unused slot
        self.rec_key = key[keep]
        self.rec_sel = _np(rv.rec_sel, c, np.uint8)[keep]
        if rv.rec_dix:  # KR_ROWS_INDEXED: DIST as an index into the batch's distinct values
            self.rec_dix = _np(rv.rec_dix, c, np.uint32)[keep]
            self.dist_list = _np(rv.dist_list, int(rv.ndist), np.float64)
            self.rec_d = self.dist_list[self.rec_dix]
        else:
            self.rec_dix = None
            self.rec_d = _np(rv.rec_d, c, np.float64)[keep]
        self.rec_v = _np(rv.rec_v, c, np.float64)[keep] if rv.rec_v else None       # NULL with KR_ROWS_ONLY
        self.rec_chisq = _np(rv.rec_chisq, c, np.float64)[keep] if rv.rec_chisq else None
        self.rec_hist = (_np(rv.rec_hist, c * np_planes, np.uint32).reshape(np_planes, -1).T[keep]
                         if copy_hist and rv.rec_hist and c else (np.zeros((0, np_planes), np.uint32) if copy_hist else None))
        # read index of every record, and offsets into the compacted arrays
        # (vectorised: a record belongs to the read whose first record is the last start at or before it)
        rr = np.zeros(c, np.uint32)
        nzr = np.nonzero(self.read_cnt)[0]
        if c and len(nzr):
            start = np.zeros(c, np.int64)
            start[self.read_off[nzr]] = self.read_off[nzr].astype(np.int64) + 1
            at = np.zeros(c + 1, np.uint32)
            at[self.read_off[nzr].astype(np.int64) + 1] = nzr
            rr = at[np.maximum.accumulate(start)]
        self.rec_read = rr[keep]
        newpos = np.cumsum(keep) - 1
        nz = self.read_cnt > 0
        self.read_off = np.where(nz, newpos[np.minimum(self.read_off, max(c - 1, 0))] if c else 0, 0).astype(np.uint32)
        self.nrecs = int(keep.sum())

    def rows(self):
        """Sorted list of (read, se, d) output rows — `krepp dist` rows as a set."""
        sel = self.rec_sel.astype(bool)
        return sorted(zip(self.rec_read[sel].tolist(), (self.rec_key[sel] >> 1).tolist(), self.rec_d[sel].tolist()))


class Stream:
    def __init__(self, dindex, params, max_reads, max_bases, max_records=0):
        self.lib = load()
        self.ix = dindex
        self.params = params
        self.h = C.c_void_p()
        check(self.lib.kr_stream_create(dindex.h, C.byref(params), int(max_reads), int(max_bases), int(max_records), C.byref(self.h)))
        self._keep = None
        self._flags = 0

    def submit(self, bases, offsets, flags=0):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._keep = (bases, offsets)
        self._flags = flags
        check(self.lib.kr_batch_submit(self.h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, flags))

    def submit_device(self, bases_ptr, offsets_ptr, nreads, flags=0):
        self._flags = flags | KR_BASES_DEVICE
        check(self.lib.kr_batch_submit(self.h, int(bases_ptr), int(offsets_ptr), int(nreads), self._flags))

    def wait(self):
        check(self.lib.kr_batch_wait(self.h))

    def collect(self):
        rv = KrResultView()
        check(self.lib.kr_batch_collect(self.h, C.byref(rv)))
        self._rv = rv
        return Result(rv, self.params.hdist_th + 1, bool(self._flags & KR_TAP_ACCS))

    def collect_view(self):
        """kr_batch_collect without building numpy copies: the raw result view (pointers into the stream's pinned buffers)."""
        rv = KrResultView()
        check(self.lib.kr_batch_collect(self.h, C.byref(rv)))
        self._rv = rv
        return rv

    def last_d2h_bytes(self):
        b = C.c_uint64(0)
        self.lib.kr_debug_last_d2h_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        check(self.lib.kr_debug_last_d2h_bytes(self.h, C.byref(b)))
        return int(b.value)

    def indexed_list(self):
        """(tests) kr_debug_indexed_list: (list positions the last KR_ROWS_INDEXED launch handed out, batches run again without the hint)"""
        e, f = C.c_uint64(0), C.c_uint64(0)
        self.lib.kr_debug_indexed_list.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        check(self.lib.kr_debug_indexed_list(self.h, C.byref(e), C.byref(f)))
        return int(e.value), int(f.value)

    def acc_paths(self):
        """(tests) kr_debug_acc_paths: {name: count} of the accumulate kernel's path witnesses for the batch last waited for (a stream
        created under KR_DEBUG_SKIP=512)"""
        a = (C.c_uint32 * len(ACC_PATHS))()
        check(self.lib.kr_debug_acc_paths(self.h, a, len(ACC_PATHS)))
        return dict(zip(ACC_PATHS, [int(x) for x in a]))

    def acc_layout(self, segs=1, multi=0):
        return acc_layout(self.params.hdist_th + 1, segs, multi, self)

    def debug_select(self, tables, flags=0, form=0):
        """(tests) kr_debug_select: crafted records (a dict as select_tables takes it) through the select and row kernels of this idle
        one-lane stream; what they wrote, as a dict of numpy arrays (record arrays as the select kernel left them, rows as the row
        kernels did), with nrows and the lane's rows_mode / rows_indexed / keep_v"""
        t, keep = select_tables(tables)
        nreads, nrecs, nprob = t.nreads, t.nrecs, t.problems
        shapes = dict(rd_na=(np.uint8, nreads), rd_rcnt=(np.uint32, nreads), rd_roff=(np.uint32, nreads), rec_sel=(np.uint8, nrecs),
                      rec_d=(np.float64, nrecs), rec_v=(np.float64, nrecs), rec_chisq=(np.float64, nrecs), rec_rep=(np.uint32, nrecs),
                      row_key=(np.uint32, nrecs), row_d=(np.float64, nrecs), row_dix=(np.uint32, nrecs), dist_list=(np.float64, nprob))
        out = {k: np.full(n * np.dtype(dt).itemsize, 0x5A, np.uint8).view(dt) for k, (dt, n) in shapes.items()}  # (0x5A: not copied back)
        r = KrSelectResult()
        for k, a in out.items():
            setattr(r, k, a.ctypes.data_as(dict(KrSelectResult._fields_)[k]) if a.size else None)
        check(self.lib.kr_debug_select(self.h, C.byref(t), int(flags), int(form), C.byref(r)))
        out.update(nrows=int(r.nrows), rows_mode=int(r.rows_mode), rows_indexed=int(r.rows_indexed), keep_v=int(r.keep_v))
        return out

    def debug_dedup(self, tables, places=0, rep_room=None, table_room=None):
        """(tests) kr_debug_dedup: crafted records (a dict as dedup_tables takes it) through the likelihood de-duplication and the
        minimisations of this idle one-lane stream; what they wrote, as a dict of numpy arrays and the numbers of kr_dedup_result.
        places: the direct places the caller expects (dd_direct / dd_dv hold that many; the stream's own count comes back as
        "places"); rep_list / rep_dv: the first rep_room entries, by default room for every record, a largest chunk per wave and 4,160
        more, so that the poison behind the list shows; dd_table: [slots, 2], by default every slot a batch of this size can use"""
        t, keep = dedup_tables(tables)
        nrecs = t.nrecs
        lay = dedup_layout()
        if rep_room is None:
            rep_room = nrecs + lay["rep_chunk_max"] * ((nrecs + 63) // 64) + 4096 + 64
        if table_room is None:
            table_room = lay["min_slots"]
            while table_room < nrecs:
                table_room *= 2
        r = KrDedupResult()
        r.rep_room, r.table_room, r.places_room = int(rep_room), int(table_room), int(places)
        out = dict(rec_rep=np.full(nrecs, 0x5A5A5A5A, np.uint32), rep_list=np.full(rep_room, 0x5A5A5A5A, np.uint32),  # (0x5A: not copied back)
                   rep_dv=np.full((rep_room, 2), np.nan), dd_direct=np.full(places, 0x5A5A5A5A, np.uint32), dd_dv=np.full((places, 2), np.nan),
                   dd_oslot=np.full(256, 0x5A, np.uint8), dd_table=np.full((table_room, 2), 0x5A5A5A5A5A5A5A5A, np.uint64))
        for k, a in out.items():
            setattr(r, k, a.ctypes.data_as(dict(KrDedupResult._fields_)[k]) if a.size else None)
        check(self.lib.kr_debug_dedup(self.h, C.byref(t), C.byref(r)))
        out["rep_list"], out["rep_dv"], out["dd_table"] = out["rep_list"][:r.rep_n], out["rep_dv"][:r.rep_n], out["dd_table"][:r.table_n]
        for k in ("problems", "err", "rep_cap", "places", "dd_nodes", "mask", "dd_slots", "dd_shift"):
            out[k] = int(getattr(r, k))
        return out

    def scan_info(self):
        """(tests) kr_debug_scan_stream: which scan kernel this stream launches, the item slots a lane's scan may use, and the item
        slots the batch last waited for asked for"""
        a = (C.c_uint32 * 4)()
        check(self.lib.kr_debug_scan_stream(self.h, a))
        return dict(pipe=bool(a[0]), filt=bool(a[1]), item_cap=int(a[2]), item_slots=int(a[3]))

    def collect_device(self):
        rv = KrResultView()
        check(self.lib.kr_batch_collect_device(self.h, C.byref(rv)))
        return rv

    def hits(self):
        p = C.POINTER(KrHit)()
        n = C.c_uint64()
        check(self.lib.kr_batch_hits(self.h, C.byref(p), C.byref(n)))
        dt = np.dtype([("read", "<u4"), ("kpos", "<u4"), ("strand", "<u4"), ("lib", "<u4"), ("cmer_index", "<u8"),
                       ("hd", "<u4"), ("se", "<u4")])
        if n.value == 0:
            return np.zeros(0, dt)
        raw = C.string_at(p, n.value * C.sizeof(KrHit))
        return np.frombuffer(raw, dtype=dt).copy()

    def readtaps(self, nreads):
        p = u32p()
        check(self.lib.kr_batch_readtaps(self.h, C.byref(p)))
        return _np(p, 2 * nreads, np.uint32).reshape(-1, 2)

    def debug_move(self, which):
        """experiments: one group of the stream's device buffers at a new address (kr_debug_stream_move)"""
        check(self.lib.kr_debug_stream_move(self.h, which))

    def item_placement(self):
        """(allocations of the item list tried, how many replaced the one before, scan ns per read on the one kept)"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_double(0)
        check(self.lib.kr_debug_item_placement(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"tried": a.value, "kept": b.value, "scan_ns_per_read": c.value}

    def debug_addrs(self):
        a = (C.c_uint64 * 8)()
        check(self.lib.kr_debug_stream_addrs(self.h, a))
        return dict(zip(("items", "counters", "cursors", "rd_off", "rd_it_off", "rd_filt", "rec_key", "dd"), [int(x) for x in a]))

    def timing(self):
        t = KrTiming()
        check(self.lib.kr_batch_timing(self.h, C.byref(t)))
        return t

    def format_seek(self, host_index, device_index, names, hdist_th=4):
        """`krepp seek` rows from the collected batch (kr_format_seek)"""
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        txt = C.c_void_p()
        ln = C.c_uint64()
        self.lib.kr_format_seek.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(KrResultView), C.c_uint32, C.POINTER(C.c_char_p),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        check(self.lib.kr_format_seek(host_index.h, device_index.h, C.byref(self._rv), hdist_th, arr, C.byref(txt), C.byref(ln)))
        s = C.string_at(txt, ln.value).decode()
        self.lib.kr_free(txt)
        return s

    def text_enable(self, host_index, max_text_bytes, max_id_bytes):
        """kr_stream_text_enable: this stream formats its rows-only batches on the device (csrc/kr_dev_text.inc)"""
        check(self.lib.kr_stream_text_enable(self.h, host_index.h, int(max_text_bytes), int(max_id_bytes)))
        self._text_on = True

    def submit_text(self, bases, offsets, names, flags=0, sep=1):
        """kr_batch_submit_text with the reads' ids packed back to back, `sep` NUL bytes behind each"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        enc = [n.encode() for n in names]
        blob = (b"\0" * sep).join(enc) + b"\0" * sep
        lens = np.fromiter((len(e) + sep for e in enc), dtype=np.uint32, count=len(enc))
        id_off = np.zeros(len(enc) + 1, dtype=np.uint32)
        np.cumsum(lens, out=id_off[1:])
        ids = np.frombuffer(blob, dtype=np.uint8)
        self._keep = (bases, offsets, ids, id_off)
        self._flags = flags | KR_ROWS_ONLY
        check(self.lib.kr_batch_submit_text(self.h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, flags, ids.ctypes.data, id_off.ctypes.data, sep))

    def submit_text_device(self, bases_ptr, offsets_ptr, nreads, names, flags=0, sep=1):
        """kr_batch_submit_text of a batch whose bases and offsets are in HBM (KR_BASES_DEVICE is added); the ids come from the host"""
        enc = [n.encode() for n in names]
        ids = np.frombuffer((b"\0" * sep).join(enc) + b"\0" * sep, dtype=np.uint8)
        id_off = np.zeros(len(enc) + 1, dtype=np.uint32)
        np.cumsum(np.fromiter((len(e) + sep for e in enc), dtype=np.uint32, count=len(enc)), out=id_off[1:])
        self._keep = (ids, id_off)
        self._flags = flags | KR_BASES_DEVICE | KR_ROWS_ONLY
        check(self.lib.kr_batch_submit_text(self.h, int(bases_ptr), int(offsets_ptr), int(nreads), flags | KR_BASES_DEVICE, ids.ctypes.data, id_off.ctypes.data, sep))

    def fastq_enable(self, max_raw_bytes):
        """kr_stream_fastq_enable: this stream can be given batches as raw FASTQ bytes (csrc/kr_dev_fastq.inc)"""
        check(self.lib.kr_stream_fastq_enable(self.h, int(max_raw_bytes)))

    def submit_fasta(self, raw, flags=0, closed=1):
        """kr_batch_submit_fasta on a page-locked copy of `raw` (kept until the next submit): the summary as a dict"""
        return self.submit_fastq(raw, flags, closed, call=self.lib.kr_batch_submit_fasta)

    def submit_fastq(self, raw, flags=0, at_eof=1, call=None):
        """kr_batch_submit_fastq on a page-locked copy of `raw` (kept until the next submit): the summary as a dict"""
        raw = bytes(raw)
        n = len(raw)
        if getattr(self, "_pinned_cap", 0) < max(n, 1):
            if getattr(self, "_pinned", None):
                self.lib.kr_host_free(self._pinned)
            self._pinned = self.lib.kr_host_alloc(max(n, 1))
            if not self._pinned:
                raise MemoryError("kr_host_alloc failed")
            self._pinned_cap = max(n, 1)
        C.memmove(self._pinned, raw, n)
        self._raw = raw
        out = KrFastqParse()
        check((call or self.lib.kr_batch_submit_fastq)(self.h, self._pinned, n, flags, at_eof, C.byref(out)))
        self._fq_nreads = out.nreads
        text = getattr(self, "_text_on", False) and not (flags & (KR_TAP_ACCS | KR_TAP_HITS))  # as kr_batch_submit_fastq decides
        self._flags = flags | KR_BASES_DEVICE | (KR_ROWS_ONLY if text else 0)
        return {f: getattr(out, f) for f in ("consumed", "nbases", "id_bytes", "newlines", "nreads", "status", "rejected", "at_eof")}

    def bgzf_enable(self, max_comp_bytes):
        """kr_stream_bgzf_enable (after fastq_enable): this stream can be given batches as whole BGZF members (csrc/kr_dev_bgzf.inc)"""
        check(self.lib.kr_stream_bgzf_enable(self.h, int(max_comp_bytes)))

    def submit_bgzf(self, comp, skip, nbytes, flags=0, fasta=False, at_eof=1, want_raw=True):
        """kr_batch_submit_bgzf on a page-locked copy of the members `comp`: (summary as a dict, the chunk's inflated bytes or None).
        The chunk is bytes [skip, skip + nbytes) of the members' inflated bytes; names are cut out of the bytes that came back."""
        comp = bytes(comp)
        n = len(comp)
        need = max(n, 1) + max(int(nbytes), 1)
        if getattr(self, "_pinned_cap", 0) < need:
            if getattr(self, "_pinned", None):
                self.lib.kr_host_free(self._pinned)
            self._pinned = self.lib.kr_host_alloc(need)
            if not self._pinned:
                raise MemoryError("kr_host_alloc failed")
            self._pinned_cap = need
        C.memmove(self._pinned, comp, n)
        raw_out = self._pinned + max(n, 1) if want_raw else None
        self._raw_out = raw_out
        out = KrFastqParse()
        check(self.lib.kr_batch_submit_bgzf(self.h, self._pinned, n, int(skip), int(nbytes), raw_out, flags, 1 if fasta else 0, at_eof, C.byref(out)))
        self._raw = C.string_at(raw_out, int(nbytes)) if want_raw else b""
        self._fq_nreads = out.nreads
        text = getattr(self, "_text_on", False) and not (flags & (KR_TAP_ACCS | KR_TAP_HITS))
        self._flags = flags | KR_BASES_DEVICE | (KR_ROWS_ONLY if text else 0)
        return {f: getattr(out, f) for f in ("consumed", "nbases", "id_bytes", "newlines", "nreads", "status", "rejected", "at_eof")}, (self._raw if want_raw else None)

    def bgzf_inflate(self, comp, cap=None):
        """(tests) kr_debug_bgzf_inflate: the inflate kernel alone on whole members, all their bytes"""
        comp = bytes(comp)
        cap = (len(comp) // 28 + 1) * 65536 if cap is None else int(cap)
        out = np.zeros(max(1, cap), np.uint8)
        n = C.c_uint64(0)
        check(self.lib.kr_debug_bgzf_inflate(self.h, comp, len(comp), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].tobytes()

    def bgzf_ms(self):
        """(measurements) kr_debug_bgzf_ms: device time of the last chunk's inflate kernel, -1 before the first measured one"""
        ms = C.c_float(0)
        check(self.lib.kr_debug_bgzf_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def fastq_names(self):
        """kr_batch_fastq_names: the accepted records' names, cut out of the bytes given to submit_fastq"""
        pos, ln = u64p(), u32p()
        check(self.lib.kr_batch_fastq_names(self.h, C.byref(pos), C.byref(ln)))
        n = self._fq_nreads
        if n == 0:
            return []
        p = np.ctypeslib.as_array(pos, shape=(n,))
        q = np.ctypeslib.as_array(ln, shape=(n,))
        return [self._raw[int(a):int(a) + int(b)].decode("latin-1") for a, b in zip(p, q)]

    def place_ids(self):
        """(tests) kr_debug_place_ids: the reads' ids as the device laid them out for the last kr_place_stream_parsed call on this
        stream (Placer.place_parsed with device text), as a list of bytes"""
        n = self._fq_nreads
        id_off = np.zeros(n + 1, np.uint32)
        ids = np.zeros(max(1, len(self._raw)), np.uint8)  # (the names are pieces of the chunk)
        check(self.lib.kr_debug_place_ids(self.h, ids.ctypes.data, id_off.ctypes.data))
        assert id_off[0] == 0
        return [ids[int(id_off[i]):int(id_off[i + 1])].tobytes() for i in range(n)]

    def fastq_batch(self, summary):
        """(tests) the accepted records' sequences as the record finder wrote them (kr_debug_fastq_batch)"""
        offs = np.zeros(summary["nreads"] + 1, np.uint64)
        bases = np.zeros(max(1, summary["nbases"]), np.uint8)
        check(self.lib.kr_debug_fastq_batch(self.h, bases.ctypes.data, offs.ctypes.data))
        return [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(summary["nreads"])]

    def tile_layout(self, nreads):
        """(tests) kr_debug_tile_layout: the tiled form of the batch last submitted as it lies on the device, as a dict of
        nv, nlong and the arrays voff, vtile, rfirst, longs, bases; nv == 0 (and no arrays) when the batch is not tiled"""
        nv, nl = C.c_uint32(0), C.c_uint32(0)
        check(self.lib.kr_debug_tile_layout(self.h, C.byref(nv), C.byref(nl), None, None, None, None, None))
        out = {"nv": int(nv.value), "nlong": int(nl.value)}
        if out["nv"] == 0:
            return out
        voff, vtile = np.zeros(out["nv"] + 1, np.uint64), np.zeros(out["nv"], np.uint8)
        rfirst, longs = np.zeros(nreads, np.uint32), np.zeros(2 * out["nlong"], np.uint32)
        check(self.lib.kr_debug_tile_layout(self.h, C.byref(nv), C.byref(nl), voff.ctypes.data, vtile.ctypes.data, rfirst.ctypes.data,
                                            longs.ctypes.data, None))
        bases = np.zeros(max(1, int(voff[-1])), np.uint8)
        check(self.lib.kr_debug_tile_layout(self.h, C.byref(nv), C.byref(nl), None, None, None, None, bases.ctypes.data))
        out.update(voff=voff, vtile=vtile, rfirst=rfirst, longs=longs.reshape(-1, 2), bases=bases[:int(voff[-1])])
        return out

    def collect_text(self):
        """kr_batch_collect_text: the batch's report rows as the bytes the device wrote"""
        txt = C.c_void_p()
        ln = C.c_uint64()
        check(self.lib.kr_batch_collect_text(self.h, C.byref(txt), C.byref(ln)))
        return C.string_at(txt, ln.value) if ln.value else b""

    def bgzf_out_enable(self):
        """kr_stream_bgzf_out_enable (after text_enable or seek_enable with text buffers): this stream can hand its report text out as
        BGZF members deflated on the device (csrc/kr_dev_deflate.inc)"""
        check(self.lib.kr_stream_bgzf_out_enable(self.h))

    def bgzf_out_level(self, level):
        """kr_stream_bgzf_out_level: the level of this stream's later collect_text_bgzf / bgzf_deflate (1: fixed codes, 2: dynamic)"""
        check(self.lib.kr_stream_bgzf_out_level(self.h, int(level)))

    def bgzf_member(self, member_bytes):
        """kr_stream_bgzf_member: input bytes of a member (256 .. 65,280) of this stream's later device deflates"""
        check(self.lib.kr_stream_bgzf_member(self.h, int(member_bytes)))

    def place_bgzf(self, level):
        """kr_stream_place_bgzf: kr_place_stream's text comes back as BGZF members (0: off, 1 / 2: the encoder's level)"""
        check(self.lib.kr_stream_place_bgzf(self.h, int(level)))

    def bgzf_deflate_at(self, data, skip, cap=None):
        """(tests) kr_debug_bgzf_deflate_at: `data` goes to the device, data[skip:] is deflated from the device address of byte skip"""
        data = bytes(data)
        cap = bgzf_deflate_bound(len(data)) * 2 + 4096 if cap is None else int(cap)
        out = np.zeros(max(1, cap), np.uint8)
        n = C.c_uint64(0)
        check(self.lib.kr_debug_bgzf_deflate_at(self.h, data, len(data), int(skip), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].tobytes()

    def collect_text_bgzf(self, level=None):
        """kr_batch_collect_text_bgzf: (the batch's report text as BGZF members, the bytes they inflate to); level: bgzf_out_level first"""
        if level is not None:
            self.bgzf_out_level(level)
        comp = C.c_void_p()
        ln, tl = C.c_uint64(), C.c_uint64()
        check(self.lib.kr_batch_collect_text_bgzf(self.h, C.byref(comp), C.byref(ln), C.byref(tl)))
        return (C.string_at(comp, ln.value) if ln.value else b""), int(tl.value)

    def bgzf_deflate(self, data, cap=None, level=None):
        """(tests) kr_debug_bgzf_deflate: any bytes through the deflate kernels, the members back; level: bgzf_out_level first"""
        if level is not None:
            self.bgzf_out_level(level)
        data = bytes(data)
        cap = bgzf_deflate_bound(len(data)) if cap is None else int(cap)
        out = np.zeros(max(1, cap), np.uint8)
        n = C.c_uint64(0)
        check(self.lib.kr_debug_bgzf_deflate(self.h, data, len(data), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value].tobytes()

    def huffman_lengths(self, freq, maxbits, level=2):
        """(tests) kr_debug_huffman_lengths_device: as capi.huffman_lengths, through the builder kernel on this stream's device"""
        return _huffman_lengths(lambda *a: self.lib.kr_debug_huffman_lengths_device(self.h, *a), freq, maxbits, level)

    def bgzf_deflate_ms(self):
        """(measurements) kr_debug_bgzf_deflate_ms: device time of the last deflate's kernels, -1 before the first measured one"""
        ms = C.c_float(0)
        check(self.lib.kr_debug_bgzf_deflate_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def seek_enable(self, max_text_bytes=0, max_id_bytes=0):
        """kr_stream_seek_enable: this stream takes batches flagged KR_SEEK (csrc/kr_dev_seek.inc); 0, 0: values only, no text"""
        check(self.lib.kr_stream_seek_enable(self.h, int(max_text_bytes), int(max_id_bytes)))

    def collect_seek(self):
        """kr_batch_collect_seek: numpy copies of the seek batch's values -- d [nreads], d_strand [nreads, 2], hist [nreads, 2, np],
        onmers [nreads]"""
        v = KrSeekView()
        check(self.lib.kr_batch_collect_seek(self.h, C.byref(v)))
        n, npl = int(v.nreads), int(v.np)
        return {"nreads": n, "np": npl, "d": _np(v.d, n, np.float64), "d_strand": _np(v.d_strand, 2 * n, np.float64).reshape(n, 2),
                "hist": _np(v.hist, n * 2 * npl, np.uint32).reshape(n, 2, npl), "onmers": _np(v.onmers, n, np.uint32)}

    def seek_ms(self):
        """kr_debug_seek_ms: device milliseconds of the last seek batch's hist, solve and text stages"""
        ms = (C.c_float * 3)()
        check(self.lib.kr_debug_seek_ms(self.h, ms))
        return tuple(float(x) for x in ms)

    def extract_enable(self, max_dist=float("nan")):
        """kr_stream_extract_enable (after seek_enable and fastq_enable): the reads of this stream's raw-bytes seek batches are split into
        matched and unmatched bytes on the device (csrc/kr_dev_extract.inc); NaN: every read with a DIST is matched"""
        check(self.lib.kr_stream_extract_enable(self.h, float(max_dist)))

    def extract_max(self, max_dist):
        """kr_stream_extract_max: the threshold of the batches submitted from now on (NaN: none)"""
        check(self.lib.kr_stream_extract_max(self.h, float(max_dist)))

    @staticmethod
    def _extract_dict(v):
        return {"nreads": int(v.nreads), "nmatched": int(v.nmatched), "matched_bytes": int(v.matched_bytes), "unmatched_bytes": int(v.unmatched_bytes),
                "matched": None if not v.matched else C.string_at(v.matched, v.matched_len),
                "unmatched": None if not v.unmatched else C.string_at(v.unmatched, v.unmatched_len)}

    def collect_extract(self, which=KR_EXTRACT_MATCHED | KR_EXTRACT_UNMATCHED):
        """kr_batch_collect_extract: the counts and copies of the parts named in `which` (a part not asked for is None)"""
        v = KrExtractView()
        check(self.lib.kr_batch_collect_extract(self.h, int(which), C.byref(v)))
        return self._extract_dict(v)

    def collect_extract_bgzf(self, level, which=KR_EXTRACT_MATCHED | KR_EXTRACT_UNMATCHED):
        """kr_batch_collect_extract_bgzf: as collect_extract with each part as BGZF members deflated on the device (an empty part: b"")"""
        v = KrExtractView()
        check(self.lib.kr_batch_collect_extract_bgzf(self.h, int(which), int(level), C.byref(v)))
        return self._extract_dict(v)

    def extract_defer(self, on=True):
        """kr_stream_extract_defer: a raw-bytes seek submit leaves the split to extract_pair (paired reads); False: as before"""
        check(self.lib.kr_stream_extract_defer(self.h, 1 if on else 0))

    def extract_pair(self, other, rule=KR_PAIR_ANY):
        """kr_batch_extract_pair: this stream's batch and `other`'s hold the mates (other is self: one interleaved batch); both are split
        by the pair's verdict (KR_PAIR_ANY / KR_PAIR_BOTH), then collect_extract / collect_extract_bgzf on each stream"""
        check(self.lib.kr_batch_extract_pair(self.h, other.h, int(rule)))

    def extract_ms(self):
        """kr_debug_extract_ms: device milliseconds of the last batch's extract kernels"""
        ms = C.c_float(0)
        check(self.lib.kr_debug_extract_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def format_dist(self, host_index, names):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        txt = C.c_void_p()
        ln = C.c_uint64()
        check(self.lib.kr_format_dist(host_index.h, C.byref(self._rv), arr, C.byref(txt), C.byref(ln)))
        s = C.string_at(txt, ln.value).decode()
        self.lib.kr_free(txt)
        return s

    def close(self):
        if self.h:
            self.lib.kr_stream_destroy(self.h)
            self.h = C.c_void_p()
        if getattr(self, "_pinned", None):
            self.lib.kr_host_free(self._pinned)
            self._pinned, self._pinned_cap = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def acc_layout(np_planes, segs=1, multi=0, stream=None):
    """(tests) kr_debug_acc_layout: the event region of an accumulate instantiation; the spill capacities are the stream's (0 without one)"""
    a = (C.c_uint32 * 8)()
    check(load().kr_debug_acc_layout(stream.h if stream is not None else None, int(np_planes), int(segs), int(multi), a))
    assert a[3] == len(ACC_PATHS)
    return dict(ev_cap=int(a[0]), ev_words=int(a[1]), key_words=int(a[2]), ev_spill=int(a[4]), tab_spill=int(a[5]), kt_spill=int(a[6]))


SCAN_LAYOUT = ("G", "CPL", "PPS", "W", "CAP", "step_bits", "list_cap", "item_stage", "item_chunk", "read_chunk", "cursors", "seg_pos",
               "line_codes", "slot_codes", "slotted", "filt_max_th")


SELECT_LAYOUT = ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs", "big_step2", "row_block", "row_round")


def select_layout():
    """(tests) kr_debug_select_layout: the constants of the select and row kernels, by name"""
    a = (C.c_uint32 * 8)()
    check(load().kr_debug_select_layout(a))
    return dict(zip(SELECT_LAYOUT, [int(x) for x in a]))


def select_tables(t):
    """KrSelectTables over the arrays of dict `t` (keys as the structure's fields; rec_hist [nrecs, th + 1] and rec_read optional,
    counts taken from the arrays unless given); returns it with the arrays that must outlive it"""
    spec = dict(rd_off=np.uint32, rd_cnt=np.uint32, rd_onmers=np.uint32, rec_key=np.uint32, rec_rep=np.uint32, rec_w0=np.uint64,
                rec_hist=np.uint32, rec_read=np.uint32, rep_dv=np.float64, dd_direct=np.uint32, dd_dv=np.float64)
    keep = {k: np.ascontiguousarray(t[k], dtype=dt) for k, dt in spec.items() if t.get(k) is not None}
    s = KrSelectTables()
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(dict(KrSelectTables._fields_)[k]) if a.size else None)
    s.nreads = int(t.get("nreads", len(keep["rd_off"])))
    s.nrecs = int(t.get("nrecs", len(keep["rec_key"]) if "rec_key" in keep else 0))
    s.nrep = int(t.get("nrep", keep["rep_dv"].size // 2 if "rep_dv" in keep else 0))
    s.ndirect = int(t.get("ndirect", len(keep["dd_direct"]) if "dd_direct" in keep else 0))
    s.problems = int(t.get("problems", s.nrep))
    return s, keep


def select_check(t, max_reads, max_records, nnodes, hdist_th=4, direct_nodes=0):
    """(tests, no device) kr_debug_select_check: the return code.  direct_nodes: the nodes the stream's direct part is laid out for"""
    s, keep = select_tables(t)
    return load().kr_debug_select_check(C.byref(s), int(max_reads), int(max_records), int(nnodes), int(hdist_th), int(direct_nodes))


DEDUP_LAYOUT = ("oslots", "classes", "max_events", "min_slots", "probe_rounds", "rep_chunk", "rep_chunk_max", "dedup_blocks", "oslot_reads",
                "hash_word_lo", "hash_word_hi", "hash_leaf")


def dedup_layout():
    """(tests) kr_debug_dedup_layout: the constants of the de-duplication kernels, by name; hash_word: the 64-bit multiplier"""
    a = (C.c_uint32 * 12)()
    check(load().kr_debug_dedup_layout(a))
    d = dict(zip(DEDUP_LAYOUT, [int(x) for x in a]))
    d["hash_word"] = d.pop("hash_word_hi") << 32 | d.pop("hash_word_lo")
    return d


def dedup_tables(t):
    """KrDedupTables over the arrays of dict `t` (keys as the structure's fields; rec_hist [nrecs, th + 1] and rec_read optional, counts
    taken from the arrays unless given); returns it with the arrays that must outlive it"""
    spec = dict(rd_off=np.uint32, rd_cnt=np.uint32, rd_onmers=np.uint32, rec_key=np.uint32, rec_w0=np.uint64, rec_hist=np.uint32, rec_read=np.uint32)
    keep = {k: np.ascontiguousarray(t[k], dtype=dt) for k, dt in spec.items() if t.get(k) is not None}
    s = KrDedupTables()
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(dict(KrDedupTables._fields_)[k]) if a.size else None)
    s.nreads = int(t.get("nreads", len(keep["rd_off"]) if "rd_off" in keep else 0))
    s.nrecs = int(t.get("nrecs", len(keep["rec_key"]) if "rec_key" in keep else 0))
    return s, keep


def dedup_check(t, max_reads, max_records, nnodes, hdist_th=4):
    """(tests, no device) kr_debug_dedup_check: the return code"""
    s, keep = dedup_tables(t)
    return load().kr_debug_dedup_check(C.byref(s), int(max_reads), int(max_records), int(nnodes), int(hdist_th))


def seek_layout():
    """kr_debug_seek_layout (no device): positions per unit, positions per segment, waves per workgroup of the hist kernel, reads per
    prefix block"""
    out = (C.c_uint32 * 4)()
    check(load().kr_debug_seek_layout(out))
    return {"unit": int(out[0]), "segment": int(out[1]), "hist_waves": int(out[2]), "row_block": int(out[3])}


def scan_layout(slot_format, log_g=0):
    """(tests) kr_debug_scan_layout: the numbers of the scan shape chosen for a table of this slot format (0: packed, shape by log_g)"""
    a = (C.c_uint32 * 16)()
    check(load().kr_debug_scan_layout(int(slot_format), int(log_g), a))
    return dict(zip(SCAN_LAYOUT, [int(x) for x in a]))


def fasta_chunk_cut(buf):
    """kr_fasta_chunk_cut: the position of the last record start ('>' behind a newline) in buf[1:], 0 when there is none"""
    buf = bytes(buf)
    return int(load().kr_fasta_chunk_cut(buf, len(buf)))


def fastq_pair_cut(a, b=None, max_records=0xFFFFFFFF):
    """kr_fastq_pair_cut: (cut_a, cut_b, n) -- the largest n <= max_records such that a and b both hold 4n complete lines, and the byte
    behind the 4n-th newline of each; b None: the interleaved form, the largest even n of a (cut_b is 0)"""
    ca, cb, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    a = bytes(a)
    b = None if b is None else bytes(b)
    check(load().kr_fastq_pair_cut(a, len(a), b, 0 if b is None else len(b), int(max_records), C.byref(ca), C.byref(cb), C.byref(n)))
    return int(ca.value), int(cb.value), int(n.value)


def fastq_chunk_cut(buf):
    """kr_fastq_chunk_cut: the last line start in buf's last MiB that begins with '@' and whose second next line begins with '+'
    (that '+' still inside buf), 0 when there is none"""
    buf = bytes(buf)
    return int(load().kr_fastq_chunk_cut(buf, len(buf)))


def bgzf_inflate_host(comp, cap=None):
    """kr_debug_bgzf_inflate_host: whole BGZF members through the decoder's host instantiation (no device), all their bytes"""
    comp = bytes(comp)
    cap = (len(comp) // 28 + 1) * 65536 if cap is None else int(cap)
    out = np.zeros(max(1, cap), np.uint8)
    n = C.c_uint64(0)
    check(load().kr_debug_bgzf_inflate_host(comp, len(comp), out.ctypes.data, cap, C.byref(n)))
    return out[: n.value].tobytes()


GZDEV_COUNTERS = ("super_chunks", "linked", "without_start", "dropped", "host_ranges", "redone_bytes")
GZDEV_STATUS = ("idle", "linked", "member_end", "input_end", "overflow", "bad")


class GzdevResult:
    """What kr_debug_gzdev_inflate(_host) returns: the bytes handed out, the error (None, or the KrError raised behind the bytes), the
    rows of every super-chunk's sub-chunks one after the other, the counters"""

    def __init__(self, data, error, tables, counters):
        self.data, self.error, self.tables, self.counters = data, error, tables, counters

    def same_tables(self, other):
        return all(np.array_equal(self.tables[k], other.tables[k]) for k in self.tables) and self.counters == other.counters


def gzdev_inflate(comp, sub=32768, ratio=16, max_comp=64 << 20, cap=None, device=None):
    """kr_debug_gzdev_inflate (device = an ordinal) / kr_debug_gzdev_inflate_host (device = None): a whole ordinary gzip buffer through
    the inflater's four stages.  A damaged buffer gives the bytes in front of the damage and `.error`."""
    comp = bytes(comp)
    cap = max(1 << 16, 40 * len(comp)) if cap is None else int(cap)
    out = np.zeros(max(1, cap), np.uint8)
    tab_cap = (len(comp) // int(sub) + 2) * 64 + 64
    tabs = {k: np.zeros(tab_cap, np.uint32) for k in ("S", "end", "status", "link", "length", "crc")}
    ctr = np.zeros(6, np.uint64)
    n, nt = C.c_uint64(0), C.c_uint64(0)
    tail = [int(sub), int(ratio), int(max_comp), out.ctypes.data, cap, C.byref(n), tab_cap] + [tabs[k].ctypes.data for k in tabs] + [
        C.byref(nt), ctr.ctypes.data_as(C.POINTER(C.c_uint64))]
    if device is None:
        rc = load().kr_debug_gzdev_inflate_host(comp, len(comp), *tail)
    else:
        rc = load().kr_debug_gzdev_inflate(int(device), comp, len(comp), *tail)
    err = None
    if rc == KR_ERR_IO:
        err = KrError(rc, load().kr_last_error().decode(errors="replace"))
    else:
        check(rc)
    return GzdevResult(out[: n.value].tobytes(), err, {k: v[: nt.value].copy() for k, v in tabs.items()},
                       dict(zip(GZDEV_COUNTERS, (int(x) for x in ctr))))


def gzdev_point_host(comp, inflated_off, sub=32768, ratio=16, max_comp=64 << 20):
    """kr_debug_gzdev_point_host: the restart point the serial twin keeps at or in front of inflated_off"""
    comp = bytes(comp)
    pt = KrGzipPoint()
    check(load().kr_debug_gzdev_point_host(comp, len(comp), int(sub), int(ratio), int(max_comp), int(inflated_off), C.byref(pt)))
    return pt


class Gzdev:
    """kr_gzdev: an ordinary gzip file inflated on a device, super-chunk by super-chunk"""

    def __init__(self, path, device=0, max_comp=64 << 20, sub=32768, ratio=16, keep_points=4):
        self.lib = load()
        self.h = C.c_void_p()
        check(self.lib.kr_gzdev_open(os.fsencode(str(path)), int(device), int(max_comp), int(sub), int(ratio), int(keep_points), C.byref(self.h)))

    def read(self, cap=1 << 20):
        """the next inflated bytes (at most cap); b"" at the end"""
        buf = np.zeros(int(cap), np.uint8)
        n = C.c_uint64(0)
        check(self.lib.kr_gzdev_read(self.h, buf.ctypes.data, int(cap), C.byref(n)))
        return buf[: n.value].tobytes()

    def point(self, inflated_off):
        pt = KrGzipPoint()
        check(self.lib.kr_gzdev_point(self.h, int(inflated_off), C.byref(pt)))
        return pt

    def counters(self):
        c = np.zeros(11, np.uint64)
        check(self.lib.kr_gzdev_counters(self.h, c.ctypes.data_as(C.POINTER(C.c_uint64))))
        d = dict(zip(GZDEV_COUNTERS, (int(x) for x in c[:6])))
        d.update(us_search=int(c[6]), us_decode=int(c[7]), us_chain=int(c[8]), us_resolve=int(c[9]), us_copy=int(c[10]))
        return d

    def close(self):
        if self.h:
            self.lib.kr_gzdev_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        self.close()


def bgzf_member_size(buf):
    """kr_bgzf_member_size: the size of the BGZF member that `buf` starts with, 0 when it does not start with one"""
    buf = bytes(buf)
    return int(load().kr_bgzf_member_size(buf, len(buf)))


def bgzf_walk(buf, max_inflated):
    """kr_bgzf_walk: (members, compressed bytes, inflated bytes) of the whole members at the front of buf within max_inflated"""
    buf = bytes(buf)
    k, c, u = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    check(load().kr_bgzf_walk(buf, len(buf), int(max_inflated), C.byref(k), C.byref(c), C.byref(u)))
    return int(k.value), int(c.value), int(u.value)


BGZF_DEFLATE_STATS = ("members", "stored", "literals", "matches", "longest", "farthest")
BGZF_DEFLATE_STATS_LEVEL = BGZF_DEFLATE_STATS + ("fixed", "dynamic", "limited", "header_bits")


def bgzf_deflate_bound(n):
    """kr_bgzf_deflate_bound: the most bytes the host form or the device produce for n bytes"""
    return int(load().kr_bgzf_deflate_bound(int(n)))


def bgzf_deflate_host(text, cap=None, level=None):
    """kr_bgzf_deflate_host: `text` as BGZF members of 65,280 input bytes each (no device, no end member); with a level:
    kr_bgzf_deflate_host_level (1: fixed codes, 2: dynamic codes)"""
    text = bytes(text)
    cap = bgzf_deflate_bound(len(text)) if cap is None else int(cap)
    out = np.zeros(max(1, cap), np.uint8)
    n = C.c_uint64(0)
    if level is None:
        check(load().kr_bgzf_deflate_host(text, len(text), out.ctypes.data, cap, C.byref(n)))
    else:
        check(load().kr_bgzf_deflate_host_level(text, len(text), int(level), out.ctypes.data, cap, C.byref(n)))
    return out[: n.value].tobytes()


def bgzf_deflate_bound_member(n, member_bytes):
    """kr_bgzf_deflate_bound_member: kr_bgzf_deflate_bound for members of member_bytes input bytes (0: no such member length)"""
    return int(load().kr_bgzf_deflate_bound_member(int(n), int(member_bytes)))


def bgzf_deflate_host_member(text, level, member_bytes, cap=None):
    """kr_bgzf_deflate_host_member: `text` as BGZF members of member_bytes input bytes each, at a level (no device, no end member)"""
    text = bytes(text)
    cap = bgzf_deflate_bound_member(len(text), member_bytes) if cap is None else int(cap)
    out = np.zeros(max(1, cap), np.uint8)
    n = C.c_uint64(0)
    check(load().kr_bgzf_deflate_host_member(text, len(text), int(level), int(member_bytes), out.ctypes.data, cap, C.byref(n)))
    return out[: n.value].tobytes()


def place_bgzf_counters():
    """kr_place_bgzf_counters: (ranges deflated on the device, ranges deflated by the host encoder) of this process"""
    d, h = C.c_uint64(0), C.c_uint64(0)
    load().kr_place_bgzf_counters(C.byref(d), C.byref(h))
    return int(d.value), int(h.value)


def bgzf_eof():
    """kr_bgzf_eof: the 28-byte empty member that ends a BGZF file"""
    out = C.create_string_buffer(28)
    load().kr_bgzf_eof(out)
    return out.raw


def bgzf_deflate_stats(text, level=None):
    """(tests) kr_debug_bgzf_deflate_stats: what the host form did with `text`, as a dict of BGZF_DEFLATE_STATS; with a level:
    kr_debug_bgzf_deflate_stats_level, a dict of BGZF_DEFLATE_STATS_LEVEL"""
    text = bytes(text)
    if level is None:
        st = (C.c_uint64 * 6)()
        check(load().kr_debug_bgzf_deflate_stats(text, len(text), st))
        return dict(zip(BGZF_DEFLATE_STATS, [int(x) for x in st]))
    st = (C.c_uint64 * 10)()
    check(load().kr_debug_bgzf_deflate_stats_level(text, len(text), int(level), st))
    return dict(zip(BGZF_DEFLATE_STATS_LEVEL, [int(x) for x in st]))


def _huffman_lengths(call, freq, maxbits, level):
    if int(level) != 2:
        raise ValueError("the code-length builder belongs to level 2")
    freq = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.zeros(max(1, len(freq)), np.uint8)
    limited = C.c_uint32(0)
    check(call(freq.ctypes.data, len(freq), int(maxbits), lens.ctypes.data, C.byref(limited)))
    return lens[: len(freq)].copy(), bool(limited.value)


def huffman_lengths(freq, maxbits, level=2):
    """(tests) kr_debug_huffman_lengths: (code lengths for the counts `freq` with none longer than maxbits, whether the limit was
    needed), from the level-2 encoder's builder on the host"""
    return _huffman_lengths(load().kr_debug_huffman_lengths, freq, maxbits, level)


def bgzf_chunk_cut(buf, skip=0, fasta=False):
    """kr_bgzf_chunk_cut on the whole members `buf`: (cut's position in the chunk or 0, member offset in buf, byte inside the member)"""
    buf = bytes(buf)
    m, u = C.c_uint64(0), C.c_uint32(0)
    cut = load().kr_bgzf_chunk_cut(buf, len(buf), int(skip), 1 if fasta else 0, C.byref(m), C.byref(u))
    return int(cut), int(m.value), int(u.value)


def tile_shape(length, k):
    """(tests) kr_debug_tile_shape: (k-mer positions, tiles of 128 positions, bases in a tiled batch) of a sequence of `length` bases"""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(load().kr_debug_tile_shape(int(length), int(k), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def debug_prefix(values, block, width):
    """(tests) the device's prefix-sum helpers on plain numbers (kr_debug_prefix): (exclusive prefix of every value, total), with
    blocks of `block` values and sums of `width` bytes."""
    values = np.ascontiguousarray(values, dtype=np.uint32)
    prefix = np.zeros(len(values), np.uint64)
    total = C.c_uint64(0)
    check(load().kr_debug_prefix(values.ctypes.data, len(values), block, width, prefix.ctypes.data, C.byref(total)))
    return prefix, total.value


def colour_classes(pse, node_kind):
    """Host pass of kr_index_upload over a colour table (no device): (cls[nsubsets], pse_dev[nsubsets, 2], lists)."""
    lib = load()
    pse = np.ascontiguousarray(pse, dtype=np.uint32).reshape(-1, 2)
    node_kind = np.ascontiguousarray(node_kind, dtype=np.uint8)
    n = len(pse)
    cls = np.zeros(n, np.uint32)
    out = np.zeros((n, 2), np.uint32)
    nl = C.c_uint64(0)
    rc = lib.kr_debug_colour_classes(pse.ctypes.data, n, node_kind.ctypes.data, len(node_kind) - 1, cls.ctypes.data, out.ctypes.data, None,
                                     C.byref(nl))
    lists = np.zeros(max(1, nl.value), np.uint32)
    if rc != 0:  # the first call sized the list buffer
        check(lib.kr_debug_colour_classes(pse.ctypes.data, n, node_kind.ctypes.data, len(node_kind) - 1, cls.ctypes.data, out.ctypes.data,
                                          lists.ctypes.data, C.byref(nl)))
    return cls, out, lists[: nl.value]


def read_fastx(path, min_bases=76800, stats=None, detach=0, offset=None, bgzf_at=None, gzip_at=None):
    """All records of a FASTA/FASTQ(.gz) file via the library's reader: (names, bases, offsets).
    detach = K > 0: every batch is taken over (kr_fastx_detach), read only when K further batches have been parsed, then handed
    back (kr_fastx_release) -- the way the CLI's workers hold batches in flight.
    offset: the sequential reader from that record start of a plain file on (kr_fastx_open_at).
    bgzf_at = (member_off, uoff): the same for a block-gzipped file (kr_fastx_open_at_bgzf).
    gzip_at = (inflated_off, KrGzipPoint or None): the same for an ordinary gzip file (kr_fastx_open_at_gzip)."""
    lib = load()
    lib.kr_fastx_parallel_chunks.restype = C.c_uint64
    lib.kr_fastx_parallel_chunks.argtypes = [C.c_void_p]
    h = C.c_void_p()
    if gzip_at is not None:
        check(lib.kr_fastx_open_at_gzip(os.fsencode(str(path)), int(gzip_at[0]), C.byref(gzip_at[1]) if gzip_at[1] is not None else None, C.byref(h)))
    elif bgzf_at is not None:
        check(lib.kr_fastx_open_at_bgzf(os.fsencode(str(path)), int(bgzf_at[0]), int(bgzf_at[1]), C.byref(h)))
    elif offset is None:
        check(lib.kr_fastx_open(os.fsencode(str(path)), C.byref(h)))
    else:
        check(lib.kr_fastx_open_at(os.fsencode(str(path)), int(offset), C.byref(h)))
    names, chunks, lens = [], [], []

    def take(b):
        if b.nreads:
            offs = np.ctypeslib.as_array(b.offsets, shape=(b.nreads + 1,)).copy()
            chunks.append(np.ctypeslib.as_array(b.bases, shape=(int(offs[-1]),)).copy() if offs[-1] else np.zeros(0, np.uint8))
            lens.extend(np.diff(offs).tolist())
            names.extend(b.names[i].decode() for i in range(b.nreads))

    held = []
    try:
        while True:
            b = KrFastxBatch()
            check(lib.kr_fastx_next(h, min_bases, C.byref(b)))
            if detach:
                hp = C.c_void_p()
                check(lib.kr_fastx_detach(h, C.byref(hp)))
                held.append((b, hp))
                while len(held) > detach:
                    ob, ohp = held.pop(0)
                    take(ob)
                    lib.kr_fastx_release(h, ohp)
            else:
                take(b)
            if not b.more:
                break
        for ob, ohp in held:
            take(ob)
            lib.kr_fastx_release(h, ohp)
    finally:
        if stats is not None:
            stats["parallel_chunks"] = int(lib.kr_fastx_parallel_chunks(h))
            a, b_, c_ = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            lib.kr_fastx_pgz_stats.restype = None
            lib.kr_fastx_pgz_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            lib.kr_fastx_pgz_stats(h, C.byref(a), C.byref(b_), C.byref(c_))
            stats["gzip_chunks"] = {"parsed": int(a.value), "discarded": int(b_.value), "gaps": int(c_.value)}
        lib.kr_fastx_close(h)
    bases = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    offsets = np.zeros(len(lens) + 1, np.uint64)
    offsets[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    return names, bases, offsets


def place_counters():
    """(batches whose `place` back end ran on the device, batches sent whole to the host back end) of this process."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    load().kr_place_counters(C.byref(a), C.byref(b), None)
    return int(a.value), int(b.value)


def place_text_counters():
    """(ranges of reads whose `place` rows were written on the device, ranges the host formatted although device text was on)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    load().kr_place_text_counters.restype = None
    load().kr_place_text_counters(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


PLACE_PATHS = ("reruns_cand", "reruns_keep", "list_cut", "given_up", "text_flag_1", "text_flag_2", "text_flag_4", "text_flag_8", "text_flag_16",
               "ranges", "cnt0", "cnt3", "cnt12", "text_bytes", "cand_cap", "keep_cap", "text_cap", "flags", "text_flags", "attempts")


def place_path_counters():
    """kr_place_path_counters as a dict: which recovery paths of the device back end of `place` ran in this process (reruns for
    candidate / kept slots, ranges with the internal candidates' list cut, ranges given up to the host back end, text fallbacks by
    flag, ranges finished: these only grow), and of the range finished last what it asked for (cnt0 candidate slots, cnt3 kept slots,
    cnt12 list entries, text_bytes) and ran with (cand_cap, keep_cap, text_cap, flags, text_flags, attempts)."""
    out = (C.c_uint64 * len(PLACE_PATHS))()
    lib = load()
    lib.kr_place_path_counters.restype = None
    lib.kr_place_path_counters.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]
    lib.kr_place_path_counters(out, len(PLACE_PATHS))
    return dict(zip(PLACE_PATHS, (int(v) for v in out)))


# kr_debug_place_paths: the path witnesses of place_read, in the order of PlaceCnt's kPlWitChained .. (kr_dev_place.inc)
PLACE_WITNESSES = ("chained", "walked_shallow", "walked_deep", "wide", "runs_off", "dup_dropped", "single", "tau_stopped", "home_lds",
                   "home_inline", "home_second", "multi_block_lanes")
PLACE_LAYOUT = ("leaves", "nodes", "block", "chain", "chunk", "chain_factor", "runs_leaves", "inline_chain")


def place_paths():
    """(tests) kr_debug_place_paths: {name: count} of place_read's path witnesses, summed over this process's `place` calls made under
    KR_DEBUG_PLACE_PATHS=1 (they only grow: take differences)."""
    out = (C.c_uint64 * len(PLACE_WITNESSES))()
    lib = load()
    lib.kr_debug_place_paths.restype = None
    lib.kr_debug_place_paths.argtypes = [C.POINTER(C.c_uint64), C.c_uint32]
    lib.kr_debug_place_paths(out, len(PLACE_WITNESSES))
    return dict(zip(PLACE_WITNESSES, (int(v) for v in out)))


def place_layout():
    """(tests) kr_debug_place_layout: the constants of the per-read kernel of `place` (no device needed)"""
    a = (C.c_uint32 * 8)()
    lib = load()
    lib.kr_debug_place_layout.argtypes = [u32p]
    check(lib.kr_debug_place_layout(a))
    return dict(zip(PLACE_LAYOUT, (int(v) for v in a)))


def place_heavy_reads():
    """Reads (upper bound, in chunks of 8) that kr_place_kernel's second launch did with its arrays in global scratch."""
    c = C.c_uint64(0)
    load().kr_place_counters(None, None, C.byref(c))
    return int(c.value)


KR_BUILD_GPU_MINIMIZERS, KR_BUILD_GPU_KEYS, KR_BUILD_GPU_COLOURS = 1, 2, 4  # bits of kr_build_params.gpu_minimizers
KR_NO_CLASS = 0xFFFFFFFF


def _gpu_build_bits(gpu_minimizers, gpu_keys, gpu_colours=False):
    return ((KR_BUILD_GPU_MINIMIZERS if gpu_minimizers else 0) | (KR_BUILD_GPU_MINIMIZERS | KR_BUILD_GPU_KEYS if gpu_keys else 0)
            | (KR_BUILD_GPU_MINIMIZERS | KR_BUILD_GPU_KEYS | KR_BUILD_GPU_COLOURS if gpu_colours else 0))


def key_groups(keys, ranks, nrows, nleaves, device=None, copy=True):
    """The key stage on its own: dict(keys, goff, ranks, inc) of the (key, rank) pairs: kr_key_groups_cpu (device=None) or _device.
    copy=False: the arrays are views of the library's memory (an inc of 2^30 rows is 8 GB), valid until the dict's "free"() is called."""
    lib = load()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint32)
    assert len(keys) == len(ranks)
    res = KrKeyGroups()
    vp = C.c_void_p
    kp = keys.ctypes.data if len(keys) else None
    rp = ranks.ctypes.data if len(ranks) else None
    lib.kr_key_groups_cpu.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(KrKeyGroups)]
    lib.kr_key_groups_device.argtypes = [C.c_int, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(KrKeyGroups)]
    lib.kr_key_groups_free.argtypes = [C.POINTER(KrKeyGroups)]
    lib.kr_key_groups_free.restype = None
    if device is None:
        check(lib.kr_key_groups_cpu(kp, rp, len(keys), nrows, nleaves, C.byref(res)))
    else:
        check(lib.kr_key_groups_device(int(device), kp, rp, len(keys), nrows, nleaves, C.byref(res)))
    if not copy:
        view = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(int(n),)).view(dt) if n and ptr else np.zeros(0, dtype=dt)
        return {"keys": view(res.keys, res.nkeys, np.uint64), "goff": view(res.goff, res.nkeys + 1, np.uint64),
                "ranks": view(res.ranks, res.npairs, np.uint32), "inc": view(res.inc, res.nrows, np.uint64),
                "free": lambda: lib.kr_key_groups_free(C.byref(res))}
    out = {"keys": _np(res.keys, res.nkeys, np.uint64), "goff": _np(res.goff, res.nkeys + 1, np.uint64),
           "ranks": _np(res.ranks, res.npairs, np.uint32), "inc": _np(res.inc, res.nrows, np.uint64)}
    lib.kr_key_groups_free(C.byref(res))
    return out


def build_keys_stats():
    """kr_debug_build_keys: the process's last kr_key_groups_device or GPU key build."""
    v = (C.c_uint64 * 8)()
    lib = load()
    lib.kr_debug_build_keys.argtypes = [C.POINTER(C.c_uint64 * 8)]
    lib.kr_debug_build_keys.restype = None
    lib.kr_debug_build_keys(C.byref(v))
    return {"pairs_in": int(v[0]), "pairs_out": int(v[1]), "keys_out": int(v[2]), "passes": int(v[3]), "pool_growths": int(v[4]),
            "path": int(v[5]), "tile": int(v[6])}


def group_colour_classes(goff, ranks, device=None):
    """The colour classes of key groups (goff / ranks as key_groups returns them): (class_of[nkeys], rep[nclasses]) from
    kr_colour_classes_cpu (device=None) or _device.  (colour_classes, above, is the upload's pass over a colour table.)"""
    lib = load()
    goff = np.ascontiguousarray(goff, dtype=np.uint64)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint32)
    assert len(goff) >= 1
    res = KrColourClasses()
    vp = C.c_void_p
    lib.kr_colour_classes_cpu.argtypes = [vp, vp, C.c_uint64, C.POINTER(KrColourClasses)]
    lib.kr_colour_classes_device.argtypes = [C.c_int, vp, vp, C.c_uint64, C.POINTER(KrColourClasses)]
    lib.kr_colour_classes_free.argtypes = [C.POINTER(KrColourClasses)]
    lib.kr_colour_classes_free.restype = None
    rp = ranks.ctypes.data if len(ranks) else None
    if device is None:
        check(lib.kr_colour_classes_cpu(goff.ctypes.data, rp, len(goff) - 1, C.byref(res)))
    else:
        check(lib.kr_colour_classes_device(int(device), goff.ctypes.data, rp, len(goff) - 1, C.byref(res)))
    out = _np(res.class_of, res.nkeys, np.uint32), _np(res.rep, res.nclasses, np.uint64)
    lib.kr_colour_classes_free(C.byref(res))
    return out


def index_stats(view_or_hx, device=None, keep_counts=False, view_flags=KR_VIEW_HOST):
    """The statistics of `krepp inspect`: a list with one dict per library (nkmers, nsubsets, r, frac, mer_value, mer_freq, deg_value,
    deg_freq, and se_count / se_outdeg with keep_counts, else None) from kr_index_stats_cpu (device=None) or _device.
    view_or_hx: a HostIndex or a KrIndexView; view_flags=KR_VIEW_DEVICE: the view's cmer / pse are device pointers."""
    lib = load()
    view = view_or_hx.view if isinstance(view_or_hx, HostIndex) else view_or_hx
    lib.kr_index_stats_cpu.argtypes = [C.POINTER(KrIndexView), C.c_uint32, C.POINTER(KrIndexStats)]
    lib.kr_index_stats_device.argtypes = [C.POINTER(KrIndexView), C.c_int, C.c_uint32, C.POINTER(KrIndexStats)]
    lib.kr_index_stats_free.argtypes = [C.POINTER(KrIndexStats)]
    lib.kr_index_stats_free.restype = None
    flags = int(view_flags) | (KR_STATS_KEEP_COUNTS if keep_counts else 0)
    res = KrIndexStats()
    if device is None:
        check(lib.kr_index_stats_cpu(C.byref(view), flags, C.byref(res)))
    else:
        check(lib.kr_index_stats_device(C.byref(view), int(device), flags, C.byref(res)))
    out = []
    for i in range(res.nlibs):
        L = res.libs[i]
        out.append({"nkmers": int(L.nkmers), "nsubsets": int(L.nsubsets), "r": int(L.r), "frac": int(L.frac),
                    "mer_value": _np(L.mer_value, L.n_mer, np.uint64), "mer_freq": _np(L.mer_freq, L.n_mer, np.uint64),
                    "deg_value": _np(L.deg_value, L.n_deg, np.uint64), "deg_freq": _np(L.deg_freq, L.n_deg, np.uint64),
                    "se_count": _np(L.se_count, L.nsubsets, np.uint64) if L.se_count else None,
                    "se_outdeg": _np(L.se_outdeg, L.nsubsets, np.uint64) if L.se_outdeg else None})
    lib.kr_index_stats_free(C.byref(res))
    return out


def format_inspect(hx, stats):
    """kr_format_inspect: the text of `krepp inspect` for the HostIndex `hx` and what index_stats returned for it (bytes)."""
    lib = load()
    lib.kr_format_inspect.argtypes = [C.c_void_p, C.POINTER(KrIndexStats), C.POINTER(C.c_void_p), u64p]
    arr = (KrLibStats * max(1, len(stats)))()
    keep = []
    for i, d in enumerate(stats):
        cols = [np.ascontiguousarray(d[k_], dtype=np.uint64) for k_ in ("mer_value", "mer_freq", "deg_value", "deg_freq")]
        keep.append(cols)
        arr[i].nkmers, arr[i].nsubsets, arr[i].r, arr[i].frac = d["nkmers"], d["nsubsets"], d["r"], d["frac"]
        arr[i].mer_value, arr[i].mer_freq = C.cast(cols[0].ctypes.data, u64p), C.cast(cols[1].ctypes.data, u64p)
        arr[i].deg_value, arr[i].deg_freq = C.cast(cols[2].ctypes.data, u64p), C.cast(cols[3].ctypes.data, u64p)
        arr[i].n_mer, arr[i].n_deg = len(cols[0]), len(cols[2])
    st = KrIndexStats(nlibs=len(stats), libs=arr)
    text, n = C.c_void_p(), C.c_uint64(0)
    check(lib.kr_format_inspect(hx.h, C.byref(st), C.byref(text), C.byref(n)))
    out = C.string_at(text, n.value)
    lib.kr_free(text)
    return out


def index_stats_debug():
    """kr_debug_index_stats / _ms: the process's last kr_index_stats_device."""
    v, ms = (C.c_uint64 * 8)(), (C.c_float * 4)()
    lib = load()
    lib.kr_debug_index_stats.argtypes = [C.POINTER(C.c_uint64 * 8)]
    lib.kr_debug_index_stats.restype = None
    lib.kr_debug_index_stats_ms.argtypes = [C.POINTER(C.c_float * 4)]
    lib.kr_debug_index_stats_ms.restype = None
    lib.kr_debug_index_stats(C.byref(v))
    lib.kr_debug_index_stats_ms(C.byref(ms))
    return {"path": int(v[0]), "chunks": int(v[1]), "lds": int(v[2]), "global": int(v[3]), "cap": int(v[4]), "passes_mer": int(v[5]),
            "passes_deg": int(v[6]), "run": int(v[7]), "copy_ms": float(ms[0]), "kernel_ms": float(ms[1]), "rest_ms": float(ms[2]),
            "total_ms": float(ms[3])}


def build_colours_stats():
    """kr_debug_build_colours: the process's last kr_colour_classes_device or index build."""
    v = (C.c_uint64 * 8)()
    lib = load()
    lib.kr_debug_build_colours.argtypes = [C.POINTER(C.c_uint64 * 8)]
    lib.kr_debug_build_colours.restype = None
    lib.kr_debug_build_colours(C.byref(v))
    return {"groups": int(v[0]), "multi": int(v[1]), "classes": int(v[2]), "raised": int(v[3]), "path": int(v[4]), "passes": int(v[5])}


def build_index(input_tsv, out_dir, nwk=None, k=29, w=35, h=13, m=4, r=1, frac=True, num_threads=1, seed=0, ppos=None,
                gpu_minimizers=False, device=0, sdust_t=0, sdust_w=0, gpu_keys=False, gpu_colours=False):
    """`krepp index` (reference: src/krepp.cpp:131-303), on the CPU unless gpu_minimizers (the leaf stage on `device`), gpu_keys
    (the key sort and grouping there too; implies the leaf stage) or gpu_colours (the groups' distinct leaf sets found there too,
    each folded into a colour once; implies both).  sdust_t, sdust_w both > 0: --sdust-t/-w masking."""
    lib = load()
    p = KrBuildParams(k=k, w=w, h=h, m=m, r=r, frac=int(frac), num_threads=num_threads, seed=seed, ppos=None,
                      gpu_minimizers=_gpu_build_bits(gpu_minimizers, gpu_keys, gpu_colours), device=device, sdust_t=sdust_t, sdust_w=sdust_w)
    keep = None
    if ppos is not None:
        keep = (C.c_uint8 * len(ppos))(*ppos)
        p.ppos = C.cast(keep, u8p)
    check(lib.kr_build_index(os.fsencode(str(input_tsv)), os.fsencode(str(nwk)) if nwk else None,
                             os.fsencode(str(out_dir)), C.byref(p)))


def build_sketch(input_path, out_path, k=26, w=None, h=None, m=4, r=1, frac=True, seed=0, ppos=None, sdust_t=0, sdust_w=0,
                 gpu_minimizers=False, gpu_keys=False, device=0):
    """`krepp sketch` (reference: src/krepp.cpp:110-129; defaults k 26, w k+6, h k-16); gpu_minimizers / gpu_keys as in build_index."""
    lib = load()
    w = k + 6 if w is None else w
    h = k - 16 if h is None else h
    p = KrBuildParams(k=k, w=w, h=h, m=m, r=r, frac=int(frac), num_threads=1, seed=seed, ppos=None,
                      gpu_minimizers=_gpu_build_bits(gpu_minimizers, gpu_keys), device=device, sdust_t=sdust_t, sdust_w=sdust_w)
    keep = None
    if ppos is not None:
        keep = (C.c_uint8 * len(ppos))(*ppos)
        p.ppos = C.cast(keep, u8p)
    lib.kr_build_sketch.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(KrBuildParams)]
    check(lib.kr_build_sketch(os.fsencode(str(input_path)), os.fsencode(str(out_path)), C.byref(p)))


def minimizers(bases, offsets, k, w, h, ppos, m=4, r=1, frac=True, device=None, sdust_t=0, sdust_w=0):
    """(keys, n1, n2) of one genome: kr_minimizers_cpu (device=None) or kr_minimizers_device."""
    lib = load()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    keep = (C.c_uint8 * len(ppos))(*ppos)
    p = KrBuildParams(k=k, w=w, h=h, m=m, r=r, frac=int(frac), num_threads=1, seed=0, ppos=C.cast(keep, u8p),
                      gpu_minimizers=0, device=0, sdust_t=sdust_t, sdust_w=sdust_w)
    res = KrMinimizerResult()
    if device is None:
        check(lib.kr_minimizers_cpu(C.byref(p), bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1, C.byref(res)))
    else:
        check(lib.kr_minimizers_device(int(device), C.byref(p), bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                       C.byref(res)))
    keys = _np(res.keys, res.nkeys, np.uint64)
    out = (keys, res.n1, res.n2)
    lib.kr_minimizers_free(C.byref(res))
    return out


def sdust(bases, offsets, T, W):
    """Per contig the sdust interval list [(start, finish), ...] (finish exclusive): kr_sdust_cpu."""
    lib = load()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    res = KrSdustResult()
    vp = C.c_void_p
    bp = bases.ctypes.data if len(bases) else (C.c_uint8 * 1)()
    lib.kr_sdust_cpu.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(KrSdustResult)]
    check(lib.kr_sdust_cpu(bp, offsets.ctypes.data, n, T, W, C.byref(res)))
    off = _np(res.offsets, n + 1, np.uint64)
    iv = _np(res.intervals, int(off[-1]), np.uint64)
    out = [[(int(v) >> 32, int(v) & 0xFFFFFFFF) for v in iv[int(off[c]):int(off[c + 1])]] for c in range(n)]
    lib.kr_sdust_free.argtypes = [C.POINTER(KrSdustResult)]
    lib.kr_sdust_free.restype = None
    lib.kr_sdust_free(C.byref(res))
    return out


PLACEMENT_DT = np.dtype([("read", "<u4"), ("edge", "<u4"), ("lwr", "<f8"), ("d_llh", "<f8"), ("v_llh", "<f8"),
                         ("pendant", "<f8"), ("distal", "<f8")])


class Placer:
    """`krepp place` on one GPU: placement tree + device index (uploaded with the tree's node kinds) + stream."""

    def __init__(self, host_index, nwk_text=None, device=0, tabular=False, max_reads=1 << 16, max_bases=None, lineage_text=None,
                 max_records=None, **place_opts):
        """tabular: False/0 jplace, True/1 --tabular, 2 --summarize; lineage_text: -l instead of a Newick tree; max_records: the
        stream's record slots (default: 128 a read)"""
        self.lib = load()
        self.hx = host_index
        self.tabular = tabular
        self.pt = C.c_void_p()
        if lineage_text is not None:
            check(self.lib.kr_place_tree_create_lineage(host_index.h, lineage_text.encode(), C.byref(self.pt)))
        else:
            check(self.lib.kr_place_tree_create(host_index.h, nwk_text.encode() if nwk_text is not None else None, C.byref(self.pt)))
        self.wcount = np.zeros(self.lib.kr_place_tree_nnodes(self.pt) + 1, np.float64)
        self.twcount = C.c_double(0.0)
        view = KrIndexView()
        C.memmove(C.byref(view), C.byref(host_index.view), C.sizeof(view))
        view.node_kind = self.lib.kr_place_tree_kinds(self.pt)
        self.dx = DeviceIndex.from_view(view, device, KR_VIEW_HOST, keep=host_index)
        # options of `place` (filter defaults to on: src/krepp.cpp:593-630)
        self.popts = default_params(no_filter=0, **place_opts)
        front = default_params(hdist_th=self.popts.hdist_th)  # multi, no_filter, no dist-max: every chosen leaf
        self.st = self.dx.stream(params=front, max_reads=max_reads, max_bases=max_bases, max_records=max_reads * 128 if max_records is None else int(max_records))
        self.prev = C.c_int(0)

    def frame(self, which, invocation="", total=0):
        txt, ln = C.c_void_p(), C.c_uint64()
        check(self.lib.kr_place_frame(self.pt, which, int(self.tabular), invocation.encode(), total, C.byref(txt), C.byref(ln)))
        s = C.string_at(txt, ln.value).decode()
        self.lib.kr_free(txt)
        return s

    def place(self, bases, offsets, names, host=False, c_names=None, want_placements=True, keep_text=True, raw_text=False):
        """One batch.  host=False: kr_place_stream (tree aggregation and likelihoods on the device);
        host=True: kr_batch_collect + kr_place_batch (aggregation on the host).  Same output.
        keep_text=False (timing): the library's text and placements are not copied into Python objects -- copying and decoding 70 MB
        of jplace text takes Python longer than the library takes to make it; returns (bytes of text, number of placements).
        raw_text=True: the text as bytes, not decoded (Stream.place_bgzf: BGZF members)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.st.submit(bases, offsets, KR_TAP_ACCS)
        arr = c_names if c_names is not None else (C.c_char_p * len(names))(*[n.encode() for n in names])
        txt, ln, pls, npl = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        if host:
            rv = KrResultView()
            check(self.lib.kr_batch_collect(self.st.h, C.byref(rv)))
            check(self.lib.kr_place_batch(self.hx.h, self.dx.h, self.pt, C.byref(rv), offsets.ctypes.data, arr, C.byref(self.popts),
                                          int(self.tabular), C.byref(self.prev), C.byref(txt), C.byref(ln),
                                          C.byref(pls) if want_placements else None, C.byref(npl) if want_placements else None))
        else:
            check(self.lib.kr_place_stream(self.hx.h, self.dx.h, self.pt, self.st.h, len(offsets) - 1, offsets.ctypes.data, arr,
                                           C.byref(self.popts), int(self.tabular), C.byref(self.prev), C.byref(txt), C.byref(ln),
                                           C.byref(pls) if want_placements else None, C.byref(npl) if want_placements else None))
        if not keep_text:
            if int(self.tabular) == 2:
                check(self.lib.kr_place_summary_add(self.pt, pls, npl.value, self.wcount.ctypes.data, C.byref(self.twcount)))
            self.lib.kr_free(txt)
            self.lib.kr_free(pls)
            return int(ln.value), int(npl.value)
        text = C.string_at(txt, ln.value)
        text = text if raw_text else text.decode()
        pl = (np.frombuffer(C.string_at(pls, npl.value * PLACEMENT_DT.itemsize), dtype=PLACEMENT_DT).copy()
              if npl.value else np.zeros(0, PLACEMENT_DT))
        if int(self.tabular) == 2:
            check(self.lib.kr_place_summary_add(self.pt, pls, npl.value, self.wcount.ctypes.data, C.byref(self.twcount)))
        self.lib.kr_free(txt)
        self.lib.kr_free(pls)
        return text, pl

    def place_parsed(self, raw, fasta=False, flags=0, want_placements=True, at_eof=1, bgzf=None, raw_text=False):
        """One batch given as raw FASTQ (fasta=True: FASTA) bytes: kr_batch_submit_fastq / _fasta with KR_TAP_ACCS | flags on a
        page-locked copy of `raw`, then kr_place_stream_parsed.  The first call runs kr_stream_fastq_enable for chunks of up to
        max(len(raw), 1 MB) bytes.  Returns (text, placements, summary): the accepted prefix of the chunk is placed, and
        summary["consumed"] says where the next submit starts.
        bgzf = (skip, nbytes): `raw` holds whole BGZF members instead and the batch is kr_batch_submit_bgzf's chunk of them."""
        if not getattr(self, "_fq_on", False):
            self.st.fastq_enable(max(len(raw), bgzf[1] if bgzf else 0, 1 << 20))
            if bgzf:
                self.st.bgzf_enable(max(len(raw), 1 << 20))
            self._fq_on = True
        if bgzf:
            summ, _ = self.st.submit_bgzf(raw, bgzf[0], bgzf[1], KR_TAP_ACCS | flags, fasta, at_eof)
            raw_ptr = self.st._raw_out
        else:
            submit = self.st.submit_fasta if fasta else self.st.submit_fastq
            summ = submit(raw, KR_TAP_ACCS | flags, at_eof)
            raw_ptr = self.st._pinned
        txt, ln, pls, npl = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        check(self.lib.kr_place_stream_parsed(self.hx.h, self.dx.h, self.pt, self.st.h, raw_ptr, C.byref(self.popts), int(self.tabular),
                                              C.byref(self.prev), C.byref(txt), C.byref(ln), C.byref(pls) if want_placements else None,
                                              C.byref(npl) if want_placements else None))
        text = C.string_at(txt, ln.value)
        text = text if raw_text else text.decode()
        pl = (np.frombuffer(C.string_at(pls, npl.value * PLACEMENT_DT.itemsize), dtype=PLACEMENT_DT).copy()
              if npl.value else np.zeros(0, PLACEMENT_DT))
        if int(self.tabular) == 2:
            check(self.lib.kr_place_summary_add(self.pt, pls, npl.value, self.wcount.ctypes.data, C.byref(self.twcount)))
        self.lib.kr_free(txt)
        self.lib.kr_free(pls)
        return text, pl, summ

    def summary(self):
        txt, ln = C.c_void_p(), C.c_uint64()
        check(self.lib.kr_place_summary_text(self.pt, self.wcount.ctypes.data, self.twcount, C.byref(txt), C.byref(ln)))
        s = C.string_at(txt, ln.value).decode()
        self.lib.kr_free(txt)
        return s

    def close(self):
        if self.pt:
            self.st.close()
            self.dx.close()
            self.lib.kr_place_tree_free(self.pt)
            self.pt = C.c_void_p()
