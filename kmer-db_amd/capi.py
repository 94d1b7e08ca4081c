"""ctypes declarations for include/kmdb_amd.h and thin numpy-facing wrappers."""
import ctypes as C
import os
import sys

import numpy as np

ABI_VERSION = 8
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class KmdbError(RuntimeError):
    pass


def lib_path():
    return os.path.join(_HERE, "libkmdb_amd.so")


class _View(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("kmer_length", C.c_uint32),
        ("n_samples", C.c_uint64), ("n_patterns", C.c_uint64),
        ("num_kmers", C.c_void_p), ("parent_id", C.c_void_p), ("num_samples", C.c_void_p),
        ("num_local", C.c_void_p), ("last_sample_id", C.c_void_p), ("num_bits", C.c_void_p),
        ("data_offset", C.c_void_p), ("data", C.c_void_p), ("n_data_words", C.c_uint64),
        ("n_buckets", C.c_uint64), ("bucket_offset", C.c_void_p), ("slots", C.c_void_p),
    ]


class _Opts(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("device", C.c_int32), ("shard_index", C.c_uint32),
        ("shard_count", C.c_uint32), ("bubble_size", C.c_uint32), ("flags", C.c_uint32),
        ("stream", C.c_void_p),
    ]


class _Sparse(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("nnz", C.c_uint64), ("row_ptr", C.POINTER(C.c_uint64)),
                ("col", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_uint32)), ("measure", C.POINTER(C.c_double))]


class _CellFilter(C.Structure):
    _fields_ = [("metric", C.c_int32), ("reserved", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


METRICS = ["jaccard", "min", "max", "cosine", "mash", "ani", "ani-shorter", "mash-query", "num-kmers"]


class _Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double),
                ("algorithmic_bytes", C.c_uint64), ("tree_updates", C.c_uint64), ("sum_pairs", C.c_uint64),
                ("device_bytes", C.c_uint64), ("n_segments", C.c_uint64), ("tile_flushes", C.c_uint64),
                ("k1_ms", C.c_double), ("k2_ms", C.c_double), ("n_records", C.c_uint64), ("k0_ms", C.c_double),
                ("k1n_ms", C.c_double), ("k1g_ms", C.c_double), ("upload_ms", C.c_double), ("n_wide", C.c_uint64),
                ("n_chunks", C.c_uint64), ("path", C.c_uint32), ("width", C.c_uint32), ("sized_call", C.c_uint32),
                ("n_joined", C.c_uint32), ("n_patterns", C.c_uint64), ("h2d_bytes", C.c_uint64), ("n_direct", C.c_uint64)]


class _NodeStats(C.Structure):
    _fields_ = [("n_shards", C.c_uint32), ("n_devices", C.c_uint32), ("rccl_version", C.c_int32), ("partition", C.c_uint32),
                ("upload_s", C.c_double), ("plan_s", C.c_double), ("call_ms", C.c_double), ("collective_ms", C.c_double), ("d2h_ms", C.c_double)]


class _NodeDeviceStats(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_shards", C.c_uint32), ("upload_s", C.c_double), ("call_ms", C.c_double), ("collective_ms", C.c_double),
                ("d2h_ms", C.c_double), ("h2d_bytes", C.c_uint64), ("n_patterns", C.c_uint64), ("n_records", C.c_uint64)]


class _SampleStats(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("rows_truncated", C.c_uint64), ("rows_refetched", C.c_uint64), ("d2h_bytes", C.c_uint64),
                ("select_ms", C.c_double), ("triangle_reads", C.c_uint32), ("reserved", C.c_uint32)]


class _Db2dbStats(C.Structure):
    _fields_ = [("tiles", C.c_uint64), ("tiles_touched", C.c_uint64), ("nnz_device", C.c_uint64), ("nnz", C.c_uint64), ("d2h_bytes", C.c_uint64),
                ("compact_ms", C.c_double)]


class _KmerLists(C.Structure):
    _fields_ = [("n_samples", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("kmers", C.POINTER(C.c_uint64))]


class _MinhashStats(C.Structure):
    _fields_ = [("pieces", C.c_uint64), ("bases", C.c_uint64), ("kept", C.c_uint64), ("unique", C.c_uint64), ("scratch_bytes", C.c_uint64),
                ("h2d_ms", C.c_double), ("count_ms", C.c_double), ("scan_ms", C.c_double), ("write_ms", C.c_double), ("sort_ms", C.c_double),
                ("unique_ms", C.c_double)]


class _MinhashLongStats(C.Structure):
    _fields_ = [("long_samples", C.c_uint64), ("sections", C.c_uint64), ("union_words_in", C.c_uint64), ("union_words_out", C.c_uint64),
                ("union_bytes", C.c_uint64), ("peak_bytes", C.c_uint64), ("union_ms", C.c_double)]


class _BuildStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("kmers_added", C.c_uint64), ("distinct_kmers", C.c_uint64), ("patterns", C.c_uint64), ("events", C.c_uint64),
                ("peak_device_bytes", C.c_uint64), ("merge_ms", C.c_double), ("lookup_ms", C.c_double), ("sort_ms", C.c_double), ("group_ms", C.c_double),
                ("encode_ms", C.c_double), ("tables_ms", C.c_double), ("copy_back_ms", C.c_double)]


class _BuildSeedStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("distinct_kmers", C.c_uint64), ("patterns", C.c_uint64), ("events", C.c_uint64), ("slots", C.c_uint64),
                ("h2d_bytes", C.c_uint64), ("upload_ms", C.c_double), ("dict_ms", C.c_double), ("tree_ms", C.c_double), ("decode_ms", C.c_double),
                ("check_ms", C.c_double)]


class _BuildHandoffStats(C.Structure):
    _fields_ = [("patterns", C.c_uint64), ("samples", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("handle_device_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64), ("with_hashtables", C.c_uint32), ("host_image", C.c_uint32), ("encode_ms", C.c_double), ("tables_ms", C.c_double),
                ("fields_ms", C.c_double), ("layout_ms", C.c_double), ("prepare_ms", C.c_double), ("copy_back_ms", C.c_double), ("total_ms", C.c_double)]


class _DistanceOpts(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("measure", C.c_int32), ("kmer_length", C.c_uint32), ("counts", C.c_void_p),
                ("n", C.c_uint64), ("filters", C.c_void_p), ("n_filters", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("stream", C.c_void_p)]


class _DistanceOut(C.Structure):
    _fields_ = [("text", C.c_void_p), ("len", C.c_size_t), ("rows", C.c_uint64)]


class _DistanceStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("rows", C.c_uint64), ("cells_read", C.c_uint64), ("cells_written", C.c_uint64), ("host_cells", C.c_uint64),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("device_bytes", C.c_uint64), ("parse_ms", C.c_double), ("measure_ms", C.c_double),
                ("format_ms", C.c_double), ("copy_ms", C.c_double)]


class _DistancePartsStats(C.Structure):
    _fields_ = [("block_rows", C.c_uint64), ("grid_cells", C.c_uint64), ("cells_in", C.c_uint64), ("cells_written", C.c_uint64), ("host_cells", C.c_uint64),
                ("peak_bytes", C.c_uint64), ("gather_ms", C.c_double)]


class _All2allRowsStats(C.Structure):
    _fields_ = [("nodes_selected", C.c_uint64), ("nodes_applied", C.c_uint64), ("updates", C.c_uint64), ("band_cells", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("select_ms", C.c_double), ("apply_ms", C.c_double)]


class _All2allRowsTiledStats(C.Structure):
    _fields_ = [("nodes_selected", C.c_uint64), ("nodes_applied", C.c_uint64), ("hits", C.c_uint64), ("jobs", C.c_uint64), ("runs", C.c_uint64),
                ("updates", C.c_uint64), ("tile_cols", C.c_uint64), ("band_cells", C.c_uint64), ("select_ms", C.c_double), ("hits_ms", C.c_double),
                ("apply_ms", C.c_double), ("scratch_bytes", C.c_uint64)]


class _All2allBandedStats(C.Structure):
    _fields_ = [("bands", C.c_uint64), ("max_band_bytes", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("hits", C.c_uint64), ("runs", C.c_uint64),
                ("updates", C.c_uint64), ("select_ms", C.c_double), ("hits_ms", C.c_double), ("apply_ms", C.c_double)]


class _All2allRowsRecordsStats(C.Structure):
    _fields_ = [("path", C.c_uint32), ("width", C.c_uint32), ("x_lo", C.c_uint32), ("x_hi", C.c_uint32), ("sized_call", C.c_uint32), ("slices", C.c_uint32),
                ("band_cells", C.c_uint64), ("records", C.c_uint64), ("units_total", C.c_uint64), ("units_run", C.c_uint64),
                ("jobs_total", C.c_uint64), ("jobs_run", C.c_uint64), ("runs_total", C.c_uint64), ("runs_run", C.c_uint64),
                ("slices_total", C.c_uint64), ("slices_run", C.c_uint64), ("tiles_total", C.c_uint64), ("tiles_run", C.c_uint64),
                ("k0_ms", C.c_double), ("k1n_ms", C.c_double), ("k1g_ms", C.c_double), ("k2_ms", C.c_double), ("kernel_ms", C.c_double),
                ("peak_device_bytes", C.c_uint64)]


class _All2allBandedRecordsStats(C.Structure):
    _fields_ = [("bands", C.c_uint64), ("units_total", C.c_uint64), ("units_run", C.c_uint64), ("ms", C.c_double)]


class _BandGeometry(C.Structure):
    _fields_ = [("x_lo", C.c_uint32), ("x_hi", C.c_uint32), ("n_rows", C.c_uint32), ("fits", C.c_uint32), ("n_streams", C.c_uint64), ("stream_base", C.c_uint64)]


class _All2allRowsBandEmitStats(C.Structure):
    _fields_ = [("form", C.c_uint32), ("x_lo", C.c_uint32), ("x_hi", C.c_uint32), ("n_rows", C.c_uint32), ("key_bits", C.c_uint32), ("row_mode", C.c_uint32),
                ("l2_on", C.c_uint32), ("attempts", C.c_uint32), ("n_streams", C.c_uint64), ("stream_base", C.c_uint64), ("records", C.c_uint64),
                ("est_records", C.c_uint64), ("state_bytes", C.c_uint64), ("whole_state_bytes", C.c_uint64)]


class _New2allSparseStats(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("nnz_device", C.c_uint64), ("nnz", C.c_uint64), ("d2h_bytes", C.c_uint64), ("compact_ms", C.c_double)]


FLAG_FORCE_GLOBAL_ATOMICS = 1
FLAG_FORCE_DIRECT = 2
FLAG_FORCE_TILE = 4
FLAG_NO_FALLBACK = 8
FLAG_ONE_SHOT = 16
DISTANCE_SPARSE_OUT, DISTANCE_SPARSE_IN, DISTANCE_TRIANGLE, DISTANCE_PHYLIP = 1, 2, 4, 8
DISTANCE_DECLINED = 2
PATH_NONE, PATH_RECORDS, PATH_TILE, PATH_GLOBAL = 0, 1, 2, 3
ROWS_RECORDS_PATH_NONE, ROWS_RECORDS_PATH_RECORDS, ROWS_RECORDS_PATH_TREE = 0, 1, 2      # kmdb_all2all_rows_records_stats.path
BAND_PATHS = ("tiled", "tree", "records")              # KMDB_BAND_PATH_*
BAND_EMIT_FORM_NONE, BAND_EMIT_FORM_WHOLE, BAND_EMIT_FORM_BAND = 0, 1, 2      # kmdb_all2all_rows_band_emit_stats.form
PARTITIONS = ("prefix", "range", "prefix-tables")      # KMDB_PARTITION_*

# every symbol include/kmdb_amd.h declares
EXPORTS = [
    "kmdb_last_error", "kmdb_abi_version", "kmdb_device_count", "kmdb_device_prepare", "kmdb_db_upload", "kmdb_db_upload_shard", "kmdb_db_upload_range", "kmdb_db_upload_query_shard", "kmdb_db_free", "kmdb_db_settle", "kmdb_db_stats", "kmdb_db_fallback_reason",
    "kmdb_node_upload", "kmdb_node_upload_partition", "kmdb_node_free", "kmdb_node_stats_get", "kmdb_node_device_stats_get", "kmdb_node_all2all_dense", "kmdb_node_all2all_sparse",
    "kmdb_node_new2all_batch", "kmdb_node_new2all_batch_seq_alphabet", "kmdb_node_new2all_batch_sparse", "kmdb_new2all_batch_device", "kmdb_new2all_batch_seq_alphabet_device",
    "kmdb_all2all_dense", "kmdb_all2all_dense_device", "kmdb_all2all_sparse", "kmdb_all2all_sparse_filtered", "kmdb_sparse_from_dense_device", "kmdbh_metric", "kmdbh_metric_id", "kmdb_sparse_free",
    "kmdb_new2all_batch", "kmdb_new2all_batch_sparse", "kmdb_new2all_batch_seq", "kmdb_new2all_batch_seq_alphabet", "kmdb_db2db_dense",
    "kmdbh_shard_plan_counts", "kmdbh_query_shard_plan_counts", "kmdbh_query_shard_runs", "kmdbh_range_plan", "kmdbh_db_load", "kmdbh_db_free", "kmdbh_db_release_patterns", "kmdbh_db_view", "kmdbh_db_kmer_length", "kmdbh_db_fraction",
    "kmdbh_db_start_fraction", "kmdbh_db_alphabet", "kmdbh_db_n_samples", "kmdbh_db_sample_name",
    "kmdbh_db_sample_kmers", "kmdbh_db_pattern_section_bytes", "kmdbh_extract_kmers", "kmdbh_extract_kmers_alphabet", "kmdbh_alphabet_table", "kmdbh_sort_unique", "kmdbh_minhash_window",
    "kmdbh_format_header", "kmdbh_format_dense_row", "kmdbh_format_sparse_row",
    "kmdb_all2all_sampled", "kmdb_sampled_from_dense_device", "kmdb_node_all2all_sampled", "kmdb_db_sample_stats", "kmdbh_sample_rows_select",
    "kmdb_db2db_sparse_filtered", "kmdb_db2db_stats_get",
    "kmdb_db2db_sampled", "kmdb_sampled_from_rect_device", "kmdb_db2db_sample_stats_get",
    "kmdb_new2all_batch_sampled", "kmdb_new2all_batch_seq_alphabet_sampled", "kmdb_sampled_from_rows_device", "kmdbh_query_rows_select", "kmdb_new2all_sample_stats_get",
    "kmdb_node_new2all_batch_sampled", "kmdb_node_new2all_batch_seq_alphabet_sampled", "kmdb_node_new2all_sample_stats_get",
    "kmdb_new2all_batch_sparse_filtered", "kmdb_new2all_batch_seq_alphabet_sparse_filtered", "kmdb_new2all_rows_sparse_device", "kmdb_new2all_sparse_stats_get",
    "kmdb_node_new2all_batch_sparse_filtered", "kmdb_node_new2all_batch_seq_alphabet_sparse_filtered", "kmdb_node_new2all_sparse_stats_get",
    "kmdb_minhash_batch_seq_alphabet", "kmdb_kmer_lists_free", "kmdb_minhash_geometry", "kmdb_minhash_stats_get", "kmdbh_minhash_store", "kmdbh_minhash_load", "kmdbh_minhash_free",
    "kmdb_minhash_long_stats_get", "kmdb_sorted_union_device", "kmdb_sorted_union_geometry",
    "kmdb_build_begin", "kmdb_build_add_kmers", "kmdb_build_add_seq_alphabet", "kmdb_build_finish", "kmdb_build_free", "kmdb_build_stats_get", "kmdbh_db_store",
    "kmdb_build_begin_from_db", "kmdb_build_seed_stats_get",
    "kmdb_build_finish_device", "kmdb_build_handoff_stats_get", "kmdbh_db_header_only",
    "kmdb_distance_begin", "kmdb_distance_rows", "kmdb_distance_out_free", "kmdb_distance_free", "kmdb_distance_stats_get", "kmdbh_format_measure",
    "kmdb_distance_take_all2all", "kmdb_distance_take_cells_device", "kmdb_distance_matrix_rows", "kmdb_distance_cells_device",
    "kmdb_distance_take_new2all_batch", "kmdb_distance_take_new2all_batch_seq_alphabet", "kmdb_distance_take_rows_device", "kmdb_distance_query_rows",
    "kmdb_distance_parts_begin_rows", "kmdb_distance_parts_add_db2db", "kmdb_distance_parts_add_all2all", "kmdb_distance_parts_add_csr_device", "kmdb_distance_take_csr_device", "kmdb_distance_csr_rows",
    "kmdb_distance_csr_device", "kmdb_distance_csr_row_ptr", "kmdb_distance_parts_stats_get",
    "kmdb_all2all_rows_device", "kmdb_all2all_rows", "kmdb_all2all_rows_stats_get", "kmdb_device_buffer_alloc", "kmdb_device_buffer_free",
    "kmdb_all2all_rows_tiled_device", "kmdb_all2all_rows_tiled", "kmdb_all2all_rows_tiled_stats_get", "kmdb_all2all_sparse_filtered_banded", "kmdb_all2all_banded_stats_get",
    "kmdb_all2all_rows_records_device", "kmdb_all2all_rows_records", "kmdb_all2all_rows_records_stats_get", "kmdb_all2all_sparse_filtered_banded_path",
    "kmdb_all2all_banded_records_stats_get",
    "kmdb_all2all_rows_band_emit_stats_get", "kmdbh_band_streams",
]


def lib():
    """Load libkmdb_amd.so; never falls back to anything else."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise KmdbError("libkmdb_amd.so is not built (run __graft_entry__.build() or `make -C kmer-db_amd`)")
    # torch ships its own copy of the HIP runtime; if the process is going to use torch as well (device
    # buffers for the RCCL reduce), it has to be the first one loaded or torch finds no device afterwards
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(p)
    L.kmdb_last_error.restype = C.c_char_p
    L.kmdb_db_upload.argtypes = [C.POINTER(_View), C.POINTER(_Opts), C.c_int, C.POINTER(C.c_void_p)]
    L.kmdb_db_upload_shard.argtypes = [C.POINTER(_View), C.POINTER(_Opts), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.kmdb_db_upload_range.argtypes = [C.POINTER(_View), C.POINTER(_Opts), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.kmdb_db_upload_query_shard.argtypes = [C.POINTER(_View), C.POINTER(_Opts), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.kmdb_new2all_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_new2all_batch_seq_alphabet_device.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                         C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_node_new2all_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_node_new2all_batch_sparse.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_node_new2all_batch_seq_alphabet.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                       C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdbh_query_shard_plan_counts.argtypes = [C.POINTER(_View), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmdbh_query_shard_runs.restype = C.c_size_t
    L.kmdbh_query_shard_runs.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t]
    L.kmdb_db_free.argtypes = [C.c_void_p]
    L.kmdb_db_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
    L.kmdb_db_fallback_reason.argtypes = [C.c_void_p]
    L.kmdb_db_fallback_reason.restype = C.c_char_p
    L.kmdb_node_upload.argtypes = [C.POINTER(_View), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]
    L.kmdb_node_upload_partition.argtypes = [C.POINTER(_View), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
    L.kmdbh_range_plan.argtypes = [C.POINTER(_View), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kmdb_node_free.argtypes = [C.c_void_p]
    L.kmdb_node_stats_get.argtypes = [C.c_void_p, C.POINTER(_NodeStats)]
    L.kmdb_node_device_stats_get.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(_NodeDeviceStats)]
    L.kmdb_node_all2all_dense.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_node_all2all_sparse.argtypes = [C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_all2all_dense.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_dense_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allRowsStats)]
    L.kmdb_all2all_rows_tiled_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_tiled.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_tiled_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allRowsTiledStats)]
    L.kmdb_all2all_sparse_filtered_banded.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_all2all_banded_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allBandedStats)]
    L.kmdb_all2all_rows_records_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_records.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_all2all_rows_records_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allRowsRecordsStats)]
    L.kmdb_all2all_sparse_filtered_banded_path.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(_Sparse),
                                                           C.POINTER(_Opts)]
    L.kmdb_all2all_banded_records_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allBandedRecordsStats)]
    L.kmdb_all2all_rows_band_emit_stats_get.argtypes = [C.c_void_p, C.POINTER(_All2allRowsBandEmitStats)]
    L.kmdbh_band_streams.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(_BandGeometry)]
    L.kmdb_device_buffer_alloc.argtypes = [C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]
    L.kmdb_device_buffer_free.restype = None
    L.kmdb_device_buffer_free.argtypes = [C.c_int32, C.c_void_p]
    L.kmdb_all2all_sparse.argtypes = [C.c_void_p, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_all2all_sparse_filtered.argtypes = [C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_sparse_from_dense_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int,
                                                C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_all2all_sampled.argtypes = [C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_sampled_from_dense_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.c_uint32,
                                                 C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_node_all2all_sampled.argtypes = [C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_db_sample_stats.argtypes = [C.c_void_p, C.POINTER(_SampleStats)]
    L.kmdbh_sample_rows_select.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.POINTER(C.POINTER(_Sparse)), C.c_size_t,
                                           C.POINTER(_Sparse)]
    L.kmdbh_metric.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.kmdbh_metric.restype = C.c_double
    L.kmdbh_metric_id.argtypes = [C.c_char_p]
    L.kmdb_sparse_free.argtypes = [C.POINTER(_Sparse)]
    L.kmdb_new2all_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_new2all_batch_sparse.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_db2db_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_db2db_sparse_filtered.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(_Sparse),
                                             C.POINTER(_Opts)]
    L.kmdb_db2db_stats_get.argtypes = [C.c_void_p, C.POINTER(_Db2dbStats)]
    L.kmdb_db2db_sampled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse),
                                     C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_sampled_from_rect_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_db2db_sample_stats_get.argtypes = [C.c_void_p, C.POINTER(_SampleStats)]
    L.kmdb_node_new2all_batch_sampled.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p,
                                                  C.c_int, C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_node_new2all_batch_seq_alphabet_sampled.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                               C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse), C.c_void_p,
                                                               C.POINTER(_Opts)]
    L.kmdb_node_new2all_sample_stats_get.argtypes = [C.c_void_p, C.POINTER(_SampleStats)]
    L.kmdb_new2all_batch_sampled.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int,
                                             C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_new2all_batch_seq_alphabet_sampled.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                          C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse), C.c_void_p,
                                                          C.POINTER(_Opts)]
    L.kmdb_sampled_from_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t,
                                                C.c_void_p, C.c_int, C.c_uint32, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdbh_query_rows_select.argtypes = [C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t,
                                          C.POINTER(C.POINTER(_Sparse)), C.c_size_t, C.POINTER(_Sparse)]
    L.kmdb_new2all_sample_stats_get.argtypes = [C.c_void_p, C.POINTER(_SampleStats)]
    for name in ("kmdb_new2all_batch_sparse_filtered", "kmdb_node_new2all_batch_sparse_filtered"):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p, C.c_int,
                                     C.POINTER(_Sparse), C.POINTER(_Opts)]
    for name in ("kmdb_new2all_batch_seq_alphabet_sparse_filtered", "kmdb_node_new2all_batch_seq_alphabet_sparse_filtered"):
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32, C.POINTER(_CellFilter),
                                     C.c_size_t, C.c_void_p, C.c_int, C.POINTER(_Sparse), C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_new2all_rows_sparse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(_CellFilter), C.c_size_t, C.c_void_p,
                                                  C.c_int, C.POINTER(_Sparse), C.POINTER(_Opts)]
    L.kmdb_new2all_sparse_stats_get.argtypes = [C.c_void_p, C.POINTER(_New2allSparseStats)]
    L.kmdb_node_new2all_sparse_stats_get.argtypes = [C.c_void_p, C.POINTER(_New2allSparseStats)]
    L.kmdb_new2all_batch_seq.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int,
                                         C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_new2all_batch_seq_alphabet.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.POINTER(_Opts)]
    L.kmdbh_db_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.kmdbh_db_free.argtypes = [C.c_void_p]
    L.kmdbh_db_release_patterns.argtypes = [C.c_void_p]
    L.kmdbh_db_release_patterns.restype = None
    L.kmdbh_db_view.restype = C.POINTER(_View)
    L.kmdbh_db_view.argtypes = [C.c_void_p]
    L.kmdbh_db_kmer_length.restype = C.c_uint32
    L.kmdbh_db_kmer_length.argtypes = [C.c_void_p]
    L.kmdbh_db_fraction.restype = C.c_double
    L.kmdbh_db_fraction.argtypes = [C.c_void_p]
    L.kmdbh_db_start_fraction.restype = C.c_double
    L.kmdbh_db_start_fraction.argtypes = [C.c_void_p]
    L.kmdbh_db_alphabet.restype = C.c_int32
    L.kmdbh_db_alphabet.argtypes = [C.c_void_p]
    L.kmdbh_db_n_samples.restype = C.c_uint64
    L.kmdbh_db_n_samples.argtypes = [C.c_void_p]
    L.kmdbh_db_sample_name.restype = C.c_char_p
    L.kmdbh_db_sample_name.argtypes = [C.c_void_p, C.c_uint64]
    L.kmdbh_db_sample_kmers.restype = C.c_uint64
    L.kmdbh_db_sample_kmers.argtypes = [C.c_void_p, C.c_uint64]
    L.kmdbh_db_pattern_section_bytes.restype = C.c_uint64
    L.kmdbh_db_pattern_section_bytes.argtypes = [C.c_void_p]
    L.kmdbh_extract_kmers.restype = C.c_size_t
    L.kmdbh_extract_kmers.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.kmdbh_extract_kmers_alphabet.restype = C.c_size_t
    L.kmdbh_extract_kmers_alphabet.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_double, C.c_double, C.c_void_p]
    L.kmdbh_alphabet_table.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    L.kmdbh_minhash_window.restype = None
    L.kmdbh_minhash_window.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.kmdbh_sort_unique.restype = C.c_size_t
    L.kmdbh_sort_unique.argtypes = [C.c_void_p, C.c_size_t]
    L.kmdb_minhash_batch_seq_alphabet.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_double, C.c_double, C.c_int32, C.POINTER(_KmerLists), C.c_void_p]
    L.kmdb_kmer_lists_free.restype = None
    L.kmdb_kmer_lists_free.argtypes = [C.POINTER(_KmerLists)]
    L.kmdb_minhash_geometry.restype = None
    L.kmdb_minhash_geometry.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.kmdb_minhash_stats_get.argtypes = [C.POINTER(_MinhashStats)]
    L.kmdb_minhash_long_stats_get.argtypes = [C.POINTER(_MinhashLongStats)]
    L.kmdb_sorted_union_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    L.kmdb_sorted_union_geometry.restype = None
    L.kmdb_sorted_union_geometry.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.kmdbh_minhash_store.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_double]
    L.kmdbh_minhash_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.kmdbh_minhash_free.restype = None
    L.kmdbh_minhash_free.argtypes = [C.POINTER(C.c_uint64)]
    L.kmdb_build_begin.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.kmdb_build_add_kmers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.kmdb_build_add_seq_alphabet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.kmdb_build_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.kmdb_build_finish_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.kmdb_build_handoff_stats_get.argtypes = [C.c_void_p, C.POINTER(_BuildHandoffStats)]
    L.kmdbh_db_header_only.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.kmdb_build_free.restype = None
    L.kmdb_build_free.argtypes = [C.c_void_p]
    L.kmdb_build_stats_get.argtypes = [C.c_void_p, C.POINTER(_BuildStats)]
    L.kmdb_build_begin_from_db.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.kmdb_build_seed_stats_get.argtypes = [C.c_void_p, C.POINTER(_BuildSeedStats)]
    L.kmdbh_db_store.argtypes = [C.c_void_p, C.c_char_p]
    L.kmdb_distance_begin.argtypes = [C.POINTER(_DistanceOpts), C.POINTER(C.c_void_p)]
    L.kmdb_distance_rows.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(_DistanceOut)]
    L.kmdb_distance_take_all2all.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(_Opts)]
    L.kmdb_distance_take_cells_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p)]
    L.kmdb_distance_matrix_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_DistanceOut)]
    L.kmdb_distance_take_new2all_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(_Opts)]
    L.kmdb_distance_take_new2all_batch_seq_alphabet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_int32,
                                                                C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(_Opts)]
    L.kmdb_distance_take_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_char_p)]
    L.kmdb_distance_query_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_DistanceOut)]
    L.kmdb_distance_parts_begin_rows.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_char_p)]
    L.kmdb_distance_parts_add_db2db.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(_Opts)]
    L.kmdb_distance_parts_add_all2all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(_Opts)]
    L.kmdb_distance_parts_add_csr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
    L.kmdb_distance_take_csr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_char_p)]
    L.kmdb_distance_csr_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(_DistanceOut)]
    L.kmdb_distance_csr_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.kmdb_distance_csr_row_ptr.argtypes = [C.c_void_p, C.c_void_p]
    L.kmdb_distance_parts_stats_get.argtypes = [C.c_void_p, C.POINTER(_DistancePartsStats)]
    L.kmdb_distance_cells_device.restype = C.c_void_p
    L.kmdb_distance_cells_device.argtypes = [C.c_void_p]
    L.kmdb_distance_out_free.restype = None
    L.kmdb_distance_out_free.argtypes = [C.POINTER(_DistanceOut)]
    L.kmdb_distance_free.restype = None
    L.kmdb_distance_free.argtypes = [C.c_void_p]
    L.kmdb_distance_stats_get.argtypes = [C.c_void_p, C.POINTER(_DistanceStats)]
    L.kmdbh_format_measure.restype = C.c_size_t
    L.kmdbh_format_measure.argtypes = [C.c_double, C.c_char_p]
    L.kmdbh_format_header.restype = C.c_size_t
    L.kmdbh_format_header.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.kmdbh_format_dense_row.restype = C.c_size_t
    L.kmdbh_format_dense_row.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_char_p]
    L.kmdbh_format_sparse_row.restype = C.c_size_t
    L.kmdbh_format_sparse_row.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p]
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise KmdbError(lib().kmdb_last_error().decode(errors="replace"))


def device_count():
    return int(lib().kmdb_device_count())


def _opts(device=0, shard=(0, 1), flags=0, stream=None, bubble=0):
    o = _Opts()
    o.abi_version = ABI_VERSION
    o.device = device
    o.shard_index, o.shard_count = shard
    o.bubble_size = bubble
    o.flags = flags
    o.stream = stream
    return o


# ------------------------------------------------------------------------------------------------
class HostDB:
    """A .db file parsed by the front-end's reader (kmdbh_db_load)."""

    def __init__(self, path, skip_hashtables=False, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:                    # a database made in memory (Builder.finish): the object owns the handle
            self._h = _handle
        else:
            _check(lib().kmdbh_db_load(os.fsencode(path), 2 if skip_hashtables else 0, C.byref(self._h)))
        L = lib()
        self.N = int(L.kmdbh_db_n_samples(self._h))
        self.k = int(L.kmdbh_db_kmer_length(self._h))
        self.fraction = float(L.kmdbh_db_fraction(self._h))
        self.start_fraction = float(L.kmdbh_db_start_fraction(self._h))
        self.alphabet = int(L.kmdbh_db_alphabet(self._h))
        self.names = [L.kmdbh_db_sample_name(self._h, i).decode() for i in range(self.N)]
        self.sample_kmers = np.array([L.kmdbh_db_sample_kmers(self._h, i) for i in range(self.N)], dtype=np.uint64)
        self.pattern_section_bytes = int(L.kmdbh_db_pattern_section_bytes(self._h))

    @property
    def view(self):
        return lib().kmdbh_db_view(self._h)

    def shard_plan_counts(self, n_shards):
        """kmdbh_shard_plan_counts: (nodes kept, k-mers owned) per prefix shard, planned on the host"""
        kept = np.zeros(n_shards, np.uint64)
        kmers = np.zeros(n_shards, np.uint64)
        L = lib()
        L.kmdbh_shard_plan_counts.argtypes = [C.POINTER(_View), C.c_uint32, C.c_void_p, C.c_void_p]
        _check(L.kmdbh_shard_plan_counts(self.view, n_shards, kept.ctypes.data, kmers.ctypes.data))
        return kept, kmers

    def query_shard_plan_counts(self, n_shards):
        """kmdbh_query_shard_plan_counts: (nodes kept, k-mers owned, slots, buckets) per query shard, planned on the host"""
        out = [np.zeros(n_shards, np.uint64) for _ in range(4)]
        _check(lib().kmdbh_query_shard_plan_counts(self.view, n_shards, *[a.ctypes.data for a in out]))
        return tuple(out)

    def range_plan(self, n_ranges):
        """kmdbh_range_plan: the tree ranges of the database, planned on the host without the hashtables — a dict of
        kept / own / cost / first_depth per range and range_of per pattern"""
        return range_plan(self.view, n_ranges)

    def release_patterns(self):
        """kmdbh_db_release_patterns: the pattern arrays' pages go back to the kernel (after the upload); names and counts stay"""
        lib().kmdbh_db_release_patterns(self._h)

    def view_arrays(self):
        """numpy copies of the flat view (for tests of the reader)."""
        v = self.view.contents
        P = int(v.n_patterns)

        def arr(ptr, n, dt):
            if not ptr or n == 0:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dt).itemsize,)).view(dt).copy()

        out = {
            "num_kmers": arr(v.num_kmers, P, np.int64), "parent_id": arr(v.parent_id, P, np.int64),
            "num_samples": arr(v.num_samples, P, np.uint32), "num_local": arr(v.num_local, P, np.uint32),
            "last_sample_id": arr(v.last_sample_id, P, np.uint32), "num_bits": arr(v.num_bits, P, np.uint32),
            "data_offset": arr(v.data_offset, P, np.uint64), "data": arr(v.data, int(v.n_data_words), np.uint64),
            "n_buckets": int(v.n_buckets),
        }
        if v.n_buckets:
            out["bucket_offset"] = arr(v.bucket_offset, int(v.n_buckets) + 1, np.uint64)
            out["slots"] = arr(v.slots, int(out["bucket_offset"][-1]), np.uint64)
        return out

    def header_only(self):
        """kmdbh_db_header_only: names, counts, k, fractions and alphabet alone — the image Builder.finish_device returns without host_image"""
        h = C.c_void_p()
        _check(lib().kmdbh_db_header_only(self._h, C.byref(h)))
        return HostDB(None, _handle=h)

    def store(self, path):
        """kmdbh_db_store: the file PrefixKmerDb::serialize(file, true) writes; the database must hold its tables"""
        _check(lib().kmdbh_db_store(self._h, os.fsencode(path)))

    def header_bytes(self):
        buf = C.create_string_buffer(20000 + 200 * self.N + sum(len(n) for n in self.names))
        n = lib().kmdbh_format_header(self._h, buf, len(buf))
        return buf.raw[:n]

    def close(self):
        if self._h:
            lib().kmdbh_db_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def range_plan(view, n_ranges):
    """kmdbh_range_plan on a view (HostDB.view, or C.pointer(view) of make_view's)"""
    R = max(int(n_ranges), 0)
    out = {"kept": np.zeros(max(R, 1), np.uint64), "own": np.zeros(max(R, 1), np.uint64), "cost": np.zeros(max(R, 1), np.uint64),
           "range_of": np.zeros(max(int(view.contents.n_patterns), 1), np.uint32), "first_depth": np.zeros(max(R, 1), np.uint32)}
    _check(lib().kmdbh_range_plan(view, int(n_ranges), out["kept"].ctypes.data, out["own"].ctypes.data, out["cost"].ctypes.data,
                                  out["range_of"].ctypes.data, out["first_depth"].ctypes.data))
    out["range_of"] = out["range_of"][: int(view.contents.n_patterns)]
    return {k: (a if k == "range_of" else a[:R]) for k, a in out.items()}


def query_shard_runs(kmers, n_shards, shard):
    """kmdbh_query_shard_runs: the (begin, end) stretches of a sorted query that query shard `shard` of n_shards owns"""
    a = np.ascontiguousarray(kmers, np.uint64)
    n = int(lib().kmdbh_query_shard_runs(a.ctypes.data, a.size, int(n_shards), int(shard), None, None, 0))
    b = np.zeros(max(n, 1), np.uint64)
    e = np.zeros(max(n, 1), np.uint64)
    lib().kmdbh_query_shard_runs(a.ctypes.data, a.size, int(n_shards), int(shard), b.ctypes.data, e.ctypes.data, n)
    return [(int(x), int(y)) for x, y in zip(b[:n], e[:n])]


def make_view(kmer_length, n_samples, num_kmers, parent_id, num_samples, num_local, last_sample_id, num_bits,
              data_offset, data, bucket_offset=None, slots=None):
    """Build a kmdb_db_view over caller-owned numpy arrays; returns (view, keepalive)."""
    keep = [np.ascontiguousarray(num_kmers, np.int64), np.ascontiguousarray(parent_id, np.int64),
            np.ascontiguousarray(num_samples, np.uint32), np.ascontiguousarray(num_local, np.uint32),
            np.ascontiguousarray(last_sample_id, np.uint32), np.ascontiguousarray(num_bits, np.uint32),
            np.ascontiguousarray(data_offset, np.uint64), np.ascontiguousarray(data, np.uint64)]
    v = _View()
    v.abi_version = ABI_VERSION
    v.kmer_length = kmer_length
    v.n_samples = n_samples
    v.n_patterns = keep[0].size
    (v.num_kmers, v.parent_id, v.num_samples, v.num_local, v.last_sample_id, v.num_bits, v.data_offset, v.data) = [
        a.ctypes.data for a in keep]
    v.n_data_words = keep[7].size
    if bucket_offset is not None:
        bo = np.ascontiguousarray(bucket_offset, np.uint64)
        sl = np.ascontiguousarray(slots, np.uint64)
        keep += [bo, sl]
        v.n_buckets = bo.size - 1
        v.bucket_offset = bo.ctypes.data
        v.slots = sl.ctypes.data
    return v, keep


def _filters(filters):
    """[(criterion name, lo, hi)], None = unbounded -> a kmdb_cell_filter array"""
    fs = (_CellFilter * max(1, len(filters)))()
    for i, (name, lo, hi) in enumerate(filters):
        fs[i].metric = METRICS.index(name)
        fs[i].lo = -np.finfo(np.float64).max if lo is None else lo
        fs[i].hi = np.finfo(np.float64).max if hi is None else hi
    return fs


def _criterion(criterion):
    """a criterion name, or the raw KMDB_METRIC_* number (passed on unchecked: the library refuses what it does not know)"""
    return METRICS.index(criterion) if isinstance(criterion, str) else int(criterion)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _kmer_queries(queries):
    """sorted unique k-mer arrays -> (keepalive, pointer array, count array, nq)"""
    qs = [np.ascontiguousarray(q, np.uint64) for q in queries]
    nq = len(qs)
    return qs, (C.c_void_p * max(nq, 1))(*[q.ctypes.data for q in qs]), (C.c_size_t * max(nq, 1))(*[q.size for q in qs]), nq


def _text_queries(seqs):
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    nq = len(bs)
    return bs, (C.c_char_p * max(nq, 1))(*bs), (C.c_size_t * max(nq, 1))(*[len(b) for b in bs]), nq


def _sample_texts(seqs):
    """the texts of minhash_batch / Builder.add_seqs -> (keepalive, pointer array, length array, n).  bytes are passed as they are; a bytearray,
    a memoryview or a uint8 array — a text of gigabytes — is passed by its address, without a copy"""
    keep, ptrs, lens = [], [], []
    for s in seqs:
        if isinstance(s, str):
            s = s.encode()
        if isinstance(s, bytes):
            keep.append(s)
            ptrs.append(C.cast(C.c_char_p(s), C.c_void_p).value or 0)
            lens.append(len(s))
        else:
            a = np.frombuffer(s, np.uint8) if not isinstance(s, np.ndarray) else np.ascontiguousarray(s).view(np.uint8).reshape(-1)
            keep.append((s, a))
            ptrs.append(a.ctypes.data if a.size else 0)
            lens.append(a.size)
    n = len(keep)
    return keep, (C.c_void_p * max(n, 1))(*ptrs), (C.c_size_t * max(n, 1))(*lens), n


def _stats_dict(fn, Struct, *args):
    """the Struct that the getter fn(*args, pointer to it) fills, as a dict of its fields (a "reserved" field left out)"""
    s = Struct()
    _check(fn(*args, C.byref(s)))
    return {f: getattr(s, f) for f, _ in Struct._fields_ if f != "reserved"}


def _rows_out(raw):
    try:
        return SparseRows(raw)
    finally:
        lib().kmdb_sparse_free(C.byref(raw))


class SparseRows:
    def __init__(self, raw):
        n, nnz = int(raw.n_rows), int(raw.nnz)
        self.row_ptr = np.ctypeslib.as_array(raw.row_ptr, shape=(n + 1,)).copy()
        self.col = np.ctypeslib.as_array(raw.col, shape=(max(nnz, 1),))[:nnz].copy()
        self.val = np.ctypeslib.as_array(raw.val, shape=(max(nnz, 1),))[:nnz].copy()
        self.n_rows, self.nnz = n, nnz
        self.measure = np.ctypeslib.as_array(raw.measure, shape=(max(nnz, 1),))[:nnz].copy() if raw.measure else None

    def row(self, i):
        a, b = int(self.row_ptr[i]), int(self.row_ptr[i + 1])
        return self.col[a:b], self.val[a:b]


def band_streams(n_samples, width, row_lo, row_hi):
    """kmdbh_band_streams (host only, no GPU): the geometry of the band [row_lo, row_hi) in the block-record pipeline's streams at block width `width`
    as a dict of kmdb_band_geometry's fields"""
    return _stats_dict(lib().kmdbh_band_streams, _BandGeometry, int(n_samples), int(width), int(row_lo), int(row_hi))


class DeviceDB:
    """A database resident in HBM (kmdb_db_upload)."""

    def __init__(self, src, device=0, with_hashtables=False, flags=0, prefix_shard=None, tree_range=None, query_shard=None):
        """query_shard=(index, count): the pruned tree of that prefix shard AND the slots of its own buckets (kmdb_db_upload_query_shard):
        new2all on it counts the k-mers of its own buckets, the rows of all shards sum to the database's.
        prefix_shard=(index, count): keep only the k-mers of the prefix buckets b with b % count == index
        (kmdb_db_upload_shard; the source must carry the hashtables).
        tree_range=(index, count): keep only the patterns of range `index` of `count` ranges of the tree's DFS pre-order, and the
        ancestors of its first node at weight 0 (kmdb_db_upload_range; all2all / all2all-sp only, no hashtables needed)."""
        self._keep = None
        if isinstance(src, HostDB):
            view = src.view
            self._keep = src
        elif isinstance(src, tuple):
            view, self._keep = C.pointer(src[0]), src
        else:
            raise TypeError("DeviceDB expects a HostDB or the (view, keepalive) pair from make_view()")
        self.device = device
        self._d = C.c_void_p()
        o = _opts(device, (0, 1), flags)
        if query_shard is not None:
            if prefix_shard is not None or tree_range is not None:
                raise ValueError("query_shard goes with neither prefix_shard nor tree_range")
            _check(lib().kmdb_db_upload_query_shard(view, C.byref(o), int(query_shard[0]), int(query_shard[1]), C.byref(self._d)))
        elif tree_range is not None:
            if prefix_shard is not None or with_hashtables:
                raise ValueError("tree_range goes with neither prefix_shard nor with_hashtables")
            _check(lib().kmdb_db_upload_range(view, C.byref(o), int(tree_range[0]), int(tree_range[1]), C.byref(self._d)))
        elif prefix_shard is None:
            _check(lib().kmdb_db_upload(view, C.byref(o), int(with_hashtables), C.byref(self._d)))
        else:
            _check(lib().kmdb_db_upload_shard(view, C.byref(o), int(with_hashtables), int(prefix_shard[0]), int(prefix_shard[1]),
                                              C.byref(self._d)))
        self.N = int(view.contents.n_samples)
        self.P = int(view.contents.n_patterns)

    @classmethod
    def _wrap(cls, handle, device, n_samples, keep=None):
        """a DeviceDB around a kmdb_db handle made elsewhere (Builder.finish_device); the object owns the handle"""
        self = cls.__new__(cls)
        self._keep, self.device, self._d, self.N = keep, device, handle, int(n_samples)
        self.P = int(self.stats()["n_patterns"])
        return self

    def tri_size(self):
        return self.N * (self.N - 1) // 2 if self.N else 0

    def all2all_dense(self, shard=(0, 1), flags=0):
        out = np.zeros(max(1, self.tri_size()), dtype=np.uint32)
        o = _opts(self.device, shard, flags)
        _check(lib().kmdb_all2all_dense(self._d, out.ctypes.data, C.byref(o)))
        return out[: self.tri_size()]

    def all2all_dense_device(self, dev_ptr, stream=None, shard=(0, 1), flags=0):
        """Result stays in device memory at dev_ptr (e.g. torch tensor .data_ptr())."""
        o = _opts(self.device, shard, flags, stream)
        _check(lib().kmdb_all2all_dense_device(self._d, C.c_void_p(dev_ptr), C.byref(o)))

    def _band_host(self, fn, row_lo, row_hi, shard, flags):
        """a band call's host form fn: the cells of the rows [row_lo, row_hi) as a numpy uint32 array"""
        lo, hi = int(row_lo), int(row_hi)
        cells = max(0, hi * (hi - 1) // 2 - lo * (lo - 1) // 2) if 0 <= lo <= hi <= self.N else 0       # (a refused range: the library says why)
        out = np.zeros(max(1, cells), dtype=np.uint32)
        o = _opts(self.device, shard, flags)
        _check(fn(self._d, lo, hi, out.ctypes.data, C.byref(o)))
        return out[:cells]

    def _band_device(self, fn, dev_ptr, row_lo, row_hi, stream, shard, flags):
        """a band call's device form fn: the same cells left in device memory at dev_ptr"""
        o = _opts(self.device, shard, flags, stream)
        _check(fn(self._d, int(row_lo), int(row_hi), C.c_void_p(dev_ptr), C.byref(o)))

    def all2all_rows(self, row_lo, row_hi, shard=(0, 1), flags=0):
        """kmdb_all2all_rows: rows [row_lo, row_hi) of the matrix alone — the cells tri(row_lo) .. tri(row_hi) of the lower triangle, tri(i) =
        i (i - 1) / 2, as a numpy uint32 array; nothing else of the triangle is computed or held anywhere"""
        return self._band_host(lib().kmdb_all2all_rows, row_lo, row_hi, shard, flags)

    def all2all_rows_device(self, dev_ptr, row_lo, row_hi, stream=None, shard=(0, 1), flags=0):
        """kmdb_all2all_rows_device: the same band left in device memory at dev_ptr (e.g. a torch tensor's .data_ptr()): the layout
        sparse_from_dense_device (cell_lo = tri(row_lo), cell_hi = tri(row_hi)) and Distance.take_cells (row_lo) take"""
        self._band_device(lib().kmdb_all2all_rows_device, dev_ptr, row_lo, row_hi, stream, shard, flags)

    def all2all_rows_stats(self):
        """kmdb_all2all_rows_stats_get: the last band call on the handle"""
        return _stats_dict(lib().kmdb_all2all_rows_stats_get, _All2allRowsStats, self._d)

    def all2all_rows_tiled(self, row_lo, row_hi, shard=(0, 1), flags=0):
        """kmdb_all2all_rows_tiled: the band of all2all_rows, bit for bit, its rows summed in LDS tiles (KMDB_ROWS_TILE_COLS, KMDB_ROWS_TILE_HITS)"""
        return self._band_host(lib().kmdb_all2all_rows_tiled, row_lo, row_hi, shard, flags)

    def all2all_rows_tiled_device(self, dev_ptr, row_lo, row_hi, stream=None, shard=(0, 1), flags=0):
        """kmdb_all2all_rows_tiled_device: the same band left in device memory at dev_ptr, the layout of all2all_rows_device"""
        self._band_device(lib().kmdb_all2all_rows_tiled_device, dev_ptr, row_lo, row_hi, stream, shard, flags)

    def all2all_rows_tiled_stats(self):
        """kmdb_all2all_rows_tiled_stats_get: the last tiled band call on the handle"""
        return _stats_dict(lib().kmdb_all2all_rows_tiled_stats_get, _All2allRowsTiledStats, self._d)

    def all2all_rows_records(self, row_lo, row_hi, shard=(0, 1), flags=0):
        """kmdb_all2all_rows_records: the band of all2all_rows, bit for bit, through the block-record pipeline (decode, emit, sort whole; the apply
        stage on the band's block rows alone)"""
        return self._band_host(lib().kmdb_all2all_rows_records, row_lo, row_hi, shard, flags)

    def all2all_rows_records_device(self, dev_ptr, row_lo, row_hi, stream=None, shard=(0, 1), flags=0):
        """kmdb_all2all_rows_records_device: the same band left in device memory at dev_ptr, the layout of all2all_rows_device"""
        self._band_device(lib().kmdb_all2all_rows_records_device, dev_ptr, row_lo, row_hi, stream, shard, flags)

    def all2all_rows_records_stats(self):
        """kmdb_all2all_rows_records_stats_get: the last band call through the block-record pipeline on the handle"""
        return _stats_dict(lib().kmdb_all2all_rows_records_stats_get, _All2allRowsRecordsStats, self._d)

    def all2all_rows_band_emit_stats(self):
        """kmdb_all2all_rows_band_emit_stats_get: the form the last records band call on the handle took (BAND_EMIT_FORM_*), its band's geometry in the
        pipeline's streams, and the band-emit state"""
        return _stats_dict(lib().kmdb_all2all_rows_band_emit_stats_get, _All2allRowsBandEmitStats, self._d)

    def band_streams(self, row_lo, row_hi, width=None):
        """kmdbh_band_streams for this handle's samples; width: the handle's block width (known after its first all2all or band call) unless given"""
        return band_streams(self.N, self.stats()["width"] if width is None else width, row_lo, row_hi)

    def all2all_banded_records_stats(self):
        """kmdb_all2all_banded_records_stats_get: the last banded call with path="records" on the handle"""
        return _stats_dict(lib().kmdb_all2all_banded_records_stats_get, _All2allBandedRecordsStats, self._d)

    def all2all_sparse_filtered_banded(self, band_rows, filters, sample_kmers, measure=None, shard=(0, 1), path=None):
        """kmdb_all2all_sparse_filtered_banded: all2all_sparse_filtered walked in bands of band_rows rows — one band resident at a time, the same
        SparseRows.  path: None (the tiled band call, kmdb_all2all_sparse_filtered_banded itself), or one of BAND_PATHS / its index
        (kmdb_all2all_sparse_filtered_banded_path)"""
        raw = _Sparse()
        o = _opts(self.device, shard)
        fs = (_CellFilter * max(1, len(filters)))()
        for i, (name, lo, hi) in enumerate(filters):
            fs[i].metric = METRICS.index(name)
            fs[i].lo = -np.finfo(np.float64).max if lo is None else lo
            fs[i].hi = np.finfo(np.float64).max if hi is None else hi
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        if path is None:
            _check(lib().kmdb_all2all_sparse_filtered_banded(self._d, int(band_rows), fs, len(filters), None if cnt is None else cnt.ctypes.data,
                                                             -1 if measure is None else METRICS.index(measure), C.byref(raw), C.byref(o)))
        else:
            _check(lib().kmdb_all2all_sparse_filtered_banded_path(self._d, int(band_rows), BAND_PATHS.index(path) if isinstance(path, str) else int(path), fs,
                                                                  len(filters), None if cnt is None else cnt.ctypes.data,
                                                                  -1 if measure is None else METRICS.index(measure), C.byref(raw), C.byref(o)))
        return _rows_out(raw)

    def all2all_banded_stats(self):
        """kmdb_all2all_banded_stats_get: the last banded call on the handle"""
        return _stats_dict(lib().kmdb_all2all_banded_stats_get, _All2allBandedStats, self._d)

    def all2all_sparse(self, shard=(0, 1)):
        raw = _Sparse()
        o = _opts(self.device, shard)
        _check(lib().kmdb_all2all_sparse(self._d, C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def all2all_sparse_filtered(self, filters, sample_kmers, measure=None):
        """filters: [(criterion name, lo, hi)], None = unbounded; measure: a criterion name whose value is returned for every kept cell"""
        raw = _Sparse()
        o = _opts(self.device)
        fs = (_CellFilter * max(1, len(filters)))()
        for i, (name, lo, hi) in enumerate(filters):
            fs[i].metric = METRICS.index(name)
            fs[i].lo = -np.finfo(np.float64).max if lo is None else lo
            fs[i].hi = np.finfo(np.float64).max if hi is None else hi
        cnt = np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_all2all_sparse_filtered(self._d, fs, len(filters), cnt.ctypes.data, -1 if measure is None else METRICS.index(measure),
                                                  C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def sparse_from_dense_device(self, dev_ptr, cell_lo=0, cell_hi=None, filters=(), sample_kmers=None, measure=None, stream=None):
        """Sparse rows of caller-accumulated cells [cell_lo, cell_hi) of the lower triangle, dev_ptr = device address of cell_lo
        (kmdb_sparse_from_dense_device): the compaction stage of all2all-sp after a multi-GPU reduce of the partial matrices."""
        raw = _Sparse()
        o = _opts(self.device, stream=stream)
        fs = (_CellFilter * max(1, len(filters)))()
        for i, (name, lo, hi) in enumerate(filters):
            fs[i].metric = METRICS.index(name)
            fs[i].lo = -np.finfo(np.float64).max if lo is None else lo
            fs[i].hi = np.finfo(np.float64).max if hi is None else hi
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_sparse_from_dense_device(self._d, C.c_void_p(dev_ptr), int(cell_lo), self.tri_size() if cell_hi is None else int(cell_hi),
                                                   fs, len(filters), None if cnt is None else cnt.ctypes.data,
                                                   -1 if measure is None else METRICS.index(measure), C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def all2all_sampled(self, criterion, count, sample_kmers, filters=(), shard=(0, 1)):
        """kmdb_all2all_sampled: per sample its `count` best neighbours by `criterion` (all2all-sp -sample-rows criterion:count) — ascending ids,
        val = common k-mers, measure = the score.  The candidates are selected on the device, the decision is the host's."""
        raw = _Sparse()
        o = _opts(self.device, shard)
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_all2all_sampled(self._d, _filters(filters), len(filters), None if cnt is None else cnt.ctypes.data, _criterion(criterion), int(count),
                                          C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def sampled_from_dense_device(self, dev_ptr, criterion, count, sample_kmers, cell_lo=0, cell_hi=None, filters=(), stream=None):
        """kmdb_sampled_from_dense_device: the candidates (symmetric rows, no measures) of caller-accumulated cells [cell_lo, cell_hi), dev_ptr =
        device address of cell_lo; the candidates of several ranges go to sample_rows_select together."""
        raw = _Sparse()
        o = _opts(self.device, stream=stream)
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_sampled_from_dense_device(self._d, C.c_void_p(dev_ptr), int(cell_lo), self.tri_size() if cell_hi is None else int(cell_hi),
                                                    _filters(filters), len(filters), None if cnt is None else cnt.ctypes.data, _criterion(criterion), int(count),
                                                    C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def sample_stats(self):
        """kmdb_db_sample_stats: the last sampled call on the handle"""
        return _stats_dict(lib().kmdb_db_sample_stats, _SampleStats, self._d)

    def new2all(self, queries):
        qs = [np.ascontiguousarray(q, np.uint64) for q in queries]
        nq = len(qs)
        ptrs = (C.c_void_p * max(nq, 1))(*[q.ctypes.data for q in qs])
        cnts = (C.c_size_t * max(nq, 1))(*[q.size for q in qs])
        out = np.zeros((nq, self.N), dtype=np.uint32)
        o = _opts(self.device)
        _check(lib().kmdb_new2all_batch(self._d, ptrs, cnts, nq, out.ctypes.data if out.size else None, C.byref(o)))
        return out

    def new2all_device(self, queries, dev_ptr, stream=None):
        """kmdb_new2all_batch_device: the rows are ADDED into the caller's zeroed nq x N uint32 device buffer at dev_ptr
        (e.g. a torch tensor's data_ptr())"""
        qs = [np.ascontiguousarray(q, np.uint64) for q in queries]
        nq = len(qs)
        ptrs = (C.c_void_p * max(nq, 1))(*[q.ctypes.data for q in qs])
        cnts = (C.c_size_t * max(nq, 1))(*[q.size for q in qs])
        o = _opts(self.device, stream=stream)
        _check(lib().kmdb_new2all_batch_device(self._d, ptrs, cnts, nq, C.c_void_p(dev_ptr), C.byref(o)))

    def new2all_seq_device(self, seqs, dev_ptr, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None, stream=None):
        """kmdb_new2all_batch_seq_alphabet_device: as new2all_seq, the rows ADDED into the device buffer at dev_ptr; returns the
        unique k-mer count per query (on a query shard: of its own buckets)"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        nq = len(bs)
        ptrs = (C.c_char_p * max(nq, 1))(*bs)
        lens = (C.c_size_t * max(nq, 1))(*[len(b) for b in bs])
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        o = _opts(self.device, stream=stream)
        _check(lib().kmdb_new2all_batch_seq_alphabet_device(self._d, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet),
                                                            C.c_void_p(dev_ptr), cnt.ctypes.data, C.byref(o)))
        return cnt[:nq]

    def db2db(self, col):
        """shared k-mers between every sample of this database (rows) and every sample of `col` (columns)"""
        out = np.zeros((self.N, col.N), dtype=np.uint32)
        buf = out if out.size else np.zeros(1, np.uint32)
        o = _opts(self.device)
        _check(lib().kmdb_db2db_dense(self._d, col._d, buf.ctypes.data, C.byref(o)))
        return out

    def db2db_sparse(self, col, filters=(), row_kmers=None, col_kmers=None, measure=None):
        """kmdb_db2db_sparse_filtered: the cell (this database's samples = rows, `col`'s = columns) as sparse rows, compacted and filtered on the
        device — db2db_sp + compact2(filter).  filters: [(criterion name, lo, hi)], None = unbounded; row_kmers / col_kmers: the k-mer counts of
        the row and the column samples (a and b of every measure, in that order); measure: a criterion name whose value is returned per kept cell."""
        raw = _Sparse()
        o = _opts(self.device)
        rk = None if row_kmers is None else np.ascontiguousarray(row_kmers, np.uint32)
        ck = None if col_kmers is None else np.ascontiguousarray(col_kmers, np.uint32)
        _check(lib().kmdb_db2db_sparse_filtered(self._d, col._d, _filters(filters), len(filters), None if rk is None else rk.ctypes.data,
                                                None if ck is None else ck.ctypes.data, -1 if measure is None else _criterion(measure),
                                                C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def db2db_stats(self):
        """kmdb_db2db_stats_get: the last db2db call with this handle as the row database"""
        return _stats_dict(lib().kmdb_db2db_stats_get, _Db2dbStats, self._d)

    def db2db_sampled(self, col, criterion, count, row_kmers, col_kmers, filters=()):
        """kmdb_db2db_sampled: the -sample-rows candidates of the cell (this database's samples = rows, `col`'s = columns), selected on the device.
        Returns (row candidates: self.N rows with ids local to `col`, column candidates: col.N rows with ids local to this database) — no
        measures; a = the row sample's k-mer count, b = the column sample's."""
        rows, cols = _Sparse(), _Sparse()
        o = _opts(self.device)
        rk = None if row_kmers is None else np.ascontiguousarray(row_kmers, np.uint32)
        ck = None if col_kmers is None else np.ascontiguousarray(col_kmers, np.uint32)
        _check(lib().kmdb_db2db_sampled(self._d, col._d, _filters(filters), len(filters), None if rk is None else rk.ctypes.data,
                                        None if ck is None else ck.ctypes.data, _criterion(criterion), int(count), C.byref(rows), C.byref(cols), C.byref(o)))
        try:
            return SparseRows(rows), SparseRows(cols)
        finally:
            lib().kmdb_sparse_free(C.byref(rows))
            lib().kmdb_sparse_free(C.byref(cols))

    def sampled_from_rect_device(self, dev_ptr, nr, nc, criterion, count, row_kmers, col_kmers, filters=(), stream=None):
        """kmdb_sampled_from_rect_device: the same on a caller-accumulated row-major nr x nc uint32 rectangle in device memory at dev_ptr."""
        rows, cols = _Sparse(), _Sparse()
        o = _opts(self.device, stream=stream)
        rk = None if row_kmers is None else np.ascontiguousarray(row_kmers, np.uint32)
        ck = None if col_kmers is None else np.ascontiguousarray(col_kmers, np.uint32)
        _check(lib().kmdb_sampled_from_rect_device(self._d, C.c_void_p(dev_ptr), int(nr), int(nc), _filters(filters), len(filters),
                                                   None if rk is None else rk.ctypes.data, None if ck is None else ck.ctypes.data, _criterion(criterion),
                                                   int(count), C.byref(rows), C.byref(cols), C.byref(o)))
        try:
            return SparseRows(rows), SparseRows(cols)
        finally:
            lib().kmdb_sparse_free(C.byref(rows))
            lib().kmdb_sparse_free(C.byref(cols))

    def db2db_sample_stats(self):
        """kmdb_db2db_sample_stats_get: the last sampled db2db (or rectangle) call with this handle as the row database"""
        return _stats_dict(lib().kmdb_db2db_sample_stats_get, _SampleStats, self._d)

    def new2all_seq(self, seqs, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """queries given as sequence text (bytes / str); k-mer extraction, minhash filter, sort + unique on the device.
        alphabet: the database's AlphabetType (HostDB.alphabet; ALPHABETS lists the names) — None: nt / nt-preserve by preserve_strand.
        Returns (similarities nq x N, unique k-mer count per query)."""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        nq = len(bs)
        ptrs = (C.c_char_p * max(nq, 1))(*bs)
        lens = (C.c_size_t * max(nq, 1))(*[len(b) for b in bs])
        out = np.zeros((nq, self.N), dtype=np.uint32)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        o = _opts(self.device)
        _check(lib().kmdb_new2all_batch_seq_alphabet(self._d, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet),
                                                     out.ctypes.data if out.size else None, cnt.ctypes.data, C.byref(o)))
        return out, cnt[:nq]

    def new2all_sparse(self, queries):
        qs = [np.ascontiguousarray(q, np.uint64) for q in queries]
        nq = len(qs)
        ptrs = (C.c_void_p * max(nq, 1))(*[q.ctypes.data for q in qs])
        cnts = (C.c_size_t * max(nq, 1))(*[q.size for q in qs])
        raw = _Sparse()
        o = _opts(self.device)
        _check(lib().kmdb_new2all_batch_sparse(self._d, ptrs, cnts, nq, C.byref(raw), C.byref(o)))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def new2all_sparse_filtered(self, queries, filters=(), sample_kmers=None, measure=None):
        """kmdb_new2all_batch_sparse_filtered: the rows of the queries (sorted unique k-mer arrays) compacted and filtered on the device — one2all_sp +
        the row's CombinedFilter.  filters: [(criterion name, lo, hi)], None = unbounded; sample_kmers: the database samples' k-mer counts (b of every
        measure; a is the query's own count); measure: a criterion name whose value is returned per kept cell."""
        keep, ptrs, cnts, nq = _kmer_queries(queries)
        raw, o, sk = _Sparse(), _opts(self.device), _u32(sample_kmers)
        _check(lib().kmdb_new2all_batch_sparse_filtered(self._d, ptrs, cnts, nq, _filters(filters), len(filters), _ptr(sk),
                                                        -1 if measure is None else _criterion(measure), C.byref(raw), C.byref(o)))
        return _rows_out(raw)

    def new2all_seq_sparse(self, seqs, filters=(), sample_kmers=None, measure=None, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """kmdb_new2all_batch_seq_alphabet_sparse_filtered: as new2all_sparse_filtered with the queries given as sequence text; returns
        (SparseRows, unique k-mer count per query)"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        keep, ptrs, lens, nq = _text_queries(seqs)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        raw, o, sk = _Sparse(), _opts(self.device), _u32(sample_kmers)
        _check(lib().kmdb_new2all_batch_seq_alphabet_sparse_filtered(self._d, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet), _filters(filters),
                                                                     len(filters), _ptr(sk), -1 if measure is None else _criterion(measure), C.byref(raw),
                                                                     cnt.ctypes.data, C.byref(o)))
        return _rows_out(raw), cnt[:nq]

    def new2all_rows_sparse_device(self, dev_ptr, nq, cell_lo=0, cell_hi=None, query_kmers=None, filters=(), sample_kmers=None, measure=None, stream=None):
        """kmdb_new2all_rows_sparse_device: the compaction alone, on the cells [cell_lo, cell_hi) of a row-major nq x N uint32 buffer the caller
        accumulated; dev_ptr = device address of cell_lo.  All nq rows come back; a row cut by a range end lists only its cells inside."""
        raw, o = _Sparse(), _opts(self.device, stream=stream)
        qk, sk = _u32(query_kmers), _u32(sample_kmers)
        _check(lib().kmdb_new2all_rows_sparse_device(self._d, C.c_void_p(dev_ptr), int(nq), int(cell_lo), int(nq) * self.N if cell_hi is None else int(cell_hi),
                                                     _ptr(qk), _filters(filters), len(filters), _ptr(sk), -1 if measure is None else _criterion(measure),
                                                     C.byref(raw), C.byref(o)))
        return _rows_out(raw)

    def new2all_sampled(self, queries, criterion, count, sample_kmers, filters=()):
        """kmdb_new2all_batch_sampled: per query (a sorted unique k-mer array) its `count` best database samples by `criterion` (new2all -sample-rows
        criterion:count) — ascending ids, val = common k-mers, measure = the score.  The candidates are selected on the device, the decision is the
        host's; a = the query's own k-mer count, b = sample_kmers[sample]."""
        keep, ptrs, cnts, nq = _kmer_queries(queries)
        raw, o, sk = _Sparse(), _opts(self.device), _u32(sample_kmers)
        _check(lib().kmdb_new2all_batch_sampled(self._d, ptrs, cnts, nq, _filters(filters), len(filters), _ptr(sk), _criterion(criterion), int(count), C.byref(raw),
                                                C.byref(o)))
        return _rows_out(raw)

    def new2all_seq_sampled(self, seqs, criterion, count, sample_kmers, filters=(), fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """kmdb_new2all_batch_seq_alphabet_sampled: as new2all_sampled with the queries given as sequence text; returns (SparseRows, unique k-mer count
        per query)"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        keep, ptrs, lens, nq = _text_queries(seqs)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        raw, o, sk = _Sparse(), _opts(self.device), _u32(sample_kmers)
        _check(lib().kmdb_new2all_batch_seq_alphabet_sampled(self._d, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet), _filters(filters),
                                                             len(filters), _ptr(sk), _criterion(criterion), int(count), C.byref(raw), cnt.ctypes.data, C.byref(o)))
        return _rows_out(raw), cnt[:nq]

    def sampled_from_rows_device(self, dev_ptr, nq, n_cols, criterion, count, query_kmers, sample_kmers, cell_lo=0, cell_hi=None, filters=(), stream=None):
        """kmdb_sampled_from_rows_device: the candidates (no measures) of the cells [cell_lo, cell_hi) of a row-major nq x n_cols uint32 buffer of query
        rows the caller accumulated; dev_ptr = device address of cell_lo.  All nq rows come back, those outside the range empty; the candidates of
        several ranges go to query_rows_select together."""
        raw, o = _Sparse(), _opts(self.device, stream=stream)
        qk, sk = _u32(query_kmers), _u32(sample_kmers)
        _check(lib().kmdb_sampled_from_rows_device(self._d, C.c_void_p(dev_ptr), int(nq), int(n_cols), int(cell_lo), int(nq) * int(n_cols) if cell_hi is None else int(cell_hi),
                                                   _ptr(qk), _filters(filters), len(filters), _ptr(sk), _criterion(criterion), int(count), C.byref(raw), C.byref(o)))
        return _rows_out(raw)

    def new2all_sample_stats(self):
        """kmdb_new2all_sample_stats_get: the last sampled new2all (or query-rows) call on the handle"""
        return _stats_dict(lib().kmdb_new2all_sample_stats_get, _SampleStats, self._d)

    def new2all_sparse_stats(self):
        """kmdb_new2all_sparse_stats_get: the last sparse new2all call on the handle"""
        return _stats_dict(lib().kmdb_new2all_sparse_stats_get, _New2allSparseStats, self._d)

    def stats(self):
        return _stats_dict(lib().kmdb_db_stats, _Stats, self._d)

    def fallback_reason(self):
        """why the last all2all call could not take the block-record pipeline ("" when it did)"""
        return lib().kmdb_db_fallback_reason(self._d).decode(errors="replace")

    def close(self):
        if self._d:
            lib().kmdb_db_free(self._d)
            self._d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NodeDB:
    """One database sharded over the devices of the node (kmdb_node_upload_partition): n_shards shards, shard s on devices[s % D];
    partition "prefix" (prefix buckets, needs the hashtables), "range" (ranges of the pattern tree, all2all without them) or
    "prefix-tables" (query shards: a prefix shard's tree and the slots of its own buckets — what new2all / one2all need)."""

    def __init__(self, src, n_shards, devices=(0,), partition="prefix"):
        self._keep = src
        view = src.view if isinstance(src, HostDB) else C.pointer(src[0])
        self._n = C.c_void_p()
        devs = (C.c_int32 * len(devices))(*devices)
        if partition not in PARTITIONS:
            raise ValueError("partition is one of " + ", ".join(PARTITIONS))
        _check(lib().kmdb_node_upload_partition(view, int(n_shards), devs, len(devices), PARTITIONS.index(partition), C.byref(self._n)))
        self.N = int(view.contents.n_samples)

    def tri_size(self):
        return self.N * (self.N - 1) // 2 if self.N else 0

    def all2all_dense(self):
        out = np.zeros(max(1, self.tri_size()), dtype=np.uint32)
        _check(lib().kmdb_node_all2all_dense(self._n, out.ctypes.data, None))
        return out[: self.tri_size()]

    def all2all_sparse(self, filters=(), sample_kmers=None, measure=None):
        raw = _Sparse()
        fs = (_CellFilter * max(1, len(filters)))()
        for i, (name, lo, hi) in enumerate(filters):
            fs[i].metric = METRICS.index(name)
            fs[i].lo = -np.finfo(np.float64).max if lo is None else lo
            fs[i].hi = np.finfo(np.float64).max if hi is None else hi
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_node_all2all_sparse(self._n, fs, len(filters), None if cnt is None else cnt.ctypes.data,
                                              -1 if measure is None else METRICS.index(measure), C.byref(raw), None))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def all2all_sampled(self, criterion, count, sample_kmers, filters=()):
        """kmdb_node_all2all_sampled: DeviceDB.all2all_sampled over the shards of the node, any partition"""
        raw = _Sparse()
        cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
        _check(lib().kmdb_node_all2all_sampled(self._n, _filters(filters), len(filters), None if cnt is None else cnt.ctypes.data, _criterion(criterion), int(count),
                                               C.byref(raw), None))
        try:
            return SparseRows(raw)
        finally:
            lib().kmdb_sparse_free(C.byref(raw))

    def new2all(self, queries):
        qs = [np.ascontiguousarray(q, np.uint64) for q in queries]
        nq = len(qs)
        ptrs = (C.c_void_p * max(nq, 1))(*[q.ctypes.data for q in qs])
        cnts = (C.c_size_t * max(nq, 1))(*[q.size for q in qs])
        out = np.zeros((nq, self.N), dtype=np.uint32)
        _check(lib().kmdb_node_new2all_batch(self._n, ptrs, cnts, nq, out.ctypes.data if out.size else None, None))
        return out

    def new2all_seq(self, seqs, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        nq = len(bs)
        ptrs = (C.c_char_p * max(nq, 1))(*bs)
        lens = (C.c_size_t * max(nq, 1))(*[len(b) for b in bs])
        out = np.zeros((nq, self.N), dtype=np.uint32)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        _check(lib().kmdb_node_new2all_batch_seq_alphabet(self._n, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet),
                                                          out.ctypes.data if out.size else None, cnt.ctypes.data, None))
        return out, cnt[:nq]

    def new2all_sparse(self, queries, filters=(), sample_kmers=None, measure=None):
        """kmdb_node_new2all_batch_sparse (no bounds, no measure) / kmdb_node_new2all_batch_sparse_filtered: DeviceDB.new2all_sparse_filtered over the
        query shards of the node — every device compacts its own chunk of the summed rows"""
        keep, ptrs, cnts, nq = _kmer_queries(queries)
        raw = _Sparse()
        if not filters and sample_kmers is None and measure is None:
            _check(lib().kmdb_node_new2all_batch_sparse(self._n, ptrs, cnts, nq, C.byref(raw), None))
        else:
            sk = _u32(sample_kmers)
            _check(lib().kmdb_node_new2all_batch_sparse_filtered(self._n, ptrs, cnts, nq, _filters(filters), len(filters), _ptr(sk),
                                                                 -1 if measure is None else _criterion(measure), C.byref(raw), None))
        return _rows_out(raw)

    def new2all_seq_sparse(self, seqs, filters=(), sample_kmers=None, measure=None, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """kmdb_node_new2all_batch_seq_alphabet_sparse_filtered: (SparseRows, unique k-mer count per query)"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        keep, ptrs, lens, nq = _text_queries(seqs)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        raw, sk = _Sparse(), _u32(sample_kmers)
        _check(lib().kmdb_node_new2all_batch_seq_alphabet_sparse_filtered(self._n, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet),
                                                                          _filters(filters), len(filters), _ptr(sk), -1 if measure is None else _criterion(measure),
                                                                          C.byref(raw), cnt.ctypes.data, None))
        return _rows_out(raw), cnt[:nq]

    def new2all_sampled(self, queries, criterion, count, sample_kmers, filters=()):
        """kmdb_node_new2all_batch_sampled: DeviceDB.new2all_sampled over the query shards of the node — every device selects on its own chunk of
        the summed rows, the host decides once"""
        keep, ptrs, cnts, nq = _kmer_queries(queries)
        raw, sk = _Sparse(), _u32(sample_kmers)
        _check(lib().kmdb_node_new2all_batch_sampled(self._n, ptrs, cnts, nq, _filters(filters), len(filters), _ptr(sk), _criterion(criterion), int(count),
                                                     C.byref(raw), None))
        return _rows_out(raw)

    def new2all_seq_sampled(self, seqs, criterion, count, sample_kmers, filters=(), fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """kmdb_node_new2all_batch_seq_alphabet_sampled: (SparseRows, unique k-mer count per query)"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        keep, ptrs, lens, nq = _text_queries(seqs)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        raw, sk = _Sparse(), _u32(sample_kmers)
        _check(lib().kmdb_node_new2all_batch_seq_alphabet_sampled(self._n, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet), _filters(filters),
                                                                  len(filters), _ptr(sk), _criterion(criterion), int(count), C.byref(raw), cnt.ctypes.data, None))
        return _rows_out(raw), cnt[:nq]

    def new2all_sample_stats(self):
        """kmdb_node_new2all_sample_stats_get: the last sampled new2all call on the node (sums over the devices, the slowest select_ms)"""
        return _stats_dict(lib().kmdb_node_new2all_sample_stats_get, _SampleStats, self._n)

    def new2all_sparse_stats(self):
        """kmdb_node_new2all_sparse_stats_get: the last sparse new2all call on the node (sums over the devices, the slowest compact_ms)"""
        return _stats_dict(lib().kmdb_node_new2all_sparse_stats_get, _New2allSparseStats, self._n)

    def stats(self):
        out = _stats_dict(lib().kmdb_node_stats_get, _NodeStats, self._n)
        out["partition"] = PARTITIONS[out["partition"]]
        out["devices"] = [_stats_dict(lib().kmdb_node_device_stats_get, _NodeDeviceStats, self._n, slot) for slot in range(out["n_devices"])]
        return out

    def close(self):
        if self._n:
            lib().kmdb_node_free(self._n)
            self._n = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
def _raw_rows(n_rows, row_ptr, col, val):
    """a kmdb_sparse_rows over caller-owned numpy arrays; returns (struct, keepalive)"""
    keep = [np.ascontiguousarray(row_ptr, np.uint64), np.ascontiguousarray(col, np.uint32), np.ascontiguousarray(val, np.uint32)]
    if keep[1].size == 0:
        keep[1] = np.zeros(1, np.uint32)
        keep[2] = np.zeros(1, np.uint32)
    r = _Sparse()
    r.n_rows = int(n_rows)
    r.nnz = int(keep[0][-1]) if keep[0].size else 0
    r.row_ptr = keep[0].ctypes.data_as(C.POINTER(C.c_uint64))
    r.col = keep[1].ctypes.data_as(C.POINTER(C.c_uint32))
    r.val = keep[2].ctypes.data_as(C.POINTER(C.c_uint32))
    return r, keep


def sample_rows_select(criterion, count, kmer_length, sample_kmers, parts, filters=()):
    """kmdbh_sample_rows_select (no GPU): parts = candidate rows, each a SparseRows or a (row_ptr, col, val) triple over the same samples ->
    SparseRows of the `count` best cells per sample that pass the filters: ascending ids, val = common k-mers, measure = the score"""
    raws, keep = [], []
    for p in parts:
        rp, col, val = (p.row_ptr, p.col, p.val) if isinstance(p, SparseRows) else p
        r, k = _raw_rows(len(rp) - 1, rp, col, val)
        raws.append(r)
        keep.append(k)
    arr = (C.POINTER(_Sparse) * max(1, len(raws)))(*[C.pointer(r) for r in raws])
    cnt = None if sample_kmers is None else np.ascontiguousarray(sample_kmers, np.uint32)
    out = _Sparse()
    _check(lib().kmdbh_sample_rows_select(_criterion(criterion), int(count), int(kmer_length), None if cnt is None else cnt.ctypes.data, _filters(filters),
                                          len(filters), arr, len(raws), C.byref(out)))
    try:
        return SparseRows(out)
    finally:
        lib().kmdb_sparse_free(C.byref(out))


def metric(criterion, common, cnt_row, cnt_col, kmer_length):
    """kmdbh_metric (no GPU): the measure of one cell — uint32 wrap-around integer parts, double arithmetic"""
    return float(lib().kmdbh_metric(_criterion(criterion), int(common), int(cnt_row), int(cnt_col), int(kmer_length)))


def query_rows_select(criterion, count, kmer_length, query_kmers, sample_kmers, parts, filters=()):
    """kmdbh_query_rows_select (no GPU): parts = candidate rows of the same nq queries, each a SparseRows or a (row_ptr, col, val) triple -> SparseRows
    of the `count` best database samples per query that pass the filters: ascending ids, val = common k-mers, measure = the score"""
    raws, keep = [], []
    for p in parts:
        rp, col, val = (p.row_ptr, p.col, p.val) if isinstance(p, SparseRows) else p
        r, k = _raw_rows(len(rp) - 1, rp, col, val)
        raws.append(r)
        keep.append(k)
    arr = (C.POINTER(_Sparse) * max(1, len(raws)))(*[C.pointer(r) for r in raws])
    qk, sk = _u32(query_kmers), _u32(sample_kmers)
    out = _Sparse()
    _check(lib().kmdbh_query_rows_select(_criterion(criterion), int(count), int(kmer_length), _ptr(qk), 0 if query_kmers is None else len(query_kmers),
                                         _ptr(sk), _filters(filters), len(filters), arr, len(raws), C.byref(out)))
    return _rows_out(out)


def extract_kmers(seq, k, fraction=1.0, start_fraction=0.0, preserve_strand=False):
    if isinstance(seq, str):
        seq = seq.encode()
    out = np.zeros(max(1, len(seq)), dtype=np.uint64)
    n = lib().kmdbh_extract_kmers(seq, len(seq), k, fraction, start_fraction, int(preserve_strand), out.ctypes.data)
    return out[:n]


ALPHABETS = ("nt", "nt-preserve", "aa", "aa11_diamond", "aa12_mmseqs", "aa6_dayhoff")      # AlphabetType order (reference src/alphabet.h:10-18)


def extract_kmers_alphabet(seq, k, alphabet, fraction=1.0, start_fraction=0.0):
    """k-mer words of a sequence over any alphabet of the reference (alphabet = index into ALPHABETS or its name)"""
    if isinstance(seq, str):
        seq = seq.encode()
    a = ALPHABETS.index(alphabet) if isinstance(alphabet, str) else int(alphabet)
    out = np.zeros(max(1, len(seq)), dtype=np.uint64)
    n = lib().kmdbh_extract_kmers_alphabet(seq, len(seq), k, a, fraction, start_fraction, out.ctypes.data)
    return out[:n]


def minhash_window(fraction, start_fraction=0.0):
    """kmdbh_minhash_window: (lo, hi) of the hash window — a k-mer is kept when lo <= hash < hi (a window that ends at 1 has hi = 0)"""
    lo, hi = C.c_uint64(), C.c_uint64()
    lib().kmdbh_minhash_window(float(fraction), float(start_fraction), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def minhash_geometry():
    """kmdb_minhash_geometry: (positions per thread R, positions per tile T) of the device extractor"""
    r, t = C.c_uint32(), C.c_uint32()
    lib().kmdb_minhash_geometry(C.byref(r), C.byref(t))
    return int(r.value), int(t.value)


def minhash_batch(seqs, k, alphabet="nt", fraction=1.0, start_fraction=0.0, device=0, stream=None):
    """kmdb_minhash_batch_seq_alphabet: the sorted unique k-mer words of every sample (its records joined by '\n'), extracted and filtered on the
    device — a list of uint64 arrays.  alphabet = index into ALPHABETS or its name."""
    a = ALPHABETS.index(alphabet) if isinstance(alphabet, str) else int(alphabet)
    keep, ptrs, lens, n = _sample_texts(seqs)
    out = _KmerLists()
    o = _opts(device, stream=stream)
    _check(lib().kmdb_minhash_batch_seq_alphabet(ptrs, lens, n, int(k), float(fraction), float(start_fraction), a, C.byref(out), C.byref(o)))
    try:
        off = np.ctypeslib.as_array(out.offsets, shape=(n + 1,)).copy()
        total = int(off[n])
        flat = np.ctypeslib.as_array(out.kmers, shape=(total,)).copy() if total else np.zeros(0, np.uint64)
        return [flat[int(off[s]): int(off[s + 1])] for s in range(n)]
    finally:
        lib().kmdb_kmer_lists_free(C.byref(out))


def minhash_stats():
    """kmdb_minhash_stats_get: the last minhash_batch call of this thread as a dict (stage times in ms from HIP events, kept / unique words,
    device bytes of the largest piece)"""
    return _stats_dict(lib().kmdb_minhash_stats_get, _MinhashStats)


def minhash_long_stats():
    """kmdb_minhash_long_stats_get: the long samples of the last minhash_batch call of this thread as a dict (samples cut into sections, their
    sections, words into and out of the merge-unions, the unions' ms from HIP events and bytes, peak device bytes)"""
    return _stats_dict(lib().kmdb_minhash_long_stats_get, _MinhashLongStats)


def sorted_union_geometry():
    """kmdb_sorted_union_geometry: (merged words per thread, merged words per tile) of the merge-union"""
    r, t = C.c_uint32(), C.c_uint32()
    lib().kmdb_sorted_union_geometry(C.byref(r), C.byref(t))
    return int(r.value), int(t.value)


def sorted_union_device(a_ptr, na, b_ptr, nb, out_ptr, cap, device=0, stream=None):
    """kmdb_sorted_union_device: the union of two strictly ascending uint64 arrays in device memory (addresses, e.g. a torch tensor's
    .data_ptr(), or None) written to out_ptr (room for `cap` >= na + nb words) -> the number of words written"""
    n = C.c_uint64()
    o = _opts(device, stream=stream)
    _check(lib().kmdb_sorted_union_device(C.c_void_p(a_ptr), int(na), C.c_void_p(b_ptr), int(nb), C.c_void_p(out_ptr), int(cap), C.byref(n), C.byref(o)))
    return int(n.value)


def minhash_store(path, kmers, k, fraction):
    """kmdbh_minhash_store: the bytes of MihashedInputFile::store; `path` is the full file name (<sample>.minhash)"""
    a = np.ascontiguousarray(kmers, np.uint64)
    _check(lib().kmdbh_minhash_store(os.fsencode(path), a.ctypes.data, a.size, int(k), float(fraction)))


def minhash_load(path):
    """kmdbh_minhash_load: (words as stored, k, fraction) of a <sample>.minhash file"""
    p, n, k, f = C.POINTER(C.c_uint64)(), C.c_size_t(), C.c_uint32(), C.c_double()
    _check(lib().kmdbh_minhash_load(os.fsencode(path), C.byref(p), C.byref(n), C.byref(k), C.byref(f)))
    try:
        words = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint64)
    finally:
        lib().kmdbh_minhash_free(p)
    return words, int(k.value), float(f.value)


class Builder:
    """kmdb_build_*: a database grown on the device from the samples' k-mer lists or texts, in the order they are added.
    finish() -> HostDB (upload it with DeviceDB, or .store(path) it)."""

    def __init__(self, k, fraction=1.0, start_fraction=0.0, alphabet="nt", device=0, stream=None):
        a = ALPHABETS.index(alphabet) if isinstance(alphabet, str) else int(alphabet)
        self._b = C.c_void_p()
        self.device = device
        o = _opts(device, stream=stream)
        _check(lib().kmdb_build_begin(int(k), float(fraction), float(start_fraction), a, C.byref(o), C.byref(self._b)))

    @classmethod
    def from_db(cls, hostdb, device=0, stream=None):
        """kmdb_build_begin_from_db: a builder seeded on the device from a HostDB that holds its tables; k, fraction, alphabet, names and
        counts are the database's, new samples are numbered from hostdb.N on"""
        self = cls.__new__(cls)
        self._b = C.c_void_p()
        self.device = device
        o = _opts(device, stream=stream)
        _check(lib().kmdb_build_begin_from_db(hostdb._h, C.byref(o), C.byref(self._b)))
        return self

    def seed_stats(self):
        return _stats_dict(lib().kmdb_build_seed_stats_get, _BuildSeedStats, self._b)

    @staticmethod
    def _names(names):
        bs = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        return bs, (C.c_char_p * max(len(bs), 1))(*bs)

    def add_kmers(self, names, lists):
        """strictly ascending uint64 lists, one per name (kmdb_build_add_kmers)"""
        keep_n, nptr = self._names(names)
        keep, ptrs, cnts, n = _kmer_queries(lists)
        assert n == len(keep_n)
        _check(lib().kmdb_build_add_kmers(self._b, nptr, ptrs, cnts, n))

    def add_seqs(self, names, seqs):
        """texts, records joined by '\n', extracted on the device with the builder's k / fraction / alphabet (kmdb_build_add_seq_alphabet)"""
        keep_n, nptr = self._names(names)
        keep, ptrs, lens, n = _sample_texts(seqs)
        assert n == len(keep_n)
        _check(lib().kmdb_build_add_seq_alphabet(self._b, nptr, ptrs, lens, n))

    def finish(self):
        h = C.c_void_p()
        _check(lib().kmdb_build_finish(self._b, C.byref(h)))
        return HostDB(None, _handle=h)

    def finish_device(self, with_hashtables=False, host_image=False, flags=0, device=None):
        """kmdb_build_finish_device: the database handed to the engine in HBM -> (DeviceDB, HostDB).  The HostDB is the image finish()
        returns with host_image, else a header-only image (names, counts, k, fractions, alphabet).  device: the builder's (another is refused)"""
        dev = self.device if device is None else device
        d, h = C.c_void_p(), C.c_void_p()
        o = _opts(dev, (0, 1), flags)
        _check(lib().kmdb_build_finish_device(self._b, C.byref(o), int(bool(with_hashtables)), int(bool(host_image)), C.byref(d), C.byref(h)))
        host = HostDB(None, _handle=h)
        return DeviceDB._wrap(d, dev, host.N), host

    def handoff_stats(self):
        return _stats_dict(lib().kmdb_build_handoff_stats_get, _BuildHandoffStats, self._b)

    def stats(self):
        return _stats_dict(lib().kmdb_build_stats_get, _BuildStats, self._b)

    def close(self):
        if self._b:
            lib().kmdb_build_free(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Distance:
    """kmdb_distance_*: the rows of a table of common k-mer counts -> the rows of one measure, parsed, measured and formatted on the device.
    counts: the table's total-kmers row; filters: [(criterion name, lo, hi)], None = unbounded, "num-kmers" among them."""

    def __init__(self, measure, k, counts, filters=(), sparse_out=False, sparse_in=False, triangle=False, phylip=False, device=0, stream=None):
        self._d = C.c_void_p()
        cnt = np.ascontiguousarray(counts, np.uint32)
        fs = _filters(filters)
        o = _DistanceOpts()
        o.abi_version, o.device, o.measure, o.kmer_length = ABI_VERSION, int(device), _criterion(measure), int(k)
        o.counts, o.n = cnt.ctypes.data, cnt.size
        o.filters, o.n_filters = C.cast(fs, C.c_void_p), len(filters)
        o.flags = (DISTANCE_SPARSE_OUT if sparse_out else 0) | (DISTANCE_SPARSE_IN if sparse_in else 0) | (DISTANCE_TRIANGLE if triangle else 0) \
            | (DISTANCE_PHYLIP if phylip else 0)
        o.stream = stream
        _check(lib().kmdb_distance_begin(C.byref(o), C.byref(self._d)))

    def rows(self, text, first_row=0):
        """a run of whole rows -> (their output text, 0), or (b"", DISTANCE_DECLINED) with the reason in .declined"""
        text = bytes(text)
        out = _DistanceOut()
        rc = lib().kmdb_distance_rows(self._d, text, len(text), int(first_row), C.byref(out))
        if rc == DISTANCE_DECLINED:
            self.declined = lib().kmdb_last_error().decode(errors="replace")
            return b"", rc
        _check(rc)
        try:
            return C.string_at(out.text, out.len), 0
        finally:
            lib().kmdb_distance_out_free(C.byref(out))

    @staticmethod
    def _names(names):
        names = [n if isinstance(n, bytes) else str(n).encode() for n in names]
        return (C.c_char_p * max(1, len(names)))(*names)

    def take_all2all(self, db, names):
        """kmdb_distance_take_all2all: the all2all triangle of a DeviceDB, computed into memory the handle owns, becomes the source of cells"""
        _check(lib().kmdb_distance_take_all2all(self._d, db._d, self._names(names), None))

    def take_cells(self, dev_ptr, row_lo, names):
        """kmdb_distance_take_cells_device: dev_ptr (e.g. a torch tensor's .data_ptr(), or None) = the first cell of row row_lo of a lower triangle
        of uint32 the caller keeps alive"""
        _check(lib().kmdb_distance_take_cells_device(self._d, C.c_void_p(dev_ptr), int(row_lo), self._names(names)))

    def cells_ptr(self):
        """kmdb_distance_cells_device: the device address of the cells taken (None before a take), for a second handle's take_cells"""
        return lib().kmdb_distance_cells_device(self._d)

    def matrix_rows(self, lo, hi):
        """kmdb_distance_matrix_rows: the text of rows [lo, hi) of the measure's table of the matrix taken"""
        out = _DistanceOut()
        _check(lib().kmdb_distance_matrix_rows(self._d, int(lo), int(hi), C.byref(out)))
        try:
            return C.string_at(out.text, out.len)
        finally:
            lib().kmdb_distance_out_free(C.byref(out))

    def take_new2all(self, db, kmer_lists, names):
        """kmdb_distance_take_new2all_batch: the new2all rows of a batch of queries (sorted unique k-mer arrays) against a DeviceDB, computed into a
        rectangle the handle owns, become the source of cells; a = the length of each list"""
        keep, ptrs, cnts, nq = _kmer_queries(kmer_lists)
        _check(lib().kmdb_distance_take_new2all_batch(self._d, db._d, ptrs, cnts, nq, self._names(names), None))

    def take_new2all_seqs(self, db, seqs, names, fraction=1.0, start_fraction=0.0, preserve_strand=False, alphabet=None):
        """kmdb_distance_take_new2all_batch_seq_alphabet: the same with the queries given as sequence text; returns the unique k-mer count per query"""
        if alphabet is None:
            alphabet = 1 if preserve_strand else 0
        keep, ptrs, lens, nq = _text_queries(seqs)
        cnt = np.zeros(max(nq, 1), dtype=np.uint64)
        _check(lib().kmdb_distance_take_new2all_batch_seq_alphabet(self._d, db._d, ptrs, lens, nq, float(fraction), float(start_fraction), int(alphabet),
                                                                   self._names(names), cnt.ctypes.data, None))
        return cnt[:nq]

    def take_rows(self, dev_ptr, nq, query_kmers, names):
        """kmdb_distance_take_rows_device: dev_ptr (e.g. a torch tensor's .data_ptr(), or None) = cell 0 of a row-major nq x N rectangle of uint32
        the caller keeps alive; query_kmers: the queries' own k-mer counts"""
        qk = np.ascontiguousarray(np.asarray(query_kmers, np.uint64) & 0xFFFFFFFF, np.uint32)
        _check(lib().kmdb_distance_take_rows_device(self._d, C.c_void_p(dev_ptr), int(nq), qk.ctypes.data, self._names(names)))

    def query_rows(self, lo, hi):
        """kmdb_distance_query_rows: the text of rows [lo, hi) of the measure's table of the batch taken"""
        out = _DistanceOut()
        _check(lib().kmdb_distance_query_rows(self._d, int(lo), int(hi), C.byref(out)))
        try:
            return C.string_at(out.text, out.len)
        finally:
            lib().kmdb_distance_out_free(C.byref(out))

    def parts_begin(self, row_kmers, names):
        """kmdb_distance_parts_begin_rows: a block row of the all2all-parts grid — the row samples' own k-mer counts and names; drops the one before"""
        rk = np.ascontiguousarray(np.asarray(row_kmers, np.uint64) & 0xFFFFFFFF, np.uint32)
        self._nr = rk.size
        _check(lib().kmdb_distance_parts_begin_rows(self._d, rk.size, rk.ctypes.data, self._names(names)))

    def parts_add_db2db(self, db_row, db_col, col_shift):
        """kmdb_distance_parts_add_db2db: the cell (db_row, db_col) of two DeviceDBs, its CSR kept in HBM; col_shift = the samples of the earlier parts"""
        _check(lib().kmdb_distance_parts_add_db2db(self._d, db_row._d, db_col._d, int(col_shift), None))

    def parts_add_all2all(self, db, col_shift):
        """kmdb_distance_parts_add_all2all: the diagonal cell, the lower triangle of a DeviceDB"""
        _check(lib().kmdb_distance_parts_add_all2all(self._d, db._d, int(col_shift), None))

    def parts_add_csr(self, row_ptr, col, val, n_cols, col_shift):
        """kmdb_distance_parts_add_csr_device: a cell the caller computed (device addresses; columns local to the cell's n_cols), copied in"""
        _check(lib().kmdb_distance_parts_add_csr_device(self._d, C.c_void_p(row_ptr), C.c_void_p(col), C.c_void_p(val), int(n_cols), int(col_shift)))

    def take_csr(self, row_ptr, col, val, nr, row_kmers, names):
        """kmdb_distance_take_csr_device: device addresses (e.g. torch tensors' .data_ptr(), or None) of a CSR the caller keeps alive — row_ptr
        uint64[nr + 1], col uint32 global 0-based ascending within a row, val uint32 > 0; row_kmers: the row samples' own k-mer counts"""
        rk = np.ascontiguousarray(np.asarray(row_kmers, np.uint64) & 0xFFFFFFFF, np.uint32)
        self._nr = int(nr)
        _check(lib().kmdb_distance_take_csr_device(self._d, C.c_void_p(row_ptr), C.c_void_p(col), C.c_void_p(val), int(nr), rk.ctypes.data, self._names(names)))

    def csr_rows(self, lo, hi):
        """kmdb_distance_csr_rows: the text of rows [lo, hi) of the measure's table of the CSR taken (the first call after the adds gathers)"""
        out = _DistanceOut()
        _check(lib().kmdb_distance_csr_rows(self._d, int(lo), int(hi), C.byref(out)))
        try:
            return C.string_at(out.text, out.len)
        finally:
            lib().kmdb_distance_out_free(C.byref(out))

    def csr_ptrs(self):
        """kmdb_distance_csr_device: (row_ptr, col, val, nr) — the device addresses of the gathered or taken CSR, for a second handle's take_csr"""
        rp, co, va, nr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().kmdb_distance_csr_device(self._d, C.byref(rp), C.byref(co), C.byref(va), C.byref(nr)))
        return rp.value, co.value, va.value, nr.value

    def csr_row_ptr(self):
        """kmdb_distance_csr_row_ptr: the row_ptr of the gathered or taken CSR on the host"""
        out = np.zeros(getattr(self, "_nr", 0) + 1, np.uint64)
        _check(lib().kmdb_distance_csr_row_ptr(self._d, out.ctypes.data))
        return out

    def parts_stats(self):
        return _stats_dict(lib().kmdb_distance_parts_stats_get, _DistancePartsStats, self._d)

    def stats(self):
        return _stats_dict(lib().kmdb_distance_stats_get, _DistanceStats, self._d)

    def close(self):
        if self._d:
            lib().kmdb_distance_free(self._d)
            self._d = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_measure(v):
    """kmdbh_format_measure: a measure as the distance mode prints it"""
    buf = C.create_string_buffer(48)
    n = lib().kmdbh_format_measure(float(v), buf)
    return buf.raw[:n]


def sort_unique(kmers):
    a = np.ascontiguousarray(kmers, np.uint64).copy()
    n = lib().kmdbh_sort_unique(a.ctypes.data, a.size)
    return a[:n]


def format_header(hostdb):
    return hostdb.header_bytes()


def format_dense_row(name, kmers, row):
    r = np.ascontiguousarray(row, np.uint32)
    buf = C.create_string_buffer(len(name) + 64 + 11 * r.size)
    n = lib().kmdbh_format_dense_row(name.encode(), int(kmers), r.ctypes.data, r.size, buf)
    return buf.raw[:n]


def format_sparse_row(name, kmers, cols, vals):
    c = np.ascontiguousarray(cols, np.uint32)
    v = np.ascontiguousarray(vals, np.uint32)
    buf = C.create_string_buffer(len(name) + 64 + 22 * c.size)
    n = lib().kmdbh_format_sparse_row(name.encode(), int(kmers), c.ctypes.data, v.ctypes.data, c.size, buf)
    return buf.raw[:n]
