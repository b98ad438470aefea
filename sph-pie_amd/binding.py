"""ctypes binding of include/pie_scan.h (libpie_hip.so).  Thin: every method is one C-ABI call.

There is no CPU fallback here: if the HIP library is missing this raises, and if no GPU is present
`PieScan()` raises with the library's own error text."""
import ctypes as C
import os

import numpy as np

from .build import HIP_LIB

PIE_GEN_INTERVAL = 1
PIE_GEN_CLUSTERED = 2
PIE_GEN_TIME_ORDERED = 4
PIE_END_NONE = -(2 ** 63)
INT64_MIN = -(2 ** 63)

PIE_E_CAPACITY = -5
PIE_E_STATE = -6
PIE_COMPACT_SHRINK = 1


class PieError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("pie_scan error %d: %s" % (code, text))
        self.code = code


class PieTableInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("has_keys", C.c_uint32), ("rows", C.c_uint64), ("users", C.c_uint64),
        ("table_bytes", C.c_uint64), ("derived_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64),
        ("index_build_ms", C.c_double), ("ordered_rows", C.c_uint64), ("ordered_bytes", C.c_uint64),
        ("ordered_build_ms", C.c_double), ("ordered_builds", C.c_uint64), ("ordered_positions", C.c_uint64),
        ("ordered_respreads", C.c_uint64), ("hot_rows", C.c_uint64), ("hot_bytes", C.c_uint64), ("hot_builds", C.c_uint64),
        ("compact_bytes", C.c_uint64), ("compactions", C.c_uint64), ("compact_count_ms", C.c_double), ("compact_write_ms", C.c_double),
        ("hot_build_ms", C.c_double), ("hot_order", C.c_uint32), ("hot_slot_bits", C.c_uint32),
        ("token_rows", C.c_uint64), ("token_bytes", C.c_uint64), ("token_builds", C.c_uint64), ("token_build_ms", C.c_double),
        ("expired_inflight_bytes", C.c_uint64), ("expired_inflight_ms", C.c_double),
    ]


class PieQuery(C.Structure):
    _fields_ = [("now", C.c_int64), ("cutoff", C.c_int64), ("mask", C.c_uint64)]


PIE_BATCH_MAX = 64
PIE_WIDE_MAX = 512


class PieStats(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_profiled", C.c_uint32), ("rows", C.c_uint64), ("users", C.c_uint64),
        ("selected", C.c_uint64), ("alg_bytes", C.c_uint64), ("k1_ms_sum", C.c_double), ("scan_ms_sum", C.c_double),
        ("max_bucket", C.c_uint32), ("n_segments", C.c_uint32), ("n_big", C.c_uint32), ("k1_blocks", C.c_uint32),
        ("k1_variant", C.c_uint32), ("key_ambiguous", C.c_uint32), ("live", C.c_uint64), ("candidates", C.c_uint64),
        ("n_small", C.c_uint32), ("n_over", C.c_uint32), ("n_hot", C.c_uint32), ("direct_shift", C.c_uint32),
    ]


# every symbol include/pie_scan.h declares: (name, restype, argtypes)
_P = C.c_void_p
_SIGS = [
    ("pie_abi_version", C.c_int, []),
    ("pie_device_count", C.c_int, []),
    ("pie_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("pie_ctx_destroy", C.c_int, [_P]),
    ("pie_last_error", C.c_char_p, [_P]),
    ("pie_ctx_set_stream", C.c_int, [_P, _P]),
    ("pie_ctx_aux_stream", C.c_int, [_P, C.POINTER(_P)]),
    ("pie_load_columns", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_int32]),
    ("pie_gen_synthetic", C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32]),
    ("pie_gen_synthetic_cdf", C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, _P]),
    ("pie_save_columns", C.c_int, [_P, C.c_char_p]),
    ("pie_load_columns_dir", C.c_int, [_P, C.c_char_p]),
    ("pie_read_columns", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t]),
    ("pie_set_end", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_set_end_last_writers", C.c_int, [_P, C.c_size_t, _P]),
    ("pie_delete_user", C.c_int, [_P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_delete_users", C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    ("pie_delete_users_plan", C.c_int, [_P, C.c_size_t, C.c_int32, _P, _P]),
    ("pie_prune_before", C.c_int, [_P, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_retention_purge", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_retention_purge_tz", C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_append_rows", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_int32]),
    ("pie_set_disciplines", C.c_int, [_P, C.c_uint64, C.c_int32]),
    ("pie_scan", C.c_int, [_P, C.c_int64, C.c_int64, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_scan_device", C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]),
    ("pie_scan_begin", C.c_int, [_P, C.c_int64, C.c_int64]),
    ("pie_scan_finish", C.c_int, [_P, C.POINTER(C.c_size_t)]),
    ("pie_scan_begin_packed", C.c_int, [_P, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("pie_scan_finish_packed", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("pie_scan_begin_packed2", C.c_int, [_P, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    ("pie_host_alloc", C.c_int, [_P, C.c_size_t, C.POINTER(_P), C.POINTER(_P)]),
    ("pie_host_free", C.c_int, [_P, _P]),
    ("pie_set_scan_form", C.c_int, [_P, C.c_int]),
    ("pie_set_ordered_run", C.c_int, [_P, C.c_int]),
    ("pie_set_wide_ordered", C.c_int, [_P, C.c_int]),
    ("pie_set_turn_ordered", C.c_int, [_P, C.c_int]),
    ("pie_set_batch_lanes", C.c_int, [_P, C.c_int]),
    ("pie_batch_lanes", C.c_int, [_P]),
    ("pie_batch_room", C.c_int, [_P]),
    ("pie_scan_batch_flush", C.c_int, [_P]),
    ("pie_batch_pack_union_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t]),
    ("pie_table_info_get", C.c_int, [_P, C.POINTER(PieTableInfo)]),
    ("pie_hot_layout", C.c_int, [_P, _P, C.POINTER(C.c_int64), _P, _P, _P, C.c_size_t, _P, C.c_size_t]),
    ("pie_hot_order_key", C.c_uint64, [C.c_uint32, C.c_int32, C.c_uint32]),
    ("pie_hot_slot_bits", C.c_uint32, [C.c_uint32]),
    ("pie_scan_batch_begin", C.c_int, [_P, C.POINTER(PieQuery), C.c_int]),
    ("pie_scan_batch_finish", C.c_int, [_P, C.POINTER(C.c_size_t)]),
    ("pie_scan_batch", C.c_int, [_P, C.POINTER(PieQuery), C.c_int, C.POINTER(C.c_size_t)]),
    ("pie_scan_batch_begin_union", C.c_int, [_P, C.POINTER(PieQuery), C.c_int, C.c_void_p, C.c_size_t, C.c_size_t]),
    ("pie_batch_union_device_ptrs", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("pie_batch_read_union", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_scan_batch_begin_packed", C.c_int, [_P, C.POINTER(PieQuery), C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]),
    ("pie_scan_batch_finish_packed", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("pie_scan_wide_begin", C.c_int, [_P, C.POINTER(PieQuery), C.c_int]),
    ("pie_scan_wide_finish", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_int)]),
    ("pie_batch_union_wide_device_ptrs", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("pie_batch_read_union_wide", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("pie_batch_pack_union_wide_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t]),
    ("pie_scan_wide_begin_union", C.c_int, [_P, C.POINTER(PieQuery), C.c_int, _P, C.c_size_t, C.c_size_t]),
    ("pie_scan_wide_finish_packed", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("pie_batch_mask_codes", C.c_int, [C.POINTER(PieQuery), C.c_int, _P, C.c_int32, _P, _P, _P, C.c_size_t, _P, _P]),
    ("pie_batch_read_results", C.c_int, [_P, C.c_int, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_batch_result_device_ptrs", C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    ("pie_batch_read_user_feed", C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_batch_fetch_requests", C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P, C.POINTER(C.c_size_t)]),
    ("pie_read_results", C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_read_user_feed", C.c_int, [_P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_result_device_ptrs", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    ("pie_copy_results_device", C.c_int, [_P, _P, _P, _P, C.c_size_t]),
    ("pie_pack_results_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t]),
    ("pie_fetch_rows", C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P]),
    ("pie_expired_queue", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_archive_queue", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_queue_info", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_queue_pack_device", C.c_int, [_P, _P, C.c_size_t, C.c_size_t]),
    ("pie_archive_stats", C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("pie_set_profiling", C.c_int, [_P, C.c_int]),
    ("pie_stats_get", C.c_int, [_P, C.POINTER(PieStats)]),
    ("pie_stats_reset", C.c_int, [_P]),
    ("pie_synchronize", C.c_int, [_P]),
    ("pie_shard_of", C.c_int32, [C.c_int32, C.c_int32]),
    ("pie_shard_table", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    ("pie_shard_maps", C.c_int, [_P, _P, _P]),
    ("pie_shard_info", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    ("pie_shard_append_rows", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    ("pie_shard_set_end", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_shard_delete_user", C.c_int, [_P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_shard_delete_users", C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    ("pie_shard_prune_before", C.c_int, [_P, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_shard_retention_purge", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_shard_retention_purge_tz", C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_shard_rows_to_local", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_shard_rows_to_global", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_shard_route", C.c_int, [_P, C.c_size_t, C.c_int32, C.c_int32, _P, C.POINTER(C.c_size_t), C.c_int32, C.c_int32, _P, C.c_size_t,
                                  C.POINTER(C.c_size_t)]),
    ("pie_compact_rows", C.c_int, [_P, C.c_int64, C.c_uint32, C.POINTER(C.c_size_t)]),
    ("pie_compact_maps", C.c_int, [_P, _P, _P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_compact_map_device_ptrs", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_compact_translate", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_compact_geometry", C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("pie_comm_create", C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(_P)]),
    ("pie_comm_unique_id", C.c_int, [_P]),
    ("pie_comm_create_rank", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    ("pie_comm_destroy", C.c_int, [_P]),
    ("pie_comm_last_error", C.c_char_p, [_P]),
    ("pie_comm_world", C.c_int32, [_P]),
    ("pie_comm_local_ranks", C.c_int32, [_P]),
    ("pie_comm_ctx", _P, [_P, C.c_int32]),
    ("pie_comm_gen_synthetic_sharded", C.c_int, [_P, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32]),
    ("pie_comm_scan_batch_gather", C.c_int, [_P, C.POINTER(PieQuery), C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    ("pie_comm_reserve", C.c_int, [_P, C.c_int32, C.c_int32, C.c_size_t]),
    ("pie_comm_needed_cap", C.c_size_t, [_P]),
    ("pie_comm_step_reserve", C.c_int, [_P, C.c_int32, C.c_int32, C.c_size_t]),
    ("pie_comm_step_begin", C.c_int, [_P, C.POINTER(PieQuery), C.c_int32]),
    ("pie_comm_step_finish", C.c_int, [_P, C.POINTER(C.c_size_t)]),
    ("pie_comm_step_collect", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("pie_comm_step_gathered_ptr", C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_comm_step_read_gathered", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_wide_step_reserve", C.c_int, [_P, C.c_int32, C.c_int32, C.c_size_t]),
    ("pie_comm_wide_step_begin", C.c_int, [_P, C.POINTER(PieQuery), C.c_int32]),
    ("pie_comm_wide_step_finish", C.c_int, [_P, C.POINTER(C.c_size_t), C.c_size_t]),
    ("pie_comm_wide_step_collect", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("pie_comm_wide_step_status", C.c_int, [_P, C.c_int64, C.POINTER(C.c_int32)]),
    ("pie_comm_wide_step_gathered_ptr", C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_int)]),
    ("pie_comm_wide_step_read_gathered", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, _P, _P, _P, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    ("pie_comm_wide_step_read_feed", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_gathered_device_ptr", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_comm_read_gathered", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_expired_queue", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_archive_queue", C.c_int, [_P, C.c_int64, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_queue_read", C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_queue_device_ptrs", C.c_int, [_P, C.c_int32, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("pie_comm_queue_timing", C.c_int, [_P, C.POINTER(C.c_float)]),
    ("pie_comm_append_rows", C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, C.c_int32, C.POINTER(C.c_int32)]),
    ("pie_comm_set_end", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_comm_delete_user", C.c_int, [_P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    ("pie_comm_delete_users", C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t), _P, _P]),
    ("pie_comm_prune_before", C.c_int, [_P, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_retention_purge", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int64, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_retention_purge_tz", C.c_int, [_P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_compact_rows", C.c_int, [_P, C.c_int64, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_comm_queue_kind", C.c_int, [_P]),
    ("pie_comm_table_size", C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("pie_token_set", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_token_append", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_token_lookup", C.c_int, [_P, _P, C.c_size_t, C.c_int64, _P, _P, _P, _P, _P]),
    ("pie_token_set_end", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int64, _P]),
    ("pie_token_layout", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _P, C.c_size_t, _P]),
    ("pie_token_slots_for", C.c_size_t, [C.c_size_t]),
    ("pie_token_homes", C.c_int, [_P, C.c_size_t, C.c_uint32, _P]),
    ("pie_token_turn_plan", C.c_int, [_P, C.c_size_t, _P, _P]),
    ("pie_token_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    ("pie_shard_token_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P]),
    ("pie_session_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    ("pie_session_turn_plan", C.c_int, [_P, C.c_size_t, C.c_int64, _P, _P, _P, C.POINTER(C.c_size_t)]),
    ("pie_shard_session_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    ("pie_shard_session_turn_plan", C.c_int, [_P, C.c_size_t, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                              C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("pie_shard_token_set",C.c_int, [_P, _P, C.c_size_t]),
    ("pie_shard_token_append", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_shard_token_lookup", C.c_int, [_P, _P, C.c_size_t, C.c_int64, _P, _P, _P, _P, _P]),
    ("pie_shard_token_set_end", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int64, _P]),
    ("pie_shard_token_layout", C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _P, C.c_size_t, _P]),
    ("pie_token_lookup_begin", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_token_lookup_finish", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_token_lookup_room", C.c_int, [_P]),
    ("pie_shard_token_lookup_begin", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_shard_token_lookup_finish", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_token_turn_begin", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_token_turn_finish", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_token_turn_room", C.c_int, [_P]),
    ("pie_shard_token_turn_begin", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_shard_token_turn_finish", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_expired_queue_begin", C.c_int, [_P, C.c_int64, C.c_int64, C.c_size_t]),
    ("pie_expired_queue_finish", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_expired_queue_room", C.c_int, [_P]),
    ("pie_shard_expired_queue_begin", C.c_int, [_P, C.c_int64, C.c_int64, C.c_size_t]),
    ("pie_shard_expired_queue_finish", C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_expired_inflight_geometry", C.c_int, [_P, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("pie_comm_token_set", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_comm_token_append", C.c_int, [_P, _P, C.c_size_t]),
    ("pie_comm_token_lookup", C.c_int, [_P, _P, C.c_size_t, C.c_int64, _P, _P, _P, _P, _P, _P]),
    ("pie_comm_token_set_end", C.c_int, [_P, _P, _P, C.c_size_t, C.c_int64, _P]),
    ("pie_comm_token_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, _P, _P, _P, _P]),
    ("pie_comm_session_turn", C.c_int, [_P, _P, C.c_size_t, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    ("pie_comm_token_lookup_begin", C.c_int, [_P, _P, _P, C.c_size_t]),
    ("pie_comm_token_lookup_finish", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_token_lookup_room", C.c_int, [_P]),
    ("pie_comm_expired_queue_begin", C.c_int, [_P, C.c_int64, C.c_int64, C.c_size_t]),
    ("pie_comm_expired_queue_finish", C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("pie_comm_expired_queue_room", C.c_int, [_P]),
    ("pie_comm_inflight_queue_device_ptrs", C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
]
ABI_SYMBOLS = [s[0] for s in _SIGS]


def hot_order_key(bin_, user, n_users):
    """Sort key of a hot-index record: (bin << hot_slot_bits(n_users)) | histogram slot of the user (pie_hot_order_key)."""
    return int(load_library().pie_hot_order_key(int(bin_), int(user), int(n_users)))


def hot_slot_bits(n_users):
    return int(load_library().pie_hot_slot_bits(int(n_users)))

_lib = None


def load_library(path=None):
    """dlopen libpie_hip.so and type its symbols.  Raises if the library was not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("PIE_HIP_LIB") or HIP_LIB   # PIE_HIP_LIB: A/B builds of the same source (tuning runs)
    if not os.path.exists(path):
        raise RuntimeError("%s is missing — build it first: python -c 'import __graft_entry__ as g; g.build()' "
                           "(there is no CPU fallback for the scan path)" % path)
    lib = C.CDLL(path)
    for name, res, args in _SIGS:
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _col(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


class PieScan:
    """One context = one GPU = one process."""

    def __init__(self, device=0, lib_path=None):
        self._lib = load_library(lib_path)
        self._ctx = _P()
        rc = self._lib.pie_ctx_create(int(device), C.byref(self._ctx))
        if rc != 0:
            text = self._lib.pie_last_error(None).decode()
            self._ctx = None
            raise PieError(rc, text)
        self.n = 0
        self.n_users = 0
        self._begun = []   # scans begun and not finished, oldest first: True = begun with scan_begin_packed
        self._m_buf, self._ready_buf = (C.c_size_t * PIE_BATCH_MAX)(), C.c_int(0)
        self._ready_ref = C.byref(self._ready_buf)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.pie_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise PieError(rc, self._lib.pie_last_error(self._ctx).decode())

    # ---- table
    def load_columns(self, start, end, user, disc, n_users):
        start, end = _col(start, np.int64), _col(end, np.int64)
        user, disc = _col(user, np.int32), _col(disc, np.int32)
        n = start.shape[0]
        if not (end.shape[0] == user.shape[0] == disc.shape[0] == n):
            raise ValueError("column lengths differ")
        self._check(self._lib.pie_load_columns(self._ctx, _ptr(start), _ptr(end), _ptr(user), _ptr(disc), n, int(n_users)))
        self.n, self.n_users = n, int(n_users)

    def gen_synthetic(self, seed, n_total, row0, n, n_users, n_disc, flags=0):
        self._check(self._lib.pie_gen_synthetic(self._ctx, seed, n_total, row0, n, n_users, n_disc, flags))
        self.n, self.n_users = int(n), int(n_users)

    def gen_synthetic_cdf(self, seed, n_total, row0, n, n_users, n_disc, flags, cdf):
        """Skewed users: cdf = n_users ascending uint64 thresholds (floor(CDF_k * 2^64))."""
        cdf = np.ascontiguousarray(cdf, np.uint64)
        if cdf.shape[0] != n_users:
            raise ValueError("cdf must have n_users entries")
        self._check(self._lib.pie_gen_synthetic_cdf(self._ctx, seed, n_total, row0, n, n_users, n_disc, flags, _ptr(cdf)))
        self.n, self.n_users = int(n), int(n_users)

    def save_columns(self, directory):
        self._check(self._lib.pie_save_columns(self._ctx, os.fsencode(directory)))

    def load_columns_dir(self, directory):
        self._check(self._lib.pie_load_columns_dir(self._ctx, os.fsencode(directory)))
        st = self.stats()
        self.n, self.n_users = int(st["rows"]), int(st["users"])

    def read_columns(self):
        n = self.n
        s, e = np.empty(n, np.int64), np.empty(n, np.int64)
        u, d = np.empty(n, np.int32), np.empty(n, np.int32)
        self._check(self._lib.pie_read_columns(self._ctx, _ptr(s), _ptr(e), _ptr(u), _ptr(d), n))
        return s, e, u, d

    def set_end(self, rows, new_end):
        """end[rows[i]] = new_end[i], the elements applied in array order: a row named more than once ends on the value of its
        last occurrence, in `end` and in every structure derived from it (pie_set_end)."""
        rows, new_end = _col(rows, np.int32), _col(new_end, np.int64)
        self._check(self._lib.pie_set_end(self._ctx, _ptr(rows), _ptr(new_end), rows.shape[0]))

    def append_rows(self, start, end, user, disc, n_users):
        start, end = _col(start, np.int64), _col(end, np.int64)
        user, disc = _col(user, np.int32), _col(disc, np.int32)
        self._check(self._lib.pie_append_rows(self._ctx, _ptr(start), _ptr(end), _ptr(user), _ptr(disc), start.shape[0], int(n_users)))
        self.n += start.shape[0]
        self.n_users = int(n_users)

    def delete_user(self, user):
        """-> ascending row indices that were tombstoned."""
        k = C.c_size_t(0)
        rows = np.empty(max(self.n, 1), np.int32)
        self._check(self._lib.pie_delete_user(self._ctx, int(user), _ptr(rows), self.n, C.byref(k)))
        return rows[: k.value].copy()

    def delete_users(self, users, cap=None):
        """deleteSessionsForUser for every id of `users` in one call (pie_delete_users) -> (rows, per_user): all tombstoned rows
        ascending, and per element the rows tombstoned for it (a repeated id counts at its first occurrence, an unknown id 0).
        cap: entries of the row list to offer (default: the table's rows); too few raises PieError(PIE_E_CAPACITY) with the
        rows tombstoned all the same."""
        users = _col(users, np.int32)
        k = C.c_size_t(0)
        cap = self.n if cap is None else int(cap)
        rows = np.empty(max(cap, 1), np.int32)
        per = np.zeros(users.shape[0], np.int32)
        self._check(self._lib.pie_delete_users(self._ctx, _ptr(users), users.shape[0], _ptr(rows), cap, C.byref(k), _ptr(per)))
        return rows[: k.value].copy(), per

    def prune_before(self, cutoff):
        """Tombstone rows with start < cutoff; -> their ascending row indices."""
        k = C.c_size_t(0)
        rows = np.empty(max(self.n, 1), np.int32)
        self._check(self._lib.pie_prune_before(self._ctx, int(cutoff), _ptr(rows), self.n, C.byref(k)))
        return rows[: k.value].copy()

    def retention_purge(self, now, months=2, tz_offset_ms=0, tz_table=None):
        """Tombstone rows with now >= addMonths(start, months) (JS calendar-month arithmetic on a LOCAL date); -> their ascending
        indices.  tz_table = (transitions_utc_ms, offsets_ms) for a zone with daylight saving (binding.tz_table(zone)); else the
        fixed offset tz_offset_ms."""
        k = C.c_size_t(0)
        rows = np.empty(max(self.n, 1), np.int32)
        if tz_table is not None:
            T, off = np.ascontiguousarray(tz_table[0], np.int64), np.ascontiguousarray(tz_table[1], np.int64)
            if off.shape[0] != T.shape[0] + 1:
                raise ValueError("a table of n transitions carries n + 1 offsets")
            self._check(self._lib.pie_retention_purge_tz(self._ctx, int(now), int(months), _ptr(T), _ptr(off), int(T.shape[0]), _ptr(rows), self.n, C.byref(k)))
        else:
            self._check(self._lib.pie_retention_purge(self._ctx, int(now), int(months), int(tz_offset_ms), _ptr(rows), self.n, C.byref(k)))
        return rows[: k.value].copy()

    def set_disciplines(self, mask, n_disc):
        self._check(self._lib.pie_set_disciplines(self._ctx, mask & (2 ** 64 - 1), int(n_disc)))

    # ---- scan
    def scan(self, now, cutoff, idx_cap=None):
        """-> (counts[U] int32, offsets[U+1] int64, idx[M] int32), host arrays."""
        U = self.n_users
        if idx_cap is None:
            # size the row list by what the scan selected (a table-sized buffer per call would cost more than the scan)
            self.scan_device(now, cutoff)
            return self.read_results()
        counts, offsets = np.empty(U, np.int32), np.empty(U + 1, np.int64)
        cap = int(idx_cap)
        idx = np.empty(max(cap, 1), np.int32)
        m = C.c_size_t(0)
        self._check(self._lib.pie_scan(self._ctx, int(now), int(cutoff), _ptr(counts), _ptr(offsets), _ptr(idx), cap, C.byref(m)))
        return counts, offsets, idx[: m.value].copy() if cap > 4 * max(m.value, 1) else idx[: m.value]

    def read_results(self):
        """Host copies (counts, offsets, idx) of the last FINISHED scan (scan_finish / scan_device / scan_pipelined)."""
        U = self.n_users
        counts, offsets = np.empty(U, np.int32), np.empty(U + 1, np.int64)
        m = C.c_size_t(0)
        self._check(self._lib.pie_read_results(self._ctx, _ptr(counts), _ptr(offsets), None, 0, C.byref(m)))
        idx = np.empty(max(m.value, 1), np.int32)
        if m.value:
            self._check(self._lib.pie_read_results(self._ctx, None, None, _ptr(idx), m.value, C.byref(m)))
        return counts, offsets, idx[: m.value]

    def read_user_feed(self, user, cap=None):
        """Rows of one user's feed from the last finished scan (two small device reads)."""
        cap = self.n if cap is None else int(cap)
        out = np.empty(max(cap, 1), np.int32)
        k = C.c_size_t(0)
        self._check(self._lib.pie_read_user_feed(self._ctx, int(user), _ptr(out), cap, C.byref(k)))
        return out[: k.value].copy()

    def read_results_into(self, counts_ptr=None, offsets_ptr=None, idx_ptr=None, idx_cap=0):
        """pie_read_results into caller-owned host memory (raw addresses, e.g. of pinned buffers).  -> M."""
        m = C.c_size_t(0)
        self._check(self._lib.pie_read_results(self._ctx, counts_ptr, offsets_ptr, idx_ptr, int(idx_cap), C.byref(m)))
        return m.value

    def scan_device(self, now, cutoff):
        m = C.c_size_t(0)
        self._check(self._lib.pie_scan_device(self._ctx, int(now), int(cutoff), C.byref(m)))
        return m.value

    def scan_begin(self, now, cutoff):
        self._check(self._lib.pie_scan_begin(self._ctx, int(now), int(cutoff)))
        self._begun.append(False)

    def scan_finish(self):
        m = C.c_size_t(0)
        rc = self._lib.pie_scan_finish(self._ctx, C.byref(m))
        if self._begun and rc != -6:   # the library dropped the oldest scan (finished or failed); PIE_E_STATE: nothing was in flight
            self._begun.pop(0)
        self._check(rc)
        return m.value

    def scan_begin_packed(self, now, cutoff, dst_ptr, u_pad, idx_cap):
        """scan_begin whose scan also writes its result message (layout of pack_results_device) into dst_ptr."""
        self._check(self._lib.pie_scan_begin_packed(self._ctx, int(now), int(cutoff), dst_ptr, int(u_pad), int(idx_cap)))
        self._begun.append(True)

    def scan_begin_packed2(self, now, cutoff, dst_ptr, u_pad, idx_cap, counts_ptr=None):
        """scan_begin_packed with a second destination for counts[U]; both may be mapped pinned host memory (host_alloc)."""
        self._check(self._lib.pie_scan_begin_packed2(self._ctx, int(now), int(cutoff), dst_ptr, int(u_pad), int(idx_cap), counts_ptr))
        self._begun.append(True)

    def host_alloc(self, n_words):
        """Mapped pinned host memory of n_words int32.  -> (numpy view of the host side, device address, host address)."""
        h, d = _P(), _P()
        self._check(self._lib.pie_host_alloc(self._ctx, int(n_words) * 4, C.byref(h), C.byref(d)))
        arr = np.ctypeslib.as_array(C.cast(h.value, C.POINTER(C.c_int32)), shape=(int(n_words),))
        return arr, d.value, h.value

    def host_free(self, host_addr):
        self._check(self._lib.pie_host_free(self._ctx, host_addr))

    def set_scan_form(self, form):
        """Pin the table-pass form (pie_stats.k1_variant codes); form < 0: adaptive."""
        self._check(self._lib.pie_set_scan_form(self._ctx, int(form)))

    def set_ordered_run(self, mode):
        """0: never (frees the run), 1: adaptive (default), 2: always (pie_set_ordered_run)."""
        self._check(self._lib.pie_set_ordered_run(self._ctx, int(mode)))

    def set_wide_ordered(self, on):
        """1: a wide batch on a table whose batches take the ordered run runs one pass there and keeps its union; 0 (default):
        it reruns its queries one by one (pie_set_wide_ordered)."""
        self._check(self._lib.pie_set_wide_ordered(self._ctx, int(on)))

    def set_turn_ordered(self, on):
        """1: a turn that logs in (session_turn with creates, also on a shard) keeps a valid ordered run where append_rows would
        keep it: the created rows are inserted in place; 0 (default): such a turn drops the run (pie_set_turn_ordered)."""
        self._check(self._lib.pie_set_turn_ordered(self._ctx, int(on)))

    def table_info(self):
        ti = PieTableInfo()
        ti.struct_size = C.sizeof(PieTableInfo)
        self._check(self._lib.pie_table_info_get(self._ctx, C.byref(ti)))
        return {k: getattr(ti, k) for k, _ in PieTableInfo._fields_}

    def hot_layout(self):
        """The hot index as the device holds it (pie_hot_layout): off[129], n_main, user / row / bin of the main records, pos[n]."""
        off, nm = np.empty(129, np.int64), C.c_int64(0)
        self._check(self._lib.pie_hot_layout(self._ctx, _ptr(off), C.byref(nm), None, None, None, 0, None, 0))
        m = nm.value
        user, row, bin_ = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.int32)
        pos = np.empty(self.n, np.int32)
        self._check(self._lib.pie_hot_layout(self._ctx, None, None, _ptr(user), _ptr(row), _ptr(bin_), m, _ptr(pos), self.n))
        return {"off": off, "n_main": m, "user": user, "row": row, "bin": bin_, "pos": pos}

    def in_flight_packed(self):
        """True when the oldest scan in flight was begun with scan_begin_packed."""
        return bool(self._begun) and self._begun[0]

    def scan_finish_packed(self):
        """-> (M, ready): ready = the message was complete in device memory on return (no stream ordering needed);
        otherwise a pack kernel was enqueued on the context's stream."""
        m, ready = C.c_size_t(0), C.c_int(0)
        rc = self._lib.pie_scan_finish_packed(self._ctx, C.byref(m), C.byref(ready))
        if self._begun and rc != -6:
            self._begun.pop(0)
        self._check(rc)
        return int(m.value), bool(ready.value)

    def scan_pipelined(self, k, now, cutoff):
        """k scans of the same query with two in flight: the table pass of scan i+1 overlaps the tail (scatter,
        per-bucket order) of scan i.  -> M of the last scan; results on the device as after scan_device()."""
        m = 0
        if k <= 0:
            return m
        self.scan_begin(now, cutoff)
        for i in range(k):
            if i + 1 < k:
                self.scan_begin(now, cutoff)
            m = self.scan_finish()
        return m

    # ---- batched scan: Q queries (now, cutoff, mask), one table pass
    _q_cache = None

    @staticmethod
    def _queries(queries):
        # the same list of queries, batch after batch, is the common case (a pipelined loop): marshal it once
        hit = PieScan._q_cache
        if hit is not None and hit[2] is queries and len(queries) == len(hit[0]):
            return hit[1]            # the very same list object again (a caller that changes it in place passes a new list)
        key = tuple(queries)
        if hit is not None and hit[0] == key:
            return hit[1]
        arr = (PieQuery * len(queries))()
        for k, (now, cutoff, mask) in enumerate(queries):
            arr[k].now, arr[k].cutoff, arr[k].mask = int(now), int(cutoff), int(mask) & (2 ** 64 - 1)
        PieScan._q_cache = (key, arr, queries)
        return arr

    def scan_batch_begin(self, queries):
        """queries: sequence of (now, cutoff, mask), at most PIE_BATCH_MAX.  Up to three batches may be in flight."""
        arr = self._queries(queries)
        self._check(self._lib.pie_scan_batch_begin(self._ctx, arr, len(queries)))
        self._batches = getattr(self, "_batches", [])
        self._batches.append(len(queries))

    def scan_batch_begin_packed(self, queries, msg_ptr, msg_stride, u_pad, idx_cap, counts_ptr=None, counts_stride=0):
        arr = self._queries(queries)
        self._check(self._lib.pie_scan_batch_begin_packed(self._ctx, arr, len(queries), msg_ptr, int(msg_stride), int(u_pad),
                                                          int(idx_cap), counts_ptr, int(counts_stride)))
        self._batches = getattr(self, "_batches", [])
        self._batches.append(len(queries))

    def scan_batch_begin_union(self, queries, msg_ptr, u_pad, cap):
        """A batch whose own kernels write the UNION exchange message [uoff[0..u_pad] | Mu | rows[cap) | mask_lo[cap) | mask_hi[cap)
        if more than 32 queries] into msg_ptr (device-visible int32 memory)."""
        arr = self._queries(queries)
        self._check(self._lib.pie_scan_batch_begin_union(self._ctx, arr, len(queries), msg_ptr, int(u_pad), int(cap)))
        self._batches = getattr(self, "_batches", [])
        self._batches.append(len(queries))

    def batch_read_union(self):
        """The primary result of the last finished batch: (uoff[U+1] int64, rows[Mu] int32, masks[Mu] uint64);
        Feed(q, u) = rows[uoff[u]:uoff[u+1]][(masks[uoff[u]:uoff[u+1]] >> q) & 1 == 1].  None when the batch has no union
        (queries fell back to the general path, or it ran on the ordered run)."""
        a, b, lo, hi, mu = _P(), _P(), _P(), _P(), C.c_size_t(0)
        self._check(self._lib.pie_batch_union_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(lo), C.byref(hi), C.byref(mu)))
        if not a.value:
            return None
        uoff = np.empty(self.n_users + 1, np.int64)
        rows, masks = np.empty(max(mu.value, 1), np.int32), np.empty(max(mu.value, 1), np.uint64)
        self._check(self._lib.pie_batch_read_union(self._ctx, _ptr(uoff), _ptr(rows), _ptr(masks), mu.value, C.byref(mu)))
        return uoff, rows[: mu.value], masks[: mu.value]

    def batch_union_device_ptrs(self):
        """-> (uoff, rows, mask_lo, mask_hi device addresses or None, Mu)"""
        a, b, lo, hi, mu = _P(), _P(), _P(), _P(), C.c_size_t(0)
        self._check(self._lib.pie_batch_union_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(lo), C.byref(hi), C.byref(mu)))
        return a.value, b.value, lo.value, hi.value, int(mu.value)

    def scan_batch_finish(self, packed=False, want_m=True):
        """-> list of M per query of the oldest batch in flight (packed: (list, ready)).  want_m=False: the list is not built
        (a step loop that only moves messages: 64 Python ints per step are a microsecond it does not have)."""
        nq = self._batches[0] if getattr(self, "_batches", None) else PIE_BATCH_MAX
        m = self._m_buf
        ready = self._ready_buf
        rc = self._lib.pie_scan_batch_finish_packed(self._ctx, m, self._ready_ref)
        if getattr(self, "_batches", None) and rc != -6:
            self._batches.pop(0)
        if rc:
            self._check(rc)
        ms = m[:nq] if want_m else None
        return (ms, bool(ready.value)) if packed else ms

    # ---- wide batches: up to PIE_WIDE_MAX queries, one table pass (same semantics as scan_batch)
    @staticmethod
    def _wide_queries(queries):
        # marshalled on every call: no identity cache (a list changed in place must not re-run the old queries)
        arr = (PieQuery * max(len(queries), 1))()
        for k, (now, cutoff, mask) in enumerate(queries):
            arr[k].now, arr[k].cutoff, arr[k].mask = int(now), int(cutoff), int(mask) & (2 ** 64 - 1)
        return arr

    def scan_wide_begin(self, queries):
        """queries: sequence of (now, cutoff, mask), 1..PIE_WIDE_MAX.  Shares the lanes and the FIFO with scan_batch_begin."""
        queries = list(queries)
        self._check(self._lib.pie_scan_wide_begin(self._ctx, self._wide_queries(queries), len(queries)))
        self._batches = getattr(self, "_batches", [])
        self._batches.append(len(queries))

    def scan_wide_finish(self):
        """-> list of M per query of the oldest batch in flight, wide or not."""
        m = (C.c_size_t * PIE_WIDE_MAX)()
        nq = C.c_int(0)
        rc = self._lib.pie_scan_wide_finish(self._ctx, m, PIE_WIDE_MAX, C.byref(nq))
        if getattr(self, "_batches", None) and rc not in (-6, PIE_E_CAPACITY):
            self._batches.pop(0)
        self._check(rc)
        return [int(x) for x in m[: nq.value]]

    def scan_wide_begin_union(self, queries, msg_ptr, u_pad, cap):
        """A wide batch whose own tail writes the wide union message (layout: split_wide_message) into msg_ptr, device-visible
        int32 memory of u_pad + 2 + cap * (1 + 2 * ceil(len(queries) / 64)) words."""
        queries = list(queries)
        self._check(self._lib.pie_scan_wide_begin_union(self._ctx, self._wide_queries(queries), len(queries), msg_ptr, int(u_pad), int(cap)))
        self._batches = getattr(self, "_batches", [])
        self._batches.append(len(queries))

    def scan_wide_finish_packed(self):
        """-> (list of M per query of the oldest batch in flight, ready).  ready: the batch kept its union and its message was
        complete on return; otherwise the header says Mu = -1 once the context's stream has passed."""
        m = (C.c_size_t * PIE_WIDE_MAX)()
        nq, ready = C.c_int(0), C.c_int(0)
        rc = self._lib.pie_scan_wide_finish_packed(self._ctx, m, PIE_WIDE_MAX, C.byref(nq), C.byref(ready))
        if getattr(self, "_batches", None) and rc not in (-6, PIE_E_CAPACITY):
            self._batches.pop(0)
        self._check(rc)
        return [int(x) for x in m[: nq.value]], bool(ready.value)

    def scan_wide(self, queries):
        """-> [(counts, offsets, idx)] per query; bit for bit what scan() gives for each (now, cutoff) under its mask."""
        queries = list(queries)
        self.scan_wide_begin(queries)
        self.scan_wide_finish()
        return [self.batch_read_results(k) for k in range(len(queries))]

    def batch_read_union_wide(self):
        """Union of the last finished wide batch: (uoff[U+1] int64, rows[Mu] int32, masks[Mu, words] uint64) — bit q of row r is
        masks[r, q // 64] >> (q % 64) & 1 — or None when the batch has no union (queries fell back)."""
        a, b, mk, words, mu = _P(), _P(), _P(), C.c_int(0), C.c_size_t(0)
        rc = self._lib.pie_batch_union_wide_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(mk), C.byref(words), C.byref(mu))
        if rc == -6 and b"has no union result" in (self._lib.pie_last_error(self._ctx) or b""):
            return None              # the last batch is wide and its queries fell back; any other misuse raises
        self._check(rc)
        w, n = int(words.value), int(mu.value)
        uoff = np.empty(self.n_users + 1, np.int64)
        rows, masks = np.empty(max(n, 1), np.int32), np.empty((max(n, 1), w), np.uint64)
        self._check(self._lib.pie_batch_read_union_wide(self._ctx, _ptr(uoff), _ptr(rows), _ptr(masks), n, C.byref(words), C.byref(mu)))
        return uoff, rows[:n], masks[:n]

    def batch_union_wide_device_ptrs(self):
        """-> (uoff, rows, masks device addresses, words, Mu) of the last finished wide batch (PieError PIE_E_STATE without a union)"""
        a, b, mk, words, mu = _P(), _P(), _P(), C.c_int(0), C.c_size_t(0)
        self._check(self._lib.pie_batch_union_wide_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(mk), C.byref(words), C.byref(mu)))
        return a.value, b.value, mk.value, int(words.value), int(mu.value)

    def batch_pack_union_wide_device(self, dst_ptr, u_pad, cap):
        """Wide union message into device memory (pie_batch_pack_union_wide_device); enqueued on the context's stream."""
        self._check(self._lib.pie_batch_pack_union_wide_device(self._ctx, dst_ptr, int(u_pad), int(cap)))

    def batch_pack_union_device(self, dst_ptr, u_pad, cap):
        """Union message of the last finished batch into device memory (pie_batch_pack_union_device); enqueued, not waited for."""
        self._check(self._lib.pie_batch_pack_union_device(self._ctx, dst_ptr, int(u_pad), int(cap)))

    def batch_read_results(self, qi):
        """Host copies (counts, offsets, idx) of query qi of the last finished batch."""
        U = self.n_users
        counts, offsets = np.empty(U, np.int32), np.empty(U + 1, np.int64)
        m = C.c_size_t(0)
        self._check(self._lib.pie_batch_read_results(self._ctx, int(qi), _ptr(counts), _ptr(offsets), None, 0, C.byref(m)))
        idx = np.empty(max(m.value, 1), np.int32)
        if m.value:
            self._check(self._lib.pie_batch_read_results(self._ctx, int(qi), None, None, _ptr(idx), m.value, C.byref(m)))
        return counts, offsets, idx[: m.value]

    def scan_batch(self, queries):
        """-> [(counts, offsets, idx)] per query; bit for bit what scan() gives for each (now, cutoff) under its mask."""
        self.scan_batch_begin(queries)
        self.scan_batch_finish()
        return [self.batch_read_results(k) for k in range(len(queries))]

    def batch_read_user_feed(self, qi, user, cap=None):
        """Rows of one user's feed of query qi of the last finished batch."""
        cap = self.n if cap is None else int(cap)
        out = np.empty(max(cap, 1), np.int32)
        k = C.c_size_t(0)
        self._check(self._lib.pie_batch_read_user_feed(self._ctx, int(qi), int(user), _ptr(out), cap, C.byref(k)))
        return out[: k.value].copy()

    def batch_fetch_requests(self, qis, users, cap_rows=None):
        """Feeds of many (query, user) requests of the last finished batch in one call.
        -> (off[n + 1] int64, idx, start, end, disc): request i's rows are idx[off[i]:off[i + 1]] (feed order) with their columns."""
        qis, users = _col(qis, np.int32), _col(users, np.int32)
        n = qis.shape[0]
        cap = int(cap_rows) if cap_rows is not None else 64 * max(n, 1)
        off = np.empty(n + 1, np.int64)
        total = C.c_size_t(0)
        while True:
            idx, disc = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32)
            start, end = np.empty(max(cap, 1), np.int64), np.empty(max(cap, 1), np.int64)
            rc = self._lib.pie_batch_fetch_requests(self._ctx, _ptr(qis), _ptr(users), n, cap, _ptr(off), _ptr(idx), _ptr(start), _ptr(end),
                                                    _ptr(disc), C.byref(total))
            # the default room is 64 rows per request; a union on the ordered run has no such bound per user: the call says how
            # many rows there are
            if rc == PIE_E_CAPACITY and cap_rows is None and total.value > cap:
                cap = int(total.value)
                continue
            self._check(rc)
            break
        t = total.value
        return off, idx[:t], start[:t], end[:t], disc[:t]

    def batch_result_device_ptrs(self, qi):
        a, b, c = _P(), _P(), _P()
        self._check(self._lib.pie_batch_result_device_ptrs(self._ctx, int(qi), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_batch_lanes(self, n_lanes):
        """Lanes of the batched scan (independent streams, three batches in flight on each): 1..4, 0 = by table size."""
        self._check(self._lib.pie_set_batch_lanes(self._ctx, int(n_lanes)))

    def batch_lanes(self):
        return int(self._lib.pie_batch_lanes(self._ctx))

    def batch_room(self):
        """batches scan_batch_begin would take right now (pie_batch_room)"""
        return int(self._lib.pie_batch_room(self._ctx))

    def scan_batch_pipelined(self, k, queries, depth=3):
        """k batches of the same queries with up to `depth` (<= 3) in flight PER LANE: the next launch is queued before the host
        waits for a summary.  -> list of M of the last batch."""
        ms, begun, done = [], 0, 0
        depth = depth * self.batch_lanes()
        room = self._lib.pie_batch_room
        while done < k:
            while begun < k and begun - done < depth and room(self._ctx) > 0:
                self.scan_batch_begin(queries)
                begun += 1
                if begun == k:   # the burst ends here: the lanes' last tails go out together, not one by one as they are finished
                    self._check(self._lib.pie_scan_batch_flush(self._ctx))
            ms = self.scan_batch_finish()
            done += 1
        return ms

    def scan_batch_flush(self):
        """No further begin is coming for now: queue the waiting tails of all lanes at once (pie_scan_batch_flush)."""
        self._check(self._lib.pie_scan_batch_flush(self._ctx))

    def result_device_ptrs(self):
        a, b, c = _P(), _P(), _P()
        self._check(self._lib.pie_result_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def copy_results_device(self, counts_ptr=None, offsets_ptr=None, idx_ptr=None, idx_cap=0):
        """D2D copy into caller-owned device buffers (raw pointers, e.g. tensor.data_ptr()), on the ctx stream."""
        self._check(self._lib.pie_copy_results_device(self._ctx, counts_ptr, offsets_ptr, idx_ptr, int(idx_cap)))

    def pack_results_device(self, dst_ptr, u_pad, idx_cap):
        """[off[0..u_pad] | M | idx[:min(M, cap)]] as int32 (u_pad+2+cap words) into caller-owned device memory."""
        self._check(self._lib.pie_pack_results_device(self._ctx, dst_ptr, int(u_pad), int(idx_cap)))

    def fetch_rows(self, idx):
        idx = _col(idx, np.int32)
        m = idx.shape[0]
        s, e = np.empty(m, np.int64), np.empty(m, np.int64)
        u, d = np.empty(m, np.int32), np.empty(m, np.int32)
        self._check(self._lib.pie_fetch_rows(self._ctx, _ptr(idx), m, _ptr(s), _ptr(e), _ptr(u), _ptr(d)))
        return s, e, u, d

    def expired_queue(self, prev_now, now, fetch=True):
        """Ascending rows with prev_now < end <= now.  fetch=False: leave the queue on the device, return its length."""
        q = C.c_size_t(0)
        if not fetch:
            self._check(self._lib.pie_expired_queue(self._ctx, int(prev_now), int(now), None, 0, C.byref(q)))
            return q.value
        out = np.empty(max(self.n, 1), np.int32)
        self._check(self._lib.pie_expired_queue(self._ctx, int(prev_now), int(now), _ptr(out), self.n, C.byref(q)))
        return out[: q.value].copy()

    def archive_queue(self, now, window_ms=43200000, fetch=True):
        """Rows of every group (user) whose earliest start is at least window_ms old, groups in first-appearance order.
        fetch=False: leave the queue on the device, return its length."""
        q = C.c_size_t(0)
        if not fetch:
            self._check(self._lib.pie_archive_queue(self._ctx, int(now), int(window_ms), None, 0, C.byref(q)))
            return q.value
        out = np.empty(max(self.n, 1), np.int32)
        self._check(self._lib.pie_archive_queue(self._ctx, int(now), int(window_ms), _ptr(out), self.n, C.byref(q)))
        return out[: q.value].copy()

    def queue_info(self):
        """-> (kind, rows, groups) of the queue the last expired_queue / archive_queue left on the device (kind 1 expired,
        2 archive).  PieError(PIE_E_STATE) when there is none or the table has rows its shard map does not cover."""
        kind, rows, groups = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_queue_info(self._ctx, C.byref(kind), C.byref(rows), C.byref(groups)))
        return kind.value, rows.value, groups.value

    def queue_pack_device(self, dst_ptr, cap_rows, cap_groups):
        """Pack that queue into device memory: [n_rows | n_groups | global rows (cap_rows) | local rows (cap_rows) |
        group offsets (cap_groups + 1)] int32 words, on the context's stream."""
        self._check(self._lib.pie_queue_pack_device(self._ctx, dst_ptr, int(cap_rows), int(cap_groups)))

    def archive_stats(self):
        """-> (device ms summed over the profiled archive chains, their number, algorithmic bytes of the last one)"""
        ms, calls, alg = C.c_double(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.pie_archive_stats(self._ctx, C.byref(ms), C.byref(calls), C.byref(alg)))
        return ms.value, calls.value, alg.value

    # ---- sharding on the device
    # ---- token index (pie_token_*): keys are uint64 arrays of shape (k, 2), see token_key
    def token_set(self, keys):
        """Keys for rows [0, len(keys)); replaces any earlier column and builds the index."""
        keys = _keys(keys)
        self._check(self._lib.pie_token_set(self._ctx, _ptr(keys), keys.shape[0]))

    def token_append(self, keys):
        """Keys for the rows behind the covered prefix; queued, not waited for."""
        keys = _keys(keys)
        self._check(self._lib.pie_token_append(self._ctx, _ptr(keys), keys.shape[0]))

    def token_lookup(self, keys, now):
        """getSession for every key -> dict of arrays: row (-1: not found), live, user, start, end."""
        keys = _keys(keys)
        k = keys.shape[0]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        self._check(self._lib.pie_token_lookup(self._ctx, _ptr(keys), k, int(now), _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]),
                                               _ptr(out["start"]), _ptr(out["end"])))
        return out

    def token_set_end(self, keys, new_end, now):
        """touchSession / deleteSession by token -> the row written per element (-1: unknown, expired or tombstoned)."""
        keys, new_end = _keys(keys), _col(new_end, np.int64)
        if new_end.shape[0] != keys.shape[0]:
            raise ValueError("one new_end per key")
        rows = np.empty(keys.shape[0], np.int32)
        self._check(self._lib.pie_token_set_end(self._ctx, _ptr(keys), _ptr(new_end), keys.shape[0], int(now), _ptr(rows)))
        return rows

    def _token_turn(self, fn, ops):
        ops = turn_ops(ops)
        k = ops.shape[0]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        self._check(fn(self._ctx, _ptr(ops), k, _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"])))
        return out

    def token_turn(self, ops):
        """A whole turn in one launch: ops is a TURN_OP array (or what turn_ops takes), applied in order, each op with its own
        clock -> the dict token_lookup returns, one entry per op (pie_token_turn: live = the call succeeded, end = the row's end
        after the op)."""
        return self._token_turn(self._lib.pie_token_turn, ops)

    def session_turn(self, ops, user=None, disc=None, n_users=None):
        """A turn that may log in (pie_session_turn): ops may carry kind TURN_CREATE, whose row is made of tok, start = now,
        end = new_end, user[i] and disc[i] (one entry per op; read at creates only; both may be None in a turn without one).
        n_users: the user count after the turn (default: unchanged) -> the dict token_turn returns."""
        ops = turn_ops(ops)
        k = ops.shape[0]
        user = None if user is None else _col(user, np.int32)
        disc = None if disc is None else _col(disc, np.int32)
        for a in (user, disc):
            if a is not None and a.shape != (k,):
                raise ValueError("one user and one disc per op")
        n_users = self.n_users if n_users is None else int(n_users)
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        self._check(self._lib.pie_session_turn(self._ctx, _ptr(ops), k, _ptr(user), _ptr(disc), n_users, _ptr(out["row"]), _ptr(out["live"]),
                                               _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"])))
        self.n += int(np.count_nonzero(ops["kind"] == TURN_CREATE))
        self.n_users = n_users
        return out

    def token_layout(self):
        """-> (covered, slots, slot_row[slots], keys[covered, 2]) of the index, for tests and tools."""
        cov, slots = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_token_layout(self._ctx, C.byref(cov), C.byref(slots), None, 0, None))
        slot_row, keys = np.empty(slots.value, np.int32), np.empty((cov.value, 2), np.uint64)
        self._check(self._lib.pie_token_layout(self._ctx, C.byref(cov), C.byref(slots), _ptr(slot_row), slots.value, _ptr(keys)))
        return cov.value, slots.value, slot_row, keys

    # ---- token lookups beside scans and batches (pie_token_lookup_begin / _finish): up to four begun and not finished
    def _token_lookup_begin(self, fn, keys, now):
        keys = _keys(keys)
        k = keys.shape[0]
        now = np.ascontiguousarray(np.broadcast_to(np.asarray(now, dtype=np.int64), (k,)))  # one clock per key
        self._check(fn(self._ctx, _ptr(keys), _ptr(now), k))
        self._lookups = getattr(self, "_lookups", [])
        self._lookups.append(k)   # keys of the lookups begun and not finished, oldest first: the sizes finish allocates

    def _token_lookup_finish(self, fn):
        begun = getattr(self, "_lookups", [])
        k = begun[0] if begun else 0   # (none begun: the library refuses with PIE_E_STATE below)
        got = C.c_size_t(0)
        while True:
            out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
                   "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
            rc = fn(self._ctx, _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"]), k, C.byref(got))
            if rc != PIE_E_CAPACITY or got.value <= k:
                break
            k = got.value   # a lookup begun past this object (the raw ABI): the library says how many keys it carries
        if begun and rc != PIE_E_STATE:   # the library returned the slot, finished or failed
            begun.pop(0)
        self._check(rc)
        return {name: a[: got.value] for name, a in out.items()}

    def token_lookup_begin(self, keys, now):
        """Queue getSession for every key (now: one clock for all, or one per key) whatever scans and batches are in flight."""
        self._token_lookup_begin(self._lib.pie_token_lookup_begin, keys, now)

    def token_lookup_finish(self):
        """The oldest lookup begun -> the dict token_lookup returns."""
        return self._token_lookup_finish(self._lib.pie_token_lookup_finish)

    def token_lookup_room(self):
        """Lookups token_lookup_begin would take now."""
        return int(self._lib.pie_token_lookup_room(self._ctx))

    def shard_token_lookup_begin(self, keys, now):
        """token_lookup_begin on a sharded context: rows and users will be answered as GLOBAL ids."""
        self._token_lookup_begin(self._lib.pie_shard_token_lookup_begin, keys, now)

    def shard_token_lookup_finish(self):
        """The oldest lookup begun -> the dict shard_token_lookup returns."""
        return self._token_lookup_finish(self._lib.pie_shard_token_lookup_finish)

    # ---- turns beside scans and batches (pie_token_turn_begin / _finish): up to four begun and not finished
    def _token_turn_begin(self, fn, ops):
        ops = turn_ops(ops)
        self._check(fn(self._ctx, _ptr(ops), ops.shape[0]))

    def _token_turn_finish(self, fn):
        got = C.c_size_t(0)
        rc = fn(self._ctx, None, None, None, None, None, 0, C.byref(got))   # its size (k = 0 finishes here); none begun: PIE_E_STATE
        if rc != PIE_E_CAPACITY:
            self._check(rc)
        k = got.value
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        if rc == PIE_E_CAPACITY:
            self._check(fn(self._ctx, _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"]), k, C.byref(got)))
        return out

    def token_turn_begin(self, ops):
        """Queue a whole turn (what token_turn takes) whatever scans and batches are in flight: scans and batches begun before
        it answer for the table before the turn, those begun after it see its writes."""
        self._token_turn_begin(self._lib.pie_token_turn_begin, ops)

    def token_turn_finish(self):
        """The oldest turn begun -> the dict token_turn returns."""
        return self._token_turn_finish(self._lib.pie_token_turn_finish)

    def token_turn_room(self):
        """Turns token_turn_begin would take now."""
        return int(self._lib.pie_token_turn_room(self._ctx))

    def shard_token_turn_begin(self, ops):
        """token_turn_begin on a sharded context: rows and users will be answered as GLOBAL ids."""
        self._token_turn_begin(self._lib.pie_shard_token_turn_begin, ops)

    def shard_token_turn_finish(self):
        """The oldest turn begun -> the dict shard_token_turn returns."""
        return self._token_turn_finish(self._lib.pie_shard_token_turn_finish)

    # ---- the expired queue beside scans and batches (pie_expired_queue_begin / _finish): one begun and not finished
    def _expired_queue_begin(self, fn, prev_now, now, cap_rows):
        cap = self.n if cap_rows is None else int(cap_rows)
        self._check(fn(self._ctx, int(prev_now), int(now), cap))
        self._expq_cap = cap   # the room the finish has to offer

    def _expired_queue_finish(self, fn):
        cap = getattr(self, "_expq_cap", 0)
        out = np.empty(max(cap, 1), np.int32)
        q = C.c_size_t(0)
        rc = fn(self._ctx, _ptr(out) if cap else None, cap, C.byref(q))
        if rc == PIE_E_CAPACITY:   # the queue outgrew the begin's cap_rows: its length and its first cap_rows rows go with the error
            err = PieError(rc, self._lib.pie_last_error(self._ctx).decode())
            err.length, err.prefix = q.value, out[:cap].copy()
            raise err
        self._check(rc)
        return out[: q.value].copy() if cap else q.value

    def expired_queue_begin(self, prev_now, now, cap_rows=None):
        """Queue the expired queue (ascending rows with prev_now < end <= now) whatever scans and batches are in flight.
        cap_rows: rows to make room for (default: every row of the table); 0 counts only."""
        self._expired_queue_begin(self._lib.pie_expired_queue_begin, prev_now, now, cap_rows)

    def expired_queue_finish(self):
        """The queue begun -> its rows (its length when the begin said cap_rows=0).  A queue longer than the begin's cap_rows
        raises PieError(PIE_E_CAPACITY) carrying .length and .prefix."""
        return self._expired_queue_finish(self._lib.pie_expired_queue_finish)

    def expired_queue_room(self):
        """1 when expired_queue_begin would be taken now, 0 while one is begun and not finished."""
        return int(self._lib.pie_expired_queue_room(self._ctx))

    def shard_expired_queue_begin(self, prev_now, now, cap_rows=None):
        """expired_queue_begin on a sharded context: the rows will be answered as GLOBAL rows."""
        self._expired_queue_begin(self._lib.pie_shard_expired_queue_begin, prev_now, now, cap_rows)

    def shard_expired_queue_finish(self):
        return self._expired_queue_finish(self._lib.pie_shard_expired_queue_finish)

    def expired_inflight_geometry(self, n):
        """How the in-flight pass cuts a table of n rows -> (rows_per_wave_step, rows_per_unit, blocks)."""
        step, unit, blocks = C.c_int32(0), C.c_int64(0), C.c_int32(0)
        self._check(self._lib.pie_expired_inflight_geometry(self._ctx, int(n), C.byref(step), C.byref(unit), C.byref(blocks)))
        return step.value, unit.value, blocks.value

    def shard_table(self, rank, world):
        """Keep only the rows of the users that hash to `rank` of `world`, users re-numbered densely.  -> (n_rows, n_users)"""
        n, u = C.c_size_t(0), C.c_int32(0)
        self._check(self._lib.pie_shard_table(self._ctx, int(rank), int(world), C.byref(n), C.byref(u)))
        self.n, self.n_users = int(n.value), int(u.value)
        return self.n, self.n_users

    def shard_maps(self, n_users_real=None):
        """-> (rows_global[n] int32, users_global[k] int32): local row -> global row, local user -> global user."""
        rows = np.empty(max(self.n, 1), np.int32)
        users = np.full(max(self.n_users, 1), -1, np.int32)
        self._check(self._lib.pie_shard_maps(self._ctx, _ptr(rows), _ptr(users)))
        return rows[: self.n], users

    # ---- a live sharded table: mutators by GLOBAL id (every shard is given the same call and keeps what is its own)
    def shard_info(self):
        """-> {rank, world, rows_global (N_g), users_global (U_g), map_bytes} of a context pie_shard_table left."""
        r, w, n, u, b = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int32(0), C.c_uint64(0)
        self._check(self._lib.pie_shard_info(self._ctx, C.byref(r), C.byref(w), C.byref(n), C.byref(u), C.byref(b)))
        return {"rank": r.value, "world": w.value, "rows_global": n.value, "users_global": u.value, "map_bytes": b.value}

    def shard_append_rows(self, start, end, user_global, disc, n_users_global, local_size=None):
        """The rows are rows [N_g, N_g + k) of the unsharded table, users as GLOBAL ids; this shard keeps the rows whose user
        hashes to it.  local_size = (rows, users) of the shard after the call, for a caller that knows them and must not
        wait: without it they are asked of pie_table_info_get, which waits once for the timing event of a hot-index build.
        -> (first global row, rows kept)"""
        start, end = _col(start, np.int64), _col(end, np.int64)
        user_global, disc = _col(user_global, np.int32), _col(disc, np.int32)
        k = start.shape[0]
        if not (end.shape[0] == user_global.shape[0] == disc.shape[0] == k):
            raise ValueError("column lengths differ")
        first, kept = C.c_int32(0), C.c_size_t(0)
        self._check(self._lib.pie_shard_append_rows(self._ctx, _ptr(start), _ptr(end), _ptr(user_global), _ptr(disc), k, int(n_users_global),
                                                    C.byref(first), C.byref(kept)))
        if local_size is not None:
            self.n, self.n_users = int(local_size[0]), int(local_size[1])
        else:
            ti = self.table_info()  # the shard's own rows and users, from the context (host state, but see local_size)
            self.n, self.n_users = int(ti["rows"]), int(ti["users"])
        return int(first.value), int(kept.value)

    def shard_set_end(self, rows_global, new_end):
        """end = new_end by GLOBAL row; rows this shard does not hold are skipped; repeats: the last element wins."""
        rows_global, new_end = _col(rows_global, np.int32), _col(new_end, np.int64)
        if rows_global.shape[0] != new_end.shape[0]:
            raise ValueError("rows and values differ in length")
        self._check(self._lib.pie_shard_set_end(self._ctx, _ptr(rows_global), _ptr(new_end), rows_global.shape[0]))

    # ---- the token column of a sharded context, by GLOBAL row (pie_shard_token_*)
    def shard_token_set(self, keys):
        """Keys for the global rows [0, len(keys)); the shard keeps those of the rows it holds.  Replaces any earlier column."""
        keys = _keys(keys)
        self._check(self._lib.pie_shard_token_set(self._ctx, _ptr(keys), keys.shape[0]))

    def shard_token_append(self, keys):
        """Keys for the global rows behind covered_g; queued, not waited for (unless the slot table must grow)."""
        keys = _keys(keys)
        self._check(self._lib.pie_shard_token_append(self._ctx, _ptr(keys), keys.shape[0]))

    def shard_token_lookup(self, keys, now):
        """getSession on this shard -> dict of arrays: row and user as GLOBAL ids (-1: this shard does not hold the key), live,
        start, end."""
        keys = _keys(keys)
        k = keys.shape[0]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        self._check(self._lib.pie_shard_token_lookup(self._ctx, _ptr(keys), k, int(now), _ptr(out["row"]), _ptr(out["live"]),
                                                     _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"])))
        return out

    def shard_token_set_end(self, keys, new_end, now):
        """touchSession / deleteSession by token on this shard -> the GLOBAL row written per element (-1: none)."""
        keys, new_end = _keys(keys), _col(new_end, np.int64)
        if new_end.shape[0] != keys.shape[0]:
            raise ValueError("one new_end per key")
        rows = np.empty(keys.shape[0], np.int32)
        self._check(self._lib.pie_shard_token_set_end(self._ctx, _ptr(keys), _ptr(new_end), keys.shape[0], int(now), _ptr(rows)))
        return rows

    def shard_session_turn(self, ops, user_global=None, disc=None, n_users_global=None, local_size=None):
        """A turn that may log in, on this shard (pie_shard_session_turn): every shard is given the same ops, users as GLOBAL
        ids (one per op, read at creates only; both arrays may be None in a turn without one).  n_users_global: the table's
        user count after the turn (default: unchanged).  local_size as in shard_append_rows -> the dict shard_token_turn
        returns; a create another shard keeps answers row -1 / live 0 / end PIE_END_NONE / user -1."""
        ops = turn_ops(ops)
        k = ops.shape[0]
        user_global = None if user_global is None else _col(user_global, np.int32)
        disc = None if disc is None else _col(disc, np.int32)
        for a in (user_global, disc):
            if a is not None and a.shape != (k,):
                raise ValueError("one user and one disc per op")
        if n_users_global is None:
            n_users_global = self.shard_info()["users_global"]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64)}
        self._check(self._lib.pie_shard_session_turn(self._ctx, _ptr(ops), k, _ptr(user_global), _ptr(disc), int(n_users_global),
                                                     _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]), _ptr(out["start"]),
                                                     _ptr(out["end"])))
        if local_size is not None:
            self.n, self.n_users = int(local_size[0]), int(local_size[1])
        else:
            ti = self.table_info()
            self.n, self.n_users = int(ti["rows"]), int(ti["users"])
        return out

    @staticmethod
    def shard_session_turn_plan(ops, user_global, rows_global0, rows_local0, rank, world):
        """Host only: see the module's shard_session_turn_plan."""
        return shard_session_turn_plan(ops, user_global, rows_global0, rows_local0, rank, world)

    def shard_token_turn(self, ops):
        """token_turn on this shard's column: rows and users as GLOBAL ids; a key the shard does not hold answers -1 / 0."""
        return self._token_turn(self._lib.pie_shard_token_turn, ops)

    def shard_token_layout(self):
        """-> (covered_global, covered_local, slots, slot_row[slots] of LOCAL rows, keys[covered_local, 2]), for tests and tools."""
        cg, cl, slots = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_shard_token_layout(self._ctx, C.byref(cg), C.byref(cl), C.byref(slots), None, 0, None))
        slot_row, keys = np.empty(slots.value, np.int32), np.empty((cl.value, 2), np.uint64)
        self._check(self._lib.pie_shard_token_layout(self._ctx, C.byref(cg), C.byref(cl), C.byref(slots), _ptr(slot_row), slots.value, _ptr(keys)))
        return cg.value, cl.value, slots.value, slot_row, keys

    def shard_delete_user(self, user_global):
        """-> ascending GLOBAL rows that were tombstoned (empty on a shard the user does not hash to)."""
        k = C.c_size_t(0)
        rows = np.empty(max(self.n, 1), np.int32)
        self._check(self._lib.pie_shard_delete_user(self._ctx, int(user_global), _ptr(rows), self.n, C.byref(k)))
        return rows[: k.value].copy()

    def shard_delete_users(self, users_global):
        """pie_delete_users by GLOBAL ids -> (ascending GLOBAL rows tombstoned, per_user); ids of other shards count 0."""
        users = _col(users_global, np.int32)
        k = C.c_size_t(0)
        rows = np.empty(max(self.n, 1), np.int32)
        per = np.zeros(users.shape[0], np.int32)
        self._check(self._lib.pie_shard_delete_users(self._ctx, _ptr(users), users.shape[0], _ptr(rows), self.n, C.byref(k), _ptr(per)))
        return rows[: k.value].copy(), per

    def shard_prune_before(self, cutoff, cap=None):
        """pie_prune_before on a shard -> the ascending GLOBAL rows tombstoned (cap: entries offered, default the shard's rows)."""
        k = C.c_size_t(0)
        cap = self.n if cap is None else int(cap)
        rows = np.empty(max(cap, 1), np.int32)
        self._check(self._lib.pie_shard_prune_before(self._ctx, int(cutoff), _ptr(rows), cap, C.byref(k)))
        return rows[: k.value].copy()

    def shard_retention_purge(self, now, months=2, tz_offset_ms=0, tz_table=None, cap=None):
        """pie_retention_purge / _tz on a shard -> the ascending GLOBAL rows tombstoned; tz_table as in retention_purge."""
        k = C.c_size_t(0)
        cap = self.n if cap is None else int(cap)
        rows = np.empty(max(cap, 1), np.int32)
        if tz_table is not None:
            T, off = _tz_pair(tz_table)
            self._check(self._lib.pie_shard_retention_purge_tz(self._ctx, int(now), int(months), _ptr(T), _ptr(off), int(T.shape[0]), _ptr(rows), cap,
                                                               C.byref(k)))
        else:
            self._check(self._lib.pie_shard_retention_purge(self._ctx, int(now), int(months), int(tz_offset_ms), _ptr(rows), cap, C.byref(k)))
        return rows[: k.value].copy()

    def shard_rows_to_local(self, rows_global):
        """Global rows -> this shard's local rows (-1: not held), as a new int32 array."""
        rows = np.array(rows_global, dtype=np.int32, copy=True).reshape(-1)
        self._check(self._lib.pie_shard_rows_to_local(self._ctx, _ptr(rows), rows.shape[0]))
        return rows

    def shard_rows_to_global(self, rows_local):
        """Local rows -> global rows (-1: outside the map), as a new int32 array."""
        rows = np.array(rows_local, dtype=np.int32, copy=True).reshape(-1)
        self._check(self._lib.pie_shard_rows_to_global(self._ctx, _ptr(rows), rows.shape[0]))
        return rows

    # ---- compaction on the device
    def compact_rows(self, dead_before=INT64_MIN, shrink=False):
        """Keep, in table order, the rows with end > dead_before (the default drops tombstones only); shrink: also re-size the
        table and its workspace to the kept rows.  -> the new row count."""
        k = C.c_size_t(0)
        self._check(self._lib.pie_compact_rows(self._ctx, int(dead_before), PIE_COMPACT_SHRINK if shrink else 0, C.byref(k)))
        self.n = int(k.value)
        return self.n

    def compact_maps(self):
        """-> (new_of_old[n_old] int32, -1 = dropped; old_of_new[n_kept] int32, ascending) of the last compaction."""
        n_old, n_kept = C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_compact_map_device_ptrs(self._ctx, None, None, C.byref(n_old), C.byref(n_kept)))
        new_of_old, old_of_new = np.empty(n_old.value, np.int32), np.empty(n_kept.value, np.int32)
        self._check(self._lib.pie_compact_maps(self._ctx, _ptr(new_of_old), _ptr(old_of_new), None, None))
        return new_of_old, old_of_new

    def compact_map_device_ptrs(self):
        """-> (new_of_old device address, old_of_new device address, n_old, n_kept)"""
        a, b, n_old, n_kept = _P(), _P(), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_compact_map_device_ptrs(self._ctx, C.byref(a), C.byref(b), C.byref(n_old), C.byref(n_kept)))
        return a.value, b.value, n_old.value, n_kept.value

    def compact_translate(self, rows):
        """Old row indices -> their new ones (-1: dropped, or not a row of the old table), as a new int32 array."""
        rows = np.array(rows, dtype=np.int32, copy=True).reshape(-1)
        self._check(self._lib.pie_compact_translate(self._ctx, _ptr(rows), rows.shape[0]))
        return rows

    def compact_geometry(self, n=None):
        """How the compaction passes cut a table of n rows (default: the resident one) ->
        {rows_per_wave_step, rows_per_block_step, rows_per_unit, blocks}."""
        a, b, u, g = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int32(0)
        self._check(self._lib.pie_compact_geometry(self._ctx, int(self.n if n is None else n), C.byref(a), C.byref(b), C.byref(u), C.byref(g)))
        return {"rows_per_wave_step": a.value, "rows_per_block_step": b.value, "rows_per_unit": u.value, "blocks": g.value}

    # ---- measurement / plumbing
    def set_stream(self, hip_stream):
        self._check(self._lib.pie_ctx_set_stream(self._ctx, hip_stream))

    def aux_stream(self):
        """hipStream_t (as int) on which scan tails and result copies / packs run."""
        p = _P()
        self._check(self._lib.pie_ctx_aux_stream(self._ctx, C.byref(p)))
        return p.value

    def set_profiling(self, every=1):
        """0/False: off; n: every n-th scan carries timing events."""
        self._check(self._lib.pie_set_profiling(self._ctx, int(every)))

    def stats(self):
        st = PieStats()
        st.struct_size = C.sizeof(PieStats)
        self._check(self._lib.pie_stats_get(self._ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in PieStats._fields_}

    def stats_reset(self):
        self._check(self._lib.pie_stats_reset(self._ctx))

    def synchronize(self):
        self._check(self._lib.pie_synchronize(self._ctx))


class PieComm:
    """The sharded table behind the C ABI: one scan context per GPU + an RCCL communicator (pie_comm_*).
    PieComm(device_ids) = one process drives all GPUs; PieComm.for_rank(id, rank, world, device) = one process per GPU."""

    def __init__(self, device_ids=None, _handle=None):
        self._lib = load_library()
        self._c = _P()
        if _handle is not None:
            self._c = _handle
        else:
            ids = (C.c_int32 * len(device_ids))(*[int(d) for d in device_ids])
            rc = self._lib.pie_comm_create(ids, len(device_ids), C.byref(self._c))
            if rc != 0:
                text = self._lib.pie_comm_last_error(None).decode()
                self._c = None
                raise PieError(rc, text)
        self.world = int(self._lib.pie_comm_world(self._c))
        self._step_nq, self._wide_nq = [], []   # n_q of the ordinary / wide steps begun and not yet finished, oldest first

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.pie_comm_unique_id(buf)
        if rc != 0:
            raise PieError(rc, lib.pie_comm_last_error(None).decode())
        return buf.raw

    @classmethod
    def for_rank(cls, unique_id, rank, world, device):
        lib = load_library()
        h = _P()
        rc = lib.pie_comm_create_rank(C.c_char_p(unique_id), int(rank), int(world), int(device), C.byref(h))
        if rc != 0:
            raise PieError(rc, lib.pie_comm_last_error(None).decode())
        return cls(_handle=h)

    def close(self):
        if getattr(self, "_c", None):
            self._lib.pie_comm_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise PieError(rc, self._lib.pie_comm_last_error(self._c).decode())

    def ctx(self, rank):
        """The shard's scan context as a PieScan (owned by the communicator: do not close it)."""
        h = self._lib.pie_comm_ctx(self._c, int(rank))
        if not h:
            raise PieError(-1, "rank %d is not local to this communicator" % rank)
        p = PieScan.__new__(PieScan)
        p._lib, p._ctx, p._begun = self._lib, _P(h), []
        p._m_buf, p._ready_buf = (C.c_size_t * PIE_BATCH_MAX)(), C.c_int(0)
        p._ready_ref = C.byref(p._ready_buf)
        st = PieStats()
        st.struct_size = C.sizeof(PieStats)
        p._check(self._lib.pie_stats_get(p._ctx, C.byref(st)))
        p.n, p.n_users = int(st.rows), int(st.users)
        p.close = lambda: None
        return p

    def gen_synthetic_sharded(self, seed, n_total, n_users, n_disc, flags=0):
        self._check(self._lib.pie_comm_gen_synthetic_sharded(self._c, seed, n_total, n_users, n_disc, flags))

    def reserve(self, n_q, u_pad, idx_cap):
        self._check(self._lib.pie_comm_reserve(self._c, int(n_q), int(u_pad), int(idx_cap)))

    def scan_batch_gather(self, queries, u_pad=0):
        """-> M[local rank][query]"""
        arr = PieScan._queries(queries)
        nl = int(self._lib.pie_comm_local_ranks(self._c))
        m = (C.c_size_t * (nl * len(queries)))()
        self._check(self._lib.pie_comm_scan_batch_gather(self._c, arr, len(queries), int(u_pad), m))
        return [[int(m[k * len(queries) + q]) for q in range(len(queries))] for k in range(nl)]

    # ---- the pipelined union exchange (pie_comm_step_*)
    def needed_cap(self):
        return int(self._lib.pie_comm_needed_cap(self._c))

    def step_reserve(self, n_q, u_pad=0, union_cap=1024):
        self._check(self._lib.pie_comm_step_reserve(self._c, int(n_q), int(u_pad), int(union_cap)))

    def step_begin(self, queries):
        arr = PieScan._queries(queries)
        self._check(self._lib.pie_comm_step_begin(self._c, arr, len(queries)))
        self._step_nq.append(len(queries))

    def step_finish(self):
        """-> M[local rank][query] of the oldest begun step; its exchange is queued, not waited for."""
        nq = self._step_nq.pop(0)
        nl = int(self._lib.pie_comm_local_ranks(self._c))
        m = (C.c_size_t * (nl * nq))()
        self._check(self._lib.pie_comm_step_finish(self._c, m))
        return [[int(m[k * nq + q]) for q in range(nq)] for k in range(nl)]

    def step_collect(self):
        """Wait for the oldest queued exchange.  -> its step number; PieError(PIE_E_CAPACITY) on every rank alike when a union
        outgrew the reserved capacity (needed_cap() says what to reserve)."""
        step = C.c_int64(-1)
        self._check(self._lib.pie_comm_step_collect(self._c, C.byref(step)))
        return int(step.value)

    def step_read_gathered(self, at_rank, src_rank, step):
        """-> (uoff[u_pad + 1] int32, rows[Mu] int32, masks[Mu] uint64) of src_rank's union message of `step` as at_rank holds it."""
        base, rs, up, cap = _P(), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_comm_step_gathered_ptr(self._c, int(at_rank), int(step), C.byref(base), C.byref(rs), C.byref(up), C.byref(cap)))
        uoff = np.empty(up.value + 1, np.int32)
        mu = C.c_size_t(0)
        self._check(self._lib.pie_comm_step_read_gathered(self._c, int(at_rank), int(src_rank), int(step), _ptr(uoff), None, None, 0, C.byref(mu)))
        rows, masks = np.empty(max(mu.value, 1), np.int32), np.empty(max(mu.value, 1), np.uint64)
        self._check(self._lib.pie_comm_step_read_gathered(self._c, int(at_rank), int(src_rank), int(step), None, _ptr(rows), _ptr(masks), mu.value, C.byref(mu)))
        return uoff, rows[: mu.value], masks[: mu.value]

    # ---- the pipelined WIDE union exchange (pie_comm_wide_step_*): up to PIE_WIDE_MAX queries per step
    def wide_step_reserve(self, n_q_max, u_pad=0, union_cap=1024):
        self._check(self._lib.pie_comm_wide_step_reserve(self._c, int(n_q_max), int(u_pad), int(union_cap)))

    def wide_step_begin(self, queries):
        queries = list(queries)      # marshalled on every call: no identity cache
        self._check(self._lib.pie_comm_wide_step_begin(self._c, PieScan._wide_queries(queries), len(queries)))
        self._wide_nq.append(len(queries))

    def wide_step_finish(self):
        """-> M[local rank][query] of the oldest begun wide step; its exchange is queued, not waited for."""
        nq = self._wide_nq[0]
        nl = int(self._lib.pie_comm_local_ranks(self._c))
        m = (C.c_size_t * (nl * nq))()
        rc = self._lib.pie_comm_wide_step_finish(self._c, m, nl * nq)
        if rc != PIE_E_CAPACITY:
            self._wide_nq.pop(0)
        self._check(rc)
        return [[int(m[k * nq + q]) for q in range(nq)] for k in range(nl)]

    def wide_step_collect(self):
        """Wait for the oldest queued wide exchange.  -> its step number.  PieError(PIE_E_CAPACITY) on every rank alike when a
        union outgrew the reserved capacity (needed_cap()) or some rank kept no union (wide_step_status shows -1: repeat)."""
        step = C.c_int64(-1)
        self._check(self._lib.pie_comm_wide_step_collect(self._c, C.byref(step)))
        return int(step.value)

    def wide_step_status(self, step):
        """-> int32[world]: the gathered Mu word of every rank for a collected step (-1: that rank kept no union)."""
        mu = np.empty(self.world, np.int32)
        self._check(self._lib.pie_comm_wide_step_status(self._c, int(step), mu.ctypes.data_as(C.POINTER(C.c_int32))))
        return mu

    def wide_step_read_gathered(self, at_rank, src_rank, step):
        """-> (uoff[u_pad + 1] int32, rows[k] int32, masks[k, words] uint64, Mu) of src_rank's wide message of `step` as at_rank
        holds it; k = min(Mu, reserved capacity)."""
        base, rs, up, cap, words = _P(), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        self._check(self._lib.pie_comm_wide_step_gathered_ptr(self._c, int(at_rank), int(step), C.byref(base), C.byref(rs), C.byref(up), C.byref(cap),
                                                              C.byref(words)))
        uoff = np.empty(up.value + 1, np.int32)
        mu = C.c_size_t(0)
        self._check(self._lib.pie_comm_wide_step_read_gathered(self._c, int(at_rank), int(src_rank), int(step), _ptr(uoff), None, None, 0, C.byref(words),
                                                               C.byref(mu)))
        k, w = min(mu.value, cap.value), int(words.value)
        rows, masks = np.empty(max(k, 1), np.int32), np.empty((max(k, 1), w), np.uint64)
        self._check(self._lib.pie_comm_wide_step_read_gathered(self._c, int(at_rank), int(src_rank), int(step), None, _ptr(rows), _ptr(masks), k,
                                                               C.byref(words), C.byref(mu)))
        return uoff, rows[:k], masks[:k], int(mu.value)

    def wide_step_read_feed(self, at_rank, src_rank, step, qi, local_user, idx_cap=64):
        """-> Feed(qi, local_user) of src_rank's shard (its local rows) read from the gathered message of `step`."""
        idx, k = np.empty(max(int(idx_cap), 1), np.int32), C.c_size_t(0)
        self._check(self._lib.pie_comm_wide_step_read_feed(self._c, int(at_rank), int(src_rank), int(step), int(qi), int(local_user), _ptr(idx),
                                                           int(idx_cap), C.byref(k)))
        return idx[: k.value].copy()

    # ---- cross-shard dispatch queues (pie_comm_expired_queue / pie_comm_archive_queue)
    def local_ranks(self):
        return [r for r in range(self.world) if self._lib.pie_comm_ctx(self._c, r)]

    def _queue(self, rc, sources):
        self._check(rc)
        return self.queue_read(self.local_ranks()[0], sources)

    def expired_queue(self, prev_now, now, sources=False):
        """Ascending global rows with prev_now < end <= now over every shard, merged on the devices.  sources=True:
        (rows, src_rank, src_row) — the shard that holds each row and its local row there."""
        q = C.c_size_t(0)
        return self._queue(self._lib.pie_comm_expired_queue(self._c, int(prev_now), int(now), None, 0, C.byref(q)), sources)

    def archive_queue(self, now, window_ms=43200000, sources=False):
        """The archive queue of the whole table (groups = users, ordered by the global row of their first queued row), merged on
        the devices.  sources=True: (rows, src_rank, src_row)."""
        q = C.c_size_t(0)
        return self._queue(self._lib.pie_comm_archive_queue(self._c, int(now), int(window_ms), None, 0, C.byref(q)), sources)

    # ---- a live sharded table (pie_comm_append_rows ...): GLOBAL ids, nothing exchanged
    def table_size(self):
        """-> (rows, users) of the whole table"""
        n, u = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.pie_comm_table_size(self._c, C.byref(n), C.byref(u)))
        return int(n.value), int(u.value)

    def append_rows(self, start, end, user, disc, n_users):
        """createSession on every local shard; -> the table's row count before the call (the first new global row)."""
        start, end = _col(start, np.int64), _col(end, np.int64)
        user, disc = _col(user, np.int32), _col(disc, np.int32)
        k = start.shape[0]
        if not (end.shape[0] == user.shape[0] == disc.shape[0] == k):
            raise ValueError("column lengths differ")
        first = C.c_int32(0)
        self._check(self._lib.pie_comm_append_rows(self._c, _ptr(start), _ptr(end), _ptr(user), _ptr(disc), k, int(n_users), C.byref(first)))
        return int(first.value)

    def set_end(self, rows, new_end):
        """touchSession / deleteSession by global row on every local shard."""
        rows, new_end = _col(rows, np.int32), _col(new_end, np.int64)
        if rows.shape[0] != new_end.shape[0]:
            raise ValueError("rows and values differ in length")
        self._check(self._lib.pie_comm_set_end(self._c, _ptr(rows), _ptr(new_end), rows.shape[0]))

    def delete_user(self, user):
        """deleteSessionsForUser by global id -> (ascending global rows tombstoned, owning rank or -1)."""
        cap = max(self.table_size()[0], 1)
        rows, k, owner = np.empty(cap, np.int32), C.c_size_t(0), C.c_int32(-1)
        self._check(self._lib.pie_comm_delete_user(self._c, int(user), _ptr(rows), cap, C.byref(k), C.byref(owner)))
        return rows[: k.value].copy(), int(owner.value)

    def delete_users(self, users):
        """deleteSessionsForUser for a set of global ids in one call on every local shard -> (ascending global rows tombstoned,
        per_user counts, owning rank per id or -1)."""
        users = _col(users, np.int32)
        cap = max(self.table_size()[0], 1)
        rows, k = np.empty(cap, np.int32), C.c_size_t(0)
        per, owners = np.zeros(users.shape[0], np.int32), np.full(users.shape[0], -1, np.int32)
        self._check(self._lib.pie_comm_delete_users(self._c, _ptr(users), users.shape[0], _ptr(rows), cap, C.byref(k), _ptr(per), _ptr(owners)))
        return rows[: k.value].copy(), per, owners

    # ---- a sharded table that ages (pie_comm_prune_before / _retention_purge* / _compact_rows)
    def local_rank_ids(self):
        """The ranks this process drives, ascending."""
        return [r for r in range(self.world) if self._lib.pie_comm_ctx(self._c, r)]

    def _maint(self, call, cap, sources):
        """cap: entries of the list to offer (default: the table's rows); the merged list stays readable through queue_read."""
        cap = max(self.table_size()[0], 1) if cap is None else int(cap)
        rows, k = np.empty(max(cap, 1), np.int32), C.c_size_t(0)
        self.last_n = 0
        rc = call(_ptr(rows), cap, C.byref(k))
        self.last_n = int(k.value)
        self._check(rc)
        if sources:
            return self.queue_read(self.local_rank_ids()[0], sources=True)
        return rows[: k.value].copy()

    def prune_before(self, cutoff, cap=None, sources=False):
        """_pruneCalendarEvents on every local shard -> the ascending global rows tombstoned, merged on the first local rank's
        device; sources=True: (rows, source rank, source local row).  last_n holds the total, also after PIE_E_CAPACITY."""
        return self._maint(lambda r, c, k: self._lib.pie_comm_prune_before(self._c, int(cutoff), r, c, k), cap, sources)

    def retention_purge(self, now, months=2, tz_offset_ms=0, tz_table=None, cap=None, sources=False):
        """_purgeExpiredArchives on every local shard (tz_table as in PieScan.retention_purge) -> as prune_before."""
        if tz_table is not None:
            T, off = _tz_pair(tz_table)
            return self._maint(lambda r, c, k: self._lib.pie_comm_retention_purge_tz(self._c, int(now), int(months), _ptr(T), _ptr(off),
                                                                                     int(T.shape[0]), r, c, k), cap, sources)
        return self._maint(lambda r, c, k: self._lib.pie_comm_retention_purge(self._c, int(now), int(months), int(tz_offset_ms), r, c, k),
                           cap, sources)

    def compact_rows(self, dead_before=INT64_MIN, shrink=False):
        """pie_compact_rows on every local shard; global rows keep their numbers -> (kept rows in all, kept rows per local shard)."""
        n_local = int(self._lib.pie_comm_local_ranks(self._c))
        total, per = C.c_size_t(0), (C.c_size_t * max(n_local, 1))()
        self._check(self._lib.pie_comm_compact_rows(self._c, int(dead_before), PIE_COMPACT_SHRINK if shrink else 0, C.byref(total), per))
        return int(total.value), [int(v) for v in per][:n_local]

    def queue_kind(self):
        """-> 0 none, 1 expired queue, 2 archive queue, 3 the list of a prune / retention purge"""
        return int(self._lib.pie_comm_queue_kind(self._c))

    # ---- the token column behind the communicator (pie_comm_token_*): keys are uint64 arrays of shape (k, 2), GLOBAL ids out
    def token_set(self, keys):
        """Keys for the global rows [0, len(keys)) on every local shard."""
        keys = _keys(keys)
        self._check(self._lib.pie_comm_token_set(self._c, _ptr(keys), keys.shape[0]))

    def token_append(self, keys):
        """Keys for the global rows behind the covered ones, on every local shard."""
        keys = _keys(keys)
        self._check(self._lib.pie_comm_token_append(self._c, _ptr(keys), keys.shape[0]))

    def token_lookup(self, keys, now):
        """getSession across the local shards -> dict of arrays: row (largest global row under the key, -1: none), live, user,
        start, end, owner (the rank that answered, -1: none)."""
        keys = _keys(keys)
        k = keys.shape[0]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64), "owner": np.empty(k, np.int32)}
        self._check(self._lib.pie_comm_token_lookup(self._c, _ptr(keys), k, int(now), _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]),
                                                    _ptr(out["start"]), _ptr(out["end"]), _ptr(out["owner"])))
        return out

    def token_set_end(self, keys, new_end, now):
        """touchSession / deleteSession by token -> the global row written per element (-1: unknown, expired or tombstoned)."""
        keys, new_end = _keys(keys), _col(new_end, np.int64)
        if new_end.shape[0] != keys.shape[0]:
            raise ValueError("one new_end per key")
        rows = np.empty(keys.shape[0], np.int32)
        self._check(self._lib.pie_comm_token_set_end(self._c, _ptr(keys), _ptr(new_end), keys.shape[0], int(now), _ptr(rows)))
        return rows

    def token_turn(self, ops):
        """A whole turn on every local shard, merged per op -> the dict token_lookup returns (owner included), one entry per op."""
        ops = turn_ops(ops)
        k = ops.shape[0]
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64), "owner": np.empty(k, np.int32)}
        self._check(self._lib.pie_comm_token_turn(self._c, _ptr(ops), k, _ptr(out["row"]), _ptr(out["live"]), _ptr(out["owner"]),
                                                  _ptr(out["user"]), _ptr(out["start"]), _ptr(out["end"])))
        return out

    def session_turn(self, ops, user=None, disc=None, n_users=None):
        """A turn that may log in, on every local shard, merged per op (pie_comm_session_turn): user / disc one entry per op in
        GLOBAL ids (read at creates only), n_users the table's user count after the turn (default: unchanged) -> the dict
        token_turn returns (owner included)."""
        ops = turn_ops(ops)
        k = ops.shape[0]
        user = None if user is None else _col(user, np.int32)
        disc = None if disc is None else _col(disc, np.int32)
        for a in (user, disc):
            if a is not None and a.shape != (k,):
                raise ValueError("one user and one disc per op")
        n_users = self.table_size()[1] if n_users is None else int(n_users)
        out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
               "start": np.empty(k, np.int64), "end": np.empty(k, np.int64), "owner": np.empty(k, np.int32)}
        self._check(self._lib.pie_comm_session_turn(self._c, _ptr(ops), k, _ptr(user), _ptr(disc), n_users, _ptr(out["row"]),
                                                    _ptr(out["live"]), _ptr(out["owner"]), _ptr(out["user"]), _ptr(out["start"]),
                                                    _ptr(out["end"])))
        return out

    # ---- token lookups and the expired queue while steps are in flight (pie_comm_token_lookup_begin ..., pie_comm_expired_queue_begin ...)
    def token_lookup_begin(self, keys, now):
        """Queue getSession for every key on every local shard (now: one clock for all, or one per key), whatever steps are in
        flight.  Up to four may be begun and not finished."""
        keys = _keys(keys)
        k = keys.shape[0]
        now = np.ascontiguousarray(np.broadcast_to(np.asarray(now, dtype=np.int64), (k,)))
        self._check(self._lib.pie_comm_token_lookup_begin(self._c, _ptr(keys), _ptr(now), k))

    def token_lookup_finish(self):
        """The oldest lookup begun -> the dict token_lookup returns (owner included)."""
        got = C.c_size_t(0)
        rc = self._lib.pie_comm_token_lookup_finish(self._c, None, None, None, None, None, None, 0, C.byref(got))   # its size; k = 0 finishes here
        if rc == PIE_E_CAPACITY:
            k = got.value
            out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32),
                   "start": np.empty(k, np.int64), "end": np.empty(k, np.int64), "owner": np.empty(k, np.int32)}
            rc = self._lib.pie_comm_token_lookup_finish(self._c, _ptr(out["row"]), _ptr(out["live"]), _ptr(out["user"]), _ptr(out["start"]),
                                                        _ptr(out["end"]), _ptr(out["owner"]), k, C.byref(got))
        else:
            out = {"row": np.empty(0, np.int32), "live": np.empty(0, np.uint8), "user": np.empty(0, np.int32),
                   "start": np.empty(0, np.int64), "end": np.empty(0, np.int64), "owner": np.empty(0, np.int32)}
        self._check(rc)
        return out

    def token_lookup_room(self):
        """Lookups token_lookup_begin would take now: the smallest room any local shard has left."""
        return int(self._lib.pie_comm_token_lookup_room(self._c))

    def expired_queue_begin(self, prev_now, now, cap_rows=None):
        """Queue the expired queue on every local shard, whatever steps are in flight.  cap_rows: rows to make room for (default:
        every row of the table); 0 counts only."""
        cap = self.table_size()[0] if cap_rows is None else int(cap_rows)
        self._check(self._lib.pie_comm_expired_queue_begin(self._c, int(prev_now), int(now), cap))
        self._expq_cap = cap

    def expired_queue_finish(self):
        """The queue begun -> (ascending global rows, owning rank of each), merged on the first local rank's device; its length
        when the begin said cap_rows=0.  A queue longer than the begin's cap_rows raises PieError(PIE_E_CAPACITY) carrying
        .length, .prefix and .prefix_owner."""
        cap = getattr(self, "_expq_cap", 0)
        rows, owner = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32)
        q = C.c_size_t(0)
        rc = self._lib.pie_comm_expired_queue_finish(self._c, _ptr(rows) if cap else None, _ptr(owner) if cap else None, cap, C.byref(q))
        if rc == PIE_E_CAPACITY:
            err = PieError(rc, self._lib.pie_comm_last_error(self._c).decode())
            err.length, err.prefix, err.prefix_owner = q.value, rows[:cap].copy(), owner[:cap].copy()
            raise err
        self._check(rc)
        return (rows[: q.value].copy(), owner[: q.value].copy()) if cap else q.value

    def expired_queue_room(self):
        """1 when expired_queue_begin would be taken now, else 0."""
        return int(self._lib.pie_comm_expired_queue_room(self._c))

    def inflight_queue_device_ptrs(self):
        """-> (rows device pointer, owner-rank device pointer, rows held, total) of the last expired_queue_finish."""
        rows, owner, n, q = _P(), _P(), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_comm_inflight_queue_device_ptrs(self._c, C.byref(rows), C.byref(owner), C.byref(n), C.byref(q)))
        return rows.value, owner.value, int(n.value), int(q.value)

    def queue_read(self, at_rank, sources=False):
        """The merged queue of the last queue call as local rank at_rank holds it."""
        q = C.c_size_t(0)
        self._check(self._lib.pie_comm_queue_read(self._c, int(at_rank), None, None, None, 0, C.byref(q)))
        rows, src_rank, src_row = (np.empty(max(q.value, 1), np.int32) for _ in range(3))
        self._check(self._lib.pie_comm_queue_read(self._c, int(at_rank), _ptr(rows), _ptr(src_rank) if sources else None,
                                                  _ptr(src_row) if sources else None, q.value, C.byref(q)))
        n = q.value
        return (rows[:n].copy(), src_rank[:n].copy(), src_row[:n].copy()) if sources else rows[:n].copy()

    def queue_timing(self):
        """-> device ms of the last queue call's phases on the first local rank's stream: (local queue + header exchange,
        pack, payload exchange, merge)"""
        ms = (C.c_float * 4)()
        self._check(self._lib.pie_comm_queue_timing(self._c, ms))
        return tuple(float(v) for v in ms)

    def read_gathered(self, at_rank, src_rank, qi):
        """-> (offsets[u_pad + 1] int32, idx[M] int32) of (src_rank, query qi) as rank at_rank holds it."""
        base, rs, qs, up = _P(), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._lib.pie_comm_gathered_device_ptr(self._c, int(at_rank), C.byref(base), C.byref(rs), C.byref(qs), C.byref(up)))
        off = np.empty(up.value + 1, np.int32)
        m = C.c_size_t(0)
        self._check(self._lib.pie_comm_read_gathered(self._c, int(at_rank), int(src_rank), int(qi), _ptr(off), None, 0, C.byref(m)))
        idx = np.empty(max(m.value, 1), np.int32)
        self._check(self._lib.pie_comm_read_gathered(self._c, int(at_rank), int(src_rank), int(qi), None, _ptr(idx), m.value, C.byref(m)))
        return off, idx[: m.value]


def split_wide_message(msg, u_pad, cap, words):
    """Pure numpy: a wide union message [uoff[0..u_pad] | Mu | rows[0..cap) | masks[0..cap) as 2 * words int32 per row] ->
    (uoff int32[u_pad + 1], Mu, rows int32[k], masks uint64[k, words]) with k = min(max(Mu, 0), cap); Mu = -1: no union."""
    msg = np.ascontiguousarray(msg, np.int32)
    u_pad, cap, words = int(u_pad), int(cap), int(words)
    if msg.shape[0] < u_pad + 2 + cap * (1 + 2 * words):
        raise ValueError("message shorter than u_pad + 2 + cap * (1 + 2 * words)")
    uoff = msg[: u_pad + 1].copy()
    mu = int(msg[u_pad + 1])
    k = min(max(mu, 0), cap)
    rows = msg[u_pad + 2: u_pad + 2 + k].copy()
    base = u_pad + 2 + cap
    masks = msg[base: base + k * 2 * words].astype("<i4").view("<u8").reshape(k, words).astype(np.uint64)
    return uoff, mu, rows, masks


def _keys(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.ndim != 2 or keys.shape[1] != 2:
        raise ValueError("token keys are a uint64 array of shape (k, 2)")
    return keys


def token_key(token):
    """The key of a session token: the first 16 bytes of sha256(token) (the reference's Map key, server/sessionStore.js:8-10)
    as two little-endian 64-bit words -> uint64 array of shape (2,)."""
    import hashlib
    if isinstance(token, str):
        token = token.encode("utf-8")
    return np.frombuffer(hashlib.sha256(token).digest()[:16], dtype="<u8").astype(np.uint64)


# pie_turn_op (include/pie_scan.h): one op of a turn, 40 bytes without padding
TURN_GET, TURN_TOUCH, TURN_DELETE = 0, 1, 2
TURN_CREATE = 3  # pie_session_turn, pie_shard_session_turn and pie_comm_session_turn only
TURN_OP = np.dtype([("tok", "<u8", (2,)), ("now", "<i8"), ("new_end", "<i8"), ("kind", "<i4"), ("reserved", "<i4")])
assert TURN_OP.itemsize == 40


def turn_ops(ops=None, keys=None, now=None, new_end=None, kind=None):
    """-> a contiguous TURN_OP array: `ops` as given (a TURN_OP array), or built from keys (k, 2), and now / new_end / kind
    (one value for all, or one per op)."""
    if ops is not None:
        ops = np.ascontiguousarray(ops)
        if ops.dtype != TURN_OP or ops.ndim != 1:
            raise ValueError("a turn is a one-dimensional array of binding.TURN_OP")
        return ops
    keys = _keys(keys)
    out = np.zeros(keys.shape[0], TURN_OP)
    out["tok"], out["now"], out["kind"] = keys, now, kind
    out["new_end"] = 0 if new_end is None else new_end
    return out


def token_turn_plan(ops):
    """Host only (pie_token_turn_plan): (next int32[k], head uint8[k]) — the next op with the same key (-1: none) and whether
    the op is the first of its key: the chains the device walks."""
    ops = turn_ops(ops)
    k = ops.shape[0]
    nxt, head = np.empty(k, np.int32), np.empty(k, np.uint8)
    rc = load_library().pie_token_turn_plan(_ptr(ops), k, _ptr(nxt), _ptr(head))
    if rc != 0:
        raise PieError(rc, "pie_token_turn_plan: bad argument")
    return nxt, head


def session_turn_plan(ops, row0):
    """Host only (pie_session_turn_plan): token_turn_plan's (next, head) plus new_row int32[k] — the row every TURN_CREATE op
    gets on a table of row0 rows (-1 for the other kinds) — and the number of creates."""
    ops = turn_ops(ops)
    k = ops.shape[0]
    nxt, head, new_row = np.empty(k, np.int32), np.empty(k, np.uint8), np.empty(k, np.int32)
    n_create = C.c_size_t(0)
    rc = load_library().pie_session_turn_plan(_ptr(ops), k, int(row0), _ptr(nxt), _ptr(head), _ptr(new_row), C.byref(n_create))
    if rc != 0:
        raise PieError(rc, "pie_session_turn_plan: bad argument")
    return nxt, head, new_row, int(n_create.value)


def shard_session_turn_plan(ops, user_global, rows_global0, rows_local0, rank, world):
    """Host only (pie_shard_session_turn_plan): token_turn_plan's (next, head), then new_row_global int32[k] — rows_global0 + j for
    the j-th TURN_CREATE op — and new_row_local int32[k] — rows_local0 + (the creates before it that rank `rank` of `world` keeps)
    for a create whose user hashes to the rank — both -1 elsewhere, then the number of creates and of kept creates."""
    ops = turn_ops(ops)
    k = ops.shape[0]
    user_global = None if user_global is None else _col(user_global, np.int32)
    if user_global is not None and user_global.shape != (k,):
        raise ValueError("one user per op")
    nxt, head = np.empty(k, np.int32), np.empty(k, np.uint8)
    row_g, row_l = np.empty(k, np.int32), np.empty(k, np.int32)
    n_create, n_kept = C.c_size_t(0), C.c_size_t(0)
    rc = load_library().pie_shard_session_turn_plan(_ptr(ops), k, _ptr(user_global), int(rows_global0), int(rows_local0), int(rank), int(world),
                                                    _ptr(nxt), _ptr(head), _ptr(row_g), _ptr(row_l), C.byref(n_create), C.byref(n_kept))
    if rc != 0:
        raise PieError(rc, "pie_shard_session_turn_plan: bad argument")
    return nxt, head, row_g, row_l, int(n_create.value), int(n_kept.value)


def token_slots_for(covered):
    return int(load_library().pie_token_slots_for(int(covered)))


def token_homes(keys, log2_slots):
    """Home slot of every key in an index of 2 ** log2_slots slots (pie_token_homes: the rule the device applies)."""
    keys = _keys(keys)
    out = np.empty(keys.shape[0], np.uint32)
    rc = load_library().pie_token_homes(_ptr(keys), keys.shape[0], int(log2_slots), _ptr(out))
    if rc != 0:
        raise PieError(rc, "pie_token_homes")
    return out


def shard_of(user, n_shards):
    return load_library().pie_shard_of(int(user), int(n_shards))


def shard_route(user_global, rank, world, users_before=0, users_after=0, cap=None):
    """Host only (pie_shard_route): (keep uint8[k], new users int32[]) — which rows of an append rank `rank` of `world` keeps, and
    the ascending ids in [users_before, users_after) that hash to it.  cap: room for the new users (default: all of them; a
    smaller one raises PieError -5 whose .n_new holds the number)."""
    user_global = _col(user_global, np.int32)
    k = user_global.shape[0]
    keep = np.empty(k, np.uint8)
    n_kept, n_new = C.c_size_t(0), C.c_size_t(0)
    room = max(int(users_after) - int(users_before), 0) if cap is None else int(cap)
    new = np.empty(max(room, 1), np.int32)
    rc = load_library().pie_shard_route(_ptr(user_global), k, int(rank), int(world), _ptr(keep), C.byref(n_kept), int(users_before),
                                        int(users_after), _ptr(new), room, C.byref(n_new))
    if rc != 0:
        err = PieError(rc, "pie_shard_route: %s" % ("cap %d < %d new users" % (room, n_new.value) if rc == -5 else "bad argument"))
        err.n_new = int(n_new.value)
        raise err
    assert int(keep.sum()) == n_kept.value
    return keep, new[: n_new.value].copy()


def set_end_last_writers(rows):
    """Host only (pie_set_end_last_writers): uint8[k], 1 where the element is the last occurrence of its row in `rows` — the
    elements of a set_end call that reach the device."""
    rows = _col(rows, np.int32)
    keep = np.empty(rows.shape[0], np.uint8)
    rc = load_library().pie_set_end_last_writers(_ptr(rows), rows.shape[0], _ptr(keep))
    if rc != 0:
        raise PieError(rc, "pie_set_end_last_writers: bad argument")
    return keep


def delete_users_plan(users, n_users):
    """Host only (pie_delete_users_plan): what delete_users uploads -> (bits uint64[(n_users + 63) // 64], first uint8[k]): the
    membership bitmap of the ids in [0, n_users), and 1 where an element is valid and the first occurrence of its value."""
    users = _col(users, np.int32)
    bits = np.full((max(int(n_users), 0) + 63) // 64, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)   # the call clears it
    first = np.full(users.shape[0], 255, np.uint8)
    rc = load_library().pie_delete_users_plan(_ptr(users), users.shape[0], int(n_users), _ptr(bits), _ptr(first))
    if rc != 0:
        raise PieError(rc, "pie_delete_users_plan: bad argument")
    return bits, first


def batch_mask_codes(queries, n_disc, start, end, disc, fallback=None):
    """Host only (pie_batch_mask_codes): per row the 20-bit code r | w << 7 | d << 14 the batched pass stores in a bucket slot,
    and that code expanded to the row's 64-bit query mask through the tables the library builds for `queries`.
    -> (codes uint32[n], masks uint64[n])"""
    arr = (PieQuery * len(queries))()
    for k, (now, cutoff, mask) in enumerate(queries):
        arr[k].now, arr[k].cutoff, arr[k].mask = int(now), int(cutoff), int(mask) & (2 ** 64 - 1)
    start, end, disc = _col(start, np.int64), _col(end, np.int64), _col(disc, np.int32)
    fb = None if fallback is None else _col(fallback, np.uint8)
    n = start.shape[0]
    codes, masks = np.empty(n, np.uint32), np.empty(n, np.uint64)
    rc = load_library().pie_batch_mask_codes(arr, len(queries), _ptr(fb), int(n_disc), _ptr(start), _ptr(end), _ptr(disc), n, _ptr(codes), _ptr(masks))
    if rc != 0:
        raise PieError(rc, "pie_batch_mask_codes: bad argument")
    return codes, masks


def _tz_pair(tz_table):
    T, off = np.ascontiguousarray(tz_table[0], np.int64), np.ascontiguousarray(tz_table[1], np.int64)
    if off.shape[0] != T.shape[0] + 1:
        raise ValueError("a table of n transitions carries n + 1 offsets")
    return T, off


def tz_table(zone, from_ms=0, to_ms=4102444800000):
    """Transition table of an IANA zone for retention_purge(tz_table=...): (transitions_utc_ms[n], offsets_ms[n + 1]), from
    Python's zoneinfo, probed day by day and bisected to the millisecond (the Node host builds the same table from the JS
    engine: host/tzTable.js)."""
    import datetime
    import zoneinfo
    z = zoneinfo.ZoneInfo(zone)
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    ms1 = datetime.timedelta(milliseconds=1)

    def off(ms):
        return int((epoch + datetime.timedelta(milliseconds=int(ms))).astimezone(z).utcoffset() / ms1)

    day = 86400000
    trans, offs = [], [off(from_ms)]
    prev_t, prev_o, t = from_ms, offs[0], from_ms + day
    while prev_t < to_ms:
        at = min(t, to_ms)
        o = off(at)
        if o != prev_o:
            lo, hi = prev_t, at
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if off(mid) == prev_o:
                    lo = mid
                else:
                    hi = mid
            trans.append(hi)
            offs.append(o)
            prev_o = o
        prev_t = at
        t += day
    return np.array(trans, np.int64), np.array(offs, np.int64)
