"""ctypes binding of libxflow_amd.so (include/xflow_amd.h).

The library is the product; this module only marshals pointers.  It never falls back to
a CPU implementation: a missing library or a missing GPU raises.
"""
import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XF_LIB") or os.path.join(_HERE, "lib", "libxflow_amd.so")

XF_OK = 0
OPT_FTRL, OPT_SGD = 0, 1
INIT_ZERO, INIT_CONST, INIT_HASHNORM = 0, 1, 2
# xf_table_defrag_path
(DEFRAG_NONE, DEFRAG_SORTFREE, DEFRAG_RADIX_ASKED, DEFRAG_RADIX_EXTENT, DEFRAG_RADIX_COUNT,
 DEFRAG_RADIX_CLUSTER) = range(6)
HEAVY_SEG = 64
FM_REFERENCE, FM_CANONICAL, FM_FIELD_AWARE = 0, 1, 2
FM_MODES = {"reference": FM_REFERENCE, "canonical": FM_CANONICAL, "field_aware": FM_FIELD_AWARE}
# xf_scalar_probe / xf_scalar_sweep
SCALAR_SIGMOID, SCALAR_SQRT, SCALAR_DIV, SCALAR_DIV_ROWS = range(4)

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
f32p = C.POINTER(C.c_float)
vp = C.c_void_p


class XFError(RuntimeError):
    pass


class TableConfig(C.Structure):
    _fields_ = [("opt_kind", C.c_int32), ("dim", C.c_int32), ("init_kind", C.c_int32),
                ("init_const", C.c_float), ("seed", C.c_uint64), ("alpha", C.c_float),
                ("beta", C.c_float), ("lambda1", C.c_float), ("lambda2", C.c_float),
                ("lr", C.c_float), ("capacity", C.c_uint64), ("shard", C.c_uint32),
                ("nshards", C.c_uint32)]


class ShardedConfig(C.Structure):
    _fields_ = [("model", C.c_int32), ("optimizer", C.c_int32), ("k", C.c_int32),
                ("schedule", C.c_int32), ("capacity", C.c_uint64), ("seed", C.c_uint64),
                ("alpha", C.c_float), ("beta", C.c_float), ("lambda1", C.c_float),
                ("lambda2", C.c_float), ("lr", C.c_float), ("host_key_build", C.c_int32),
                ("update_rule", C.c_int32)]


class DevBatch(C.Structure):
    _fields_ = [("R", C.c_uint32), ("NNZ", C.c_uint32), ("U", C.c_uint32), ("H", C.c_uint32),
                ("rowptr", vp), ("uidx", vp), ("ukeys", vp), ("segptr", vp), ("coo_row", vp),
                ("labels", vp), ("heavy", vp), ("P", C.c_uint32), ("fwd_ntiles", C.c_uint32),
                ("pptr", vp), ("pidx", vp), ("fwd_scratch", vp), ("fwd_tile_ptr", vp),
                ("fwd_panel_first", vp), ("fwd_grid", C.c_uint32), ("pad3_", C.c_uint32),
                ("ntiles", C.c_uint32),
                ("n_heavy_chunks", C.c_uint32), ("tile_ptr", vp), ("heavy_chunk_ptr", vp),
                ("heavy_scratch", vp)]


# name -> (restype, argtypes); every symbol include/xflow_amd.h declares
SIGNATURES = {
    "xf_last_error": (C.c_char_p, []),
    "xf_version": (C.c_int, []),
    "xf_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "xf_hash_bytes": (C.c_uint64, [C.c_char_p, C.c_size_t]),
    "xf_shard_of": (C.c_uint32, [C.c_uint64, C.c_uint32]),
    "xf_hash_decimal_range": (C.c_int, [C.c_uint64, C.c_size_t, u64p]),
    "xf_hash_decimal_ids": (C.c_int, [u64p, C.c_size_t, u64p]),
    "xf_reader_open": (C.c_int, [C.POINTER(vp), C.c_char_p, C.c_size_t]),
    "xf_reader_open_cached": (C.c_int, [C.POINTER(vp), C.c_char_p, C.c_size_t, C.c_char_p,
                                        C.POINTER(C.c_int)]),
    "xf_reader_close": (C.c_int, [vp]),
    "xf_reader_mapped": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "xf_block_create": (C.c_int, [C.POINTER(vp)]),
    "xf_block_destroy": (C.c_int, [vp]),
    "xf_reader_next_into": (C.c_int, [vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                      C.POINTER(u64p), C.POINTER(u64p), C.POINTER(i32p),
                                      C.POINTER(i32p)]),
    "xf_reader_peek_text": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
    "xf_reader_skip_text": (C.c_int, [vp]),
    "xf_reader_copy_text": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]),
    "xf_reader_parse_text": (C.c_int, [vp, vp, C.c_size_t, vp, C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_size_t), C.POINTER(u64p), C.POINTER(u64p),
                                       C.POINTER(i32p), C.POINTER(i32p)]),
    "xf_copy_to_host": (C.c_int, [vp, vp, C.c_size_t]),
    "xf_ingest_create": (C.c_int, [C.POINTER(vp), C.c_size_t]),
    "xf_ingest_destroy": (C.c_int, [vp]),
    "xf_ingest_staging": (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
    "xf_ingest_upload": (C.c_int, [vp, C.c_size_t, vp]),
    "xf_ingest_block": (C.c_int, [vp, vp, C.c_size_t, vp, C.POINTER(vp), C.POINTER(vp),
                                  C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_int)]),
    "xf_ingest_set_fields": (C.c_int, [vp, C.c_int, C.c_int]),
    "xf_ingest_fields": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "xf_reader_next": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                 C.POINTER(u64p), C.POINTER(u64p), C.POINTER(i32p),
                                 C.POINTER(i32p)]),
    "xf_reader_set_values": (C.c_int, [vp, C.c_int]),
    "xf_reader_values": (C.c_int, [vp, C.POINTER(f32p)]),
    "xf_block_values": (C.c_int, [vp, C.POINTER(f32p)]),
    "xf_batch_compile_valued": (C.c_int, [C.POINTER(vp), u64p, u64p, f32p, i32p, C.c_size_t,
                                          C.c_size_t]),
    "xf_batch_compile_valued_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, C.c_uint32,
                                              C.c_uint32, vp]),
    "xf_batch_compile_valued_gpu": (C.c_int, [C.POINTER(vp), u64p, u64p, f32p, i32p, C.c_size_t,
                                              C.c_size_t, vp]),
    "xf_batch_compile_fielded": (C.c_int, [C.POINTER(vp), u64p, u64p, i32p, f32p, i32p, C.c_size_t,
                                           C.c_size_t, C.c_int]),
    "xf_batch_compile_fielded_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, vp, C.c_uint32,
                                               C.c_uint32, C.c_int, vp]),
    "xf_batch_compile_fielded_gpu": (C.c_int, [C.POINTER(vp), u64p, u64p, i32p, f32p, i32p,
                                               C.c_size_t, C.c_size_t, C.c_int, vp]),
    "xf_batch_fields_dev": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(vp), C.POINTER(vp)]),
    "xf_batch_fields_host": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(u32p),
                                       C.POINTER(u32p)]),
    "xf_sharded_compile_fielded": (C.c_int, [vp, C.POINTER(vp), u64p, u64p, i32p, f32p, i32p,
                                             C.c_size_t, C.c_size_t, C.c_int]),
    "xf_sharded_compile_fielded_dev": (C.c_int, [vp, C.POINTER(vp), vp, vp, vp, vp, vp,
                                                 C.c_uint32, C.c_uint32, C.c_int]),
    "xf_sharded_set_fm_fields": (C.c_int, [vp, C.c_int]),
    "xf_workspace_fm_fields": (C.c_int, [vp, C.c_int]),
    "xf_batch_values_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "xf_batch_values_host": (C.c_int, [vp, C.POINTER(f32p), C.POINTER(f32p)]),
    "xf_sharded_compile_valued": (C.c_int, [vp, C.POINTER(vp), u64p, u64p, f32p, i32p,
                                            C.c_size_t, C.c_size_t, C.c_int]),
    "xf_sharded_compile_valued_dev": (C.c_int, [vp, C.POINTER(vp), vp, vp, vp, vp, C.c_uint32,
                                                C.c_uint32, C.c_int]),
    "xf_scratch_reserve": (C.c_int, [C.c_size_t]),
    "xf_batch_pool_reserve": (C.c_int, [C.c_size_t]),
    "xf_batch_compile": (C.c_int, [C.POINTER(vp), u64p, u64p, i32p, C.c_size_t, C.c_size_t]),
    "xf_batch_free": (C.c_int, [vp]),
    "xf_batch_compile_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, C.c_uint32, C.c_uint32, vp]),
    "xf_batch_compile_gpu": (C.c_int, [C.POINTER(vp), u64p, u64p, i32p, C.c_size_t,
                                       C.c_size_t, vp]),
    "xf_batch_compile_fm_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, vp, C.c_uint32,
                                          C.c_uint32, vp, C.POINTER(C.c_int)]),
    "xf_batch_compile_fm": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, vp, C.c_size_t,
                                      C.c_size_t, vp, C.POINTER(C.c_int)]),
    "xf_batch_download": (C.c_int, [vp]),
    "xf_batch_compile_local_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, C.c_uint32,
                                             C.c_uint32, C.c_int, vp]),
    "xf_batch_compile_local": (C.c_int, [C.POINTER(vp), vp, u64p, u64p, i32p, C.c_size_t,
                                         C.c_size_t, C.c_int, vp]),
    "xf_batch_compile_local_valued": (C.c_int, [C.POINTER(vp), vp, u64p, u64p, f32p, i32p,
                                                C.c_size_t, C.c_size_t, C.c_int, vp]),
    "xf_batch_compile_local_valued_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, vp,
                                                    C.c_uint32, C.c_uint32, C.c_int, vp]),
    "xf_batch_cells_info": (C.c_int, [vp, u32p]),
    "xf_sbatch_cells_info": (C.c_int, [vp, u32p]),
    "xf_batch_fwd_info": (C.c_int, [vp, u32p]),
    "xf_sbatch_fwd_info": (C.c_int, [vp, u32p]),
    "xf_fwd_windows_rule": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_int, u32p]),
    "xf_source_hash": (C.c_char_p, []),
    "xf_workspace_capture": (C.c_int, [vp, C.c_int]),
    "xf_workspace_parity": (C.c_int, [vp, C.c_int]),
    "xf_workspace_fm_mode": (C.c_int, [vp, C.c_int]),
    "xf_batch_dims": (C.c_int, [vp, u32p, u32p, u32p, u32p]),
    "xf_batch_host": (C.c_int, [vp, C.POINTER(u64p), C.POINTER(u32p), C.POINTER(u32p),
                                C.POINTER(u32p), C.POINTER(u32p), C.POINTER(i32p),
                                C.POINTER(u32p)]),
    "xf_batch_panels": (C.c_int, [vp, u32p, C.POINTER(u32p), C.POINTER(u32p)]),
    "xf_tune": (C.c_int, [C.c_char_p, C.c_double]),
    "xf_batch_tiles": (C.c_int, [vp, u32p, C.POINTER(u32p)]),
    "xf_batch_heavy_chunks": (C.c_int, [vp, u32p, C.POINTER(u32p)]),
    "xf_batch_fwd_tiles": (C.c_int, [vp, u32p, C.POINTER(u32p), C.POINTER(u32p), u32p]),
    "xf_batch_upload": (C.c_int, [vp, vp]),
    "xf_batch_dev_view": (C.c_int, [vp, C.POINTER(DevBatch)]),
    "xf_table_config_default": (None, [C.POINTER(TableConfig)]),
    "xf_table_create": (C.c_int, [C.POINTER(vp), C.POINTER(TableConfig)]),
    "xf_table_destroy": (C.c_int, [vp]),
    "xf_table_size": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "xf_table_settled": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "xf_table_defrag_path": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "xf_table_prepare_defrag": (C.c_int, [vp]),
    "xf_table_capacity": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "xf_table_reserve": (C.c_int, [vp, C.c_uint64]),
    "xf_table_defrag": (C.c_int, [vp]),
    "xf_table_evict": (C.c_int, [vp, C.c_float, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "xf_evict_shape": (None, [C.POINTER(C.c_uint32)]),
    "xf_table_set_hyper": (C.c_int, [vp] + [C.c_float] * 5),
    "xf_table_pull": (C.c_int, [vp, u64p, C.c_size_t, f32p]),
    "xf_table_push": (C.c_int, [vp, u64p, C.c_size_t, f32p]),
    "xf_table_resolve_dev": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "xf_table_gather_dev": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "xf_table_update_dev": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "xf_table_pull_dev": (C.c_int, [vp, vp, C.c_size_t, vp, vp, vp]),
    "xf_table_pull_ordered_dev": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, vp]),
    "xf_table_update_merged_dev": (C.c_int, [vp, vp, vp, C.c_size_t, vp, vp, vp]),
    "xf_lr_grad_update_dev": (C.c_int, [vp, C.POINTER(DevBatch), vp, vp, vp, vp, vp]),
    "xf_table_check": (C.c_int, [vp, vp]),
    "xf_table_export": (C.c_int, [vp, u64p, f32p, f32p, f32p, C.c_size_t,
                                  C.POINTER(C.c_size_t)]),
    "xf_table_import": (C.c_int, [vp, u64p, C.c_size_t, f32p, f32p, f32p]),
    "xf_table_w_derived": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "xf_table_div_exact": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "xf_div_by_const_probe": (C.c_int, [f32p, C.c_size_t, C.c_float, C.c_int, f32p]),
    "xf_scalar_probe": (C.c_int, [C.c_int, f32p, f32p, C.c_uint32, C.c_size_t, f32p]),
    "xf_scalar_sweep": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, u64p]),
    "xf_lr_forward_dev": (C.c_int, [C.POINTER(DevBatch), vp, vp, vp, vp]),
    "xf_lr_grad_dev": (C.c_int, [C.POINTER(DevBatch), vp, vp, vp]),
    "xf_fm_forward_dev": (C.c_int, [C.POINTER(DevBatch), C.c_int, vp, vp, vp, vp, vp, vp]),
    "xf_fm_grad_dev": (C.c_int, [C.POINTER(DevBatch), C.c_int, vp, vp, vp, vp, vp, vp]),
    "xf_fm_grad_update_dev": (C.c_int, [vp, vp, C.POINTER(DevBatch)] + [vp] * 9),
    "xf_workspace_create": (C.c_int, [C.POINTER(vp)]),
    "xf_workspace_destroy": (C.c_int, [vp]),
    "xf_lr_step": (C.c_int, [vp, vp, vp, vp]),
    "xf_lr_update_dev": (C.c_int, [C.POINTER(vp), vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int,
                                   vp, vp]),
    "xf_fm_step": (C.c_int, [vp, vp, vp, vp, vp]),
    "xf_lr_predict": (C.c_int, [vp, vp, vp, f32p]),
    "xf_fm_predict": (C.c_int, [vp, vp, vp, vp, f32p]),
    "xf_workspace_fetch": (C.c_int, [vp, f32p, f32p, f32p, C.c_size_t, C.c_size_t]),
    "xf_workspace_profile": (C.c_int, [vp, C.c_int]),
    "xf_workspace_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "xf_stream_sync": (C.c_int, [vp]),
    "xf_calib_stream": (C.c_int, [C.c_int, C.c_size_t, C.c_int]),
    "xf_group_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                  C.c_int]),
    "xf_group_destroy": (C.c_int, [vp]),
    "xf_group_abort": (C.c_int, [vp]),
    "xf_group_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "xf_group_barrier": (C.c_int, [vp]),
    "xf_group_allgather_host": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "xf_group_gatherv_host": (C.c_int, [vp, vp, C.c_size_t, vp, u64p]),
    "xf_group_alltoallv": (C.c_int, [vp, vp, u64p, vp, u64p, C.c_size_t, C.c_int, vp]),
    "xf_group_alltoallv_ch": (C.c_int, [vp, C.c_int, vp, u64p, vp, u64p, C.c_size_t, C.c_int,
                                        vp]),
    "xf_group_selftest": (C.c_int, [vp, C.c_size_t]),
    "xf_kb_debug_read": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_size_t, u32p]),
    "xf_sort_key_pos": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp, vp,
                                  C.POINTER(C.c_int)]),
    "xf_sharded_config_default": (None, [C.POINTER(ShardedConfig)]),
    "xf_sharded_create": (C.c_int, [C.POINTER(vp), vp, C.POINTER(ShardedConfig)]),
    "xf_sharded_destroy": (C.c_int, [vp]),
    "xf_sharded_compile": (C.c_int, [vp, C.POINTER(vp), u64p, u64p, i32p, C.c_size_t,
                                     C.c_size_t, C.c_int]),
    "xf_sharded_compile_dev": (C.c_int, [vp, C.POINTER(vp), vp, vp, vp, C.c_uint32, C.c_uint32,
                                         C.c_int]),
    "xf_sbatch_free": (C.c_int, [vp]),
    "xf_sbatch_dims": (C.c_int, [vp, u32p, u32p, u32p, u64p]),
    "xf_sbatch_fm_keyed": (C.c_int, [vp]),
    "xf_sharded_step": (C.c_int, [vp, vp]),
    "xf_sharded_predict": (C.c_int, [vp, vp, f32p]),
    "xf_sharded_flush": (C.c_int, [vp]),
    "xf_sharded_defrag": (C.c_int, [vp]),
    "xf_sharded_evict": (C.c_int, [vp, C.c_float, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64)]),
    "xf_sharded_check": (C.c_int, [vp]),
    "xf_sharded_set_schedule": (C.c_int, [vp, C.c_int]),
    "xf_sharded_set_parity": (C.c_int, [vp, C.c_int]),
    "xf_sharded_set_fm_mode": (C.c_int, [vp, C.c_int]),
    "xf_sharded_tables": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "xf_sharded_stream": (C.c_int, [vp, C.POINTER(vp)]),
    "xf_sharded_profile": (C.c_int, [vp, C.c_int]),
    "xf_sharded_profile_read": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "xf_sharded_save": (C.c_int, [vp, C.c_char_p]),
    "xf_sharded_load": (C.c_int, [vp, C.c_char_p]),
    "xf_auc_logloss": (C.c_int, [i32p, f32p, C.c_size_t, f32p, f32p, C.POINTER(C.c_int),
                                 C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "xf_admit_slot": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_int, C.c_int]),
    "xf_admit_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_uint64]),
    "xf_admit_create_shared": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int,
                                         C.c_uint64]),
    "xf_admit_range": (C.c_int, [C.c_int, C.c_int, C.c_int, u64p, u64p]),
    "xf_admit_range_of": (C.c_int, [vp, u64p, u64p]),
    "xf_admit_destroy": (C.c_int, [vp]),
    "xf_admit_params": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_uint64)]),
    "xf_admit_apply_dev": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp,
                                     C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(C.c_uint32)]),
    "xf_admit_apply": (C.c_int, [vp, C.c_int, u64p, u64p, i32p, f32p, i32p, C.c_size_t,
                                 C.c_size_t, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                 C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32)]),
    "xf_admit_export": (C.c_int, [vp, C.POINTER(C.c_uint8)]),
    "xf_admit_import": (C.c_int, [vp, C.POINTER(C.c_uint8)]),
    "xf_admit_save": (C.c_int, [vp, C.c_char_p]),
    "xf_admit_load": (C.c_int, [vp, C.c_char_p]),
    "xf_admit_stats": (C.c_int, [vp, u64p, u64p]),
    "xf_negsample_create": (C.c_int, [C.POINTER(vp), C.c_float, C.c_uint64]),
    "xf_negsample_destroy": (C.c_int, [vp]),
    "xf_negsample_params": (C.c_int, [vp, C.POINTER(C.c_float), u64p]),
    "xf_negsample_weight": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "xf_negsample_keep": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_float]),
    "xf_negsample_apply_dev": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp,
                                         C.c_uint32, C.c_uint32, vp, C.POINTER(vp),
                                         C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                         C.POINTER(vp), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32)]),
    "xf_negsample_apply": (C.c_int, [vp, C.c_uint64, C.c_uint64, u64p, u64p, i32p, f32p, i32p,
                                     C.c_size_t, C.c_size_t, vp, C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "xf_negsample_stats": (C.c_int, [vp, u64p, u64p, u64p, u64p]),
    "xf_workspace_neg_weight": (C.c_int, [vp, C.c_float]),
    "xf_weigh_negatives_launches": (C.c_uint64, []),
    "xf_lr_grad_launches": (None, [u64p]),
    "xf_cells_finalize_rows": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                         vp, vp, vp]),
    "xf_sharded_set_neg_weight": (C.c_int, [vp, C.c_float]),
    "xf_progress_create": (C.c_int, [C.POINTER(vp)]),
    "xf_progress_destroy": (C.c_int, [vp]),
    "xf_progress_rank": (C.c_uint32, [C.c_float]),
    "xf_progress_accumulate_dev": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
    "xf_progress_read": (C.c_int, [vp, u64p, u64p, C.c_int]),
    "xf_progress_launches": (C.c_uint64, []),
    "xf_progress_shape": (None, [C.POINTER(C.c_uint32)]),
    "xf_progress_summary": (C.c_int, [u64p, u64p, C.c_float, vp]),
    "xf_workspace_progress": (C.c_int, [vp, vp]),
    "xf_sharded_progress": (C.c_int, [vp, C.c_int]),
    "xf_sharded_progress_read": (C.c_int, [vp, u64p, u64p, C.c_int, C.c_int]),
    "xf_sharded_last_loss": (C.c_int, [vp, vp, f32p, C.c_size_t]),
    "xf_holdout_create": (C.c_int, [C.POINTER(vp), C.c_float, C.c_uint64]),
    "xf_holdout_destroy": (C.c_int, [vp]),
    "xf_holdout_params": (C.c_int, [vp, C.POINTER(C.c_float), u64p]),
    "xf_holdout_held": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_float]),
    "xf_holdout_split_dev": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp,
                                       C.c_uint32, C.c_uint32, vp, vp, vp]),
    "xf_holdout_split": (C.c_int, [vp, C.c_uint64, C.c_uint64, u64p, u64p, i32p, f32p, i32p,
                                   C.c_size_t, C.c_size_t, vp, vp, vp]),
    "xf_holdout_stats": (C.c_int, [vp, u64p, u64p, u64p]),
    "xf_holdout_shape": (None, [C.POINTER(C.c_uint32)]),
    "xf_holdout_should_stop": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double,
                                         C.POINTER(C.c_int)]),
    "xf_lr_validate": (C.c_int, [vp, vp, vp, vp]),
    "xf_fm_validate": (C.c_int, [vp, vp, vp, vp, vp]),
    "xf_sharded_holdout": (C.c_int, [vp, C.c_int]),
    "xf_sharded_validate": (C.c_int, [vp, vp]),
    "xf_sharded_holdout_read": (C.c_int, [vp, u64p, u64p, C.c_int, C.c_int]),
    "xf_slices_home": (C.c_uint64, [C.c_uint64, C.c_int]),
    "xf_slices_terms": (C.c_int, [C.POINTER(C.c_uint32)]),
    "xf_slices_check": (C.c_int, [C.c_int64, C.c_int64]),
    "xf_slices_summary": (C.c_int, [u64p, C.c_float, vp]),
    "xf_slices_create": (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int]),
    "xf_slices_destroy": (C.c_int, [vp]),
    "xf_slices_params": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "xf_slices_extract_dev": (C.c_int, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp,
                                        C.POINTER(vp)]),
    "xf_slices_extract": (C.c_int, [vp, u64p, u64p, i32p, C.c_size_t, C.c_size_t, vp,
                                    C.POINTER(vp), C.POINTER(C.c_uint32)]),
    "xf_slices_accumulate_dev": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp]),
    "xf_slices_read": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, C.c_int]),
    "xf_slices_launches": (C.c_uint64, []),
    "xf_slices_shape": (None, [C.POINTER(C.c_uint32)]),
    "xf_gauc_code": (C.c_uint32, [C.c_float, C.c_int32]),
    "xf_gauc_summary": (C.c_int, [u64p, C.c_uint64, u64p, u64p, vp, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
    "xf_gauc_create": (C.c_int, [C.POINTER(vp)]),
    "xf_gauc_destroy": (C.c_int, [vp]),
    "xf_gauc_reserve": (C.c_int, [vp, C.c_uint64]),
    "xf_gauc_append_dev": (C.c_int, [vp, vp, vp, vp, C.c_uint32, vp]),
    "xf_gauc_append": (C.c_int, [vp, u64p, C.POINTER(C.c_uint32), C.c_uint64]),
    "xf_gauc_export": (C.c_int, [vp, u64p, C.POINTER(C.c_uint32), C.c_uint64, u64p]),
    "xf_gauc_reduce": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, C.c_int]),
    "xf_gauc_launches": (C.c_uint64, []),
    "xf_gauc_shape": (None, [C.POINTER(C.c_uint32)]),
    "xf_workspace_gauc": (C.c_int, [vp, vp]),
    "xf_workspace_gauc_ids": (C.c_int, [vp, vp, C.c_uint32]),
    "xf_sharded_gauc": (C.c_int, [vp, C.c_int]),
    "xf_sharded_gauc_read": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, C.c_int,
                                       C.c_int]),
    "xf_workspace_slices": (C.c_int, [vp, vp]),
    "xf_workspace_slice_ids": (C.c_int, [vp, vp, C.c_uint32]),
    "xf_sharded_slices": (C.c_int, [vp, C.c_int, C.c_int32, C.c_int]),
    "xf_sbatch_set_slices": (C.c_int, [vp, vp, C.c_uint32]),
    "xf_sharded_slices_read": (C.c_int, [vp, u64p, C.c_uint64, u64p, u64p, u64p, C.c_int,
                                         C.c_int]),
    "xf_cross_key": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_int32, C.c_int32]),
    "xf_cross_parse": (C.c_int, [C.c_char_p, i32p, i32p, C.c_int, C.POINTER(C.c_int)]),
    "xf_cross_create": (C.c_int, [C.POINTER(vp), i32p, i32p, C.c_int, C.c_int32]),
    "xf_cross_destroy": (C.c_int, [vp]),
    "xf_cross_params": (C.c_int, [vp, i32p, i32p, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int32)]),
    "xf_cross_apply_dev": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_int,
                                     C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(C.c_uint32)]),
    "xf_cross_apply": (C.c_int, [vp, u64p, u64p, i32p, f32p, i32p, C.c_size_t, C.c_size_t, vp,
                                 C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                 C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32)]),
    "xf_cross_stats": (C.c_int, [vp, u64p, u64p, u64p]),
    "xf_rownorm_create": (C.c_int, [C.POINTER(vp), C.c_int]),
    "xf_rownorm_destroy": (C.c_int, [vp]),
    "xf_rownorm_apply_dev": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(vp),
                                       C.POINTER(vp)]),
    "xf_rownorm_apply": (C.c_int, [vp, u64p, u64p, i32p, f32p, i32p, C.c_size_t, C.c_size_t, vp,
                                   C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                   C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(vp)]),
    "xf_rownorm_row": (C.c_int, [f32p, C.c_size_t, f32p, C.POINTER(C.c_double)]),
    "xf_rownorm_stats": (C.c_int, [vp, u64p, u64p]),
    "xf_rownorm_shape": (None, [u32p]),
    "xf_rownorm_launches": (C.c_uint64, []),
    "XFCreate": (C.c_int, [C.POINTER(vp), C.c_char_p, C.c_char_p]),
    "XFStartTrain": (C.c_int, [C.POINTER(vp)]),
    "XFDestroy": (C.c_int, [C.POINTER(vp)]),
    "XFSetParam": (C.c_int, [vp, C.c_char_p, C.c_char_p]),
    "XFGetMetric": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_double)]),
    "XFGetTables": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "XFSaveModel": (C.c_int, [vp, C.c_char_p]),
    "XFLoadModel": (C.c_int, [vp, C.c_char_p]),
    "XFPredict": (C.c_int, [vp]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The torch wheel bundles its own libamdhip64.so.7; this
    library links the one under /opt/rocm.  Both have the same SONAME, so whichever is mapped
    first serves everybody — and torch finds no GPU when it is handed /opt/rocm's.  When torch
    is installed (it is only plumbing here: device buffers and process groups of the multi-GPU
    driver and of some tests) map ITS runtime first, whether or not torch gets imported later."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        try:
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the shared library; raise (never fall back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise XFError("libxflow_amd.so is not built: run `python -m xflow_amd.build` "
                          "(there is no CPU fallback)")
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        # the library says which sources it was built from: a prebuilt .so that is older than
        # the sources next to it (file times do not survive a snapshot) is an error, not a
        # silent stand-in.  XF_LIB (an experiment's variant build) is taken as it is.
        if "XF_LIB" not in os.environ:
            from . import build as _build
            built, want = L.xf_source_hash().decode(), _build.source_hash()
            if built != want:
                raise XFError("libxflow_amd.so was built from other sources (library %s, "
                              "sources %s): run `python -m xflow_amd.build`" % (built, want))
        _lib = L
    return _lib


def check(rc):
    if rc != XF_OK:
        raise XFError("xflow_amd error %d: %s" % (rc, lib().xf_last_error().decode()))


def require_gpu():
    n = C.c_int(0)
    check(lib().xf_device_count(C.byref(n)))
    if n.value < 1:
        raise XFError("no HIP device visible: the xflow_amd hot path runs only on the GPU")
    return n.value


def _p(a, t):
    return a.ctypes.data_as(t)


def hash_str(s):
    b = s if isinstance(s, bytes) else str(s).encode()
    return int(lib().xf_hash_bytes(b, len(b)))


_tuned = {}


def tune(name, value):
    check(lib().xf_tune(name.encode(), float(value)))
    _tuned[name] = float(value)


def tuned(name, default=0.0):
    """the value tune() last gave a knob in this process (the library's default: `default`)"""
    return _tuned.get(name, default)


def hash_decimal_range(start, n):
    out = np.empty(n, dtype=np.uint64)
    check(lib().xf_hash_decimal_range(start, n, _p(out, u64p)))
    return out


def sort_key_pos(keys, lo=0, span=2**64 - 1, repeat=0):
    """xf_sort_key_pos on a host array (through torch: plumbing): (sorted keys, their positions,
    by_hand[, ms per call over `repeat` calls])"""
    import torch
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n = len(keys)
    dk = torch.from_numpy(keys.view(np.int64).copy()).cuda() if n else torch.zeros(1, dtype=torch.int64).cuda()
    sk = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
    sp = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h = C.c_int(0)
    args = (dk.data_ptr(), n, lo, span, sk.data_ptr(), sp.data_ptr(), None, C.byref(h))
    check(lib().xf_sort_key_pos(*args))
    ms = None
    if repeat:
        import time
        check(lib().xf_stream_sync(None))
        t0 = time.perf_counter()
        for _ in range(repeat):
            check(lib().xf_sort_key_pos(*args))
        check(lib().xf_stream_sync(None))
        ms = (time.perf_counter() - t0) * 1e3 / repeat
    out = (sk.cpu().numpy().view(np.uint64)[:n], sp.cpu().numpy().view(np.uint32)[:n], bool(h.value))
    return out + (ms,) if repeat else out


def hash_decimal_ids(ids):
    """hash of the decimal string of every id (io.h:53 on str(id))"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    out = np.empty(len(ids), dtype=np.uint64)
    check(lib().xf_hash_decimal_ids(_p(ids, u64p), len(ids), _p(out, u64p)))
    return out


def read_blocks(path, cap_bytes, cache_path=None, info=None, values=False):
    """Yield (rowptr, keys, fgid, labels) numpy copies per text block.  With `cache_path` the
    blocks come from / go to the binarized block cache; info["from_cache"] says which.
    values=True: the feature values (float32, beside keys) as a fifth array."""
    L = lib()
    h = vp()
    if cache_path is None:
        check(L.xf_reader_open(C.byref(h), path.encode(), cap_bytes))
    else:
        hit = C.c_int(0)
        check(L.xf_reader_open_cached(C.byref(h), path.encode(), cap_bytes, cache_path.encode(),
                                      C.byref(hit)))
        if info is not None:
            info["from_cache"] = bool(hit.value)
    try:
        if values:
            check(L.xf_reader_set_values(h, 1))
        while True:
            rows, nnz = C.c_size_t(0), C.c_size_t(0)
            rp, ks, fg, lb = u64p(), u64p(), i32p(), i32p()
            check(L.xf_reader_next(h, C.byref(rows), C.byref(nnz), C.byref(rp), C.byref(ks),
                                   C.byref(fg), C.byref(lb)))
            if rows.value == 0:
                return
            r, n = rows.value, nnz.value
            blk = (np.ctypeslib.as_array(rp, (r + 1,)).copy(),
                   np.ctypeslib.as_array(ks, (n,)).copy() if n else np.zeros(0, np.uint64),
                   np.ctypeslib.as_array(fg, (n,)).copy() if n else np.zeros(0, np.int32),
                   np.ctypeslib.as_array(lb, (r,)).copy())
            if values:
                vs = f32p()
                check(L.xf_reader_values(h, C.byref(vs)))
                blk += (np.ctypeslib.as_array(vs, (n,)).copy() if n else np.zeros(0, np.float32),)
            yield blk
    finally:
        L.xf_reader_close(h)


def read_text_blocks(path, cap_bytes):
    """Yield every block of `path` as TEXT (bytes), by the reader's block rule
    (xf_reader_peek_text / xf_reader_skip_text)."""
    L = lib()
    r = vp()
    check(L.xf_reader_open(C.byref(r), path.encode(), cap_bytes))
    try:
        while True:
            t, n = vp(), C.c_size_t()
            check(L.xf_reader_peek_text(r, C.byref(t), C.byref(n)))
            if n.value == 0:
                return
            yield C.string_at(t.value, n.value)
            check(L.xf_reader_skip_text(r))
    finally:
        L.xf_reader_close(r)


def parse_text_block(text, cap_bytes=1 << 26, values=False):
    """(rowptr, keys, fgid, labels) of one block's text through the HOST parser
    (xf_reader_parse_text); raises XFError where the host parser rejects the block.
    values=True: the feature values (float32, beside keys) as a fifth array."""
    import tempfile
    L = lib()
    r, blk = vp(), vp()
    with tempfile.NamedTemporaryFile() as f:     # (a reader to borrow the thread team from)
        f.write(b"0\t0:0:0\n")
        f.flush()
        check(L.xf_reader_open(C.byref(r), f.name.encode(), cap_bytes))
    check(L.xf_block_create(C.byref(blk)))
    try:
        if values:
            check(L.xf_reader_set_values(r, 1))
        rows, nnz = C.c_size_t(), C.c_size_t()
        rp, ks, fg, lb = u64p(), u64p(), i32p(), i32p()
        buf = C.create_string_buffer(text, len(text) + 16)
        check(L.xf_reader_parse_text(r, buf, len(text), blk, C.byref(rows), C.byref(nnz),
                                     C.byref(rp), C.byref(ks), C.byref(fg), C.byref(lb)))
        R, N = rows.value, nnz.value
        out = (np.ctypeslib.as_array(rp, (R + 1,)).copy(),
               np.ctypeslib.as_array(ks, (max(N, 1),))[:N].copy(),
               np.ctypeslib.as_array(fg, (max(N, 1),))[:N].copy(),
               np.ctypeslib.as_array(lb, (max(R, 1),))[:R].copy())
        if values:
            vs = f32p()
            check(L.xf_block_values(blk, C.byref(vs)))
            out += (np.ctypeslib.as_array(vs, (N,)).copy() if N else np.zeros(0, np.float32),)
        return out
    finally:
        L.xf_block_destroy(blk)
        L.xf_reader_close(r)


class Ingest:
    """The GPU tokeniser (xf_ingest_*): text block -> device arrays (keys, rowptr, labels; after
    fields(): also fgid and the feature values)."""

    def __init__(self, max_text_bytes=1 << 26):
        self.h = vp()
        check(lib().xf_ingest_create(C.byref(self.h), max_text_bytes))

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_ingest_destroy(self.h)
            self.h = None

    def block_dev(self, text, stream=None):
        """(ok, rows, nnz, d_keys, d_rowptr, d_labels): device pointers owned by the object"""
        dk, dr, dl = vp(), vp(), vp()
        rows, nnz, ok = C.c_uint32(), C.c_uint32(), C.c_int()
        buf = C.create_string_buffer(text, len(text) + 1)
        check(lib().xf_ingest_block(self.h, buf, len(text), stream, C.byref(dk), C.byref(dr),
                                    C.byref(dl), C.byref(rows), C.byref(nnz), C.byref(ok)))
        return bool(ok.value), rows.value, nnz.value, dk.value, dr.value, dl.value

    def block(self, text):
        """(ok, rowptr, keys, labels) as numpy arrays (copied back from the device); the arrays
        are None when the block is not of the common shape"""
        ok, R, N, dk, dr, dl = self.block_dev(text)
        if not ok:
            return False, None, None, None
        rp, ks, lb = np.zeros(R + 1, np.uint32), np.zeros(N, np.uint64), np.zeros(R, np.int32)
        for a, ptr in ((rp, dr), (ks, dk), (lb, dl)):
            if a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return True, rp, ks, lb

    def fields(self, fgid=False, values=False):
        """the blocks that follow: field0 read as fgid and / or the third field as the feature
        value (xf_ingest_set_fields); tokens outside the two classes hand their block back"""
        check(lib().xf_ingest_set_fields(self.h, 1 if fgid else 0, 1 if values else 0))
        return self

    def block_fields(self, text):
        """(ok, rowptr, keys, labels, fgid, vals): block() with the arrays fields() asked for
        (int32 / float32 beside keys; None for one that was not asked for, all None when the
        block was handed back)"""
        ok, R, N, dk, dr, dl = self.block_dev(text)
        if not ok:
            return False, None, None, None, None, None
        dfg, dv = vp(), vp()
        check(lib().xf_ingest_fields(self.h, C.byref(dfg), C.byref(dv)))
        rp, ks, lb = np.zeros(R + 1, np.uint32), np.zeros(N, np.uint64), np.zeros(R, np.int32)
        fg = np.zeros(N, np.int32) if dfg.value else None
        vs = np.zeros(N, np.float32) if dv.value else None
        for a, ptr in ((rp, dr), (ks, dk), (lb, dl), (fg, dfg.value), (vs, dv.value)):
            if a is not None and a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return True, rp, ks, lb, fg, vs


def admit_slot(key, seed, log2_slots, j):
    """slot_j(key) of a filter with this seed and 2^log2_slots counters (xf_admit_slot; host code)"""
    return int(lib().xf_admit_slot(int(key), int(seed), int(log2_slots), int(j)))


def admit_range(log2_slots, world, rank):
    """(first slot, number of slots) that `rank` of `world` owns of a shared filter's 2^log2_slots
    counters (xf_admit_range; host code)"""
    first, n = C.c_uint64(), C.c_uint64()
    check(lib().xf_admit_range(int(log2_slots), int(world), int(rank), C.byref(first),
                               C.byref(n)))
    return first.value, n.value


class AdmitDev(collections.namedtuple(
        "AdmitDev", "d_keys d_rowptr d_labels R NNZ d_fgid d_vals")):
    """A filtered minibatch on the device: pointers (ints; None for an array that was not given)
    owned by the Admit object, valid until its next apply.  The first five fields are
    Sharded.compile_dev's arguments, compile_valued_dev takes d_vals in second place."""


class Admit:
    """Feature admission (xf_admit_*): a counting Bloom filter over 2^log2_slots saturating 8-bit
    counters.  apply() counts a minibatch's nonzeros (update=True) and returns the minibatch
    without the nonzeros whose key the filter has not seen `count` times.  group: one filter
    shared by the group's ranks (xf_admit_create_shared) — creation, apply, save and load are
    collective, export / import_ move this rank's range [first_slot, first_slot + n_slots)."""

    def __init__(self, log2_slots, count, hashes=3, seed=0, group=None):
        self.h = vp()
        self.log2_slots, self.count, self.hashes, self.seed = log2_slots, count, hashes, seed
        self.group = group          # (the filter uses the group: it must outlive it)
        if group is None:
            check(lib().xf_admit_create(C.byref(self.h), log2_slots, hashes, count, seed))
        else:
            check(lib().xf_admit_create_shared(C.byref(self.h), group.h, log2_slots, hashes,
                                               count, seed))

    def _range(self):
        first, n = C.c_uint64(), C.c_uint64()
        check(lib().xf_admit_range_of(self.h, C.byref(first), C.byref(n)))
        return first.value, n.value

    first_slot = property(lambda self: self._range()[0])
    n_slots = property(lambda self: self._range()[1])

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_admit_destroy(self.h)
            self.h = None

    def slot(self, key, j):
        return admit_slot(key, self.seed, self.log2_slots, j)

    def apply_dev(self, rowptr, keys, labels=None, fgid=None, values=None, update=True,
                  stream=None):
        """host arrays in (uploaded as they are), the filtered minibatch as an AdmitDev out"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(rowptr) >= 1 and int(rowptr[-1]) - int(rowptr[0]) <= len(keys)
        R = len(rowptr) - 1
        args = []
        for a, dt, pt in ((fgid, np.int32, i32p), (values, np.float32, f32p)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                assert len(a) == len(keys), "one entry per key"
                a = a if len(a) else np.zeros(1, dt)
            args.append((a, pt))
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            assert len(labels) == R, "one label per row"
            labels = labels if R else np.zeros(1, np.int32)
        args.append((labels, i32p))
        if len(keys) == 0:
            keys = np.zeros(1, np.uint64)
        ptr = [(_p(a, pt) if a is not None else None) for a, pt in args]
        dk, dfg, dv, dr, dl = vp(), vp(), vp(), vp(), vp()
        Ro, No = C.c_uint32(), C.c_uint32()
        check(lib().xf_admit_apply(self.h, 1 if update else 0, _p(rowptr, u64p), _p(keys, u64p),
                                   ptr[0], ptr[1], ptr[2], 0, R, stream, C.byref(dk),
                                   C.byref(dfg), C.byref(dv), C.byref(dr), C.byref(dl),
                                   C.byref(Ro), C.byref(No)))
        return AdmitDev(dk.value, dr.value, dl.value, Ro.value, No.value, dfg.value, dv.value)

    def filter_dev(self, d_keys, d_rowptr, R, NNZ, d_fgid=None, d_vals=None, update=True,
                   stream=None):
        """xf_admit_apply_dev: device pointers in (ints), (d_keys, d_rowptr, NNZ, d_fgid, d_vals)
        of the filtered minibatch out; labels and R are the caller's, untouched"""
        dk, dfg, dv, dr = vp(), vp(), vp(), vp()
        No = C.c_uint32()
        check(lib().xf_admit_apply_dev(self.h, 1 if update else 0, d_keys, d_fgid, d_vals,
                                       d_rowptr, R, NNZ, stream, C.byref(dk), C.byref(dfg),
                                       C.byref(dv), C.byref(dr), C.byref(No)))
        return dk.value, dr.value, No.value, dfg.value, dv.value

    def apply(self, rowptr, keys, labels=None, fgid=None, values=None, update=True):
        """the filtered host arrays (downloaded): (rowptr uint32, keys) and then, for each of
        labels / fgid / values that was given, its filtered array in that order"""
        d = self.apply_dev(rowptr, keys, labels, fgid, values, update)
        rp, ks = np.zeros(d.R + 1, np.uint32), np.zeros(d.NNZ, np.uint64)
        out = [(rp, d.d_rowptr), (ks, d.d_keys)]
        if labels is not None:
            out.append((np.zeros(d.R, np.int32), d.d_labels))
        if fgid is not None:
            out.append((np.zeros(d.NNZ, np.int32), d.d_fgid))
        if values is not None:
            out.append((np.zeros(d.NNZ, np.float32), d.d_vals))
        for a, ptr in out:
            if a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return tuple(a for a, _ in out)

    def export(self):
        n = self.n_slots
        out = np.empty(max(n, 1), np.uint8)
        check(lib().xf_admit_export(self.h, _p(out, C.POINTER(C.c_uint8))))
        return out[:n]

    def import_(self, counters):
        counters = np.ascontiguousarray(counters, dtype=np.uint8)
        assert len(counters) == self.n_slots
        counters = counters if len(counters) else np.zeros(1, np.uint8)
        check(lib().xf_admit_import(self.h, _p(counters, C.POINTER(C.c_uint8))))

    def save(self, path):
        check(lib().xf_admit_save(self.h, str(path).encode()))

    def load(self, path):
        check(lib().xf_admit_load(self.h, str(path).encode()))

    def stats(self):
        """(nonzeros seen, nonzeros kept), summed over the update=True applies"""
        seen, kept = C.c_uint64(), C.c_uint64()
        check(lib().xf_admit_stats(self.h, C.byref(seen), C.byref(kept)))
        return seen.value, kept.value


def negsample_keep(seed, stream, ordinal, keep):
    """whether a NEGATIVE row of this ordinal is kept (xf_negsample_keep; host code, the kernels'
    own definition)"""
    return bool(lib().xf_negsample_keep(int(seed), int(stream), int(ordinal), float(keep)))


class NegSample:
    """Negative subsampling (xf_negsample_*): apply() keeps every positive row of a minibatch and
    a negative row with probability `keep`, decided by a hash of (seed, stream, the row's ordinal);
    weight is what a trainer multiplies a kept negative's loss by (Workspace.neg_weight,
    Sharded.set_neg_weight).  Stateless but for the statistics."""

    def __init__(self, keep, seed=0):
        self.h = vp()
        self.keep, self.seed = float(np.float32(keep)), seed
        check(lib().xf_negsample_create(C.byref(self.h), keep, seed))

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_negsample_destroy(self.h)
            self.h = None

    @property
    def weight(self):
        w = C.c_float()
        check(lib().xf_negsample_weight(self.h, C.byref(w)))
        return np.float32(w.value)

    def params(self):
        keep, seed = C.c_float(), C.c_uint64()
        check(lib().xf_negsample_params(self.h, C.byref(keep), C.byref(seed)))
        return keep.value, seed.value

    def apply_dev(self, stream_id, first_ordinal, rowptr, keys, labels, fgid=None, values=None,
                  stream=None):
        """host arrays in (uploaded as they are), the sampled minibatch as an AdmitDev out (device
        pointers owned by the sampler, valid until its next apply)"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(rowptr) >= 1 and int(rowptr[-1]) - int(rowptr[0]) <= len(keys)
        R = len(rowptr) - 1
        args = []
        for a, dt, pt in ((fgid, np.int32, i32p), (values, np.float32, f32p)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                assert len(a) == len(keys), "one entry per key"
                a = a if len(a) else np.zeros(1, dt)
            args.append((a, pt))
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        assert len(labels) == R, "one label per row"
        labels = labels if R else np.zeros(1, np.int32)
        if len(keys) == 0:
            keys = np.zeros(1, np.uint64)
        ptr = [(_p(a, pt) if a is not None else None) for a, pt in args]
        dk, dfg, dv, dr, dl = vp(), vp(), vp(), vp(), vp()
        Ro, No = C.c_uint32(), C.c_uint32()
        check(lib().xf_negsample_apply(self.h, int(stream_id), int(first_ordinal),
                                       _p(rowptr, u64p), _p(keys, u64p), ptr[0], ptr[1],
                                       _p(labels, i32p), 0, R, stream, C.byref(dk), C.byref(dfg),
                                       C.byref(dv), C.byref(dr), C.byref(dl), C.byref(Ro),
                                       C.byref(No)))
        return AdmitDev(dk.value, dr.value, dl.value, Ro.value, No.value, dfg.value, dv.value)

    def sample_dev(self, stream_id, first_ordinal, d_keys, d_rowptr, d_labels, R, NNZ,
                   d_fgid=None, d_vals=None, stream=None):
        """xf_negsample_apply_dev: device pointers in (ints), the sampled minibatch as an AdmitDev"""
        dk, dfg, dv, dr, dl = vp(), vp(), vp(), vp(), vp()
        Ro, No = C.c_uint32(), C.c_uint32()
        check(lib().xf_negsample_apply_dev(self.h, int(stream_id), int(first_ordinal), d_keys,
                                           d_fgid, d_vals, d_rowptr, d_labels, R, NNZ, stream,
                                           C.byref(dk), C.byref(dfg), C.byref(dv), C.byref(dr),
                                           C.byref(dl), C.byref(Ro), C.byref(No)))
        return AdmitDev(dk.value, dr.value, dl.value, Ro.value, No.value, dfg.value, dv.value)

    def apply(self, stream_id, first_ordinal, rowptr, keys, labels, fgid=None, values=None):
        """the sampled host arrays (downloaded): (rowptr uint32, keys, labels) and then, for each
        of fgid / values that was given, its sampled array in that order"""
        d = self.apply_dev(stream_id, first_ordinal, rowptr, keys, labels, fgid, values)
        check(lib().xf_stream_sync(None))
        out = [(np.zeros(d.R + 1, np.uint32), d.d_rowptr), (np.zeros(d.NNZ, np.uint64), d.d_keys),
               (np.zeros(d.R, np.int32), d.d_labels)]
        if fgid is not None:
            out.append((np.zeros(d.NNZ, np.int32), d.d_fgid))
        if values is not None:
            out.append((np.zeros(d.NNZ, np.float32), d.d_vals))
        for a, ptr in out:
            if a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return tuple(a for a, _ in out)

    def stats(self):
        """(rows seen, rows kept, negatives seen, negatives kept), summed over the applies"""
        v = [C.c_uint64() for _ in range(4)]
        check(lib().xf_negsample_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


def holdout_held(seed, stream, ordinal, share):
    """whether the row of this ordinal is held out of training (xf_holdout_held; host code, the
    kernels' own definition)"""
    return bool(lib().xf_holdout_held(int(seed) & (2**64 - 1), int(stream) & (2**64 - 1),
                                      int(ordinal) & (2**64 - 1), float(share)))


def holdout_should_stop(logloss, patience, delta=0.0):
    """xf_holdout_should_stop (host code) on one held-out logloss per validated epoch ->
    (stop, index of the best epoch or -1)"""
    a = np.ascontiguousarray(logloss, dtype=np.float64)
    best = C.c_int(-1)
    stop = lib().xf_holdout_should_stop(a.ctypes.data_as(C.POINTER(C.c_double)) if len(a) else None,
                                        len(a), int(patience), float(delta), C.byref(best))
    return bool(stop), best.value


def holdout_shape():
    """{tile (rows of a workgroup), chunk (output nonzeros of a copy workgroup), align (elements
    the held part is aligned to)} of the split kernels"""
    out = (C.c_uint32 * 3)()
    lib().xf_holdout_shape(out)
    return {"tile": out[0], "chunk": out[1], "align": out[2]}


class HoldoutPart(C.Structure):
    _fields_ = [("d_keys", vp), ("d_fgid", vp), ("d_vals", vp), ("d_rowptr", vp),
                ("d_labels", vp), ("R", C.c_uint32), ("NNZ", C.c_uint32)]

    def dev(self):
        return AdmitDev(self.d_keys, self.d_rowptr, self.d_labels, self.R, self.NNZ, self.d_fgid,
                        self.d_vals)


class Holdout:
    """Held-out validation's row split (xf_holdout_*): split() sends a hash-chosen share of a
    minibatch's rows — decided by a hash of (seed, stream, the row's ordinal) alone — into a held
    minibatch and the rest, in order, into a train minibatch.  Stateless but for the statistics."""

    def __init__(self, share, seed=0):
        self.h = vp()
        self.share, self.seed = float(np.float32(share)), seed
        check(lib().xf_holdout_create(C.byref(self.h), share, seed))

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_holdout_destroy(self.h)
            self.h = None

    def params(self):
        share, seed = C.c_float(), C.c_uint64()
        check(lib().xf_holdout_params(self.h, C.byref(share), C.byref(seed)))
        return share.value, seed.value

    def split_dev(self, stream_id, first_ordinal, rowptr, keys, labels, fgid=None, values=None,
                  stream=None):
        """host arrays in (uploaded as they are), (train, held) as two AdmitDev out (device
        pointers owned by the object, valid until its next split)"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(rowptr) >= 1 and int(rowptr[-1]) - int(rowptr[0]) <= len(keys)
        R = len(rowptr) - 1
        args = []
        for a, dt, pt in ((fgid, np.int32, i32p), (values, np.float32, f32p)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                assert len(a) == len(keys), "one entry per key"
                a = a if len(a) else np.zeros(1, dt)
            args.append((a, pt))
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        assert len(labels) == R, "one label per row"
        labels = labels if R else np.zeros(1, np.int32)
        if len(keys) == 0:
            keys = np.zeros(1, np.uint64)
        ptr = [(_p(a, pt) if a is not None else None) for a, pt in args]
        train, held = HoldoutPart(), HoldoutPart()
        check(lib().xf_holdout_split(self.h, int(stream_id), int(first_ordinal) & (2**64 - 1),
                                     _p(rowptr, u64p), _p(keys, u64p), ptr[0], ptr[1],
                                     _p(labels, i32p), 0, R, stream, C.byref(train),
                                     C.byref(held)))
        return train.dev(), held.dev()

    def part_dev(self, stream_id, first_ordinal, d_keys, d_rowptr, d_labels, R, NNZ, d_fgid=None,
                 d_vals=None, stream=None):
        """xf_holdout_split_dev: device pointers in (ints), (train, held) as two AdmitDev"""
        train, held = HoldoutPart(), HoldoutPart()
        check(lib().xf_holdout_split_dev(self.h, int(stream_id), int(first_ordinal) & (2**64 - 1),
                                         d_keys, d_fgid, d_vals, d_rowptr, d_labels, R, NNZ,
                                         stream, C.byref(train), C.byref(held)))
        return train.dev(), held.dev()

    @staticmethod
    def download(d, fgid=False, values=False):
        """the host arrays of one part: (rowptr uint32, keys, labels) and then, for each of fgid /
        values asked for, its array in that order"""
        check(lib().xf_stream_sync(None))
        out = [(np.zeros(d.R + 1, np.uint32), d.d_rowptr), (np.zeros(d.NNZ, np.uint64), d.d_keys),
               (np.zeros(d.R, np.int32), d.d_labels)]
        if fgid:
            out.append((np.zeros(d.NNZ, np.int32), d.d_fgid))
        if values:
            out.append((np.zeros(d.NNZ, np.float32), d.d_vals))
        for a, ptr in out:
            if a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return tuple(a for a, _ in out)

    def split(self, stream_id, first_ordinal, rowptr, keys, labels, fgid=None, values=None):
        """(train, held), each the downloaded host arrays of that part (download())"""
        t, h = self.split_dev(stream_id, first_ordinal, rowptr, keys, labels, fgid, values)
        return (self.download(t, fgid is not None, values is not None),
                self.download(h, fgid is not None, values is not None))

    def stats(self):
        """(rows seen, rows held, nonzeros held), summed over the splits"""
        v = [C.c_uint64() for _ in range(3)]
        check(lib().xf_holdout_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


def cross_key(ka, kb, fa, fb):
    """the key of the nonzero that crosses key ka of field fa with key kb of field fb
    (xf_cross_key; host code, the kernels' own definition)"""
    return int(lib().xf_cross_key(int(ka) & (2**64 - 1), int(kb) & (2**64 - 1), int(fa), int(fb)))


def cross_parse(spec):
    """"2*3,16*17" as a list of (fa, fb) pairs (xf_cross_parse; a malformed spec raises, naming
    the offending piece)"""
    fa, fb = np.zeros(32, np.int32), np.zeros(32, np.int32)
    n = C.c_int()
    check(lib().xf_cross_parse(str(spec).encode(), _p(fa, i32p), _p(fb, i32p), 32, C.byref(n)))
    return [(int(fa[p]), int(fb[p])) for p in range(n.value)]


PROGRESS_MANT = 10
PROGRESS_CENTER = 0x3f000000 >> (23 - PROGRESS_MANT)
PROGRESS_RANKS = 2 * PROGRESS_CENTER + 1


class ProgressMetrics(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("rows_pos", "rows_neg", "saturated", "other", "logloss", "logloss_bound", "auc",
                 "auc_slack", "ctr", "pctr")]


def progress_rank(loss):
    """the rank of a row's loss (xf_progress_rank; host code, the kernel's own definition):
    0 .. 2C for q = |loss| in [0, 1], PROGRESS_RANKS for NaN and q > 1"""
    return int(lib().xf_progress_rank(float(np.float32(loss))))


def progress_summary(counts, other, neg_weight=1.0):
    """xf_progress_summary (host code): counts uint64 [2, PROGRESS_RANKS] (class 0 = label 0 first),
    other uint64 [2]; a dict of the metrics' fields"""
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    other = np.ascontiguousarray(other, dtype=np.uint64).reshape(-1)
    assert counts.size == 2 * PROGRESS_RANKS and other.size == 2
    m = ProgressMetrics()
    check(lib().xf_progress_summary(_p(counts, u64p), _p(other, u64p), float(neg_weight),
                                    C.byref(m)))
    return {n: getattr(m, n) for n, _ in ProgressMetrics._fields_}


def progress_launches():
    return int(lib().xf_progress_launches())


def progress_shape():
    """{rows of a workgroup, slots and probes of its LDS table} of the accumulate kernel"""
    out = (C.c_uint32 * 3)()
    lib().xf_progress_shape(out)
    return dict(zip(("rows", "slots", "probe"), list(out)))


def evict_shape():
    """{rows of a workgroup, lanes of a wavefront} of the eviction kernels (xf_evict_shape)"""
    out = (C.c_uint32 * 2)()
    lib().xf_evict_shape(out)
    return dict(zip(("rows", "wave"), list(out)))


class Progress:
    """Progressive validation (xf_progress_*): counts of the ranks of the training rows' losses,
    kept on the GPU.  Attach it to a Workspace (Workspace.progress) or feed it device arrays
    (accumulate); read() is the one stream wait; summary() forms the metrics on the host."""

    rank = staticmethod(progress_rank)

    def __init__(self):
        require_gpu()
        self.h = vp()
        check(lib().xf_progress_create(C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_progress_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def accumulate(self, d_loss, d_labels, R, stream=None):
        """device pointers (ints): R losses (f32) and labels (i32); one launch, no wait"""
        check(lib().xf_progress_accumulate_dev(self.h, d_loss, d_labels, int(R), stream))

    def read(self, reset=False):
        """(counts [2, PROGRESS_RANKS], other [2]) as uint64 arrays"""
        counts = np.empty((2, PROGRESS_RANKS), np.uint64)
        other = np.empty(2, np.uint64)
        check(lib().xf_progress_read(self.h, _p(counts, u64p), _p(other, u64p),
                                     1 if reset else 0))
        return counts, other

    def summary(self, neg_weight=1.0, reset=False):
        counts, other = self.read(reset)
        return progress_summary(counts, other, neg_weight)


SLICE_NONE = 2**64 - 1
SLICE_WORDS = 7
SLICE_NAMES = ("n0", "n1", "qsum0", "qsum1", "llsum0", "llsum1", "other")


class SliceMetrics(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("rows", "other", "ctr", "pctr", "logloss", "logloss_bound", "pctr_bound")]


def slices_home(key, log2_slots):
    """the home slot of a slice's key in a table of 2^log2_slots entries (xf_slices_home; host
    code, the kernel's own definition)"""
    return int(lib().xf_slices_home(int(key) & (2**64 - 1), int(log2_slots)))


def slices_terms():
    """the fixed-point row terms ll_fix[rank], uint32 [PROGRESS_RANKS] (xf_slices_terms)"""
    out = np.empty(PROGRESS_RANKS, np.uint32)
    check(lib().xf_slices_terms(out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def slices_check(field, log2_slots):
    """the parameter check of xf_slices_create without a device (raises XFError)"""
    check(lib().xf_slices_check(int(field), int(log2_slots)))


def slices_summary(words, neg_weight=1.0):
    """xf_slices_summary (host code): a slice's seven words -> a dict of the metrics' fields"""
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    assert words.size == SLICE_WORDS
    m = SliceMetrics()
    check(lib().xf_slices_summary(_p(words, u64p), float(neg_weight), C.byref(m)))
    return {n: getattr(m, n) for n, _ in SliceMetrics._fields_}


def slices_launches():
    return int(lib().xf_slices_launches())


def slices_shape():
    """{rows of an accumulate workgroup, entries and probes of its LDS table, the cap of the
    global probe limit, rows of an extract workgroup}"""
    out = (C.c_uint32 * 5)()
    lib().xf_slices_shape(out)
    return dict(zip(("rows", "slots", "probe", "global_probe", "extract_rows"), list(out)))


def _slices_result(entries, n, none, overflow):
    e = entries[:n]
    return e[:, 0].copy(), e[:, 1:].copy(), none, overflow


class Slices:
    """Sliced progressive validation (xf_slices_*): progressive validation's counters per value
    of field F, in a device table of 2^log2_slots entries.  extract() names the rows' slices,
    accumulate() adds; attach it to a Workspace (Workspace.slices / slice_ids); read() returns
    (keys ascending, words [n, 7], none [7], overflow [7])."""

    home = staticmethod(slices_home)

    def __init__(self, field, log2_slots=16):
        require_gpu()
        self.h = vp()
        check(lib().xf_slices_create(C.byref(self.h), int(field), int(log2_slots)))
        self.field, self.log2_slots = int(field), int(log2_slots)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_slices_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def params(self):
        f, b = C.c_int32(), C.c_int()
        check(lib().xf_slices_params(self.h, C.byref(f), C.byref(b)))
        return f.value, b.value

    def extract_dev(self, d_keys, d_fgid, d_rowptr, R, NNZ, stream=None):
        """device pointers in (ints); the device pointer of the R ids out (owned by the object,
        valid until its next extract, written in the order of `stream`)"""
        out = vp()
        check(lib().xf_slices_extract_dev(self.h, d_keys, d_fgid, d_rowptr, int(R), int(NNZ),
                                          stream, C.byref(out)))
        return out.value

    def extract_host_dev(self, rowptr, keys, fgid, row_begin=0, row_end=None, stream=None):
        """host arrays and a row slice in (uploaded); (device pointer of the ids, R) out"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        fgid = np.ascontiguousarray(fgid, dtype=np.int32)
        assert len(rowptr) >= 1 and len(fgid) == len(keys), "one field id per key"
        row_end = len(rowptr) - 1 if row_end is None else row_end
        if len(keys) == 0:
            keys, fgid = np.zeros(1, np.uint64), np.zeros(1, np.int32)
        out, R = vp(), C.c_uint32()
        check(lib().xf_slices_extract(self.h, _p(rowptr, u64p), _p(keys, u64p), _p(fgid, i32p),
                                      row_begin, row_end, stream, C.byref(out), C.byref(R)))
        return out.value, R.value

    def extract(self, rowptr, keys, fgid, row_begin=0, row_end=None):
        """the ids of rows [row_begin, row_end) as a uint64 array (downloaded)"""
        d, R = self.extract_host_dev(rowptr, keys, fgid, row_begin, row_end)
        return self.download_ids(d, R)

    @staticmethod
    def download_ids(d_id, R):
        check(lib().xf_stream_sync(None))
        ids = np.zeros(R, np.uint64)
        if R:
            check(lib().xf_copy_to_host(ids.ctypes.data, d_id, ids.nbytes))
        return ids

    def accumulate(self, d_loss, d_labels, d_id, R, stream=None):
        """device pointers (ints): R losses (f32), labels (i32) and ids (u64); one launch, no
        wait"""
        check(lib().xf_slices_accumulate_dev(self.h, d_loss, d_labels, d_id, int(R), stream))

    def count(self):
        """the occupied entries (a read that copies none of them)"""
        n = C.c_uint64()
        check(lib().xf_slices_read(self.h, None, 0, C.byref(n), None, None, 0))
        return n.value

    def read(self, reset=False):
        cap = 1 << self.log2_slots if self.log2_slots <= 16 else max(self.count(), 1)
        entries = np.zeros((cap, SLICE_WORDS + 1), np.uint64)
        none, overflow = np.zeros(SLICE_WORDS, np.uint64), np.zeros(SLICE_WORDS, np.uint64)
        n = C.c_uint64()
        check(lib().xf_slices_read(self.h, _p(entries, u64p), cap, C.byref(n), _p(none, u64p),
                                   _p(overflow, u64p), 1 if reset else 0))
        return _slices_result(entries, n.value, none, overflow)


GAUC_WORDS = 4
GAUC_OTHER = 2**32 - 1
u32p = C.POINTER(C.c_uint32)


class GaucMetrics(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("gauc", "gauc_slack", "macro_auc")] + \
               [(n, C.c_uint64) for n in ("groups", "groups_scored", "rows", "rows_scored",
                                          "rows_one_class", "none_rows", "other_rows")]


def gauc_code(loss, label):
    """the code of a row's record (xf_gauc_code; host code, the kernel's own definition):
    (score << 1) | pos, GAUC_OTHER for a NaN loss and q > 1"""
    return int(lib().xf_gauc_code(float(np.float32(loss)), int(np.int32(label))))


def gauc_summary(ids, figures, none=None, other=None):
    """xf_gauc_summary (host code): ids uint64 [n] ascending, figures uint64 [n, 4] = P, N, U2, T
    -> (a dict of the metrics' fields, auc [n], slack [n])"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
    figures = np.ascontiguousarray(figures, dtype=np.uint64).reshape(-1, GAUC_WORDS)
    assert len(ids) == len(figures)
    n = len(ids)
    entries = np.zeros((max(n, 1), GAUC_WORDS + 1), np.uint64)
    entries[:n, 0] = ids
    entries[:n, 1:] = figures
    none = np.ascontiguousarray(none if none is not None else [0, 0], dtype=np.uint64)
    other = np.ascontiguousarray(other if other is not None else [0, 0], dtype=np.uint64)
    auc, slack = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    m = GaucMetrics()
    dp = C.POINTER(C.c_double)
    check(lib().xf_gauc_summary(_p(entries, u64p), n, _p(none, u64p), _p(other, u64p),
                                C.byref(m), _p(auc, dp), _p(slack, dp)))
    return {k: getattr(m, k) for k, _ in GaucMetrics._fields_}, auc[:n], slack[:n]


def gauc_launches():
    return int(lib().xf_gauc_launches())


def gauc_shape():
    """{rows of a pack workgroup, records of a reduce workgroup}"""
    out = (C.c_uint32 * 2)()
    lib().xf_gauc_shape(out)
    return dict(zip(("pack_rows", "reduce_records"), list(out)))


def _gauc_result(entries, n, none, other):
    e = entries[:n]
    return e[:, 0].copy(), e[:, 1:].copy(), none, other


class Gauc:
    """Grouped AUC on the held-out rows (xf_gauc_*): a device log of (id, code) records.
    append_dev() packs rows' records, append() takes ready-made ones; attach it to a Workspace
    (Workspace.gauc / gauc_ids); reduce() returns (ids ascending, figures [n, 4] = P, N, U2, T,
    none [2], other [2]); summary() forms the metrics on the host."""

    code = staticmethod(gauc_code)

    def __init__(self):
        require_gpu()
        self.h = vp()
        check(lib().xf_gauc_create(C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_gauc_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def reserve(self, rows):
        check(lib().xf_gauc_reserve(self.h, int(rows)))

    def append_dev(self, d_loss, d_labels, d_id, R, stream=None):
        """device pointers (ints): R losses (f32), labels (i32) and ids (u64); one launch"""
        check(lib().xf_gauc_append_dev(self.h, d_loss, d_labels, d_id, int(R), stream))

    def append(self, ids, codes):
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        assert len(ids) == len(codes)
        check(lib().xf_gauc_append(self.h, _p(ids, u64p) if len(ids) else None,
                                   _p(codes, u32p) if len(ids) else None, len(ids)))

    def count(self):
        n = C.c_uint64()
        check(lib().xf_gauc_export(self.h, None, None, 0, C.byref(n)))
        return n.value

    def export(self):
        """(ids, codes) of the log as it stands, in the log's order"""
        cap = max(self.count(), 1)
        ids, codes = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
        n = C.c_uint64()
        check(lib().xf_gauc_export(self.h, _p(ids, u64p), _p(codes, u32p), cap, C.byref(n)))
        return ids[:n.value].copy(), codes[:n.value].copy()

    def groups(self):
        """the distinct ids (a reduce that copies no entry)"""
        n = C.c_uint64()
        check(lib().xf_gauc_reduce(self.h, None, 0, C.byref(n), None, None, 0))
        return n.value

    def reduce(self, reset=False, cap=None):
        cap = max(self.groups(), 1) if cap is None else int(cap)
        entries = np.zeros((max(cap, 1), GAUC_WORDS + 1), np.uint64)
        none, other = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        n = C.c_uint64()
        check(lib().xf_gauc_reduce(self.h, _p(entries, u64p), cap, C.byref(n), _p(none, u64p),
                                   _p(other, u64p), 1 if reset else 0))
        return _gauc_result(entries, n.value, none, other)

    def summary(self, reset=False):
        ids, fig, none, other = self.reduce(reset)
        return gauc_summary(ids, fig, none, other)[0]


def slice_ids(rowptr, keys, fgid, field, row_begin=0, row_end=None):
    """the slice ids of the rows of host arrays for field `field`, computed on the GPU (a
    throw-away Slices object's extract)"""
    return Slices(field, 2).extract(rowptr, keys, fgid, row_begin, row_end)


class Cross:
    """Feature crosses (xf_cross_*): apply() returns a minibatch with, behind every row's own
    nonzeros, one nonzero per listed pair of fields and per (member of the first, member of the
    second), keyed by cross_key, with fgid fgid_base + the pair's index and the product of the two
    values.  spec_or_pairs: "2*3,16*17" or a list of (fa, fb).  Stateless but for the statistics."""

    def __init__(self, spec_or_pairs, fgid_base=0):
        self.h = vp()
        pairs = cross_parse(spec_or_pairs) if isinstance(spec_or_pairs, str) else \
            [(int(a), int(b)) for a, b in spec_or_pairs]
        fa = np.array([a for a, _ in pairs] or [0], np.int32)
        fb = np.array([b for _, b in pairs] or [0], np.int32)
        check(lib().xf_cross_create(C.byref(self.h), _p(fa, i32p), _p(fb, i32p), len(pairs),
                                    int(fgid_base)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_cross_destroy(self.h)
            self.h = None

    def params(self):
        """(pairs, fgid_base)"""
        fa, fb = np.zeros(32, np.int32), np.zeros(32, np.int32)
        n, base = C.c_int(), C.c_int32()
        check(lib().xf_cross_params(self.h, _p(fa, i32p), _p(fb, i32p), 32, C.byref(n),
                                    C.byref(base)))
        return [(int(fa[p]), int(fb[p])) for p in range(n.value)], base.value

    def apply_dev(self, rowptr, keys, fgid, labels=None, values=None, want_fgid=True,
                  row_begin=0, row_end=None, stream=None):
        """host arrays in (rows [row_begin, row_end) uploaded as they are), the crossed minibatch
        as an AdmitDev out (device pointers owned by the stage, valid until its next apply).  The
        arrays are WRITTEN IN THE ORDER OF `stream` and the call does not wait for them: hand them
        to work on the same stream (Sharded.stream() for a trainer's compile_dev), or wait for
        `stream` first"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(rowptr) >= 1
        row_end = len(rowptr) - 1 if row_end is None else row_end
        args = []
        for a, dt, pt in ((fgid, np.int32, i32p), (values, np.float32, f32p)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                assert len(a) == len(keys), "one entry per key"
                a = a if len(a) else np.zeros(1, dt)
            args.append((a, pt))
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            assert len(labels) == len(rowptr) - 1, "one label per row"
            labels = labels if len(labels) else np.zeros(1, np.int32)
        args.append((labels, i32p))
        if len(keys) == 0:
            keys = np.zeros(1, np.uint64)
        ptr = [(_p(a, pt) if a is not None else None) for a, pt in args]
        dk, dfg, dv, dr, dl = vp(), vp(), vp(), vp(), vp()
        Ro, No = C.c_uint32(), C.c_uint32()
        check(lib().xf_cross_apply(self.h, _p(rowptr, u64p), _p(keys, u64p), ptr[0], ptr[1],
                                   ptr[2], row_begin, row_end, stream, 1 if want_fgid else 0,
                                   C.byref(dk), C.byref(dfg), C.byref(dv), C.byref(dr),
                                   C.byref(dl), C.byref(Ro), C.byref(No)))
        return AdmitDev(dk.value, dr.value, dl.value, Ro.value, No.value, dfg.value, dv.value)

    def cross_dev(self, d_keys, d_rowptr, R, NNZ, d_fgid, d_vals=None, want_fgid=True,
                  stream=None):
        """xf_cross_apply_dev: device pointers in (ints), (d_keys, d_rowptr, NNZ, d_fgid, d_vals)
        of the crossed minibatch out; labels and R are the caller's, untouched"""
        dk, dfg, dv, dr = vp(), vp(), vp(), vp()
        No = C.c_uint32()
        check(lib().xf_cross_apply_dev(self.h, d_keys, d_fgid, d_vals, d_rowptr, R, NNZ, stream,
                                       1 if want_fgid else 0, C.byref(dk), C.byref(dfg),
                                       C.byref(dv), C.byref(dr), C.byref(No)))
        return dk.value, dr.value, No.value, dfg.value, dv.value

    def apply(self, rowptr, keys, fgid, labels=None, values=None, want_fgid=True, row_begin=0,
              row_end=None):
        """the crossed host arrays (downloaded): (rowptr uint32, keys) and then, for each of
        labels / fgid (want_fgid) / values that was given, its array in that order"""
        d = self.apply_dev(rowptr, keys, fgid, labels, values, want_fgid, row_begin, row_end)
        check(lib().xf_stream_sync(None))
        out = [(np.zeros(d.R + 1, np.uint32), d.d_rowptr), (np.zeros(d.NNZ, np.uint64), d.d_keys)]
        if labels is not None:
            out.append((np.zeros(d.R, np.int32), d.d_labels))
        if want_fgid:
            out.append((np.zeros(d.NNZ, np.int32), d.d_fgid))
        if values is not None:
            out.append((np.zeros(d.NNZ, np.float32), d.d_vals))
        for a, ptr in out:
            if a.nbytes:
                check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return tuple(a for a, _ in out)

    def stats(self):
        """(rows seen, input nonzeros, crossed nonzeros), summed over the applies"""
        v = [C.c_uint64() for _ in range(3)]
        check(lib().xf_cross_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


ROWNORM_L2 = 1


def rownorm_row(x):
    """(y, s): one row's values normalised to unit L2 length and its sum of squares, by the
    definition of csrc/xf_rownorm.h as host code (xf_rownorm_row; no GPU)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    s = C.c_double()
    one = np.zeros(1, np.float32)
    check(lib().xf_rownorm_row(_p(x if len(x) else one, f32p), len(x),
                               _p(y if len(y) else one, f32p), C.byref(s)))
    return y, s.value


class RowNorm:
    """Row normalisation (xf_rownorm_*): every row of a minibatch scaled to unit L2 length over
    its nonzeros; a row whose sum of squares is 0, infinite or NaN is left as it is.  Only the
    values change.  Stateless but for the statistics."""

    def __init__(self, kind=ROWNORM_L2):
        self.h = vp()
        check(lib().xf_rownorm_create(C.byref(self.h), int(kind)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().xf_rownorm_destroy(self.h)
            self.h = None

    @staticmethod
    def shape():
        """(lanes that share a row, rows of a workgroup)"""
        out = np.zeros(2, np.uint32)
        lib().xf_rownorm_shape(_p(out, u32p))
        return int(out[0]), int(out[1])

    @staticmethod
    def launches():
        """kernels launched by the stage in this process"""
        return int(lib().xf_rownorm_launches())

    def apply_dev(self, rowptr, keys, values, labels=None, fgid=None, row_begin=0, row_end=None,
                  stream=None):
        """host arrays in (rows [row_begin, row_end) uploaded by the stage), the minibatch with
        normalised values as an AdmitDev out, and the device pointer of the rows' sums of squares
        (device arrays owned by the stage, valid until its next apply).  WRITTEN IN THE ORDER OF
        `stream`; the call does not wait: hand them to work on the same stream or wait first"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(rowptr) >= 1
        row_end = len(rowptr) - 1 if row_end is None else row_end
        args = []
        for a, dt, pt in ((fgid, np.int32, i32p), (values, np.float32, f32p)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=dt)
                assert len(a) == len(keys), "one entry per key"
                a = a if len(a) else np.zeros(1, dt)
            args.append((a, pt))
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            assert len(labels) == len(rowptr) - 1, "one label per row"
            labels = labels if len(labels) else np.zeros(1, np.int32)
        args.append((labels, i32p))
        if len(keys) == 0:
            keys = np.zeros(1, np.uint64)
        ptr = [(_p(a, pt) if a is not None else None) for a, pt in args]
        dk, dfg, dv, dr, dl, ds = vp(), vp(), vp(), vp(), vp(), vp()
        Ro, No = C.c_uint32(), C.c_uint32()
        check(lib().xf_rownorm_apply(self.h, _p(rowptr, u64p), _p(keys, u64p), ptr[0], ptr[1],
                                     ptr[2], row_begin, row_end, stream, C.byref(dk),
                                     C.byref(dfg), C.byref(dv), C.byref(dr), C.byref(dl),
                                     C.byref(Ro), C.byref(No), C.byref(ds)))
        return AdmitDev(dk.value, dr.value, dl.value, Ro.value, No.value, dfg.value,
                        dv.value), ds.value

    def norm_dev(self, d_vals, d_rowptr, R, NNZ, stream=None, want_sumsq=True):
        """xf_rownorm_apply_dev: device pointers in (ints), (d_vals_out, d_sumsq_out) out"""
        dv, ds = vp(), vp()
        check(lib().xf_rownorm_apply_dev(self.h, d_vals, d_rowptr, R, NNZ, stream, C.byref(dv),
                                         C.byref(ds) if want_sumsq else None))
        return dv.value, ds.value

    @staticmethod
    def download(ptr, n, dtype):
        """n entries of a device array, after a wait for the device"""
        check(lib().xf_stream_sync(None))
        a = np.zeros(n, dtype)
        if a.nbytes:
            check(lib().xf_copy_to_host(a.ctypes.data, ptr, a.nbytes))
        return a

    def apply(self, rowptr, keys, values, labels=None, fgid=None, row_begin=0, row_end=None):
        """the host arrays of the normalised minibatch (downloaded): (rowptr uint32, keys, values,
        sums of squares float64) and then, for each of labels / fgid that was given, its array"""
        d, ds = self.apply_dev(rowptr, keys, values, labels, fgid, row_begin, row_end)
        out = [self.download(d.d_rowptr, d.R + 1, np.uint32),
               self.download(d.d_keys, d.NNZ, np.uint64),
               self.download(d.d_vals, d.NNZ, np.float32), self.download(ds, d.R, np.float64)]
        if labels is not None:
            out.append(self.download(d.d_labels, d.R, np.int32))
        if fgid is not None:
            out.append(self.download(d.d_fgid, d.NNZ, np.int32))
        return tuple(out)

    def stats(self):
        """(rows seen, rows scaled), summed over the applies; reading waits for the device"""
        v = [C.c_uint64() for _ in range(2)]
        check(lib().xf_rownorm_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class Batch:
    """A compiled minibatch (host arrays; device mirror after upload())."""

    def __init__(self, rowptr, keys, labels, row_begin=0, row_end=None, on_gpu=False,
                 values=None, fields=None, fgid=None):
        """on_gpu=False: host key build (xf_batch_compile); True: the GPU one
        (xf_batch_compile_gpu), the batch is then already device-resident.  values (float32,
        beside keys): a minibatch with feature values (xf_batch_compile_valued / _gpu).
        fields (1 .. 64) with fgid (int32, beside keys): a minibatch with its fields, for
        field-aware FM (xf_batch_compile_fielded / _gpu; with or without values)."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if row_end is None:
            row_end = len(rowptr) - 1
        self.h = vp()
        self.valued = values is not None
        self.fields = int(fields) if fields is not None else 0
        if self.valued:
            values = np.ascontiguousarray(values, dtype=np.float32)
            assert len(values) == len(keys), "one value per key"
            if len(values) == 0:
                values = np.zeros(1, np.float32)   # a non-null pointer
        if fields is not None:
            assert fgid is not None, "fields needs the nonzeros' fgid"
            fgid = np.ascontiguousarray(fgid, dtype=np.int32)
            assert len(fgid) == len(keys), "one fgid per key"
            if len(fgid) == 0:
                fgid = np.zeros(1, np.int32)
            vptr = _p(values, f32p) if self.valued else None
            if on_gpu:
                check(lib().xf_batch_compile_fielded_gpu(
                    C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p), _p(fgid, i32p), vptr,
                    _p(labels, i32p), row_begin, row_end, self.fields, None))
            else:
                check(lib().xf_batch_compile_fielded(
                    C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p), _p(fgid, i32p), vptr,
                    _p(labels, i32p), row_begin, row_end, self.fields))
        elif self.valued:
            if on_gpu:
                check(lib().xf_batch_compile_valued_gpu(
                    C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p), _p(values, f32p),
                    _p(labels, i32p), row_begin, row_end, None))
            else:
                check(lib().xf_batch_compile_valued(
                    C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p), _p(values, f32p),
                    _p(labels, i32p), row_begin, row_end))
        elif on_gpu:
            check(lib().xf_batch_compile_gpu(C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p),
                                             _p(labels, i32p), row_begin, row_end, None))
        else:
            check(lib().xf_batch_compile(C.byref(self.h), _p(rowptr, u64p), _p(keys, u64p),
                                         _p(labels, i32p), row_begin, row_end))
        R, N, U, H = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().xf_batch_dims(self.h, C.byref(R), C.byref(N), C.byref(U), C.byref(H)))
        self.R, self.NNZ, self.U, self.H = R.value, N.value, U.value, H.value
        self.on_gpu = on_gpu

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_batch_free(self.h)
                self.h = None
        except Exception:      # interpreter shutdown: the module globals may be gone
            pass

    def host(self):
        uk, rp, ui, sp, cr, hv = u64p(), u32p(), u32p(), u32p(), u32p(), u32p()
        lb = i32p()
        check(lib().xf_batch_host(self.h, C.byref(uk), C.byref(rp), C.byref(ui), C.byref(sp),
                                  C.byref(cr), C.byref(lb), C.byref(hv)))

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, dt)
        return dict(ukeys=arr(uk, self.U, np.uint64), rowptr=arr(rp, self.R + 1, np.uint32),
                    uidx=arr(ui, self.NNZ, np.uint32), segptr=arr(sp, self.U + 1, np.uint32),
                    coo_row=arr(cr, self.NNZ, np.uint32), labels=arr(lb, self.R, np.int32),
                    heavy=arr(hv, self.H, np.uint32))

    def values(self):
        """(xval, coo_val) of a valued minibatch: the values in CSR order and grouped by key"""
        xv, cv = f32p(), f32p()
        check(lib().xf_batch_values_host(self.h, C.byref(xv), C.byref(cv)))
        if not self.valued or self.NNZ == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        return (np.ctypeslib.as_array(xv, (self.NNZ,)).copy(),
                np.ctypeslib.as_array(cv, (self.NNZ,)).copy())

    def field_arrays(self):
        """(xfg, coo_pos) of a minibatch compiled with fields: the nonzeros' fields in CSR order
        and the occurrences' CSR positions grouped by key"""
        F, xg, cp = C.c_int(0), u32p(), u32p()
        check(lib().xf_batch_fields_host(self.h, C.byref(F), C.byref(xg), C.byref(cp)))
        if not F.value or self.NNZ == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return (np.ctypeslib.as_array(xg, (self.NNZ,)).copy(),
                np.ctypeslib.as_array(cp, (self.NNZ,)).copy())

    def panels(self):
        P, pp, pi = C.c_uint32(0), u32p(), u32p()
        check(lib().xf_batch_panels(self.h, C.byref(P), C.byref(pp), C.byref(pi)))
        if P.value == 0:
            return 0, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return (P.value, np.ctypeslib.as_array(pp, (P.value * (self.R + 1),)).copy(),
                np.ctypeslib.as_array(pi, (self.NNZ,)).copy())

    def fwd_tiles(self):
        """(tile_ptr[ntiles+1], panel_first[P+1], grid) of the forward tiles"""
        n, tp, pf, g = C.c_uint32(0), u32p(), u32p(), C.c_uint32(0)
        check(lib().xf_batch_fwd_tiles(self.h, C.byref(n), C.byref(tp), C.byref(pf),
                                       C.byref(g)))
        if n.value == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), 0
        P = self.panels()[0]
        return (np.ctypeslib.as_array(tp, (n.value + 1,)).copy(),
                np.ctypeslib.as_array(pf, (P + 1,)).copy(), g.value)

    def heavy_chunks(self):
        n, cp = C.c_uint32(0), u32p()
        check(lib().xf_batch_heavy_chunks(self.h, C.byref(n), C.byref(cp)))
        return np.ctypeslib.as_array(cp, (n.value + 1,)).copy()

    def tiles(self):
        n, tp = C.c_uint32(0), u32p()
        check(lib().xf_batch_tiles(self.h, C.byref(n), C.byref(tp)))
        return np.ctypeslib.as_array(tp, (n.value + 1,)).copy()

    def upload(self, stream=None):
        check(lib().xf_batch_upload(self.h, stream))
        return self

    def dev_view(self):
        if not self.on_gpu:
            self.upload()
        v = DevBatch()
        check(lib().xf_batch_dev_view(self.h, C.byref(v)))
        return v


class FmBatch(Batch):
    """xf_batch_compile_fm_dev: the FM key build against the (w, v) tables' settled tiers
    (`keyed` says whether the fast build ran; else it is the sort-based one).  The raw arrays go
    to the device through torch (plumbing)."""

    def __init__(self, wt, vt, rowptr, keys, labels):
        import torch
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        rp = np.ascontiguousarray(rowptr, dtype=np.uint64)
        rp32 = (rp - rp[0]).astype(np.uint32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        R, NNZ = len(rp32) - 1, int(rp32[-1])
        dk = torch.from_numpy(keys[int(rp[0]):int(rp[0]) + NNZ].view(np.int64).copy()).cuda()
        dr = torch.from_numpy(rp32.view(np.int32)).cuda()
        dl = torch.from_numpy(labels[:max(R, 1)] if R else np.zeros(1, np.int32)).cuda()
        torch.cuda.synchronize()
        self.h = vp()
        keyed = C.c_int(0)
        check(lib().xf_batch_compile_fm_dev(C.byref(self.h), wt.h, vt.h, dk.data_ptr(),
                                            dr.data_ptr(), dl.data_ptr(), R, NNZ, None,
                                            C.byref(keyed)))
        self.keyed = bool(keyed.value)
        Rr, N, U, H = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().xf_batch_dims(self.h, C.byref(Rr), C.byref(N), C.byref(U), C.byref(H)))
        self.R, self.NNZ, self.U, self.H = Rr.value, N.value, U.value, H.value
        self.on_gpu = True


class LocalBatch:
    """A minibatch compiled straight against one table on this GPU (xf_batch_compile_local):
    raw keys -> state rows -> cells; no key list.  Feeds lr_step / lr_predict on that table.
    values (one fp32 per nonzero): feature values — xf_batch_compile_local_valued, the cells
    carry them."""

    def __init__(self, table, rowptr, keys, labels, row_begin=0, row_end=None, retain_keys=True,
                 values=None):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if row_end is None:
            row_end = len(rowptr) - 1
        self.h = vp()
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float32)
            assert len(values) == len(keys), "one value per nonzero"
            check(lib().xf_batch_compile_local_valued(
                C.byref(self.h), table.h, _p(rowptr, u64p), _p(keys, u64p), _p(values, f32p),
                _p(labels, i32p), row_begin, row_end, 1 if retain_keys else 0, None))
        else:
            check(lib().xf_batch_compile_local(C.byref(self.h), table.h, _p(rowptr, u64p),
                                               _p(keys, u64p), _p(labels, i32p), row_begin,
                                               row_end, 1 if retain_keys else 0, None))
        R, N = C.c_uint32(), C.c_uint32()
        check(lib().xf_batch_dims(self.h, C.byref(R), C.byref(N), None, None))
        self.R, self.NNZ, self.U, self.H = R.value, N.value, 0, 0

    @classmethod
    def update(cls, table, ws, rowptr, keys, labels, retain_keys=True):
        """xf_lr_update_dev: the key build and the step of a fresh minibatch in one call (the
        raw arrays go to the GPU through torch first); returns the compiled minibatch"""
        import torch
        rp = np.ascontiguousarray(rowptr, dtype=np.uint64)
        rp32 = (rp - rp[0]).astype(np.uint32)
        kk = np.ascontiguousarray(keys, dtype=np.uint64)[int(rp[0]):int(rp[-1])]
        lb = np.ascontiguousarray(labels, dtype=np.int32)
        d_rp = torch.from_numpy(rp32.view(np.int32)).cuda()
        d_kk = torch.from_numpy(kk.view(np.int64).copy()).cuda() if len(kk) else None
        d_lb = torch.from_numpy(lb.copy()).cuda() if len(lb) else None
        torch.cuda.synchronize()
        self = cls.__new__(cls)
        self.h = vp()
        check(lib().xf_lr_update_dev(C.byref(self.h), table.h,
                                     d_kk.data_ptr() if d_kk is not None else None,
                                     d_rp.data_ptr(),
                                     d_lb.data_ptr() if d_lb is not None else None,
                                     len(rp32) - 1, len(kk), 1 if retain_keys else 0, ws.h, None))
        check(lib().xf_stream_sync(None))     # (the torch arrays go away with this frame)
        R, N = C.c_uint32(), C.c_uint32()
        check(lib().xf_batch_dims(self.h, C.byref(R), C.byref(N), None, None))
        self.R, self.NNZ, self.U, self.H = R.value, N.value, 0, 0
        return self

    def cells_info(self):
        return cells_info(self)

    def fwd_info(self):
        return fwd_info(self)

    def upload(self, stream=None):
        return self

    __del__ = Batch.__del__


FWD_INFO = ["W_f", "nwin_f", "G_f", "split", "copy_ready", "used"]


def fwd_info(batch):
    """the forward's own row windows over the batch's key-sorted copy (xf_batch_fwd_info)"""
    out = (C.c_uint32 * 6)()
    check(lib().xf_batch_fwd_info(batch.h, out))
    return dict(zip(FWD_INFO, list(out)))


def fwd_windows_rule(R, NNZ, M, kept=True, w_fixed=False, valued=False, tune=0):
    """the rule that picks them, by itself (no GPU): nwin_f, W_f, G_f and the gradient's nwin"""
    out = (C.c_uint32 * 4)()
    flags = (1 if kept else 0) | (2 if w_fixed else 0) | (4 if valued else 0)
    check(lib().xf_fwd_windows_rule(R, NNZ, M, flags, int(tune), out))
    return dict(zip(["nwin_f", "W_f", "G_f", "nwin"], list(out)))


def cells_info(batch):
    out = (C.c_uint32 * 8)()
    check(lib().xf_batch_cells_info(batch.h, out))
    names = ["W", "nwin", "nchunk", "G", "nitems", "segments", "nsplit_chunks", "M"]
    return dict(zip(names, list(out)))


LR_GRAD_KINDS = ("dense_masked", "dense_full", "dense_derived", "cells", "split_finish")


def lr_grad_launches():
    """launches of the LR gradient kernels so far, by kind (xf_lr_grad_launches): k_lr_grad_dense
    with byte-masked / whole-line stores, those of them that derived the old weight, the
    one-source k_lr_grad_cells, k_lr_grad_split_finish.  Subtract two readings."""
    out = np.zeros(len(LR_GRAD_KINDS), np.uint64)
    lib().xf_lr_grad_launches(_p(out, u64p))
    return dict(zip(LR_GRAD_KINDS, (int(x) for x in out)))


def div_by_const_probe(x, d, exact=False):
    """the FTRL step's x / d on the GPU, element by element (xf_div_by_const_probe): with the
    guard of the subnormal range, or — exact — the bare product with 1 / d"""
    require_gpu()
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    check(lib().xf_div_by_const_probe(_p(x, f32p), x.size, d, int(bool(exact)), _p(out, f32p)))
    return out


def scalar_probe(op, a, b=None, param=0):
    """a scalar function of the kernels on the GPU, element by element (xf_scalar_probe):
    SCALAR_SIGMOID sigmoid_ref(a), SCALAR_SQRT sqrtf(a), SCALAR_DIV a / b, SCALAR_DIV_ROWS
    div_by_rows(a, param)"""
    require_gpu()
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = np.empty_like(a)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        assert b.shape == a.shape, "one divisor per dividend"
    check(lib().xf_scalar_probe(op, _p(a, f32p), _p(b, f32p) if b is not None else None,
                                int(param), a.size, _p(out, f32p)))
    return out


def scalar_sweep(op, param=0, first_block=0, nblocks=1 << 16):
    """the digests of blocks first_block .. first_block + nblocks of the 65536 blocks of 65536
    floats each (xf_scalar_sweep): the wrapping sum of mix64(bits(a) << 32 | bits(op(a))) over
    the block, every NaN result counted as 0x7fc00000"""
    require_gpu()
    out = np.empty(nblocks, np.uint64)
    check(lib().xf_scalar_sweep(op, int(param), first_block, nblocks, _p(out, u64p)))
    return out


class Table:
    """One GPU's shard of the parameter table (ps-lite server replacement)."""

    def __init__(self, opt=OPT_FTRL, dim=1, init=INIT_ZERO, init_const=0.0, seed=0,
                 capacity=1 << 20, shard=0, nshards=1, **hyper):
        require_gpu()
        c = TableConfig()
        lib().xf_table_config_default(C.byref(c))
        c.opt_kind, c.dim, c.init_kind, c.init_const, c.seed = opt, dim, init, init_const, seed
        c.capacity, c.shard, c.nshards = capacity, shard, nshards
        for k, v in hyper.items():
            setattr(c, k, v)
        self.dim, self.opt = dim, opt
        self.h = vp()
        check(lib().xf_table_create(C.byref(self.h), C.byref(c)))

    @classmethod
    def from_handle(cls, h, dim, opt=OPT_FTRL):
        """Non-owning view of a table owned by a worker (XFGetTables)."""
        t = cls.__new__(cls)
        t.h, t.dim, t.opt, t._borrowed = h, dim, opt, True
        return t

    def __del__(self):
        try:
            if getattr(self, "h", None) and not getattr(self, "_borrowed", False):
                lib().xf_table_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        n = C.c_uint64(0)
        check(lib().xf_table_size(self.h, C.byref(n)))
        return n.value

    @property
    def settled(self):
        n = C.c_uint64(0)
        check(lib().xf_table_settled(self.h, C.byref(n)))
        return n.value

    @property
    def defrag_path(self):
        """how the last defrag() ordered the keys: one of the DEFRAG_* values"""
        p = C.c_int(0)
        check(lib().xf_table_defrag_path(self.h, C.byref(p)))
        return p.value

    @property
    def capacity(self):
        n = C.c_uint64(0)
        check(lib().xf_table_capacity(self.h, C.byref(n)))
        return n.value

    def reserve(self, capacity):
        check(lib().xf_table_reserve(self.h, capacity))

    def defrag(self):
        check(lib().xf_table_defrag(self.h))

    def evict(self, n_below):
        """drop every row with w == 0 and n < n_below (xf_table_evict: FTRL, dim 1; inf: every
        zero-weight row, 0: nothing) -> (rows seen, rows dropped)"""
        seen, dropped = C.c_uint64(0), C.c_uint64(0)
        check(lib().xf_table_evict(self.h, C.c_float(n_below), C.byref(seen),
                                   C.byref(dropped)))
        return seen.value, dropped.value

    def pull(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.empty(len(keys) * self.dim, dtype=np.float32)
        check(lib().xf_table_pull(self.h, _p(keys, u64p), len(keys), _p(out, f32p)))
        return out.reshape(len(keys), self.dim) if self.dim > 1 else out

    def push(self, keys, grads):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        grads = np.ascontiguousarray(grads, dtype=np.float32).ravel()
        assert grads.size == len(keys) * self.dim
        check(lib().xf_table_push(self.h, _p(keys, u64p), len(keys), _p(grads, f32p)))

    def export(self):
        n = C.c_size_t(0)
        check(lib().xf_table_export(self.h, None, None, None, None, 0, C.byref(n)))
        m = n.value
        keys = np.empty(m, dtype=np.uint64)
        w = np.empty(m * self.dim, dtype=np.float32)
        nn = np.empty(m * self.dim, dtype=np.float32)
        z = np.empty(m * self.dim, dtype=np.float32)
        if m:
            check(lib().xf_table_export(self.h, _p(keys, u64p), _p(w, f32p), _p(nn, f32p),
                                        _p(z, f32p), m, C.byref(n)))
        sh = (m, self.dim) if self.dim > 1 else (m,)
        return keys, w.reshape(sh), nn.reshape(sh), z.reshape(sh)

    def import_(self, keys, w, n=None, z=None):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32).ravel()
                for a in (w, n, z)]
        check(lib().xf_table_import(self.h, _p(keys, u64p), len(keys),
                                    *[None if a is None else _p(a, f32p) for a in arrs]))

    def set_hyper(self, alpha, beta, l1, l2, lr=0.001):
        check(lib().xf_table_set_hyper(self.h, alpha, beta, l1, l2, lr))

    def w_derived(self):
        """the gradient + Push kernels derive the old weight from (n, z) (xf_table_w_derived)"""
        yes = C.c_int(0)
        check(lib().xf_table_w_derived(self.h, C.byref(yes)))
        return bool(yes.value)

    def div_exact(self):
        """the table found its alpha an exact divisor: its steps divide by it without the guard
        of the subnormal range (xf_table_div_exact)"""
        yes = C.c_int(0)
        check(lib().xf_table_div_exact(self.h, C.byref(yes)))
        return bool(yes.value)

    # device-pointer API (ints = raw device addresses, e.g. torch.Tensor.data_ptr())
    def resolve_dev(self, d_keys, n, d_slots, stream=None):
        check(lib().xf_table_resolve_dev(self.h, d_keys, n, d_slots, stream))

    def gather_dev(self, d_slots, n, d_vals, stream=None):
        check(lib().xf_table_gather_dev(self.h, d_slots, n, d_vals, stream))

    def update_dev(self, d_slots, n, d_grads, stream=None):
        check(lib().xf_table_update_dev(self.h, d_slots, n, d_grads, stream))

    def check(self, stream=None):
        check(lib().xf_table_check(self.h, stream))


class Workspace:
    def __init__(self, capture=False):
        """capture=True: LR steps also keep the pulled weights and gradients per unique key for
        fetch() (the parity hook; the production step never forms them)."""
        self.h = vp()
        check(lib().xf_workspace_create(C.byref(self.h)))
        if capture:
            check(lib().xf_workspace_capture(self.h, 1))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_workspace_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def parity(self, mode):
        """'exact' (default) or 'reference_order' (fp32 running row sums in the reference's
        order: slow, for checking)"""
        check(lib().xf_workspace_parity(self.h, {"exact": 0, "reference_order": 1}[mode]))

    def fm_mode(self, mode):
        """FM form of fm_step / fm_predict: 'reference' (default: the reference's pooled
        second-order term) or 'canonical' (Rendle's per-factor sums)"""
        check(lib().xf_workspace_fm_mode(self.h, FM_MODES[mode]))

    def fm_fields(self, fields):
        """the number of fields of 'field_aware' (1 .. 64): before fm_mode('field_aware')"""
        check(lib().xf_workspace_fm_fields(self.h, int(fields)))

    def neg_weight(self, weight):
        """the weight of a kept negative (negative subsampling, NegSample.weight): every training
        step multiplies the losses of its label-0 rows by it; 1 (default): nothing is launched"""
        check(lib().xf_workspace_neg_weight(self.h, float(weight)))

    def progress(self, p):
        """attach a Progress (None: off, the default): every training step counts its losses
        after the forward has written them and before the negatives' weight touches them"""
        check(lib().xf_workspace_progress(self.h, p.h if p is not None else None))
        self._progress = p   # (the workspace holds a pointer to it)

    def slices(self, s):
        """attach a Slices (None: off, the default): a training step that was given its rows' ids
        (slice_ids) adds them to the slices right after the progress has counted them"""
        check(lib().xf_workspace_slices(self.h, s.h if s is not None else None))
        self._slices = s

    def slice_ids(self, d_id, R):
        """the ids (a device pointer the caller keeps alive until the step has run) of the NEXT
        training step's R rows; None: that step counts no slice"""
        check(lib().xf_workspace_slice_ids(self.h, d_id, int(R)))

    def gauc(self, g):
        """attach a Gauc (None: off, the default): a VALIDATE that was given its rows' ids
        (gauc_ids) appends their records right after the progress has counted them"""
        check(lib().xf_workspace_gauc(self.h, g.h if g is not None else None))
        self._gauc = g

    def gauc_ids(self, d_id, R):
        """the group ids (a device pointer the caller keeps alive until the validate has run) of
        the NEXT lr_validate / fm_validate's R rows; None: that validate appends nothing"""
        check(lib().xf_workspace_gauc_ids(self.h, d_id, int(R)))

    def fetch(self, U, R):
        wu = np.empty(U, np.float32)
        loss = np.empty(R, np.float32)
        g = np.empty(U, np.float32)
        check(lib().xf_workspace_fetch(self.h, _p(wu, f32p), _p(loss, f32p), _p(g, f32p), U, R))
        return wu, loss, g

    def fetch_loss(self, R):
        loss = np.empty(R, np.float32)
        check(lib().xf_workspace_fetch(self.h, None, _p(loss, f32p), None, 0, R))
        return loss

    def profile(self, enable):
        check(lib().xf_workspace_profile(self.h, 1 if enable else 0))

    def profile_read(self):
        ms = (C.c_double * 5)()
        steps = C.c_long(0)
        check(lib().xf_workspace_profile_read(self.h, ms, C.byref(steps)))
        names = ["resolve", "gather", "forward", "gradient", "update"]
        return {k: ms[i] for i, k in enumerate(names)}, steps.value


def lr_step(table, batch, ws, stream=None):
    check(lib().xf_lr_step(table.h, batch.h, ws.h, stream))


def fm_step(wt, vt, batch, ws, stream=None):
    check(lib().xf_fm_step(wt.h, vt.h, batch.h, ws.h, stream))


def lr_predict(table, batch, ws):
    out = np.empty(batch.R, np.float32)
    check(lib().xf_lr_predict(table.h, batch.h, ws.h, _p(out, f32p)))
    return out


def fm_predict(wt, vt, batch, ws):
    out = np.empty(batch.R, np.float32)
    check(lib().xf_fm_predict(wt.h, vt.h, batch.h, ws.h, _p(out, f32p)))
    return out


def lr_validate(table, batch, ws, progress):
    """xf_lr_predict's forward; the rows' losses counted into `progress` (a Progress) instead of
    pctr copied out"""
    check(lib().xf_lr_validate(table.h, batch.h, ws.h, progress.h))


def fm_validate(wt, vt, batch, ws, progress):
    check(lib().xf_fm_validate(wt.h, vt.h, batch.h, ws.h, progress.h))


def stream_sync(stream=None):
    check(lib().xf_stream_sync(stream))


def auc_logloss(labels, pctr, acc=0.0):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    pctr = np.ascontiguousarray(pctr, dtype=np.float32)
    ll, auc = C.c_float(acc), C.c_float(0)
    tp, fp = C.c_int(0), C.c_int(0)
    nat = C.c_double(0)
    check(lib().xf_auc_logloss(_p(labels, i32p), _p(pctr, f32p), len(labels), C.byref(ll),
                               C.byref(auc), C.byref(tp), C.byref(fp), C.byref(nat)))
    return ll.value, auc.value, tp.value, fp.value, nat.value


TRANSPORT_RCCL, TRANSPORT_HOST, TRANSPORT_AUTO = 0, 1, 2


class Group:
    """The process group of a multi-GPU run (xf_group_*): TCP bootstrap around rank 0, RCCL
    (or, for tests, host-staged) all-to-all-v."""

    def __init__(self, rank=-1, world=0, addr=None, port=0, transport=TRANSPORT_RCCL, device=-1):
        """device: >= 0 a GPU index, -1 the current device, -2 by rank (LOCAL_RANK, else rank
        modulo the visible devices)"""
        self.h = vp()
        check(lib().xf_group_create(C.byref(self.h), rank, world,
                                    addr.encode() if addr else None, port, transport, device))
        r, w, t = C.c_int(), C.c_int(), C.c_int()
        check(lib().xf_group_info(self.h, C.byref(r), C.byref(w), C.byref(t)))
        self.rank, self.world, self.transport = r.value, w.value, t.value

    def close(self):
        if getattr(self, "h", None):
            lib().xf_group_destroy(self.h)
            self.h = None

    __del__ = close

    def barrier(self):
        check(lib().xf_group_barrier(self.h))

    def allgather(self, arr):
        """every rank's (same-shaped) numpy array, stacked along a new first axis"""
        a = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + a.shape, a.dtype)
        check(lib().xf_group_allgather_host(self.h, a.ctypes.data, a.nbytes, out.ctypes.data))
        return out

    def gatherv(self, arr):
        """rank 0 gets the concatenation of every rank's 1-d array, the others None"""
        a = np.ascontiguousarray(arr)
        sizes = self.allgather(np.array([a.nbytes], np.uint64)).ravel()
        out = np.empty(int(sizes.sum()) // a.itemsize, a.dtype) if self.rank == 0 else None
        check(lib().xf_group_gatherv_host(self.h, a.ctypes.data, a.nbytes,
                                          out.ctypes.data if out is not None else None,
                                          _p(sizes, u64p)))
        return out

    def alltoallv_host(self, send, send_counts):
        """host arrays through the group (any transport that can move host memory)"""
        a = np.ascontiguousarray(send)
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        rc = np.ascontiguousarray(self.allgather(sc)[:, self.rank])
        out = np.empty(int(rc.sum()), a.dtype)
        check(lib().xf_group_alltoallv(self.h, a.ctypes.data, _p(sc, u64p), out.ctypes.data,
                                       _p(rc, u64p), a.itemsize, 1, None))
        return out, rc

    def alltoallv_dev(self, d_send, send_counts, d_recv, recv_counts, elem_bytes, stream=None,
                      channel=0):
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.uint64)
        check(lib().xf_group_alltoallv_ch(self.h, channel, d_send, _p(sc, u64p), d_recv,
                                          _p(rc, u64p), elem_bytes, 0, stream))

    def selftest(self, nbytes=1 << 20):
        """COLLECTIVE: both RCCL communicators driven at once from two streams"""
        check(lib().xf_group_selftest(self.h, nbytes))


SCHEDULE_SEQUENTIAL, SCHEDULE_STALE1, SCHEDULE_OWNER, SCHEDULE_OWNER_STALE1 = 0, 1, 2, 3
_SCHEDULES = {"sequential": SCHEDULE_SEQUENTIAL, "stale1": SCHEDULE_STALE1,
              "owner": SCHEDULE_OWNER, "owner_stale1": SCHEDULE_OWNER_STALE1}


class ShardedBatch:
    def __init__(self, h, owner=None):
        self.h = h
        # xf_sbatch_free looks at the trainer that compiled the minibatch (an outstanding
        # stale1 Push): the trainer must outlive its minibatches
        self._owner = owner
        R, N, U, own = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().xf_sbatch_dims(h, C.byref(R), C.byref(N), C.byref(U), C.byref(own)))
        self.R, self.NNZ, self.U, self.n_owned = R.value, N.value, U.value, own.value
        self.keyed = lib().xf_sbatch_fm_keyed(h) == 1

    def local_cells_info(self):
        """cells_info() of the minibatch's cells over the table's rows (a one-rank LR minibatch
        of the local builds: which build a compile took); XFError where it has none"""
        out = (C.c_uint32 * 8)()
        check(lib().xf_sbatch_cells_info(self.h, out))
        names = ["W", "nwin", "nchunk", "G", "nitems", "segments", "nsplit_chunks", "M"]
        return dict(zip(names, list(out)))

    def local_fwd_info(self):
        """fwd_info() of the same cells"""
        out = (C.c_uint32 * 6)()
        check(lib().xf_sbatch_fwd_info(self.h, out))
        return dict(zip(FWD_INFO, list(out)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().xf_sbatch_free(self.h)
                self.h = None
        except Exception:
            pass


class Sharded:
    """xf_sharded_*: LRWorker / FMWorker::update across the ranks of a Group (C++ + RCCL; this
    class only marshals).  group=None: one rank, the fused single-shard step."""

    def __init__(self, group=None, model="lr", optimizer="ftrl", k=10, capacity=1 << 22,
                 schedule="sequential", seed=0, host_key_build=False, update="rank_ordered",
                 fm_mode="reference", fields=None, **hyper):
        """fm_mode="canonical": Rendle's FM (xf_sharded_set_fm_mode); fm_mode="field_aware" with
        fields=F: k factors per field, v rows F k wide.  Both, and minibatches with feature values
        (compile(values=)), run on one rank and on a group of several ranks with schedule
        "sequential" or "stale1" (the weight / gradient exchange moves whole rows); the
        owner-compute schedules ("owner", "owner_stale1") and update="sum_then_step" refuse them"""
        require_gpu()
        c = ShardedConfig()
        lib().xf_sharded_config_default(C.byref(c))
        c.model = 0 if model == "lr" else 1
        c.optimizer = OPT_FTRL if optimizer == "ftrl" else OPT_SGD
        self.fields = int(fields) if fields is not None else 0
        assert fm_mode != "field_aware" or 1 <= self.fields <= 64, \
            "fm_mode='field_aware' needs fields=F, 1 .. 64"
        vdim = k * self.fields if fm_mode == "field_aware" else k
        c.k, c.capacity, c.seed = vdim, capacity, seed
        c.schedule = _SCHEDULES[schedule]
        c.host_key_build = 1 if host_key_build else 0
        c.update_rule = {"rank_ordered": 0, "sum_then_step": 1}[update]
        for name, v in hyper.items():
            setattr(c, name, v)
        self.group = group
        self.model, self.k = model, k
        self.h = vp()
        check(lib().xf_sharded_create(C.byref(self.h), group.h if group is not None else None,
                                      C.byref(c)))
        w, v = vp(), vp()
        check(lib().xf_sharded_tables(self.h, C.byref(w), C.byref(v)))
        self.w = Table.from_handle(w, 1, c.optimizer)
        self.v = Table.from_handle(v, vdim, c.optimizer) if v else None
        if fm_mode == "field_aware":
            check(lib().xf_sharded_set_fm_fields(self.h, self.fields))
        if fm_mode != "reference":
            self.set_fm_mode(fm_mode)

    def set_fm_mode(self, mode):
        """'reference', 'canonical' or 'field_aware': before the first step (the tables empty);
        several ranks: schedules 'sequential' and 'stale1' only"""
        check(lib().xf_sharded_set_fm_mode(self.h, FM_MODES[mode]))

    def stream(self):
        """the stream the trainer compiles and steps on (xf_sharded_stream; non-blocking): what a
        stage whose outputs are written in stream order — Cross.apply_dev — is given"""
        st = vp()
        check(lib().xf_sharded_stream(self.h, C.byref(st)))
        return st

    def set_neg_weight(self, weight):
        """the weight of a kept negative (Workspace.neg_weight); several ranks: schedules
        'sequential' and 'stale1' only"""
        check(lib().xf_sharded_set_neg_weight(self.h, float(weight)))

    def set_progress(self, enable):
        """progressive validation on the trainer's training steps (xf_sharded_progress); several
        ranks: schedules 'sequential' and 'stale1' only"""
        check(lib().xf_sharded_progress(self.h, 1 if enable else 0))

    def progress_read(self, reset=False, merged=False):
        """(counts, other) of this rank; merged=True: COLLECTIVE, the sum over the ranks"""
        counts = np.empty((2, PROGRESS_RANKS), np.uint64)
        other = np.empty(2, np.uint64)
        check(lib().xf_sharded_progress_read(self.h, _p(counts, u64p), _p(other, u64p),
                                             1 if reset else 0, 1 if merged else 0))
        return counts, other

    def set_holdout(self, enable):
        """held-out validation (xf_sharded_holdout): a second progress, counted by validate()
        alone; several ranks: schedules 'sequential' and 'stale1' only"""
        check(lib().xf_sharded_holdout(self.h, 1 if enable else 0))

    def validate(self, b):
        """predict's forward of minibatch b, its losses counted (xf_sharded_validate; COLLECTIVE)"""
        check(lib().xf_sharded_validate(self.h, b.h))

    def holdout_read(self, reset=False, merged=False):
        """(counts, other) of this rank's validates; merged=True: COLLECTIVE, the ranks' sum"""
        counts = np.empty((2, PROGRESS_RANKS), np.uint64)
        other = np.empty(2, np.uint64)
        check(lib().xf_sharded_holdout_read(self.h, _p(counts, u64p), _p(other, u64p),
                                            1 if reset else 0, 1 if merged else 0))
        return counts, other

    def set_gauc(self, enable):
        """the grouped AUC of the held rows (xf_sharded_gauc): validate() appends the records of
        minibatches that carry ids (batch_slices); needs set_holdout(True)"""
        check(lib().xf_sharded_gauc(self.h, 1 if enable else 0))

    def gauc_read(self, reset=False, merged=False, cap=None):
        """(ids ascending, figures [n, 4] = P, N, U2, T, none [2], other [2]) of this rank's
        records; merged=True: COLLECTIVE, every rank's records reduced on rank 0 (the others get
        n = 0)"""
        n = C.c_uint64()
        if cap is None:
            check(lib().xf_sharded_gauc_read(self.h, None, 0, C.byref(n), None, None, 0,
                                             1 if merged else 0))
            cap = n.value
        cap = max(int(cap), 1)
        entries = np.zeros((cap, GAUC_WORDS + 1), np.uint64)
        none, other = np.zeros(2, np.uint64), np.zeros(2, np.uint64)
        check(lib().xf_sharded_gauc_read(self.h, _p(entries, u64p), cap, C.byref(n),
                                         _p(none, u64p), _p(other, u64p), 1 if reset else 0,
                                         1 if merged else 0))
        return _gauc_result(entries, n.value, none, other)

    def set_slices(self, enable, field=0, log2_slots=16):
        """sliced progressive validation on the trainer's training steps (xf_sharded_slices);
        needs set_progress(True)"""
        check(lib().xf_sharded_slices(self.h, 1 if enable else 0, int(field), int(log2_slots)))
        self._slices_b = int(log2_slots)

    def batch_slices(self, b, d_id, R):
        """the ids of minibatch b's rows (xf_sbatch_set_slices: copied, in the order of
        stream()); None: the minibatch counts no slice"""
        check(lib().xf_sbatch_set_slices(b.h, d_id, int(R)))

    def slices_read(self, reset=False, merged=False):
        """(keys ascending, words [n, 7], none, overflow) of this rank; merged=True: COLLECTIVE,
        the ranks' entries merged by key"""
        n = C.c_uint64()
        check(lib().xf_sharded_slices_read(self.h, None, 0, C.byref(n), None, None, 0,
                                           1 if merged else 0))
        cap = max(n.value, 1)
        entries = np.zeros((cap, SLICE_WORDS + 1), np.uint64)
        none, overflow = np.zeros(SLICE_WORDS, np.uint64), np.zeros(SLICE_WORDS, np.uint64)
        check(lib().xf_sharded_slices_read(self.h, _p(entries, u64p), cap, C.byref(n),
                                           _p(none, u64p), _p(overflow, u64p),
                                           1 if reset else 0, 1 if merged else 0))
        return _slices_result(entries, n.value, none, overflow)

    def last_loss(self, b):
        """the (weighted) losses the last step of minibatch b left (xf_sharded_last_loss)"""
        out = np.empty(max(b.R, 1), np.float32)
        check(lib().xf_sharded_last_loss(self.h, b.h, _p(out, f32p), b.R))
        return out[:b.R]

    def close(self):
        if getattr(self, "h", None):
            lib().xf_sharded_destroy(self.h)
            self.h = None

    __del__ = close

    def compile(self, rowptr, keys, labels, row_begin=0, row_end=None, keep=True, values=None,
                fgid=None):
        """values (float32, beside keys): a minibatch with feature values; fgid (int32, beside
        keys): a minibatch with its fields, for fm_mode='field_aware'.  COLLECTIVE on a group: every
        rank compiles (a rank without rows: empty arrays), and an fgid outside [0, fields) on one
        rank is an XFError on every rank"""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.uint64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if len(labels) == 0:
            labels = np.zeros(1, np.int32)       # a non-null pointer for an empty minibatch
        if row_end is None:
            row_end = len(rowptr) - 1
        h = vp()
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float32)
            assert len(values) == len(keys), "one value per key"
            if len(values) == 0:
                values = np.zeros(1, np.float32)
        if fgid is not None:
            fgid = np.ascontiguousarray(fgid, dtype=np.int32)
            assert len(fgid) == len(keys), "one fgid per key"
            if len(fgid) == 0:
                fgid = np.zeros(1, np.int32)
            check(lib().xf_sharded_compile_fielded(
                self.h, C.byref(h), _p(rowptr, u64p), _p(keys, u64p), _p(fgid, i32p),
                _p(values, f32p) if values is not None else None, _p(labels, i32p), row_begin,
                row_end, 1 if keep else 0))
            return ShardedBatch(h, self)
        if values is not None:
            check(lib().xf_sharded_compile_valued(
                self.h, C.byref(h), _p(rowptr, u64p), _p(keys, u64p), _p(values, f32p),
                _p(labels, i32p), row_begin, row_end, 1 if keep else 0))
            return ShardedBatch(h, self)
        check(lib().xf_sharded_compile(self.h, C.byref(h), _p(rowptr, u64p), _p(keys, u64p),
                                       _p(labels, i32p), row_begin, row_end, 1 if keep else 0))
        return ShardedBatch(h, self)

    def compile_dev(self, d_keys, d_rowptr, d_labels, R, NNZ, keep=True):
        """device pointers (ints): raw keys in CSR order (u64), row offsets (u32, R + 1), labels
        (i32); the arrays may be released when this returns"""
        h = vp()
        check(lib().xf_sharded_compile_dev(self.h, C.byref(h), d_keys, d_rowptr, d_labels, R, NNZ,
                                           1 if keep else 0))
        return ShardedBatch(h, self)

    def compile_valued_dev(self, d_keys, d_vals, d_rowptr, d_labels, R, NNZ, keep=True):
        """compile_dev with the feature values (f32, beside the keys) as a device pointer"""
        h = vp()
        check(lib().xf_sharded_compile_valued_dev(self.h, C.byref(h), d_keys, d_vals, d_rowptr,
                                                  d_labels, R, NNZ, 1 if keep else 0))
        return ShardedBatch(h, self)

    def step(self, b):
        check(lib().xf_sharded_step(self.h, b.h))

    def predict(self, b):
        out = np.empty(max(b.R, 1), np.float32)
        check(lib().xf_sharded_predict(self.h, b.h, _p(out, f32p)))
        return out[:b.R]

    def flush(self):
        check(lib().xf_sharded_flush(self.h))

    def defrag(self):
        check(lib().xf_sharded_defrag(self.h))

    def evict(self, n_below):
        """drop this rank's zero-weight rows with n < n_below (xf_sharded_evict; local to the
        rank) -> (seen, dropped)"""
        seen, dropped = C.c_uint64(0), C.c_uint64(0)
        check(lib().xf_sharded_evict(self.h, C.c_float(n_below), C.byref(seen),
                                     C.byref(dropped)))
        return seen.value, dropped.value

    def check(self):
        check(lib().xf_sharded_check(self.h))

    def set_schedule(self, schedule):
        check(lib().xf_sharded_set_schedule(
            self.h, _SCHEDULES[schedule]))

    def save(self, prefix):
        check(lib().xf_sharded_save(self.h, prefix.encode()))

    def load(self, prefix):
        check(lib().xf_sharded_load(self.h, prefix.encode()))

    def profile(self, enable):
        check(lib().xf_sharded_profile(self.h, 1 if enable else 0))

    def profile_read(self):
        ms = (C.c_double * 6)()
        steps = C.c_long(0)
        check(lib().xf_sharded_profile_read(self.h, ms, C.byref(steps)))
        names = ["owner_pull", "a2a_weights", "forward", "gradient", "a2a_grads", "owner_update"]
        return {k: ms[i] for i, k in enumerate(names)}, steps.value


class XFlow:
    """XFCreate / XFSetParam / XFStartTrain / XFGetMetric / XFDestroy.  Every keyword is an
    XFSetParam name (include/xflow_amd.h lists them): cross="2*3", row_norm="l2", ..."""

    def __init__(self, train_prefix, test_prefix, **params):
        self.h = vp()
        check(lib().XFCreate(C.byref(self.h), train_prefix.encode(), test_prefix.encode()))
        for k, v in params.items():
            self.set(k, v)

    def set(self, name, value):
        check(lib().XFSetParam(self.h, name.encode(), str(value).encode()))

    def train(self):
        require_gpu()
        check(lib().XFStartTrain(C.byref(self.h)))

    def save(self, path):
        check(lib().XFSaveModel(self.h, path.encode()))

    def load(self, path):
        require_gpu()
        check(lib().XFLoadModel(self.h, path.encode()))

    def predict(self):
        check(lib().XFPredict(self.h))

    def metric(self, name):
        v = C.c_double(0)
        check(lib().XFGetMetric(self.h, name.encode(), C.byref(v)))
        return v.value

    def tables(self):
        w, v = vp(), vp()
        check(lib().XFGetTables(self.h, C.byref(w), C.byref(v)))
        return w, v

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().XFDestroy(C.byref(self.h))
        except Exception:
            pass
