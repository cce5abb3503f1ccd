"""ctypes loader for libmeepo_hip.so — the C-ABI declared in include/meepo_embedding.h.

There is no CPU fallback: if the HIP extension is missing this module raises, and every operator raises
`MeepoError` if the library reports an error (e.g. no gfx950 device).  torch is imported first on purpose:
the extension's `libamdhip64.so.7` dependency must resolve to the HIP runtime torch already loaded, so that
torch's streams and device pointers are valid inside the library.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEE_LIB_PATH") or os.path.join(_HERE, "libmeepo_hip.so")  # MEE_LIB_PATH: A/B against another build

OK = 0
ERR_INVALID_ARG, ERR_OUT_OF_MEMORY, ERR_HIP, ERR_NO_DEVICE, ERR_BATCH_TOO_LARGE, ERR_UNSUPPORTED, ERR_RCCL = -1, -2, -3, -4, -5, -6, -7
OPT_NONE, OPT_ADAGRAD, OPT_ADAM, OPT_FTRL = 0, 1, 2, 3
INIT_CONSTANT, INIT_UNIFORM = 0, 1
STATUS_TABLE_FULL, STATUS_RESERVED_KEY, STATUS_STALE_HANDLE, STATUS_INTERNAL = 1, 2, 4, 8
FIND_DEFAULT, FIND_STREAM_STORES, FIND_CACHED_STORES, FIND_STREAM_ROWS, FIND_STREAM_BUCKETS = 0, 1, 2, 4, 8   # mee_find_ex flags
HANDLE_SLOT_MASK = (1 << 40) - 1   # a located-find handle: bits 0..39 the slot (as mee_locate reports it), bits 40..61 the table's layout epoch
MEM_HBM, MEM_HOST_PINNED = 0, 1
DTYPE_F32, DTYPE_BF16 = 0, 1   # MEE_DTYPE_*: the row type of a typed-output lookup (mee_*_as)
DTYPE_INT8 = 2                 # ... a row STORAGE type only (mee_table_value_dtype of an int8-row table), never an out / in dtype
FLAG_INT8_ROWS = 8   # a serving table whose value plane holds int8 codes and one fp32 scale per row (SPEC.md §3 "Row storage type")
FLAG_TRACK_HITS, FLAG_ADMISSION, FLAG_BF16_ROWS = 1, 2, 4   # BF16_ROWS: a serving table whose value plane holds bf16 rows (SPEC.md §3 "Row storage type")
TIER_COUNT_COLD, TIER_COUNT_HOT = 1, 2   # mee_find_pooled_tiered flags
EVICT_LEAST, EVICT_RESET = 1, 2          # mee_evict flags
PAD_KEEP_FIRST, PAD_KEEP_LAST = 0, 1     # mee_find_padded_as flags: which end of a bag longer than max_len is kept
ABI_VERSION = 2   # MEE_ABI_VERSION of include/meepo_embedding.h this loader was written against
EMPTY_KEY = -(1 << 63)
RECLAIMED_KEY = EMPTY_KEY + 1
BUCKET_WIDTH = 16


class MeepoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"meepo error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("capacity", C.c_uint64), ("dim", C.c_uint32),
        ("optimizer", C.c_uint32), ("max_batch", C.c_uint64), ("default_value", C.c_float),
        ("initial_accumulator", C.c_float), ("initializer", C.c_uint32), ("init_scale", C.c_float),
        ("init_seed", C.c_uint64), ("value_memory", C.c_uint32), ("flags", C.c_uint32),
    ]


class FindRequest(C.Structure):
    _fields_ = [("d_keys", C.c_void_p), ("n", C.c_size_t), ("d_out", C.c_void_p), ("d_found", C.c_void_p)]


class Calibration(C.Structure):
    """mee_calibration: what mee_device_calibration measured (the apply's bucket-pair split by block-index parity)"""
    _fields_ = [("struct_size", C.c_uint32), ("xcd_split", C.c_uint32), ("from_env", C.c_uint32), ("placement_consistent", C.c_uint32),
                ("odd_over_even", C.c_float * 2), ("block_us_by_index_mod_8", C.c_float * 8), ("xcc_of_index_mod_8", C.c_uint32 * 8)]


class ShardedOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("max_batch", C.c_uint64), ("pad_slack", C.c_double),
                ("cold", C.c_void_p), ("hot_key_limit", C.c_uint64)]


SHARDED_DEDUP = 1


class TableInfo(C.Structure):
    _fields_ = [
        ("capacity", C.c_uint64), ("n_buckets", C.c_uint64), ("max_batch", C.c_uint64), ("dim", C.c_uint32),
        ("optimizer", C.c_uint32), ("table_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64),
    ]


class ChangesInfo(C.Structure):
    """mee_changes_info: a change log's capacity and its two device words"""
    _fields_ = [("capacity", C.c_uint64), ("size", C.c_uint64), ("invalid", C.c_uint32), ("pad", C.c_uint32)]


_vp, _sz, _u64, _u32, _i32, _f32 =C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_int32, C.c_float

# name -> (restype, argtypes); this is the full export list of include/meepo_embedding.h
PROTOTYPES = {
    "mee_abi_version": (C.c_int, []),
    "mee_last_error": (C.c_char_p, []),
    "mee_table_create": (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    "mee_table_destroy": (C.c_int, [_vp]),
    "mee_table_info_get": (C.c_int, [_vp, C.POINTER(TableInfo)]),
    "mee_clear": (C.c_int, [_vp, _vp]),
    "mee_set_tuning": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "mee_find": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_find_ex": (C.c_int, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp]),
    # typed output (fp32 | bf16 rows): d_out is followed by out_dtype
    "mee_find_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _u32, _vp]),
    # typed input (fp32 | bf16 rows): d_values is followed by in_dtype; bf16 rows go verbatim into a bf16-row table
    "mee_insert_as": (C.c_int, [_vp, _vp, _vp, _u32, _sz, _vp]),
    "mee_assign_as": (C.c_int, [_vp, _vp, _vp, _u32, _sz, _vp, _vp]),
    "mee_table_value_dtype": (C.c_int, [_vp, C.POINTER(_u32)]),
    "mee_find_located_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_find_located_prepare_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_find_or_insert_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp]),
    "mee_find_or_insert_located_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_find_or_insert_located_prepare_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_find_pooled_as": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _u32, _vp, _vp, C.c_int, _vp]),
    "mee_find_grouped_as": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _u32, _vp, _vp]),
    "mee_group_find_or_insert_as": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _u32, _vp, _vp]),
    "mee_group_find_pooled_as": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _u32, _vp, _vp, C.c_int, _vp]),
    # padded sequence lookup: (table | group), keys, n, bag offsets, (n_bags | bags_per_table), max_len, flags, out, out_dtype, found, lengths, step_keys, grad_index, stream
    "mee_find_padded_as": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "mee_group_find_padded_as": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    # ... over a hot/cold pair or a group of pairs: (hot, cold), then the same with count_flags (TIER_COUNT_*) behind flags (PAD_KEEP_*)
    "mee_find_padded_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "mee_group_find_padded_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _sz, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "mee_find_missing": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_find_counted": (C.c_int, [_vp, _vp, _sz, _vp, _vp, C.c_int, _vp]),
    "mee_hits_scan": (C.c_int, [_vp, _u32, _u32, C.c_int, _vp, _sz, C.POINTER(_sz), _vp]),
    # eviction by the hit counters: (t, max_hits, max_evict, flags, keys_out, values_out, state1_out, state2_out, hits_out, cap, d_n_out, stream)
    "mee_evict": (C.c_int, [_vp, _u32, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "mee_hits_find": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "mee_hits_assign": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "mee_hits_decay": (C.c_int, [_vp, _u32, _vp]),
    "mee_insert": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "mee_insert_missing": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "mee_find_or_insert_missing": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_assign": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "mee_find_plane": (C.c_int, [_vp, _u32, _vp, _sz, _vp, _vp, _vp]),
    "mee_assign_plane": (C.c_int, [_vp, _u32, _vp, _vp, _sz, _vp, _vp]),
    "mee_remove": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "mee_find_or_insert": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_export": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "mee_group_create": (C.c_int, [C.POINTER(_vp), _u32, _u64, C.POINTER(_vp)]),
    "mee_group_find_pooled": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, C.c_int, _vp]),
    "mee_group_apply_adagrad_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_group_apply_adam_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_group_find_pooled_jagged": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "mee_group_apply_adagrad_indexed": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _vp]),
    "mee_group_apply_adam_indexed": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_group_find_or_insert": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_group_apply_adagrad": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_group_apply_adam": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_group_destroy": (C.c_int, [_vp]),
    "mee_group_set_tuning": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "mee_group_value_dtype": (C.c_int, [_vp, C.POINTER(_u32)]),
    "mee_find_grouped": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    # mixed groups: members of different dims, class-major output (meepo_mixed.hip)
    "mee_mixed_group_create": (C.c_int, [C.POINTER(_vp), _u32, _u64, C.POINTER(_vp)]),
    "mee_mixed_group_destroy": (C.c_int, [_vp]),
    "mee_mixed_group_layout": (C.c_int, [_vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "mee_mixed_group_find_pooled": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp, C.c_int, C.c_int, _vp]),
    "mee_mixed_group_apply_adagrad_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_mixed_group_apply_adam_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_mixed_group_set_tuning": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    # keyed output of the pooled group lookups ([bags_per_table, sum of dims]): ..., out, out_dtype, out_row_stride (elements; 0 = the width), found,
    # [located,] step_index, mode, [insert_missing | flags,] stream
    "mee_group_find_pooled_keyed": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _sz, _vp, _vp, _vp, C.c_int, _vp]),
    "mee_group_find_pooled_tiered_keyed": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _sz, _vp, _vp, C.c_int, _u32, _vp]),
    "mee_mixed_group_find_pooled_keyed": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _sz, _vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "mee_mixed_group_keyed_layout": (C.c_int, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    # the keyed gradient taken apart into the class-major step buffer: group, keyed grads, in_dtype, row_stride, bags_per_table, bag offsets (mean), mode, out, stream
    "mee_mixed_group_keyed_grads": (C.c_int, [_vp, _vp, _u32, _sz, _sz, _vp, C.c_int, _vp, _vp]),
    "mee_find_pooled": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, C.c_int, _vp]),
    "mee_find_pooled_weighted": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "mee_find_pooled_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, C.c_int, _u32, _vp]),   # a hot/cold pair (tiered.py)
    # a group of hot/cold pairs (tiered.py, TieredTableGroup): hot group, cold group, ...
    "mee_group_find_pooled_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, C.c_int, _u32, _vp]),
    # ... with a jagged bag -> member map: keys, n, bag offsets, n_bags, member_bags, out (fp32), found, mode, flags, stream
    "mee_group_find_pooled_tiered_jagged": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, C.c_int, _u32, _vp]),
    "mee_group_ensure_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    # ... the unpooled forms: keys, member offsets, n, out, out_dtype, found, [to_cold,] flags, stream
    "mee_group_find_tiered": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _u32, _vp, _u32, _vp]),
    "mee_group_find_or_insert_tiered": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _u32, _vp, _vp, _u32, _vp]),
    # tier migration: src, dst, keys, [member offsets,] n, max_moves (a value | per-member limits on the device), moved mask, moved count(s), stream
    "mee_move": (C.c_int, [_vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp]),
    "mee_group_move": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_pooled_weighted_backward": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "mee_group_find_pooled_weighted": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "mee_group_pooled_weighted_backward": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    # max pooling: (table | group), keys, n, bag offsets, (n_bags | bags_per_table), out, out_dtype, found, argmax, stream; its backward: (table | group), n,
    # bag offsets, (n_bags | bags_per_table), argmax, bag grads, grads, stream
    "mee_find_pooled_max": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_group_find_pooled_max": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp, _vp]),
    "mee_pooled_max_backward": (C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_group_pooled_max_backward": (C.c_int, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_apply_adagrad_indexed": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _vp]),
    "mee_apply_adam_indexed": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_dedup_keys": (C.c_int, [_vp, _vp, _sz, _vp, _vp, C.c_int64, _vp]),
    "mee_reserve": (C.c_int, [_vp, _u64, _vp]),
    "mee_export_range": (C.c_int, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "mee_size": (C.c_int, [_vp, C.POINTER(_sz), _vp]),
    "mee_status": (C.c_int, [_vp, C.POINTER(_u32), _vp]),
    "mee_clear_status": (C.c_int, [_vp, _vp]),
    "mee_find_unordered": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_find_many": (C.c_int, [_vp, C.POINTER(FindRequest), _u32, _vp]),
    "mee_find_capture_stats": (C.c_int, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "mee_find_located": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_find_or_insert_located": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_find_located_prepare": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_find_or_insert_located_prepare": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_apply_adagrad_located": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_apply_adam_located": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_find_or_insert_admit": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _u32, _vp]),
    "mee_admission_decay": (C.c_int, [_vp, _u32, _vp]),
    "mee_group_find_or_insert_admit": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _u32, _vp, _u32, _vp, _vp]),
    "mee_group_admission_decay": (C.c_int, [_vp, _u32, _vp]),
    # admission into a hot/cold pair (the sketch is the hot table's): creating table, counting table, keys, n, out, found, min_count, stream
    "mee_find_or_insert_admit_missing": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _u32, _vp]),
    # ... over a group of pairs: hot, cold, keys, member offsets, n, out, out_dtype, found, to_cold, min_count, min_counts, flags, stream
    "mee_group_find_or_insert_admit_tiered": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp]),
    # ... in front of the pooled launch: hot, cold, keys, n, bag offsets, bags_per_table, found, to_cold, min_count, min_counts, stream
    "mee_group_ensure_admit_tiered": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _u32, _vp, _vp]),
    "mee_locate": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_table_plane": (C.c_int, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_u32)]),
    "mee_device_calibration": (C.c_int, [C.c_int32, C.POINTER(Calibration)]),
    "mee_probe_length": (C.c_int, [_vp, _vp, _sz, C.POINTER(_u64), _vp]),
    "mee_probe_histogram": (C.c_int, [_vp, _vp, _sz, C.POINTER(C.c_uint64), _vp]),
    "mee_apply_adagrad": (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_apply_adam": (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    # FTRL-Proximal: the Adagrad forms with (beta, l1, l2) after lr
    "mee_apply_ftrl": (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_apply_ftrl_located": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_apply_ftrl_indexed": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_group_apply_ftrl": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_group_apply_ftrl_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_group_apply_ftrl_indexed": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_mixed_group_apply_ftrl_pooled": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _vp]),
    "mee_apply_prepare": (C.c_int, [_vp, _vp, _sz, _vp]),
    "mee_apply_discard": (C.c_int, [_vp, _vp]),
    "mee_dedup_sum": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "mee_hash_batch": (C.c_int, [_vp, _sz, _u64, _u32, _vp, _vp, _vp, _vp]),
    "mee_router_create": (C.c_int, [_i32, _u64, _u32, C.POINTER(_vp)]),
    "mee_router_destroy": (C.c_int, [_vp]),
    "mee_partition_padded": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_partition": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_p2p_create": (C.c_int, [_i32, _u32, _u32, _u64, _u64, _u32, C.c_int, C.POINTER(_vp)]),
    "mee_p2p_barrier": (C.c_int, [_vp, _vp]),
    "mee_p2p_push_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mee_p2p_inbox": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "mee_p2p_destroy": (C.c_int, [_vp]),
    "mee_p2p_export": (C.c_int, [_vp, _vp]),
    "mee_p2p_connect": (C.c_int, [_vp, _vp]),
    "mee_p2p_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mee_p2p_push": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mee_p2p_find": (C.c_int, [_vp, _vp, _vp]),
    "mee_p2p_status": (C.c_int, [_vp, C.POINTER(_u32), _vp]),
    "mee_scatter_rows": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    "mee_gather_rows": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp]),
    # embedding bags over a sharded table: run bookkeeping and the combination of the owners' partial rows (meepo_router.hip)
    "mee_bag_runs": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "mee_run_offsets": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "mee_combine_bag_runs": (C.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _u32, C.c_int, _vp, _u32, _vp]),
    "mee_segment_counts": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "mee_regroup": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp]),
    # row-sharded table over RCCL (meepo_sharded.hip)
    "mee_comm_unique_id": (C.c_int, [_vp]),
    "mee_comm_create": (C.c_int, [_vp, _u32, _u32, _i32, C.POINTER(_vp)]),
    "mee_comm_destroy": (C.c_int, [_vp]),
    "mee_comm_aborted": (C.c_int, [_vp]),
    "mee_sharded_create": (C.c_int, [_vp, _vp, _u64, C.c_double, C.POINTER(_vp)]),
    "mee_sharded_create_ex": (C.c_int, [_vp, _vp, C.POINTER(ShardedOptions), C.POINTER(_vp)]),
    "mee_sharded_clear_status": (C.c_int, [_vp, _vp]),
    "mee_sharded_destroy": (C.c_int, [_vp]),
    "mee_sharded_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64)]),
    "mee_sharded_find": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_sharded_find_or_insert": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "mee_sharded_find_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp]),
    "mee_sharded_find_or_insert_as": (C.c_int, [_vp, _vp, _sz, _vp, _u32, _vp, _vp]),
    "mee_sharded_traffic": (C.c_int, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "mee_sharded_insert": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "mee_sharded_assign": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "mee_sharded_remove": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "mee_sharded_apply_adagrad": (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _vp]),
    "mee_sharded_apply_adam": (C.c_int, [_vp, _vp, _vp, _sz, _f32, _f32, _f32, _f32, _u64, _vp]),
    "mee_sharded_size": (C.c_int, [_vp, C.POINTER(_sz), _vp]),
    "mee_sharded_status": (C.c_int, [_vp, C.POINTER(_u32), _vp]),
    # change log (a device key set) and the delta export: note (log, keys, n, stream); group note (group, keys, member offsets, n, stream);
    # export_changed (table, log, slot_begin, slot_end, keys_out, values_out, state1_out, state2_out, cap, removed_out, removed_cap, counts_out [2], stream)
    "mee_changes_create": (C.c_int, [_i32, _u64, C.POINTER(_vp)]),
    "mee_changes_destroy": (C.c_int, [_vp]),
    "mee_changes_note": (C.c_int, [_vp, _vp, _sz, _vp]),
    "mee_changes_group_create": (C.c_int, [C.POINTER(_vp), _u32, C.POINTER(_vp)]),
    "mee_changes_group_destroy": (C.c_int, [_vp]),
    "mee_changes_group_note": (C.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "mee_changes_info_get": (C.c_int, [_vp, C.POINTER(ChangesInfo)]),
    "mee_changes_clear": (C.c_int, [_vp, _vp]),
    "mee_changes_invalidate": (C.c_int, [_vp, _vp]),
    "mee_export_changed": (C.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    # publish (src table, log, dst table, slot_begin, slot_end, counts_out [4], stream); group form (src group, log group, dst group, counts_out [n_tables][4], stream)
    "mee_publish_changed": (C.c_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "mee_group_publish_changed": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
}

_NARROW_ROWS = {torch.bfloat16: "a bf16-row table (value_dtype=torch.bfloat16) is a serving table with find, find_pooled, insert, assign, ",
                torch.int8: "an int8-row table (int8_rows=True) is a serving table with find, insert, assign, "}


def refuse_narrow_rows(who: str, *tables) -> None:
    """Groups, tiered pairs, sharded / peer tables and the nn layers are built over fp32 tables: a serving table — LookupTable(value_dtype=torch.bfloat16) or
    LookupTable(int8_rows=True), whose .value_dtype is torch.int8 — alone or as a member of a group handed in — is refused at construction, before anything is created; the message
    names the row type."""
    for t in tables:
        if t is None:
            continue
        for m in [t, *getattr(t, "tables", ())]:
            kind = _NARROW_ROWS.get(getattr(m, "value_dtype", torch.float32))
            if kind:
                raise MeepoError(ERR_UNSUPPORTED, f"{who}: {kind}remove, export and reserve of its own; it cannot be a member of a group, a tier, a shard or a trained layer")


def group_row_dtype(who: str, *tables) -> torch.dtype:
    """The row storage type of a uniform group: torch.float32, or torch.bfloat16 when EVERY member is a bf16-row table (a serving group: lookups only).
    A mix is refused as refuse_narrow_rows refuses a bf16-row table — one storage type per group; an int8-row table is no member of any group (refused
    through refuse_narrow_rows).  Only .value_dtype is looked at (absent: fp32)."""
    refuse_narrow_rows(who, *[t for t in tables if getattr(t, "value_dtype", torch.float32) == torch.int8])
    kinds = {getattr(t, "value_dtype", torch.float32) == torch.bfloat16 for t in tables}
    if kinds == {True}:
        return torch.bfloat16
    if True in kinds:
        raise MeepoError(ERR_UNSUPPORTED, f"{who}: a bf16-row table (value_dtype=torch.bfloat16) and an fp32-row table cannot share a group — "
                                          "a group holds fp32-row tables or bf16-row tables, never both (serving_copy() makes the bf16-row twin of a whole group)")
    return torch.float32


_lib = None


def lib() -> C.CDLL:
    """Load the HIP extension (once).  Raises ImportError loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). meepoembedding_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        older = os.environ.get("MEE_LIB_OLDER_BUILD") == "1"   # A/B runs of tools/ against an earlier round's library (MEE_LIB_PATH): entry points it lacks stay unbound
        for name, (res, args) in PROTOTYPES.items():
            if older and not hasattr(L, name):
                continue
            fn = getattr(L, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if L.mee_abi_version() != ABI_VERSION:  # noqa: PLR2004
            raise ImportError(f"{LIB_PATH}: ABI version {L.mee_abi_version()} != {ABI_VERSION}")
        _lib = L
    return _lib


def device_calibration(device: int = 0) -> dict:
    """mee_device_calibration as a dict (runs the probe if no table with an optimizer has been created on the device yet)"""
    c = Calibration(struct_size=C.sizeof(Calibration))
    check(lib().mee_device_calibration(int(device), C.byref(c)))
    return {"xcd_split": c.xcd_split, "from_env": bool(c.from_env), "placement_consistent": bool(c.placement_consistent),
            "odd_over_even": [round(float(x), 4) for x in c.odd_over_even], "block_us_by_index_mod_8": [round(float(x), 2) for x in c.block_us_by_index_mod_8],
            "xcc_of_index_mod_8": [int(x) for x in c.xcc_of_index_mod_8]}


def check(rc: int) -> None:
    if rc != OK:
        raise MeepoError(rc, lib().mee_last_error().decode("utf-8", "replace"))
