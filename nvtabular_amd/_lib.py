"""ctypes binding of the C ABI in ``include/nvt_hip.h`` (``libnvt_hip.so``).

The north star asks for cffi; cffi is not installed in this image, so the thin
FFI layer is stdlib ``ctypes`` over the same ``extern "C"`` entry points.

There is deliberately NO fallback: if the shared library is missing or a GPU is
not visible, every compute entry raises.  (The oracle under ``oracle/`` is test
infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# NVT_HIP_LIB: an alternative build of the same library (A / B measurements of kernel variants)
LIB_PATH = os.environ.get("NVT_HIP_LIB") or os.path.join(_HERE, "libnvt_hip.so")

# dtype codes (include/nvt_hip.h)
NVT_F32, NVT_F64, NVT_I32, NVT_I64, NVT_U8 = 0, 1, 2, 3, 4
NVT_I8, NVT_I16 = 5, 6   # outputs of nvt_cast_many only
NVT_GB_SUMSQ, NVT_GB_MINMAX = 1, 2
NVT_EINVAL, NVT_EHIP, NVT_ENOMEM, NVT_EUNSUPPORTED = -1, -2, -3, -4   # include/nvt_hip.h
ENCODE_HEAD_BYTES = 12288 * 12 + 64   # NVT_ENCODE_HEAD_BYTES
ST_NULLS, ST_SENTINEL, ST_OCCUPIED, ST_OVERFLOW, ST_ROWS = 0, 1, 2, 3, 4
ST_MAXCOUNT = 8
ST_BIG = 9
ST_NEED = 10
STATE_WORDS = 16

_vp, _u64, _i64, _i32, _u32, _dbl = (
    C.c_void_p,
    C.c_uint64,
    C.c_int64,
    C.c_int,
    C.c_uint32,
    C.c_double,
)
_pp = C.POINTER(C.c_void_p)

# name -> argtypes (restype is int unless listed in _RESTYPES)
SIGNATURES = {
    "nvt_version": [],
    "nvt_last_error": [],
    "nvt_count_table_bytes": [_i32, _u64, C.POINTER(_u64)],
    "nvt_count_clear": [_vp, _i32, _u64, _vp, _vp],
    "nvt_count_i32": [_vp, _vp, _u64, _vp, _u64, _vp, _vp],
    "nvt_count_i64": [_vp, _vp, _u64, _vp, _u64, _vp, _vp],
    "nvt_count_merge_i32": [_vp, _vp, _u64, _vp, _u64, _vp, _vp],
    "nvt_count_merge_i64": [_vp, _vp, _u64, _vp, _u64, _vp, _vp],
    "nvt_count_compact_i32": [_vp, _u64, _vp, _vp, _vp, _vp],
    "nvt_count_compact_i64": [_vp, _u64, _vp, _vp, _vp, _vp],
    "nvt_dense_count_ws_bytes": [_i32, _u64, _i32, _i32, C.POINTER(_u64)],
    "nvt_range_table_bytes": [_i32, C.POINTER(_u64)],
    "nvt_dense_count_i32": [_vp, _vp, _vp, _u64, _i32, _vp, _vp, _vp, _u64, _vp, _vp],
    "nvt_dense_count_i64": [_vp, _vp, _vp, _u64, _i32, _vp, _vp, _vp, _u64, _vp, _vp],
    "nvt_vocab_sort_tmp_bytes": [_i32, _u64, C.POINTER(_u64)],
    "nvt_vocab_order_tmp_bytes": [_u64, _u64, C.POINTER(_u64)],
    "nvt_class_hist": [_vp, _u64, _vp, _vp],
    "nvt_vocab_sort_i32": [_vp, _vp, _u64, _i64, _vp, _vp],
    "nvt_vocab_sort_i64": [_vp, _vp, _u64, _i64, _vp, _vp],
    "nvt_encode_table_bytes": [_i32, _u64, C.POINTER(_u64)],
    "nvt_encode_build_i32": [_vp, _u64, _i64, _vp, _u64, _vp, _i32, _vp],
    "nvt_encode_build_i64": [_vp, _u64, _i64, _vp, _u64, _vp, _i32, _vp],
    "nvt_encode_i32": [_vp, _vp, _u64, _vp, _u64, _vp, _i64, _i64, _u32, _vp, _i32, _vp, _u64, _i64,
                       _vp],
    "nvt_encode_i64": [_vp, _vp, _u64, _vp, _u64, _vp, _i64, _i64, _u32, _vp, _i32, _vp, _u64, _i64,
                       _vp],
    "nvt_hash_bucket_i32": [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp],
    "nvt_hash_bucket_i64": [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp],
    "nvt_moments_scratch_bytes": [],
    "nvt_moments": [_vp, _i32, _vp, _u64, _i32, _dbl, _vp, _vp, _vp],
    "nvt_minmax": [_vp, _i32, _vp, _u64, _i32, _vp, _vp, _vp],
    "nvt_fill_normalize": [_vp, _i32, _vp, _u64, _i32, _dbl, _i32, _dbl, _dbl, _vp, _i32, _vp, _vp],
    "nvt_clip_log": [_vp, _i32, _vp, _u64, _i32, _dbl, _i32, _dbl, _i32, _dbl, _i32, _vp, _i32, _vp],
    "nvt_bucketize": [_vp, _i32, _vp, _u64, _vp, _i32, _vp, _vp],
    "nvt_gb_create": [_i32, _i32, _i32, _u64, _pp],
    "nvt_gb_destroy": [_vp],
    "nvt_gb_table_bytes": [_i32, _i32, _i32, _u64, C.POINTER(_u64)],
    "nvt_gb_create_in": [_i32, _i32, _i32, _u64, _vp, _u64, _pp],
    "nvt_gb_state_ptr": [_vp],
    "nvt_gb_update_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_gb_set_workspace": [_vp, _vp, _u64],
    "nvt_gb_clear": [_vp, _vp],
    "nvt_gb_update": [_vp, _pp, _pp, _pp, C.POINTER(C.c_int), _pp, _u64, _vp],
    "nvt_gb_merge": [_vp, _pp, _vp, _vp, _vp, _pp, _pp, _pp, _pp, _u64, _vp],
    "nvt_gb_state": [_vp, C.POINTER(_u64), _vp],
    "nvt_gb_compact": [_vp, _pp, _vp, _vp, _vp, _pp, _pp, _pp, _pp, _vp, _vp],
    "nvt_gb_index_build": [_vp, _pp, _vp, _u64, _vp],
    "nvt_gb_lookup": [_vp, _pp, _pp, _u64, _vp, _vp],
    "nvt_sort_key_u64": [_vp, _i32, _vp, _u64, _i32, _vp, _vp],
    "nvt_order_rows_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_order_rows": [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp],
    "nvt_seg_aggregate": [_vp, _u64, _u64, _pp, C.POINTER(C.c_int), _pp, _i32, _vp, _vp, _vp, _vp,
                          _vp, _vp, _vp],
    "nvt_seg_nunique_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_seg_nunique": [_vp, _u64, _u64, _pp, C.POINTER(C.c_int), _pp, _i32, _vp, _vp, _vp],
    "nvt_gather_f64": [_vp, _vp, _u64, _dbl, _vp, _i32, _vp],
    "nvt_te_apply": [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _dbl, _dbl, _vp, _i32, _vp],
    "nvt_te_apply_folds": [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _u64, _dbl, _dbl, _vp, _i32, _vp],
    "nvt_sgb_sort_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_key_minmax": [_vp, _i32, _u64, _vp, _vp],
    "nvt_sgb_sort": [_vp, _i32, _i64, _vp, _i32, _u64, _vp, C.POINTER(_vp), C.POINTER(C.c_int), _vp],
    "nvt_sgb_regroup_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_sgb_regroup": [_vp, _i32, _i32, _i64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp],
    "nvt_sgb_reduce": [_vp, _i32, _i32, _pp, C.POINTER(C.c_int), _pp, _i32, _i32, _u64, _u64,
                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pp, _pp, _vp],
    "nvt_flat_lookup_gather": [_vp, _i32, _vp, _u64, _vp, _vp, _u64, _i64, _vp, _i32, _pp,
                               C.POINTER(C.c_int), C.POINTER(_dbl), _vp, _vp],
    "nvt_flat_lookup_te": [_vp, _i32, _vp, _u64, _vp, _vp, _u64, _i64, _vp, _i32, _vp, _dbl, _dbl, _vp,
                           _i32, _vp],
    "nvt_flat_lookup_image": [_vp, _i32, _vp, _u64, _vp, _vp, _u64, _i64, _vp, _vp, _vp, _u32, _i32, _pp,
                              _pp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64), _vp, _vp],
    "nvt_image_pack": [_pp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_u32), _i32, _u64, _vp,
                       _u32, _vp],
    "nvt_jg_image": [_vp, _pp, _pp, _pp, _pp, _i32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                     C.POINTER(_u32), _i32, _u64, _vp, _u32, _vp],
    "nvt_te_image": [_vp, _vp, _vp, _vp, _i32, _u64, _dbl, _dbl, _i32, _vp, _u32, _u32, _vp],
    "nvt_fold_mt19937_par_ws_bytes": [_u64, _i32, C.POINTER(_u64)],
    "nvt_fold_mt19937_par": [_u32, _i32, _u64, _vp, _vp, _u64, _vp, _vp],
    "nvt_encode_stats": [C.POINTER(_u64), _i32, _vp],
    "nvt_pq_decode_chunk": [_vp, _u64, _i32, _i32, _u64, _vp, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)],
    "nvt_pq_decode_chunk_codec": [_vp, _u64, _i32, _i32, _i32, _u64, _vp, _u64, _vp, _u64, _vp, _u64,
                                  C.POINTER(_u64), C.POINTER(_u64)],
    "nvt_pq_decode_list_chunk": [_vp, _u64, _i32, _i32, _i32, _i32, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _u64,
                                 _vp, _u64, C.POINTER(_u64)],
    "nvt_pq_decode_str_chunk": [_vp, _u64, _i32, _i32, _u64, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)],
    "nvt_pq_expand_runs": [_vp, _u64, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp],
    "nvt_expand_valid_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_expand_valid": [_vp, _i32, _vp, _u64, _vp, _vp, _vp],
    "nvt_exchange_ranges": [_vp, _i32, _vp, _vp],
    "nvt_exchange_ranges_sorted": [_vp, _i32, _vp, _vp],
    "nvt_exchange_hist": [_vp, _i32, C.POINTER(_i64), C.POINTER(_u64), _i32, _vp, _vp],
    "nvt_exchange_scatter": [_vp, _i32, C.POINTER(_i64), C.POINTER(_u64), _i32, _vp, _vp, _vp],
    "nvt_exchange_pack_ordered": [_vp, _i32, C.POINTER(_i64), C.POINTER(_u64), _i32, _vp, _vp, _vp, _vp],
    "nvt_exchange_unpack": [_vp, _u64, _vp, _vp, _i32, _vp, _vp, _vp],
    "nvt_count_merge_sorted_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_count_merge_sorted": [_vp, _u64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "nvt_flat_index_tmp_bytes": [_u64, C.POINTER(_u64)],
    "nvt_flat_index_build": [_vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp],
    "nvt_flat_lookup": [_vp, _i32, _vp, _u64, _vp, _vp, _u64, _i64, _vp, _vp],
    "nvt_widen_i64": [_vp, _i32, _u64, _vp, _vp],
    "nvt_popcount": [_vp, _u64, _vp, _vp],
    "nvt_fold_mt19937": [_u32, _i32, _u64, _vp, _vp],
    "nvt_prefix_distinct": [_vp, _i32, _vp, _vp],
    "nvt_vocab_label_shard": [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "nvt_exchange_unpack2": [_vp, _vp, _u64, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
}


class PrefixCol(C.Structure):
    _fields_ = [("keys", _vp), ("valid", _vp), ("n", _u64), ("key_bytes", _i32)]


class XCol(C.Structure):
    _fields_ = [("keys", _vp), ("counts", _vp), ("n", _u64)]


class MomentsCol(C.Structure):
    _fields_ = [("x", _vp), ("valid", _vp), ("n", _u64), ("dtype", C.c_int32),
                ("has_fill", C.c_int32), ("fill_val", _dbl), ("out3", _vp)]


class FillNormCol(C.Structure):
    _fields_ = [("x", _vp), ("valid", _vp), ("n", _u64), ("dtype", C.c_int32),
                ("has_fill", C.c_int32), ("fill_val", _dbl), ("do_norm", C.c_int32),
                ("out_dtype", C.c_int32), ("shift", _dbl), ("scale", _dbl), ("out", _vp),
                ("filled", _vp), ("moments", _vp)]


class CountCol(C.Structure):
    _fields_ = [("keys", _vp), ("valid", _vp), ("weights", _vp), ("n", _u64),
                ("key_bytes", C.c_int32), ("path", C.c_int32), ("ws", _vp), ("out_keys", _vp),
                ("out_counts", _vp), ("out_capacity", _u64), ("state", _vp), ("hot_image", _vp),
                ("range_table", _vp), ("out_slots", _vp)]


class VocabCol(C.Structure):
    _fields_ = [("keys", _vp), ("counts", _vp), ("n", _u64), ("max_count", _i64),
                ("key_bytes", C.c_int32), ("unique_keys", C.c_int32), ("sort_tmp", _vp),
                ("first_label", _i64), ("table", _vp), ("capacity", _u64),
                ("sentinel_label", _vp), ("ready_event", _vp), ("src_keys", _vp),
                ("src_counts", _vp), ("cls_hist", _vp), ("n_big", _u64), ("range_aux", _vp),
                ("range_nb_log2", C.c_int32), ("flat_slots", C.c_uint64), ("src_labels", _vp),
                ("head_image", _vp), ("src_slots", _vp)]


class MergeCol(C.Structure):
    _fields_ = [("a_keys", _vp), ("a_counts", _vp), ("na", _u64), ("b_keys", _vp),
                ("b_counts", _vp), ("nb", _u64), ("out_keys", _vp), ("out_counts", _vp),
                ("src_a", _vp), ("src_b", _vp), ("out_n", _vp)]


class PqStrStage(C.Structure):
    """nvt_pq_str_stage: the staging buffers of one string column of a partition and how far they
    are filled (nvt_pq_decode_str_chunk)."""
    _fields_ = [("offsets", _vp), ("chars", _vp), ("runs", _vp), ("packed", _vp),
                ("entries_cap", _u64), ("chars_cap", _u64), ("runs_cap", _u64), ("packed_cap", _u64),
                ("entries", _u64), ("nchars", _u64), ("nruns", _u64), ("npacked", _u64), ("nvalues", _u64)]


PQ_RUN_REPEAT, PQ_RUN_PACKED, PQ_RUN_SEQUENCE, PQ_RUN_END = 0, 1, 2, 3   # include/nvt_hip.h NVT_PQ_RUN_*
PQ_STR_GROW = 1


class ImagePart(C.Structure):
    """nvt_image_part: one operator's byte range of the records (nvt_image_build)."""
    _fields_ = [("kind", C.c_int32), ("nvals", C.c_int32), ("ncols", C.c_int32), ("kfold", C.c_int32),
                ("out_dtype", C.c_int32), ("offset", C.c_uint32), ("groups", _u64), ("count", _vp),
                ("sum", _vp), ("sumsq", _vp), ("mn", _vp), ("mx", _vp), ("kinds", _vp), ("vals", _vp),
                ("dst_dtypes", _vp), ("offs", _vp), ("tot_count", _vp), ("tot_sum", _vp),
                ("fold_count", _vp), ("fold_sum", _vp), ("p_smooth", _dbl), ("y_mean", _dbl),
                ("moments", _vp)]


IMAGE_PART_JG, IMAGE_PART_TE = 0, 1   # include/nvt_hip.h NVT_IMAGE_PART_*
IMAGE_BUILD_MAX_PARTS, IMAGE_BUILD_MAX_STRIDE = 4, 192


class EncodeCol(C.Structure):
    _fields_ = [("keys", _vp), ("valid", _vp), ("n", _u64), ("table", _vp), ("capacity", _u64),
                ("sentinel_label", _vp), ("null_label", _i64), ("oov_label", _i64),
                ("num_buckets", _u32), ("key_bytes", C.c_int32), ("out_bytes", C.c_int32),
                ("out", _vp), ("vocab_keys", _vp), ("n_vocab", _u64), ("first_label", _i64),
                ("wait_event", _vp), ("range_aux", _vp), ("head_image", _vp)]


SIGNATURES.update({
    "nvt_keydir_build": [_vp, _u64, _u64, _vp, _vp],
    "nvt_keydir_lookup_image": [_vp, _i32, _vp, _u64, _vp, _u64, _vp, _u64, _i64, _i64, _vp, _u32, _i32, _pp,
                                _pp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64), _vp, _vp],
    "nvt_image_build": [C.POINTER(ImagePart), _i32, _u64, _vp, _u32, _vp],
    "nvt_moments_many": [C.POINTER(MomentsCol), _i32, _vp, _vp],
    "nvt_fill_normalize_many": [C.POINTER(FillNormCol), _i32, _vp],
    "nvt_dense_count_many": [C.POINTER(CountCol), _i32, _vp],
    "nvt_vocab_finalize_many": [C.POINTER(VocabCol), _i32, _vp],
    "nvt_encode_many": [C.POINTER(EncodeCol), _i32, _vp],
    "nvt_merge_sorted_ws_bytes": [C.POINTER(MergeCol), _i32, C.POINTER(_u64)],
    "nvt_merge_sorted_many": [C.POINTER(MergeCol), _i32, _vp, _u64, _vp],
    "nvt_merge_payload": [_vp, _vp, _u64, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "nvt_event_create": [_pp],
    "nvt_event_destroy": [_vp],
    "nvt_stream_wait_event": [_vp, _vp],
    "nvt_mailbox_create": [_u64, _pp],
    "nvt_mailbox_destroy": [_vp],
    "nvt_mailbox_data": [_vp],
    "nvt_mailbox_capacity": [_vp],
    "nvt_mailbox_post": [_vp, _vp, _u64, _vp, C.POINTER(_u64)],
    "nvt_mailbox_wait": [_vp, _u64, _dbl],
    "nvt_prof_begin": [],
    "nvt_prof_report": [C.c_char_p, _u64, C.POINTER(_u64)],
    "nvt_range_push": [C.c_char_p],
    "nvt_range_pop": [],
    "nvt_str_hash": [_vp, _i32, _vp, _vp, _u64, _vp, _vp],
    "nvt_str_take_keys": [_vp, _u64, _vp, _i32, _vp, _u64, _vp, _vp],
    "nvt_str_dedup_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_str_dedup": [_vp, _vp, _u64, _vp, _i32, _vp, _i32, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp],
    "nvt_str_gather_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_str_gather": [_vp, _u64, _vp, _i32, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp],
})


class DropnaCol(C.Structure):
    """nvt_dropna_col: one column tested by nvt_compact_keep_dropna."""
    _fields_ = [("x", _vp), ("valid", _vp), ("dtype", C.c_int32), ("reserved", C.c_int32)]


class CompactCol(C.Structure):
    """nvt_compact_col: one column moved by nvt_compact_many."""
    _fields_ = [("src", _vp), ("dst", _vp), ("src_valid", _vp), ("dst_valid", _vp), ("plan", _vp),
                ("n", _u64), ("width", C.c_int32), ("reserved", C.c_int32)]


class FilterCol(C.Structure):
    """nvt_filter_col: one column read by nvt_compact_keep_terms."""
    _fields_ = [("x", _vp), ("valid", _vp), ("dtype", C.c_int32), ("reserved", C.c_int32)]


class FilterValue(C.Union):
    _fields_ = [("i", C.c_int64), ("f", C.c_double)]


class FilterTerm(C.Structure):
    """nvt_filter_term: one comparison of nvt_compact_keep_terms."""
    _fields_ = [("col", C.c_int32), ("op", C.c_int32), ("conj", C.c_int32), ("set_len", C.c_int32),
                ("set_off", _u64), ("value", FilterValue)]


COMPACT_MAX_COLS = 64   # include/nvt_hip.h NVT_COMPACT_MAX_COLS
FILTER_MAX_COLS, FILTER_MAX_TERMS = 16, 64   # NVT_FILTER_MAX_COLS, NVT_FILTER_MAX_TERMS
# NVT_FILTER_EQ .. NVT_FILTER_NOT_IN
FILTER_OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5, "in": 6, "not in": 7}
SIGNATURES.update({
    "nvt_compact_keep_terms": [C.POINTER(FilterCol), _i32, C.POINTER(FilterTerm), _i32, _vp, _u64, _u64, _vp, _u64,
                               _vp],
    "nvt_compact_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_compact_keep_mask": [_vp, _u64, _vp, _u64, _vp],
    "nvt_compact_keep_dropna": [C.POINTER(DropnaCol), _i32, _u64, _vp, _u64, _vp],
    "nvt_compact_list_keep": [_vp, _u64, _vp, _u64, _vp, _u64, _vp],
    "nvt_compact_plan": [_u64, _vp, _u64, _vp, _vp],
    "nvt_compact_many": [C.POINTER(CompactCol), _i32, _vp],
    "nvt_compact_list_offsets": [_vp, _u64, _vp, _vp, _u64, _vp, _vp],
})

class JoinKey(C.Structure):
    """nvt_join_key: one key component read by the join entries."""
    _fields_ = [("x", _vp), ("valid", _vp), ("dtype", C.c_int32), ("mode", C.c_int32)]


class JoinIndex(C.Structure):
    """nvt_join_index: the hash index of an external table."""
    _fields_ = [("slots", _vp), ("capacity", _u64), ("empty", _u64), ("words", _vp), ("nulls", _vp),
                ("n_ext", _u64), ("null_first", _u64), ("null_count", _u64), ("nkeys", C.c_int32),
                ("reserved", C.c_int32)]


class JoinCol(C.Structure):
    """nvt_join_col: one column moved by nvt_join_probe_gather / nvt_join_gather."""
    _fields_ = [("src", _vp), ("src_valid", _vp), ("dst", _vp), ("dst_valid", _vp), ("width", C.c_int32),
                ("reserved", C.c_int32)]


JOIN_MAX_KEYS, JOIN_MAX_COLS = 4, 16   # include/nvt_hip.h NVT_JOIN_MAX_*
JOIN_INT, JOIN_FLOAT = 0, 1
SIGNATURES.update({
    "nvt_join_table_bytes": [_u64, C.POINTER(_u64), C.POINTER(_u64)],
    "nvt_join_hash": [C.POINTER(JoinKey), _i32, _u64, _vp, _vp, _vp, _vp],
    "nvt_join_insert": [_vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
    "nvt_join_probe": [C.POINTER(JoinIndex), C.POINTER(JoinKey), _i32, _u64, _i32, _vp, _vp, _vp, _vp, _vp],
    "nvt_join_probe_gather": [C.POINTER(JoinIndex), C.POINTER(JoinKey), _i32, _u64, C.POINTER(JoinCol), _i32,
                              _vp, _vp],
    "nvt_join_scan_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_join_offsets": [_vp, _u64, _vp, _u64, _vp],
    "nvt_join_expand": [_vp, _vp, _u64, _u64, _vp, _vp, _vp],
    "nvt_join_gather": [_vp, _u64, C.POINTER(JoinCol), _i32, _vp],
})

class ListCol(C.Structure):
    """nvt_list_col: one column moved by nvt_list_slice_many."""
    _fields_ = [("src", _vp), ("dst", _vp), ("src_valid", _vp), ("dst_valid", _vp), ("pad_bits", _u64),
                ("width", C.c_int32), ("reserved", C.c_int32)]


class ListLenCol(C.Structure):
    """nvt_list_len_col: one offsets tensor reduced by nvt_list_len_minmax."""
    _fields_ = [("offsets", _vp), ("n", _u64), ("acc", _vp)]


class LagKey(C.Structure):
    """nvt_lag_key: one partition column of nvt_difference_lag_many."""
    _fields_ = [("x", _vp), ("valid", _vp), ("dtype", C.c_int32), ("reserved", C.c_int32)]


class LagCol(C.Structure):
    """nvt_lag_col: one (column, shift) output of nvt_difference_lag_many."""
    _fields_ = [("x", _vp), ("valid", _vp), ("out", _vp), ("shift", _i64), ("dtype", C.c_int32),
                ("reserved", C.c_int32)]


LIST_MAX_COLS, LAG_MAX_KEYS = 32, 4   # include/nvt_hip.h NVT_LIST_MAX_COLS / NVT_LAG_MAX_KEYS
SIGNATURES.update({
    "nvt_list_slice_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_list_slice_offsets": [_vp, _u64, _i64, _i64, _vp, _vp, _u64, _vp],
    "nvt_list_slice_many": [C.POINTER(ListCol), _i32, _vp, _u64, _i64, _i64, _vp, _u64, _u64, _vp],
    "nvt_list_len_minmax": [C.POINTER(ListLenCol), _i32, _vp],
    "nvt_difference_lag_many": [C.POINTER(LagKey), _i32, C.POINTER(LagCol), _i32, _u64, _vp],
})

class PqListCol(C.Structure):
    """nvt_pqlist_col: one definition-level stream written by nvt_pqlist_pack_many."""
    _fields_ = [("leaf_valid", _vp), ("bit0", _u64), ("nbits", _u64), ("def_out", _vp), ("nonnull", _vp)]


# include/nvt_hip.h NVT_PQLIST_MAX_COLS / NVT_PQLIST_HEADER_WORDS / NVT_PQLIST_PAGE_WORDS
PQLIST_MAX_COLS, PQLIST_HEADER_WORDS, PQLIST_PAGE_WORDS = 16, 8, 8
SIGNATURES.update({
    "nvt_pqlist_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_pqlist_plan": [_vp, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
    "nvt_pqlist_pack_many": [C.POINTER(PqListCol), _i32, _vp, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp],
    "nvt_pqlist_unpack_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_pqlist_unpack": [_vp, _vp, _i32, _u64, _i32, _i32, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
})

# include/nvt_hip.h NVT_PQ_DICT_MAX_ENTRIES / NVT_PQ_DICT_STATE_WORDS
PQ_DICT_MAX_ENTRIES, PQ_DICT_STATE_WORDS = 1 << 20, 4
SIGNATURES.update({
    "nvt_pq_dict_ws_bytes": [_u64, _u64, _u64, C.POINTER(_u64)],
    "nvt_pq_dict_build": [_vp, _i32, _u64, _u64, _vp, _vp, _vp, _u64, _vp],
    "nvt_pq_dict_pack": [_vp, _i32, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp],
})
# parquet out: string columns (kernels_parquet_str_out.py)
SIGNATURES.update({
    "nvt_pq_str_entry_ids": [_vp, _u64, _vp, _u64, _vp, _vp, _vp],
    "nvt_pq_byte_array_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_pq_byte_array_plan": [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp],
    "nvt_pq_byte_array_fill": [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp],
})

class SnappyCol(C.Structure):
    """nvt_snappy_col: the values region of one column chunk compressed by nvt_snappy_*_many."""
    _fields_ = [("src", _vp), ("page_start", _vp), ("npages", _u64), ("nbytes", _u64), ("unit", _u32),
                ("elem", _u32), ("frag_base", _u64), ("max_frags", _u64), ("dense", _vp), ("dense_cap", _u64),
                ("out", _vp)]


class SnappyBatch(C.Structure):
    """nvt_snappy_batch: the fragment arrays, slots and scan workspace the descriptors of a call share."""
    _fields_ = [("frag_table", _vp), ("frag_size", _vp), ("frag_pos", _vp), ("slots", _vp),
                ("total_frags", _u64), ("slot_cap", _u64), ("ws", _vp), ("ws_bytes", _u64)]


# include/nvt_hip.h NVT_SNAPPY_*
SNAPPY_FRAG, SNAPPY_MAX_COLS, SNAPPY_FRAG_WORDS, SNAPPY_OUT_WORDS = 32768, 16, 4, 4
SNAPPY_SLOT_BYTES = SNAPPY_FRAG + SNAPPY_FRAG // 32 + 16
SNAPPY_OUT_TOTAL, SNAPPY_OUT_ERROR, SNAPPY_OUT_FRAGS = 0, 1, 2
SNAPPY_ERR_PLAN, SNAPPY_ERR_SLOT = 1, 2
SIGNATURES.update({
    "nvt_snappy_slot_bytes": [C.POINTER(_u64)],
    "nvt_snappy_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_snappy_plan_many": [C.POINTER(SnappyCol), _i32, C.POINTER(SnappyBatch), _vp],
    "nvt_snappy_compress_many": [C.POINTER(SnappyCol), _i32, C.POINTER(SnappyBatch), _vp],
    "nvt_snappy_gather_many": [C.POINTER(SnappyCol), _i32, C.POINTER(SnappyBatch), _vp],
})


class SelectCol(C.Structure):
    """nvt_select_col: one chunk of one column read by nvt_select_hist_many."""
    _fields_ = [("x", _vp), ("valid", _vp), ("n", _u64), ("dtype", C.c_int32), ("has_fill", C.c_int32),
                ("fill_val", _dbl)]


# include/nvt_hip.h NVT_SELECT_*
SELECT_MAX_COLS, SELECT_BINS, SELECT_CAND_CAP = 32, 2048, 65536
(SELECT_ST_M, SELECT_ST_RANK_LO, SELECT_ST_RANK_HI, SELECT_ST_KEY_LO, SELECT_ST_KEY_HI, SELECT_ST_DONE,
 SELECT_ST_NCAND, SELECT_ST_USE_CAND, SELECT_ST_PATH, SELECT_ST_BITS, SELECT_ST_ALLOW_CAND) = range(11)
SELECT_ST_HIST = 16
SELECT_ST_CAND = SELECT_ST_HIST + 2 * SELECT_BINS
SELECT_STATE_WORDS = SELECT_ST_CAND + SELECT_CAND_CAP
SELECT_PATH_CAND, SELECT_PATH_FULL = 1, 2
SIGNATURES.update({
    "nvt_select_hist_many": [C.POINTER(SelectCol), _i32, _i32, _vp, _vp],
    "nvt_select_step": [_vp, _i32, _i32, _vp],
    "nvt_select_finish": [_vp, _i32, _vp],
})

class ProfileCol(C.Structure):
    """nvt_profile_col: one column read by nvt_col_profile_many."""
    _fields_ = [("x", _vp), ("valid", _vp), ("n", _u64), ("dtype", C.c_int32), ("reserved", C.c_int32),
                ("counts", _vp), ("extrema", _vp), ("sums", _vp)]


class CastCol(C.Structure):
    """nvt_cast_col: one column converted by nvt_cast_many."""
    _fields_ = [("src", _vp), ("dst", _vp), ("n", _u64), ("src_dtype", C.c_int32), ("dst_dtype", C.c_int32)]


# include/nvt_hip.h NVT_PROFILE_*
PROFILE_MAX_COLS, PROFILE_SCRATCH_BYTES = 32, 32 * 5 * 1024 * 8
SIGNATURES.update({
    "nvt_col_profile_many": [C.POINTER(ProfileCol), _i32, _vp, _vp],
    "nvt_cast_many": [C.POINTER(CastCol), _i32, _vp],
})

class PqWidenCol(C.Structure):
    """nvt_pq_widen_col: one int8 / int16 source sign-extended to int32 by nvt_pq_widen_i32_many."""
    _fields_ = [("src", _vp), ("dst", _vp), ("n", _u64), ("src_dtype", C.c_int32), ("reserved", C.c_int32)]


# parquet, flat int8 / int16 / bool columns (include/nvt_hip.h)
SIGNATURES.update({
    "nvt_pq_decode_bool_chunk": [_vp, _u64, _i32, _i32, _u64, _vp, _u64, _vp, _u64, _vp, _u64,
                                 C.POINTER(_u64), C.POINTER(_u64)],
    "nvt_expand_narrow": [_vp, _i32, _i32, _vp, _u64, _vp, _vp, _vp],
    "nvt_pq_widen_i32_many": [C.POINTER(PqWidenCol), _i32, _vp],
    "nvt_pq_bool_pack": [_vp, _vp, _vp, _u64, _vp, _vp],
})


class PartitionSeg(C.Structure):
    """nvt_partition_seg: one segment of an output partition (a DEVICE array of these is passed)."""
    _fields_ = [("idx", _vp), ("start", _u64)]


class PartitionCol(C.Structure):
    """nvt_partition_col: one column moved by nvt_partition_gather_many."""
    _fields_ = [("src", _vp), ("src_valid", _vp), ("dst", _vp), ("dst_valid", _vp), ("width", C.c_int32),
                ("reserved", C.c_int32)]


# include/nvt_hip.h NVT_PARTITION_*
PARTITION_MAX, PARTITION_MAX_COLS, PARTITION_MAX_SEGS = 4096, 16, 1024
SIGNATURES.update({
    "nvt_partition_tile_rows": [],
    "nvt_partition_ids": [_vp, _u64, _u32, _vp, _vp],
    "nvt_partition_plan_ws_bytes": [_u64, _u32, C.POINTER(_u64)],
    "nvt_partition_plan": [_vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp],
    "nvt_partition_gather_many": [C.POINTER(PartitionCol), _i32, _vp, _i32, _u64, _vp],
})

# include/nvt_hip.h NVT_LABEL_MAX
LABEL_MAX = 4096
SIGNATURES.update({
    "nvt_key_labels_tile_rows": [],
    "nvt_key_labels_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_key_labels": [_vp, _vp, _vp, _i32, _u64, _vp, _vp, _vp, _vp, _u64, _vp],
})

class TakeCol(C.Structure):
    """nvt_take_col: one column gathered by nvt_batch_take_many / nvt_take_list_many."""
    _fields_ = [("src", _vp), ("src_valid", _vp), ("dst", _vp), ("dst_valid", _vp), ("dst_stride", _i64),
                ("src_dtype", C.c_int32), ("dst_dtype", C.c_int32)]


# include/nvt_hip.h NVT_TAKE_*
TAKE_MAX_COLS, TAKE_MAX_GROUPS, TAKE_STAGE_ROW_BYTES = 64, 4, 256
SIGNATURES.update({
    "nvt_batch_take_many": [_vp, _u64, _u64, C.POINTER(TakeCol), _i32, _vp],
    "nvt_take_list_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_take_list_offsets": [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp],
    "nvt_take_list_many": [C.POINTER(TakeCol), _i32, _vp, _vp, _vp, _u64, _u64, _vp],
})
# the multi-source forms: TakeCol.src points at the column's row of the device source table, records
# of three int64 words {src, src_valid, src_dtype} (nvt_take_src), one per source
TAKE_MAX_SOURCES, TAKE_SRC_WORDS = 4096, 3
SIGNATURES.update({
    "nvt_batch_take_multi": [_vp, _u64, _vp, _i32, _u64, C.POINTER(TakeCol), _i32, _vp],
    "nvt_take_list_offsets_multi": [_vp, _vp, _i32, _u64, _vp, _u64, _vp, _vp, _u64, _vp],
    "nvt_take_list_multi": [C.POINTER(TakeCol), _i32, _vp, _vp, _i32, _vp, _vp, _u64, _u64, _vp],
})

class CsvCol(C.Structure):
    """nvt_csv_col: one numeric column parsed by nvt_csv_parse_many."""
    _fields_ = [("out", _vp), ("out_valid", _vp), ("slow", _vp), ("k", _u32), ("dtype", C.c_int32)]


# include/nvt_hip.h NVT_CSV_*
CSV_TILE, CSV_SCAN_STEP, CSV_MAX_COLS, CSV_STATE_WORDS = 4096, 256, 64, 8
(CSV_ST_FIELDS, CSV_ST_ROWS, CSV_ST_PARITY, CSV_ST_BAD_ROW, CSV_ST_QUOTE_ROW, CSV_ST_BAD_FIELD,
 CSV_ST_SLOW) = range(7)
CSV_OK, CSV_DECLINED, CSV_INVALID, CSV_OVERFLOW = 0, 1, 2, 3
SIGNATURES.update({
    "nvt_csv_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_csv_count": [_vp, _u64, _i32, _i32, _vp, _u64, _vp, _vp],
    "nvt_csv_index": [_vp, _u64, _i32, _i32, _u32, _vp, _u64, _vp, _u64, _vp, _vp],
    "nvt_csv_parse_many": [_vp, _u64, _vp, _u64, _u32, _i32, C.POINTER(CsvCol), _i32, _vp, _vp],
    "nvt_csv_str_ws_bytes": [_u64, C.POINTER(_u64)],
    "nvt_csv_str_offsets": [_vp, _u64, _vp, _u64, _u32, _u32, _i32, _vp, _vp, _vp, _u64, _vp, _vp],
    "nvt_csv_str_copy": [_vp, _u64, _vp, _u64, _u32, _u32, _i32, _vp, _vp, _u64, _vp],
    "nvt_csv_parse_f64_host": [C.c_char_p, _i32, C.POINTER(_dbl)],
    "nvt_csv_parse_i64_host": [C.c_char_p, _i32, C.POINTER(_i64)],
})

# include/nvt_hip.h NVT_DT_*
DT_S, DT_MS, DT_US, DT_NS = range(4)
(DT_YEAR, DT_MONTH, DT_DAY, DT_HOUR, DT_MINUTE, DT_SECOND, DT_WEEKDAY, DT_DAYOFYEAR, DT_QUARTER) = range(9)
SIGNATURES.update({
    "nvt_dt_field": [_vp, _vp, _u64, _i32, _i32, _vp, _vp],
    "nvt_dt_fields_host": [_vp, _u64, _i32, _i32, _vp],
    "nvt_csv_parse_datetime": [_vp, _u64, _vp, _u64, _u32, _i32, C.POINTER(CsvCol), _i32, _vp, _vp],
    "nvt_csv_parse_datetime_host": [C.c_char_p, _i32, C.POINTER(_i64)],
})

_RESTYPES = {
    "nvt_last_error": C.c_char_p,
    "nvt_moments_scratch_bytes": C.c_uint64,
    "nvt_gb_destroy": None,
    "nvt_range_push": None,
    "nvt_range_pop": None,
    "nvt_event_destroy": None,
    "nvt_mailbox_destroy": None,
    "nvt_mailbox_data": C.c_void_p,
    "nvt_gb_state_ptr": C.c_void_p,
    "nvt_mailbox_capacity": C.c_uint64,
}

_lock = threading.Lock()
_lib = None


class NvtHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load libnvt_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NvtHipError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "nvtabular_amd/csrc`). There is no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, C.c_int)
        _lib = lib
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().nvt_last_error()
        raise NvtHipError(f"{what or 'nvt call'} failed ({rc}): {msg.decode() if msg else ''}")


def require_gpu():
    import torch

    if not torch.cuda.is_available():
        raise NvtHipError(
            "no MI355X visible (torch.cuda.is_available() is False); the NVTabular hot path "
            "has no CPU fallback in this engine"
        )


def ptr_array(ptrs):
    """Host array of device pointers (void*[n]); None -> NULL."""
    arr = (C.c_void_p * max(len(ptrs), 1))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr
