"""ctypes binding of the C ABI in include/cudf_amd/gx.h.

The product path REQUIRES the HIP library: importing this module raises if
cudf_amd/libcudf_amd.so is missing (build it with ``python scripts/build_ext.py``); there is no CPU
fallback anywhere in the package.
"""
import ctypes
import os

# PyTorch's HIP runtime must be in the process BEFORE libcudf_amd.so is loaded: the kernels are handed
# torch's device pointers and streams, so both have to bind to the same libamdhip64 instance (loading the
# library first pulls in /opt/rocm's copy, torch then brings its own, and launches fail with hipErrorNoDevice).
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcudf_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the HIP extension is mandatory (no CPU fallback). "
        "Run `python scripts/build_ext.py` (needs hipcc).")

lib = ctypes.CDLL(LIB_PATH)

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_i = ctypes.c_int
_sz = ctypes.POINTER(ctypes.c_size_t)

# dtype codes (== cudf::type_id)
INT8, INT16, INT32, INT64, UINT8, UINT16, UINT32, UINT64, FLOAT32, FLOAT64, BOOL8 = range(1, 12)
OP_SUM, OP_PRODUCT, OP_MIN, OP_MAX, OP_COUNT_VALID, OP_COUNT_ALL = 0, 1, 2, 3, 4, 5
OP_MEAN = 10
CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(6)
KEEP_ANY, KEEP_FIRST, KEEP_LAST, KEEP_NONE = range(4)
# gx_binop (== cudf::binary_operator) and gx_unop (== cudf::unary_operator, IS_NAN / IS_NOT_NAN beside it)
BINOPS = ("ADD", "SUB", "MUL", "DIV", "TRUE_DIV", "FLOOR_DIV", "MOD", "PMOD", "PYMOD", "POW", "INT_POW", "LOG_BASE", "ATAN2",
          "SHIFT_LEFT", "SHIFT_RIGHT", "SHIFT_RIGHT_UNSIGNED", "BITWISE_AND", "BITWISE_OR", "BITWISE_XOR", "LOGICAL_AND", "LOGICAL_OR",
          "EQUAL", "NOT_EQUAL", "LESS", "GREATER", "LESS_EQUAL", "GREATER_EQUAL", "NULL_EQUALS", "NULL_NOT_EQUALS", "NULL_MAX",
          "NULL_MIN", "GENERIC_BINARY", "NULL_LOGICAL_AND", "NULL_LOGICAL_OR")
BINOP = {name: code for code, name in enumerate(BINOPS)}
UNOPS = ("SIN", "COS", "TAN", "ARCSIN", "ARCCOS", "ARCTAN", "SINH", "COSH", "TANH", "ARCSINH", "ARCCOSH", "ARCTANH", "EXP", "LOG",
         "SQRT", "CBRT", "CEIL", "FLOOR", "ABS", "RINT", "BIT_COUNT", "BIT_INVERT", "NOT", "NEGATE")
UNOP = {name: code for code, name in enumerate(UNOPS)}
UNOP.update(IS_NAN=100, IS_NOT_NAN=101)
# gx_ast_op (== cudf::ast::ast_operator): the binary operators, then the unary ones from IDENTITY on
AST_OPS = ("ADD", "SUB", "MUL", "DIV", "TRUE_DIV", "FLOOR_DIV", "MOD", "PYMOD", "POW", "EQUAL", "NULL_EQUAL", "NOT_EQUAL", "LESS",
           "GREATER", "LESS_EQUAL", "GREATER_EQUAL", "BITWISE_AND", "BITWISE_OR", "BITWISE_XOR", "LOGICAL_AND", "NULL_LOGICAL_AND",
           "LOGICAL_OR", "NULL_LOGICAL_OR", "IDENTITY", "IS_NULL", "SIN", "COS", "TAN", "ARCSIN", "ARCCOS", "ARCTAN", "SINH", "COSH",
           "TANH", "ARCSINH", "ARCCOSH", "ARCTANH", "EXP", "LOG", "SQRT", "CBRT", "CEIL", "FLOOR", "ABS", "RINT", "BIT_INVERT", "NOT",
           "CAST_TO_INT64", "CAST_TO_UINT64", "CAST_TO_FLOAT64")
AST_OP = {name: code for code, name in enumerate(AST_OPS)}
AST_FIRST_UNARY = AST_OP["IDENTITY"]
EXPR_COLUMN, EXPR_LITERAL, EXPR_UNARY, EXPR_BINARY = range(4)                                  # gx_expr_node_kind
EXPR_LOAD, EXPR_APPLY, EXPR_APPLY_REV, EXPR_APPLY_UNARY, EXPR_SPILL = range(5)                  # gx_expr_instr_kind
EXPR_SRC_COLUMN, EXPR_SRC_LITERAL, EXPR_SRC_SLOT = range(3)                                    # gx_expr_src_kind


class ExprNode(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("op", ctypes.c_int32), ("lhs", ctypes.c_int32), ("rhs", ctypes.c_int32)]


class ExprColumn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("begin_bit", ctypes.c_int64), ("dtype", ctypes.c_int32),
                ("table", ctypes.c_int32)]


class ExprLiteral(ctypes.Structure):
    _fields_ = [("value", ctypes.c_void_p), ("valid", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class ExprInstr(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint8) for f in ("kind", "op", "src_kind", "src_index", "in_dtype", "out_dtype", "family", "family_op")]


_pi = ctypes.POINTER(ctypes.c_int)
_pi32 = ctypes.POINTER(ctypes.c_int32)

# gx_interp (== cudf::interpolation), gx_quantile_mode, gx_quantile_path
INTERP = {"linear": 0, "lower": 1, "higher": 2, "midpoint": 3, "nearest": 4}
QUANTILE_MODE = {"auto": 0, "select": 1, "sort": 2}
QUANTILE_PATH = {1: "select", 2: "select_direct", 3: "sort"}

_PROTOS = {
    "gx_version": (ctypes.c_char_p, []),
    "gx_dtype_size": (_i, [_i]),
    "gx_sort_keys": (_i, [_i, _p, _p, _i64, _i, _p, _sz, _p]),
    "gx_sort_pairs": (_i, [_i, _p, _p, _p, _p, _i64, _i, _p, _sz, _p]),
    "gx_sorted_order": (_i, [_i, _p, _p, _i64, _i64, _i, _i, _p, _p, _sz, _p]),
    "gx_sorted_order_table": (_i, [_i, _p, _p, _p, _i64, _p, _p, _sz, _p]),
    "gx_sort_status": (_i, [_p, ctypes.POINTER(_i), _p]),
    "gx_sort_status_async": (_i, [_p, _p, _p]),
    "gx_sort_set_fault_mode": (None, [_i]),
    "gx_sort_set_order_map": (None, [_i]),
    "gx_order_map_applies": (_i, [_i, _i64]),
    "gx_sort_order_map_info": (_i, [_p, _i64, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sort_set_algorithm": (None, [_i]),
    "gx_sort_profile": (_i, [_i]),
    "gx_sort_profile_slot": (_i, [_i]),
    "gx_sort_profile_read": (_i, [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_i)]),
    "gx_sort_profile_read_hybrid": (_i, [ctypes.POINTER(ctypes.c_float)]),
    "gx_sort_set_hybrid": (None, [_i]),
    "gx_sort_set_experiment": (None, [_i]),
    "gx_sort_set_cursor_path": (None, [_i, ctypes.c_float]),
    "gx_sort_set_counting": (None, [_i]),
    "gx_sort_set_splitters": (None, [_i]),
    "gx_sort_set_float_cursor": (None, [_i]),
    "gx_sort_set_spin_limit_ms": (None, [_i]),
    "gx_sort_inject_lost_tile": (None, [ctypes.c_longlong]),
    "gx_sort_split_info": (_i, [_p, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sort_cursor_state": (_i, [_p, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sort_place_info": (_i, [_p, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sort_set_place_grid": (None, [_i]),
    "gx_sort_set_order_words": (None, [_i]),
    "gx_sort_set_cell": (None, [_i]),
    "gx_sort_set_lookback": (None, [_i]),
    "gx_sort_info": (_i, [_p, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sort_big_info": (_i, [_p, ctypes.POINTER(ctypes.c_int64), _p]),
    # the sharded sort's halves (called from C++: cudf_amd/cpp/src/distributed.cpp; bound here for the ABI check and ad-hoc use)
    "gx_sortx_sample": (_i, [_i, _p, _i64, _i64, _p, _sz, _p]),
    "gx_sortx_masks": (_i, [_p, ctypes.POINTER(ctypes.c_uint64), _p]),
    "gx_sortx_level0": (_i, [_i, _p, _i64, _i64, ctypes.POINTER(ctypes.c_uint64), _p, _p]),
    "gx_sortx_tables": (_i, [_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                             ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_sortx_level0_buffer": (_p, [_i, _p, _i64, _i64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "gx_sortx_finish": (_i, [_i, _i64, _i64, _i64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                             ctypes.POINTER(ctypes.c_uint32), _i, _p, _p, _p]),
    "gx_sortx_status": (_i, [_p, ctypes.POINTER(ctypes.c_int32), _p]),
    "gx_gather": (_i, [_i, _p, _p, _i64, _p, _i64, _i, _p, _p, _p]),
    "gx_gather_global_rows": (_i, [_p, _i64, _p, _i64, _i, _p, _p, _p, _p]),
    "gx_gather_global_rows_dev": (_i, [_p, _i64, _p, _i64, _i, _p, _p, _p]),
    "gx_widen_i32_i64": (_i, [_p, _i64, _p, _p]),
    "gx_decode_global_rows": (_i, [_p, _i64, _i, _p, _p, _p, _i, _p, _p]),
    "gx_join_build_pl": (_i, [_i, _p, _p, _p, _i64, _p, ctypes.c_size_t, ctypes.c_double, _p]),
    "gx_join_build_partitioned_pl": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, ctypes.c_double, _p, _sz, _p]),
    "gx_join_probe_partitioned_pl": (_i, [_i, _p, _p, _i64, ctypes.c_int32, _p, ctypes.c_size_t, _i, _p, _p, _i64, _p, _p, _sz, _p]),
    "gx_bitmask_set": (_i, [_p, _i64, _i64, _i, _p]),
    "gx_bitmask_count": (_i, [_p, _i64, _i64, _p, _p]),
    "gx_bitmask_and": (_i, [ctypes.POINTER(_p), _i, _i64, _p, _p, _p]),
    "gx_bitmask_first_unset": (_i, [_p, _i64, _p, _p]),
    "gx_murmur3_32": (_i, [_i, _p, _p, _i64, ctypes.c_uint32, _i, _p, _p]),
    "gx_identity_hash_32": (_i, [_i, _p, _p, _i64, _i, _p, _p]),
    "gx_hash_partition_map": (_i, [_p, _i64, _i, _p, _p, _p, _sz, _p]),
    "gx_join_table_bytes": (ctypes.c_size_t, [_i, _i64, ctypes.c_double]),
    "gx_join_build": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, ctypes.c_double, _p]),
    "gx_join_count": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, _p, _p]),
    "gx_join_probe": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, _i, _p, _p, _i64, _p, _p]),
    "gx_groupby_sum_count": (_i, [_i, _p, _p, _i, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "gx_groupby_sum_count_wide": (_i, [_i, ctypes.POINTER(_p), _i, _p, _i64, _i64, ctypes.POINTER(_p), _p, _p, _p, _p, _sz, _p]),
    "gx_groupby_min_max": (_i, [_i, _p, _p, _i, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "gx_valid_from_counts": (_i, [_p, _i64, _p, _p, _p]),
    "gx_mean_from_sum": (_i, [_i, _p, _p, _i64, _p, _p]),
    "gx_join_probe_partitioned": (_i, [_i, _p, _i64, _p, ctypes.c_size_t, _i, _p, _p, _i64, _p, _p, _sz, _p]),
    "gx_join_probe_partitioned_at": (_i, [_i, _p, _i64, ctypes.c_int32, _p, ctypes.c_size_t, _i, _p, _p, _i64, _p, _p, _sz, _p]),
    "gx_join_build_partitioned": (_i, [_i, _p, _i64, _p, ctypes.c_size_t, ctypes.c_double, _p, _sz, _p]),
    "gx_partition_rows": (_i, [_i, _p, _i64, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "gx_partition_rows_at": (_i, [_i, _p, _i64, ctypes.c_int32, _i, _i, _p, _p, _p, _p, _p, _sz, _p]),
    "gx_partition_rows_spec_at": (_i, [_i, _p, _i64, ctypes.c_int32, _i, _i, _p, _i64, _p, _p, _p, _p, _sz, _p]),
    "gx_join_count_rows": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, ctypes.c_int32, _p, _p]),
    "gx_add_i32": (_i, [_p, _i64, ctypes.c_int32, _p]),
    "gx_join_partition_bits": (_i, [_i, ctypes.c_size_t]),
    "gx_join_profile": (_i, [_i]),
    "gx_join_profile_slot": (_i, [_i]),
    "gx_join_profile_read": (_i, [ctypes.POINTER(ctypes.c_float)]),
    "gx_join_set_scatter_tile": (None, [_i]),
    "gx_join_set_experiment": (None, [_i]),
    "gx_join_set_overflow_slice": (None, [_i]),
    "gx_join_set_build_kernel": (None, [_i]),
    "gx_join_set_probe_kernel": (None, [_i]),
    "gx_join_set_partition_mode": (None, [_i, _i]),
    "gx_bitmask_copy": (_i, [_p, _i64, _p, _i64, _i64, _p]),
    "gx_pack_keys": (_i, [_i, _p, _p, _i64, _p, _p]),
    "gx_unpack_keys": (_i, [_i, _p, _p, _i64, _p, _p]),
    "gx_hash_rows64": (_i, [_i, _p, _p, _i64, ctypes.c_uint64, _p, _p]),
    "gx_rows_mismatch_count": (_i, [_i, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "gx_dense_rank": (_i, [_i, _p, _p, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "gx_square": (_i, [_i, _p, _i64, _p, _p]),
    "gx_square_centered": (_i, [_p, _p, _p, _i64, _i64, _p, _p]),
    "gx_var_from_sums": (_i, [_i, _p, _p, _p, _i64, _i, _i, _p, _p, _p, _p]),
    "gx_groupby_arg_select": (_i, [_i, _p, _p, _p, _i64, _p, _i64, _p, _p]),
    "gx_fill_nulls": (_i, [_i, _p, _p, _i64, ctypes.c_uint64, _p]),
    "gx_join_lookup": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, _p, _p]),
    "gx_join_filter": (_i, [_i, _p, _p, _i64, _p, ctypes.c_size_t, _i, _i, _p, _p, _p, _sz, _p]),
    "gx_join_complement": (_i, [_p, _i64, _i64, _p, _p, _i64, _p, _p, _sz, _p]),
    "gx_groupby_set_algorithm": (None, [_i, _i]),
    "gx_groupby_set_dense": (None, [_i]),
    "gx_groupby_plan_info": (_i, [_p, _i64, _p, _p]),
    "gx_groupby_set_partition_mode": (None, [_i]),
    "gx_groupby_set_partition_bits": (_i, [_i]),
    "gx_group_heads": (_i, [_i, _p, _p, _p, _i64, _i, _p, _p]),
    "gx_group_offsets": (_i, [_p, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "gx_segmented_reduce": (_i, [_i, _p, _p, _p, _p, _i64, _i, _p, _p, _p, _sz, _p]),
    "gx_segmented_shift": (_i, [_i, _p, _p, _p, _i64, _i64, ctypes.c_uint64, _i, _p, _p, _p]),
    "gx_segmented_fill_nulls": (_i, [_i, _p, _p, _p, _i64, _i, _p, _p, _p, _sz, _p]),
    "gx_rank_from_groups": (_i, [_p, _p, _p, _i64, _i, ctypes.c_double, _i, _p, _p, _p]),
    "gx_segment_ids": (_i, [_p, _i64, _i64, _p, _p]),
    "gx_segmented_scan": (_i, [_i, _p, _i, _p, _p, _i64, _i, _p, _p, _sz, _p]),
    "gx_reduce": (_i, [_i, _p, _p, _i64, _i, _i, _p, _p, _p, _sz, _p]),
    "gx_scan": (_i, [_i, _p, _p, _i64, _i, _i, _p, _p, _sz, _p]),
    "gx_fill_random": (_i, [_i, _p, _i64, ctypes.c_uint64, _i64, _i64, _p]),
    "gx_mix64_inplace": (_i, [_p, _i64, _p]),
    "gx_sequence_i32": (_i, [_p, _i64, ctypes.c_int32, _p]),
    "gx_copy_bytes": (_i, [_p, _p, ctypes.c_size_t, _p]),
    "gx_checksum": (_i, [_i, _p, _i64, _i, _p, _p]),
    # row filtering (gx_compact.hip): selectors write the plan, the per-column calls read it
    "gx_compact_plan_bytes": (ctypes.c_size_t, [_i64]),
    "gx_select_mask": (_i, [_p, _p, _i64, _i64, _p, _p, _sz, _p]),
    "gx_select_valid_count": (_i, [_i, ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, _i, _p, _p, _sz, _p]),
    "gx_select_not_nan": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, _i, _i, _p, _p, _sz, _p]),
    "gx_compact_column": (_i, [_i, _p, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    "gx_compact_indices": (_i, [_i64, _p, _p, _p]),
    "gx_compare_scalar": (_i, [_i, _p, _p, _i64, _i, ctypes.c_uint64, _p, _p]),
    "gx_select_set_stages": (None, [_i]),
    "gx_compact_set_kernel": (None, [_i]),
    # deduplicating selectors (gx_distinct.hip): the plan at the start of their scratch, the table behind it
    "gx_select_unique": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, _i, _i, _p, _p, _sz, _p]),
    "gx_select_distinct": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, _i, _i, _p, _p, _sz, _p]),
    "gx_distinct_set_hash_bits": (None, [_i]),
    # merging and searching sorted rows (gx_merge.hip): two sides of key columns, one order
    "gx_merge_tile_rows": (_i, []),
    "gx_merge_order": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64,
                            ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, ctypes.POINTER(_i), ctypes.POINTER(_i),
                            _p, _p, _sz, _p]),
    "gx_gather2": (_i, [_i, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _p]),
    "gx_search_bounds": (_i, [_i, ctypes.POINTER(_i), ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64,
                              ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, ctypes.POINTER(_i), ctypes.POINTER(_i),
                              _i, _p, _p]),
    # rolling windows (gx_rolling.hip): fixed or per-row windows, optional groups, no scratch
    "gx_rolling_tile_rows": (_i, []),
    "gx_rolling_max_span": (_i, []),
    "gx_rolling_window": (_i, [_i, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p]),
    "gx_rolling_set_kernel": (None, [_i]),
    # row movement (gx_copying.hip): fused concatenate (descriptors in scratch), scatter in place, copy_if_else
    "gx_concat_tile_rows": (_i, []),
    "gx_concatenate": (_i, [_i, _i, ctypes.POINTER(_p), ctypes.POINTER(_i64), ctypes.POINTER(_p), ctypes.POINTER(_i64), _p, _p, _p,
                            _p, _sz, _p]),
    "gx_scatter": (_i, [_i, _p, _p, _i64, _p, _i, _p, _i64, _p, _p, _i64, _p]),
    "gx_copy_if_else": (_i, [_i, _p, _p, _i64, _p, _i, _p, _p, _i64, _p, _i, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    # element-wise operations (gx_elementwise.hip): binary, unary, cast, bitmap -> BOOL8; the _supported tables are host code
    "gx_binary_op": (_i, [_i, _i, _p, _p, _i64, _p, _i, _i, _p, _p, _i64, _p, _i, _i64, _i, _p, _p, _p, _p]),
    "gx_unary_op": (_i, [_i, _i, _p, _i64, _i, _p, _p]),
    "gx_cast": (_i, [_i, _p, _i64, _i, _p, _p]),
    "gx_bitmask_to_bool8": (_i, [_p, _i64, _i64, _i, _p, _p]),
    "gx_binary_op_supported": (_i, [_i, _i, _i, _i]),
    "gx_unary_op_supported": (_i, [_i, _i, _i]),
    "gx_elementwise_tile_rows": (_i, []),
    "gx_elementwise_grid_cap": (_i, []),
    # expressions (gx_expression.hip): one launch per expression tree; types, plan and limits are host code
    "gx_compute_column": (_i, [ctypes.POINTER(ExprNode), _i, ctypes.POINTER(ExprColumn), _i, ctypes.POINTER(ExprLiteral), _i, _i64, _i, _p,
                               _p, _p, _p]),
    "gx_expr_result_dtype": (_i, [ctypes.POINTER(ExprNode), _i, _pi32, _i, _pi32, _i]),
    "gx_expr_plan": (_i, [ctypes.POINTER(ExprNode), _i, _pi32, _i, _pi32, _i, ctypes.POINTER(ExprInstr), _i, _pi, _pi]),
    "gx_expr_limits": (None, [_pi, _pi, _pi, _pi]),
    "gx_expression_tile_rows": (_i, []),
    "gx_expression_grid_cap": (_i, []),
    # conditional joins (gx_conditional_join.hip): the same program over row pairs; count (scratch) then write
    "gx_conditional_join_count": (_i, [ctypes.POINTER(ExprNode), _i, ctypes.POINTER(ExprColumn), _i, ctypes.POINTER(ExprLiteral), _i, _i64,
                                       _i64, _i, _p, _p, _sz, _p]),
    "gx_conditional_join_write": (_i, [ctypes.POINTER(ExprNode), _i, ctypes.POINTER(ExprColumn), _i, ctypes.POINTER(ExprLiteral), _i, _i64,
                                       _i64, _i, _i64, _i64, _p, _p, _p, _p]),
    "gx_conditional_join_tile": (None, [_pi, _pi]),
    "gx_conditional_join_grid_cap": (_i, []),
    "gx_conditional_join_pairs_per_run": (_i, []),
    "gx_conditional_join_set_shape": (_i, [_i, _i, _i]),
    # null and value replacement (gx_replace.hip): streaming passes; only the policy fill has scratch (its carry table)
    "gx_replace_tile_rows": (_i, []),
    "gx_find_and_replace_chunk": (_i, []),
    "gx_replace_nulls": (_i, [_i, _p, _p, _i64, _p, _p, _i64, _p, _i, _i64, _p, _p, _p, _p]),
    "gx_replace_nulls_policy": (_i, [_i, _p, _p, _i64, _i64, _i, _p, _p, _p, _p, _sz, _p]),
    "gx_replace_nans": (_i, [_i, _p, _p, _i64, _p, _p, _i64, _p, _i, _i64, _p, _p, _p, _p]),
    "gx_clamp": (_i, [_i, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p]),
    "gx_find_and_replace": (_i, [_i, _p, _p, _i64, _i64, _p, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    "gx_normalize_nans_and_zeros": (_i, [_i, _p, _i64, _p, _p]),
    # making and reshaping columns (gx_reshape.hip): interleave (descriptors in scratch), tile, repeat, fill, sequence
    "gx_reshape_tile_rows": (_i, []),
    "gx_interleave_tile": (_i, [_i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "gx_interleave": (_i, [_i, _i, ctypes.POINTER(_p), ctypes.POINTER(_p), ctypes.POINTER(_i64), _i64, _p, _p, _p, _p, _sz, _p]),
    "gx_tile": (_i, [_i, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p]),
    "gx_repeat_each": (_i, [_i, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p]),
    "gx_repeat_map": (_i, [_p, _i64, _i64, _p, _p, _sz, _p]),
    "gx_fill_range": (_i, [_i, _p, _i64, _i64, _p, _p]),
    "gx_sequence": (_i, [_i, _p, _i64, _p, _p, _p]),
    # quantiles (gx_quantile.hip): select / sort paths for an unsorted column, the lookup kernel for known order
    "gx_quantile_tile_rows": (_i, []),
    "gx_quantile_index": (_i, [_i64, ctypes.c_double, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64),
                               ctypes.POINTER(ctypes.c_double)]),
    "gx_quantile": (_i, [_i, _p, _p, _i64, _i64, ctypes.POINTER(ctypes.c_double), _i, _i, _i, _p, _p, _p, ctypes.POINTER(_i), _p, _sz, _p]),
    "gx_quantile_status": (_i, [_p, ctypes.POINTER(_i), _p]),
    "gx_quantile_lookup": (_i, [_i, _p, _p, _i64, _p, _i64, _p, _p, ctypes.POINTER(ctypes.c_double), _i, _i, _i, _p, _p, _p, _p]),
    "gx_quantile_set_thresholds": (None, [_i64, ctypes.c_double]),
    "gx_quantile_get_thresholds": (None, [ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_double)]),
}

for _name, (_res, _args) in _PROTOS.items():
    _f = getattr(lib, _name)  # AttributeError here == the library does not export the ABI
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = tuple(_PROTOS)


class GxError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        raise GxError(f"{what} failed with code {rc}" + (" (hipError)" if rc > 0 else ""))
