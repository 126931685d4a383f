"""CPU: the scratch sizes and return codes of every entry point that takes `size_t* tmp_bytes`, the sort's and the hash groupby's
aside (tests/test_sort_scratch_host.py and tests/test_groupby_scratch_host.py pin those).

`*tmp_bytes` is part of each entry point's contract: callers size and reuse their scratch by it.  The size query (tmp == NULL) is
host arithmetic -- argument checks, the dtype dispatch, a carve of the layout -- and returns before the first HIP call, so it runs
without a GPU.  What it returns, and in which order the checks answer (GX_EINVAL before GX_EDTYPE or the other way round), is what
a change of the host-side dispatch or of the scratch convention has to reproduce.

Grid: every query in QUERIES x all eleven dtypes and one unknown dtype (99) x the row counts in ROWS, whose last is -1.  An entry
point that takes an element size gets the dtype's size (the unknown dtype: 3), one that takes a key size the same, one that takes
neither is asked once (dtype "-").  Entry points with an operator or a mode are asked once per value that reaches another layout.
Data pointers are dummy non-null pointers: a query tests them against NULL and never reads them.  Arrays the host reads (dtypes,
column pointers, bit offsets, row counts, quantiles) are real.

No entry point is left out: none of these queries makes a HIP call before it returns (one that did would answer a positive code, a
hipError_t, on a machine without a device; test_no_query_needs_a_device says so of the table).

The pairs (return code, *tmp_bytes) are literals, printed by `python tests/test_scratch_query_host.py` (it prints EXPECT in the
form it is stored in) from the build of the commit BEFORE the dtype table (csrc/gx_dtype.hpp) and Carver::ready replaced the
per-entry-point switches and scratch blocks: that refactor had to reproduce them, and so has every later change that does not mean
to change the ABI.  *tmp_bytes starts at SENTINEL, so a call that does not store a size shows as (code, SENTINEL).  Dtypes whose
rows are equal share a row."""
import ctypes

import pytest

ROWS = (0, 1, 1000, 2**22, 10**9, 2**31 - 1, -1)
DTYPES = ("INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "FLOAT32", "FLOAT64", "BOOL8", "UNKNOWN")
CODE = {"INT8": 1, "INT16": 2, "INT32": 3, "INT64": 4, "UINT8": 5, "UINT16": 6, "UINT32": 7, "UINT64": 8, "FLOAT32": 9, "FLOAT64": 10,
        "BOOL8": 11, "UNKNOWN": 99}
SIZE = {"INT8": 1, "INT16": 2, "INT32": 4, "INT64": 8, "UINT8": 1, "UINT16": 2, "UINT32": 4, "UINT64": 8, "FLOAT32": 4, "FLOAT64": 8,
        "BOOL8": 1, "UNKNOWN": 3}
SENTINEL = 12345
DUMMY = ctypes.c_void_p(1 << 20)  # tested against NULL, never dereferenced by a query
TABLE_BYTES = 1 << 24             # a join table of 16 MiB behind DUMMY
OP_SUM, OP_PRODUCT, OP_MIN, OP_MAX, OP_COUNT_VALID, OP_COUNT_ALL, OP_COUNT_NONZERO = 0, 1, 2, 3, 4, 5, 6

_I = ctypes.c_int
_I64 = ctypes.c_int64
_P = ctypes.c_void_p


def _arr(ctype, *values):
    return (ctype * len(values))(*values)


def _keys1(dt):
    """one key column: dtypes_host, cols_host, valid_ptrs_host, begin_bits_host"""
    return _arr(_I, CODE[dt]), _arr(_P, DUMMY.value), _arr(_P, DUMMY.value), _arr(_I64, 0)


def _select_unique(entry):
    def q(lib, dt, n, nb):
        d, c, v, b = _keys1(dt)
        return getattr(lib, entry)(1, d, c, v, b, n, 1, 0, DUMMY, None, nb, None)
    return q


def _merge_order(lib, dt, n, nb):
    d, c, v, b = _keys1(dt)
    return lib.gx_merge_order(1, d, c, v, b, n, c, v, b, min(max(n, 0), 1000), _arr(_I, 0), _arr(_I, 0), DUMMY, None, nb, None)


def _reduce(op):
    return lambda lib, dt, n, nb: lib.gx_reduce(CODE[dt], DUMMY, DUMMY, n, op, CODE["INT64"], DUMMY, DUMMY, None, nb, None)


def _scan(op):
    return lambda lib, dt, n, nb: lib.gx_scan(CODE[dt], DUMMY, DUMMY, n, op, 1, DUMMY, None, nb, None)


def _partition_rows(mode):
    return lambda lib, dt, n, nb: lib.gx_partition_rows(CODE[dt], DUMMY, n, mode, 8, DUMMY, DUMMY, DUMMY, DUMMY, None, nb, None)


# name -> (what the dtype selects: "dtype", "size" or "none"; the query)
QUERIES = {
    "sorted_order_table": ("dtype", lambda lib, dt, n, nb: lib.gx_sorted_order_table(
        1, _arr(_I, CODE[dt]), _arr(_P, DUMMY.value), _arr(_I, 0), n, DUMMY, None, nb, None)),
    "select_mask": ("none", lambda lib, dt, n, nb: lib.gx_select_mask(DUMMY, DUMMY, 0, n, DUMMY, None, nb, None)),
    "select_valid_count": ("none", lambda lib, dt, n, nb: lib.gx_select_valid_count(
        1, _arr(_P, DUMMY.value), _arr(_I64, 0), n, 1, DUMMY, None, nb, None)),
    "select_not_nan": ("dtype", lambda lib, dt, n, nb: lib.gx_select_not_nan(*((1,) + _keys1(dt) + (n, 1, 1, DUMMY, None, nb, None)))),
    "select_not_nan/floats_only": ("dtype", lambda lib, dt, n, nb: lib.gx_select_not_nan(
        *((1,) + _keys1(dt) + (n, 1, 0, DUMMY, None, nb, None)))),
    "select_unique": ("dtype", _select_unique("gx_select_unique")),
    "select_distinct": ("dtype", _select_unique("gx_select_distinct")),
    "merge_order": ("dtype", _merge_order),
    "concatenate": ("size", lambda lib, dt, n, nb: lib.gx_concatenate(
        SIZE[dt], 2, _arr(_P, DUMMY.value, DUMMY.value), _arr(_I64, n, min(max(n, 0), 1000)), _arr(_P, DUMMY.value, DUMMY.value),
        _arr(_I64, 0, 0), DUMMY, DUMMY, DUMMY, None, nb, None)),
    "replace_nulls_policy": ("size", lambda lib, dt, n, nb: lib.gx_replace_nulls_policy(
        SIZE[dt], DUMMY, DUMMY, 0, n, 0, DUMMY, DUMMY, DUMMY, None, nb, None)),
    "interleave": ("size", lambda lib, dt, n, nb: lib.gx_interleave(
        SIZE[dt], 2, _arr(_P, DUMMY.value, DUMMY.value), _arr(_P, DUMMY.value, DUMMY.value), _arr(_I64, 0, 0), n, DUMMY, DUMMY, DUMMY,
        None, nb, None)),
    "repeat_map": ("none", lambda lib, dt, n, nb: lib.gx_repeat_map(DUMMY, n, n, DUMMY, None, nb, None)),
    "quantile": ("dtype", lambda lib, dt, n, nb: lib.gx_quantile(
        CODE[dt], DUMMY, None, 0, n, _arr(ctypes.c_double, 0.5), 1, 0, 0, DUMMY, DUMMY, DUMMY, None, None, nb, None)),
    "quantile/nulls": ("dtype", lambda lib, dt, n, nb: lib.gx_quantile(
        CODE[dt], DUMMY, DUMMY, 0, n, _arr(ctypes.c_double, 0.5), 1, 0, 0, DUMMY, DUMMY, DUMMY, None, None, nb, None)),
    "hash_partition_map/8": ("none", lambda lib, dt, n, nb: lib.gx_hash_partition_map(DUMMY, n, 8, DUMMY, DUMMY, None, nb, None)),
    "hash_partition_map/1000": ("none", lambda lib, dt, n, nb: lib.gx_hash_partition_map(DUMMY, n, 1000, DUMMY, DUMMY, None, nb, None)),
    "hash_partition_map/100000": ("none", lambda lib, dt, n, nb: lib.gx_hash_partition_map(DUMMY, n, 100000, DUMMY, DUMMY, None, nb, None)),
    "dense_rank": ("dtype", lambda lib, dt, n, nb: lib.gx_dense_rank(CODE[dt], DUMMY, None, n, 0, DUMMY, DUMMY, DUMMY, None, nb, None)),
    "dense_rank/nulls": ("dtype", lambda lib, dt, n, nb: lib.gx_dense_rank(
        CODE[dt], DUMMY, DUMMY, n, min(max(n, 0), 5), DUMMY, DUMMY, DUMMY, None, nb, None)),
    "join_probe_partitioned": ("size", lambda lib, dt, n, nb: lib.gx_join_probe_partitioned(
        SIZE[dt], DUMMY, n, DUMMY, TABLE_BYTES, 0, DUMMY, DUMMY, n, DUMMY, None, nb, None)),
    "join_probe_partitioned_at": ("size", lambda lib, dt, n, nb: lib.gx_join_probe_partitioned_at(
        SIZE[dt], DUMMY, n, 7, DUMMY, TABLE_BYTES, 1, DUMMY, DUMMY, n, DUMMY, None, nb, None)),
    "join_probe_partitioned_pl": ("size", lambda lib, dt, n, nb: lib.gx_join_probe_partitioned_pl(
        SIZE[dt], DUMMY, DUMMY, n, 0, DUMMY, TABLE_BYTES, 0, DUMMY, DUMMY, n, DUMMY, None, nb, None)),
    "join_build_partitioned": ("size", lambda lib, dt, n, nb: lib.gx_join_build_partitioned(
        SIZE[dt], DUMMY, n, DUMMY, TABLE_BYTES, 0.5, None, nb, None)),
    "join_build_partitioned_pl": ("size", lambda lib, dt, n, nb: lib.gx_join_build_partitioned_pl(
        SIZE[dt], DUMMY, DUMMY, n, DUMMY, TABLE_BYTES, 0.5, None, nb, None)),
    "join_filter": ("size", lambda lib, dt, n, nb: lib.gx_join_filter(
        SIZE[dt], DUMMY, DUMMY, n, DUMMY, TABLE_BYTES, 0, 0, DUMMY, DUMMY, None, nb, None)),
    "join_complement": ("none", lambda lib, dt, n, nb: lib.gx_join_complement(DUMMY, n, max(n, 0), DUMMY, DUMMY, n, DUMMY, None, nb, None)),
    "partition_rows/hash": ("dtype", _partition_rows(0)),
    "partition_rows/range": ("dtype", _partition_rows(1)),
    "partition_rows_at": ("dtype", lambda lib, dt, n, nb: lib.gx_partition_rows_at(
        CODE[dt], DUMMY, n, 7, 0, 8, DUMMY, DUMMY, DUMMY, DUMMY, None, nb, None)),
    "partition_rows_spec_at": ("dtype", lambda lib, dt, n, nb: lib.gx_partition_rows_spec_at(
        CODE[dt], DUMMY, n, 7, 0, 8, DUMMY, 4096, DUMMY, DUMMY, DUMMY, None, nb, None)),
    "groupby_sum_count_wide": ("dtype", lambda lib, dt, n, nb: lib.gx_groupby_sum_count_wide(
        2, _arr(_P, DUMMY.value, DUMMY.value), CODE[dt], DUMMY, n, 1000, _arr(_P, DUMMY.value, DUMMY.value), DUMMY, DUMMY, DUMMY,
        None, nb, None)),
    "group_offsets": ("none", lambda lib, dt, n, nb: lib.gx_group_offsets(DUMMY, n, DUMMY, DUMMY, DUMMY, DUMMY, None, nb, None)),
    "segmented_reduce/SUM": ("dtype", lambda lib, dt, n, nb: lib.gx_segmented_reduce(
        CODE[dt], DUMMY, DUMMY, DUMMY, DUMMY, n, OP_SUM, DUMMY, DUMMY, None, nb, None)),
    "segmented_fill_nulls": ("size", lambda lib, dt, n, nb: lib.gx_segmented_fill_nulls(
        SIZE[dt], DUMMY, DUMMY, DUMMY, n, 0, DUMMY, DUMMY, None, nb, None)),
    "segmented_scan/SUM": ("dtype", lambda lib, dt, n, nb: lib.gx_segmented_scan(
        CODE["INT32"], DUMMY, CODE[dt], DUMMY, DUMMY, n, OP_SUM, DUMMY, None, nb, None)),
    "segmented_scan/keys": ("dtype", lambda lib, dt, n, nb: lib.gx_segmented_scan(
        CODE[dt], DUMMY, CODE["INT32"], DUMMY, DUMMY, n, OP_MIN, DUMMY, None, nb, None)),
    "reduce/SUM": ("dtype", _reduce(OP_SUM)),
    "reduce/PRODUCT": ("dtype", _reduce(OP_PRODUCT)),
    "reduce/MIN": ("dtype", _reduce(OP_MIN)),
    "reduce/MAX": ("dtype", _reduce(OP_MAX)),
    "reduce/COUNT_NONZERO": ("dtype", _reduce(OP_COUNT_NONZERO)),
    "reduce/unknown_op": ("dtype", _reduce(77)),
    "scan/SUM": ("dtype", _scan(OP_SUM)),
    "scan/PRODUCT": ("dtype", _scan(OP_PRODUCT)),
    "scan/MIN": ("dtype", _scan(OP_MIN)),
    "scan/MAX": ("dtype", _scan(OP_MAX)),
    "scan/unknown_op": ("dtype", _scan(77)),
}


def _grouped(rows_by_dtype):
    """{dtype: row} -> {(dtypes with that row, in DTYPES order): row}"""
    out = {}
    for dt, row in rows_by_dtype.items():
        key = next((k for k, r in out.items() if r == row), None)
        if key is None:
            out[(dt,)] = row
        else:
            out[key + (dt,)] = out.pop(key)
    return out


def answers(lib, name):
    """{dtype group: [(return code, *tmp_bytes) for n in ROWS]} of one query"""
    selects, query = QUERIES[name]
    rows = {}
    for dt in (DTYPES if selects != "none" else ("-",)):
        rows[dt] = []
        for n in ROWS:
            nb = ctypes.c_size_t(SENTINEL)
            rows[dt].append((query(lib, dt, n, ctypes.byref(nb)), nb.value))
    return _grouped(rows)


EXPECT = {
    'sorted_order_table': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8', 'UNKNOWN'): [(0, 256), (0, 1124608), (0, 1156352), (0, 175185152), (0, 43051313664), (0, 69257469184), (-1, 12345)],
    },
    'select_mask': {
        ('-',): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
    },
    'select_valid_count': {
        ('-',): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
    },
    'select_not_nan': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'select_not_nan/floats_only': {
        ('FLOAT32', 'FLOAT64'): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'select_unique': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'select_distinct': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 1024), (0, 1280), (0, 13056), (0, 51389184), (0, 12841888256), (0, 26310869760), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'merge_order': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 8704), (0, 1953536), (-1, 12345), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345), (-1, 12345)],
    },
    'concatenate': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 1024), (0, 1024), (0, 1024), (0, 1024), (0, 1024), (0, 1024), (0, 1024)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345)],
    },
    'replace_nulls_policy': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 0), (0, 512), (0, 512), (0, 4352), (0, 977664), (0, 2099200), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345)],
    },
    'interleave': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 768), (0, 768), (0, 768), (0, 768), (0, 768), (0, 768), (0, 768)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345)],
    },
    'repeat_map': {
        ('-',): [(0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0)],
    },
    'quantile': {
        ('INT8', 'UINT8'): [(0, 840192), (0, 842496), (0, 844800), (0, 14471168), (0, 3250841088), (0, 6980161536), (-1, 12345)],
        ('INT16', 'UINT16'): [(0, 840192), (0, 842496), (0, 847872), (0, 27054080), (0, 6250841088), (0, 13422612480), (-1, 12345)],
        ('INT32', 'UINT32'): [(0, 840192), (0, 842496), (0, 854016), (0, 52219904), (0, 17528540928), (0, 26307514368), (-1, 12345)],
        ('INT64', 'UINT64'): [(0, 840192), (0, 842496), (0, 866304), (0, 141348864), (0, 35051031808), (0, 52077318144), (-1, 12345)],
        ('FLOAT32',): [(0, 840448), (0, 842752), (0, 854272), (0, 52221952), (0, 17529029376), (0, 26308562944), (-1, 12345)],
        ('FLOAT64',): [(0, 840448), (0, 842752), (0, 866560), (0, 141350912), (0, 35051520256), (0, 52078366720), (-1, 12345)],
        ('BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345)],
    },
    'quantile/nulls': {
        ('INT8', 'UINT8'): [(0, 840704), (0, 843008), (0, 845312), (0, 15004160), (0, 3377794560), (0, 7252791808), (-1, 12345)],
        ('INT16', 'UINT16'): [(0, 840704), (0, 843008), (0, 848384), (0, 27587072), (0, 6377794560), (0, 13695242752), (-1, 12345)],
        ('INT32', 'UINT32'): [(0, 840704), (0, 843008), (0, 854528), (0, 52752896), (0, 17655494400), (0, 26580144640), (-1, 12345)],
        ('INT64', 'UINT64'): [(0, 840704), (0, 843008), (0, 866816), (0, 141881856), (0, 35177985280), (0, 52349948416), (-1, 12345)],
        ('FLOAT32',): [(0, 840960), (0, 843264), (0, 854784), (0, 52754944), (0, 17655982848), (0, 26581193216), (-1, 12345)],
        ('FLOAT64',): [(0, 840960), (0, 843264), (0, 867072), (0, 141883904), (0, 35178473728), (0, 52350996992), (-1, 12345)],
        ('BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345)],
    },
    'hash_partition_map/8': {
        ('-',): [(0, 826368), (0, 829696), (0, 836608), (0, 36060160), (0, 8400827392), (0, 18039690240), (-1, 12345)],
    },
    'hash_partition_map/1000': {
        ('-',): [(0, 826368), (0, 829696), (0, 840704), (0, 52837376), (0, 12400827392), (0, 26629624832), (-1, 12345)],
    },
    'hash_partition_map/100000': {
        ('-',): [(0, 826368), (0, 829696), (0, 848896), (0, 86391808), (0, 20400827392), (0, 43809494016), (-1, 12345)],
    },
    'dense_rank': {
        ('INT16', 'UINT16'): [(0, 826880), (0, 829696), (0, 844800), (0, 69615104), (0, 16400827904), (0, 35219559424), (-1, 12345)],
        ('INT64', 'UINT64'): [(0, 826880), (0, 829696), (0, 857088), (0, 276184576), (0, 51051314176), (0, 86437338368), (-1, 12345)],
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 826880), (0, 829696), (0, 848896), (0, 86392320), (0, 20400827904), (0, 43809494016), (-1, 12345)],
        ('FLOAT64',): [(0, 826880), (0, 829696), (0, 857088), (0, 175521280), (0, 51051314176), (0, 86437338368), (-1, 12345)],
        ('INT8', 'UINT8', 'BOOL8'): [(0, 826880), (0, 829696), (0, 842752), (0, 61226496), (0, 14400827904), (0, 30924592128), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'dense_rank/nulls': {
        ('INT16', 'UINT16'): [(0, 826880), (0, 829696), (0, 855296), (0, 111562496), (0, 26401804544), (0, 56696493312), (-1, 12345)],
        ('INT64', 'UINT64'): [(0, 826880), (0, 829696), (0, 873728), (0, 276184576), (0, 58577409280), (0, 95351198976), (-1, 12345)],
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 826880), (0, 829696), (0, 861440), (0, 136728320), (0, 32401804544), (0, 69581395200), (-1, 12345)],
        ('FLOAT64',): [(0, 826880), (0, 829696), (0, 873728), (0, 187059968), (0, 51051314176), (0, 95351198976), (-1, 12345)],
        ('INT8', 'UINT8', 'BOOL8'): [(0, 826880), (0, 829696), (0, 852224), (0, 98979584), (0, 23401804544), (0, 50254042368), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_probe_partitioned': {
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 574720), (0, 575232), (0, 582912), (0, 34129152), (0, 8017202944), (0, 17204612864), (-1, 12345)],
        ('INT64', 'UINT64', 'FLOAT64'): [(0, 574720), (0, 575232), (0, 587008), (0, 50906368), (0, 12000574720), (0, 25770378496), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_probe_partitioned_at': {
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 574720), (0, 575232), (0, 582912), (0, 34129152), (0, 8017202944), (0, 17204612864), (-1, 12345)],
        ('INT64', 'UINT64', 'FLOAT64'): [(0, 574720), (0, 575232), (0, 587008), (0, 50906368), (0, 12000574720), (0, 25770378496), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_probe_partitioned_pl': {
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 574720), (0, 575232), (0, 582912), (0, 34129152), (0, 8017202944), (0, 17204612864), (-1, 12345)],
        ('INT64', 'UINT64', 'FLOAT64'): [(0, 574720), (0, 575232), (0, 587008), (0, 50906368), (0, 12000574720), (0, 25770378496), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_build_partitioned': {
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 1623552), (0, 1624064), (0, 1631744), (0, 72943872), (0, 8001623552), (0, 17181492736), (-1, 12345)],
        ('INT64', 'UINT64', 'FLOAT64'): [(0, 1623552), (0, 1624064), (0, 1635840), (0, 106498304), (0, 12001623552), (0, 25771427328), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_build_partitioned_pl': {
        ('INT32', 'UINT32', 'FLOAT32'): [(0, 1623552), (0, 1624064), (0, 1631744), (0, 72943872), (0, 8001623552), (0, 17181492736), (-1, 12345)],
        ('INT64', 'UINT64', 'FLOAT64'): [(0, 1623552), (0, 1624064), (0, 1635840), (0, 106498304), (0, 12001623552), (0, 25771427328), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_filter': {
        ('INT32', 'INT64', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64'): [(0, 512), (0, 512), (0, 512), (0, 532992), (0, 126953472), (0, 272630272), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'join_complement': {
        ('-',): [(0, 256), (0, 256), (0, 256), (0, 524544), (0, 125000192), (0, 268435712), (-1, 12345)],
    },
    'partition_rows/hash': {
        ('INT32', 'INT64', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64'): [(0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'partition_rows/range': {
        ('INT32', 'INT64', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64'): [(0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'partition_rows_at': {
        ('INT32', 'INT64', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64'): [(0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'partition_rows_spec_at': {
        ('INT32', 'INT64', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64'): [(0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (0, 574720), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'groupby_sum_count_wide': {
        ('INT32', 'FLOAT32'): [(0, 19591424), (0, 19591424), (0, 19679744), (0, 128726784), (0, 22673524736), (0, 46734711296), (-1, 12345)],
        ('INT64', 'FLOAT64'): [(0, 23493120), (0, 23493120), (0, 23599104), (0, 154455552), (0, 27208213248), (0, 56081637120), (-1, 12345)],
        ('INT8', 'INT16', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'BOOL8', 'UNKNOWN'): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'group_offsets': {
        ('-',): [(0, 256), (0, 256), (0, 256), (0, 4352), (0, 976640), (0, 2097408), (-1, 12345)],
    },
    'segmented_reduce/SUM': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8', 'UNKNOWN'): [(0, 256), (0, 256), (0, 256), (0, 24832), (0, 5859584), (0, 12583168), (-1, 12345)],
    },
    'segmented_fill_nulls': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8', 'UNKNOWN'): [(0, 256), (0, 512), (0, 4352), (0, 16785664), (0, 4001953280), (0, 8594129152), (-1, 12345)],
    },
    'segmented_scan/SUM': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8', 'UNKNOWN'): [(0, 256), (0, 512), (0, 1280), (0, 4210944), (0, 1003906304), (0, 2155872512), (-1, 12345)],
    },
    'segmented_scan/keys': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8', 'UNKNOWN'): [(0, 256), (0, 512), (0, 1280), (0, 4210944), (0, 1003906304), (0, 2155872512), (-1, 12345)],
    },
    'reduce/SUM': {
        ('FLOAT32', 'FLOAT64'): [(0, 256), (0, 256), (0, 256), (0, 16640), (0, 3906304), (0, 8388864), (-1, 12345)],
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'BOOL8'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'reduce/PRODUCT': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'reduce/MIN': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'reduce/MAX': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'reduce/COUNT_NONZERO': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'reduce/unknown_op': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'scan/SUM': {
        ('FLOAT32', 'FLOAT64'): [(0, 256), (0, 256), (0, 256), (0, 16640), (0, 3906304), (0, 8388864), (-1, 12345)],
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 4608), (0, 976896), (0, 2097664), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'scan/PRODUCT': {
        ('FLOAT32', 'FLOAT64'): [(0, 256), (0, 256), (0, 256), (0, 8448), (0, 1953280), (0, 4194560), (-1, 12345)],
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 4608), (0, 976896), (0, 2097664), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'scan/MIN': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 4608), (0, 976896), (0, 2097664), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'scan/MAX': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(0, 512), (0, 512), (0, 512), (0, 4608), (0, 976896), (0, 2097664), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
    'scan/unknown_op': {
        ('INT8', 'INT16', 'INT32', 'INT64', 'UINT8', 'UINT16', 'UINT32', 'UINT64', 'FLOAT32', 'FLOAT64', 'BOOL8'): [(-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345), (-1, 12345)],
        ('UNKNOWN',): [(-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-2, 12345), (-1, 12345)],
    },
}


@pytest.fixture(scope="module")
def lib():
    from cudf_amd import _lib
    return _lib.lib


@pytest.mark.parametrize("name", list(QUERIES))
def test_query(lib, name):
    got, want = answers(lib, name), EXPECT[name]
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for key in want:
        assert got[key] == want[key], (name, key)


def test_no_query_needs_a_device():
    """Of the table itself: a positive code is a hipError_t, i.e. a query that reached a HIP call -- such an entry point belongs in
    the docstring, not in QUERIES.  And every query but the two with an unknown operator answers 0 with a size for some dtype and
    row count: one that never does pins no layout."""
    for name, groups in EXPECT.items():
        pairs = [p for row in groups.values() for p in row]
        assert all(rc <= 0 for rc, _ in pairs), name
        assert name.endswith("/unknown_op") or any(rc == 0 and nbytes != SENTINEL for rc, nbytes in pairs), name


def test_a_null_tmp_bytes_is_an_argument_error(lib):
    for name, (selects, query) in QUERIES.items():
        assert query(lib, "INT32" if selects != "none" else "-", 1000, None) == -1, name


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cudf_amd import _lib
    print("EXPECT = {")
    for name in QUERIES:
        print(f"    {name!r}: {{")
        for group, row in answers(_lib.lib, name).items():
            print(f"        {group!r}: {row!r},")
        print("    },")
    print("}")
