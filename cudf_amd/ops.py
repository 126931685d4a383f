"""Host-side mirror of the libcudf operator interface for the hot path, over the C ABI.

Function names / argument meaning / error behaviour follow pylibcudf's thin wrappers
(python/pylibcudf/pylibcudf/{sorting.pyx:37-613, join.pyx:63-108, groupby.pyx:89,
reduce.pyx:48-157, copying.pyx gather}) which bind the C++ API named in SURVEY.md section 8b.
Every function here only validates, allocates (torch as the device allocator) and calls
``libcudf_amd.so``; there is no CPU implementation to fall back to.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .column import Column, device_bytes, gx_dtype, ptr, stream_ptr, bitmask_words

JOIN_NO_MATCH = -(2**31)  # cudf::JoinNoMatch

_lib = L.lib


def _query(fn, *args):
    """Run the tmp==NULL size query of a gx_* entry point; returns required bytes."""
    nbytes = ctypes.c_size_t(0)
    L.check(fn(*args, None, ctypes.byref(nbytes), stream_ptr()), fn.__name__ + " (size query)")
    return nbytes.value


def _run(fn, *args):
    nbytes = _query(fn, *args)
    tmp = device_bytes(nbytes)
    nb = ctypes.c_size_t(nbytes)
    L.check(fn(*args, ptr(tmp), ctypes.byref(nb), stream_ptr()), fn.__name__)
    return tmp


def _check_sort_status(tmp: torch.Tensor):
    """Fail loudly if the device-side look-back protocol reported a timeout (never expected).  Only status 5 is a fault -- 3 means a
    bookkeeping mismatch of the hybrid path after which the LSD passes produced a correct output (include/cudf_amd/gx.h; the C++
    face draws the same line, cudf_amd/cpp/src/device_faults.cpp)."""
    st = ctypes.c_int(0)
    L.check(_lib.gx_sort_status(ptr(tmp), ctypes.byref(st), stream_ptr()), "gx_sort_status")
    if st.value == 5:
        raise L.GxError(f"radix sort look-back timed out (status {st.value})")


def _run_sort(fn, *args):
    """a sort whose status word this caller reads: opt into the recoverable fault form for this call (default: the kernel traps)"""
    _lib.gx_sort_set_fault_mode(1)
    try:
        return _run(fn, *args)
    finally:
        _lib.gx_sort_set_fault_mode(0)


def _dev_i64(value: int = 0) -> torch.Tensor:
    return torch.full((1,), value, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------
# sorting  (cudf::sort / sorted_order / stable_sorted_order / sort_by_key: sorting.hpp:44-163)
# ------------------------------------------------------------------------------------------------

def sort(col: Column, ascending: bool = True, null_before: bool = True) -> Column:
    """cudf::sort of a one-column table (src/sort/sort.cu:52-67).  No nulls: keys-only radix sort;
    with nulls: sort_by_key(input, input) like the reference's general path (:31-50)."""
    if col.has_nulls():
        order = sorted_order(col, ascending, null_before)
        return gather(col, order)
    out = Column.empty(col.dtype, col.size)
    tmp = _run_sort(_lib.gx_sort_keys, col.gx, col.data_ptr, out.data_ptr, col.size, int(not ascending))
    _check_sort_status(tmp)
    return out


def sorted_order(col: Column, ascending: bool = True, null_before: bool = True) -> Column:
    """cudf::sorted_order == stable_sorted_order for one column (always stable here)."""
    out = Column.empty(np.int32, col.size)
    valid = col.mask_ptr if col.has_nulls() else None
    tmp = (_run if valid else _run_sort)(_lib.gx_sorted_order, col.gx, col.data_ptr, valid, col.size, col.null_count if valid else 0,
                                         int(not ascending), int(null_before), out.data_ptr)
    if not valid:
        _check_sort_status(tmp)  # plan header sits at the start of the scratch on the radix path
    return out


stable_sorted_order = sorted_order


def sorted_order_table(cols: Sequence[Column], ascending: Union[bool, Sequence[bool]] = True) -> Column:
    """cudf::sorted_order / stable_sorted_order of a table of numeric columns WITHOUT nulls (src/sort/sort_impl.cuh:61-93): the
    lexicographic order of the rows, stable; NaN equivalent and greatest in every column.  One word sort on a nested rank of the tuple
    (gx_sorted_order_table, cudf_amd/csrc/gx_order.hip) instead of one argsort + two random gathers per column."""
    cols = list(cols)
    if not 1 <= len(cols) <= 8:
        raise ValueError("sorted_order_table: 1 to 8 key columns")
    n = cols[0].size
    asc = [ascending] * len(cols) if isinstance(ascending, bool) else list(ascending)
    if len(asc) != len(cols):
        raise ValueError("Mismatch between number of columns and column order.")  # sort_impl.cuh:43-46
    for c in cols:
        if c.size != n:
            raise ValueError("sorted_order_table: columns of different lengths")
        if c.has_nulls():
            raise NotImplementedError("sorted_order_table: columns with nulls take the per-column path (DataFrame.sort_values)")
    out = Column.empty(np.int32, n)
    if n == 0:
        return out
    k = len(cols)
    dtypes = (ctypes.c_int * k)(*[c.gx for c in cols])
    datas = (ctypes.c_void_p * k)(*[c.data_ptr for c in cols])
    desc = (ctypes.c_int * k)(*[int(not a) for a in asc])
    tmp = _run_sort(_lib.gx_sorted_order_table, k, dtypes, datas, desc, n, out.data_ptr)
    _check_sort_status(tmp)
    return out


def sort_by_key(values: Sequence[Column], keys: Column, ascending: bool = True,
                null_before: bool = True) -> List[Column]:
    """cudf::sort_by_key: gather(values, sorted_order(keys)) (src/sort/sort.cu:31-50)."""
    for v in values:
        if v.size != keys.size:
            raise RuntimeError("Mismatch in number of rows for values and keys")  # sort.cu:39
    order = sorted_order(keys, ascending, null_before)
    return [gather(v, order) for v in values]


def gather(col: Column, gather_map: Column, nullify_out_of_bounds: bool = False) -> Column:
    """cudf::gather for a fixed-width column (copying.hpp; detail/gather.cuh:108-131,506-577)."""
    if gather_map.dtype != np.int32:
        raise TypeError("gather map must be INT32")
    n = gather_map.size
    need_mask = col.mask is not None or nullify_out_of_bounds
    out = Column.empty(col.dtype, n, nullable=need_mask)
    L.check(_lib.gx_gather(col.dtype.itemsize, col.data_ptr, col.mask_ptr, col.size, gather_map.data_ptr, n,
                           int(nullify_out_of_bounds), out.data_ptr, out.mask_ptr, stream_ptr()), "gx_gather")
    if need_mask:
        out.null_count = n - bitmask_count(out.mask, n)
    return out


def gather_global_rows(rows: Column, idx: Column, seg_counts: Sequence[int], seg_bases: Sequence[int]) -> Column:
    """out[j] = rows[idx[j]] + seg_bases[segment of idx[j]] as int64: received int32 local rows -> global row ids of
    the join pairs `idx` selects (segment k = the seg_counts[k] entries received from rank k)."""
    n = idx.size
    out = Column.empty(np.int64, n)
    cnt = (ctypes.c_int64 * len(seg_counts))(*[int(x) for x in seg_counts])
    bas = (ctypes.c_int64 * len(seg_bases))(*[int(x) for x in seg_bases])
    L.check(_lib.gx_gather_global_rows(rows.data_ptr, rows.size, idx.data_ptr, n, len(seg_counts), cnt, bas, out.data_ptr,
                                       stream_ptr()), "gx_gather_global_rows")
    return out


def bitmask_count(mask: torch.Tensor, nbits: int) -> int:
    cnt = _dev_i64()
    L.check(_lib.gx_bitmask_count(ptr(mask), 0, nbits, ptr(cnt), stream_ptr()), "gx_bitmask_count")
    return int(cnt.item())


# ------------------------------------------------------------------------------------------------
# hashing / partitioning
# ------------------------------------------------------------------------------------------------

def murmurhash3_x86_32(cols: Sequence[Column], seed: int = 0) -> Column:
    """cudf::hashing::murmurhash3_x86_32 row hash of fixed-width columns."""
    n = cols[0].size
    out = Column.empty(np.uint32, n)
    for k, c in enumerate(cols):
        L.check(_lib.gx_murmur3_32(c.gx, c.data_ptr, c.mask_ptr if c.has_nulls() else None, n, seed, int(k > 0),
                                   out.data_ptr, stream_ptr()), "gx_murmur3_32")
    return out


def identity_hash(cols: Sequence[Column]) -> Column:
    """Row hash over IdentityHash (cudf::hash_partition(..., hash_id::HASH_IDENTITY), partitioning.cu:852-889): the element cast to
    uint32, columns folded with hash_combine, null -> UINT32_MAX."""
    n = cols[0].size
    out = Column.empty(np.uint32, n)
    for k, c in enumerate(cols):
        L.check(_lib.gx_identity_hash_32(c.gx, c.data_ptr, c.mask_ptr if c.has_nulls() else None, n, int(k > 0), out.data_ptr, stream_ptr()),
                "gx_identity_hash_32")
    return out


def hash_partition_map(key_cols: Sequence[Column], num_partitions: int, seed: int = 0, hash_function: str = "murmur3") -> Tuple[Column, np.ndarray]:
    """cudf::hash_partition in index form: (gather map, offsets[num_partitions+1]).  hash_function: "murmur3" (HASH_MURMUR3) or
    "identity" (HASH_IDENTITY)."""
    if hash_function not in ("murmur3", "identity"):
        raise ValueError("Unsupported hash function in hash_partition")
    h = identity_hash(key_cols) if hash_function == "identity" else murmurhash3_x86_32(key_cols, seed)
    n = h.size
    out_map = Column.empty(np.int32, n)
    offs = torch.empty(num_partitions + 1, dtype=torch.int32, device="cuda")
    _run(_lib.gx_hash_partition_map, h.data_ptr, n, num_partitions, out_map.data_ptr, ptr(offs))
    return out_map, offs.cpu().numpy()


def partition_rows(col: Column, nparts: int, splitters: Optional[Sequence] = None, want_rows: bool = True):
    """One-pass partition of a key column into `nparts` groups (gx_partition_rows): by a hash that is independent of
    the join table's slot bits (splitters None; any nparts <= 16), or by range (nparts - 1 ascending splitters:
    destination = number of splitters <= key).  Returns (grouped keys, int32 row indices or None, nparts + 1 offsets).
    What a rank runs before the all-to-all of the distributed sort / join / groupby
    (cudf::hash_partition, cpp/src/partitioning/partitioning.cu:568-660)."""
    n = col.size
    out = Column.empty(col.dtype, n)
    rows = Column.empty(np.int32, n) if want_rows else None
    offs = torch.zeros(nparts + 1, dtype=torch.int64, device="cuda")
    mode = 0 if splitters is None else 1
    sp = None
    if splitters is not None:
        if len(splitters) != nparts - 1:
            raise ValueError("range partition needs nparts - 1 splitters")
        sp_np = np.asarray(list(splitters) + [0], dtype=col.dtype)   # host array the call reads synchronously
        sp = sp_np.ctypes.data_as(ctypes.c_void_p)
    _run(_lib.gx_partition_rows, col.gx, col.data_ptr, n, mode, nparts, sp, out.data_ptr, rows.data_ptr if rows is not None else None,
         ptr(offs))
    return out, rows, [int(x) for x in offs.cpu()]


def merge_sum_count(keys: Column, sums: Column, counts: Column):
    """Partial (key, sum, count) rows -> one row per distinct key, keys ascending: sorted_order of the keys, run heads
    and labels once, then two segmented reductions over the same grouping (the sort-based aggregation path:
    cpp/src/groupby/sort/aggregate.cpp:94-142).  Float sums in double-double (order independent)."""
    n = keys.size
    if n == 0:
        return Column.empty(keys.dtype, 0), Column.empty(sums.dtype, 0), Column.empty(np.int64, 0)
    order = sorted_order(keys)
    sk, ss, sc = gather(keys, order), gather(sums, order), gather(counts, order)
    heads = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(_lib.gx_group_heads(sk.gx, sk.data_ptr, None, None, n, 0, ptr(heads), stream_ptr()), "gx_group_heads")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ng = _dev_i64()
    _run(_lib.gx_group_offsets, ptr(heads), n, ptr(labels), ptr(offsets), None, ptr(ng))
    g = int(ng.item())
    out_s = Column.empty(sums.dtype if sums.dtype.kind == "f" else np.int64, g)
    out_c = Column.empty(np.int64, g)
    _run(_lib.gx_segmented_reduce, ss.gx, ss.data_ptr, None, ptr(heads), ptr(labels), n, L.OP_SUM, out_s.data_ptr, None)
    _run(_lib.gx_segmented_reduce, sc.gx, sc.data_ptr, None, ptr(heads), ptr(labels), n, L.OP_SUM, out_c.data_ptr, None)
    starts = Column(offsets[:g].contiguous().view(torch.uint8), np.int32, g)
    return gather(sk, starts), out_s, out_c


# ------------------------------------------------------------------------------------------------
# hash join  (cudf::hash_join / cudf::inner_join: join/hash_join.hpp:70-444, join/join.hpp:160-166)
# ------------------------------------------------------------------------------------------------

def _join_key(col: Column) -> Column:
    if col.dtype.itemsize not in (4, 8):
        raise TypeError("join key must be a 4- or 8-byte fixed-width column")  # data_type_error
    if col.dtype.kind == "f":
        # row equality of the reference: -0.0 == +0.0 and NaN == NaN whatever the payload
        # (detail/row_operator/common_utils.cuh:215-220); gx_pack_keys normalises both, the table compares bits
        key = pack_keys([col])
        key.mask, key.null_count = col.mask, col.null_count
        return key
    return col


class HashJoin:
    """cudf::hash_join: build once on `right`, probe many (hash_join.hpp:95-125).  The object
    views the build column: keep it alive (hash_join.hpp:83-84)."""

    def __init__(self, right: Column, nulls_equal: bool = True, load_factor: float = 0.5):
        if not (0.0 < load_factor <= 1.0):
            raise ValueError("Invalid load factor: must be greater than 0 and less than or equal to 1.")
        self.build_dtype = right.dtype
        self.build = right = _join_key(right)
        self.nulls_equal = nulls_equal
        self.key_size = right.dtype.itemsize
        self.load_factor = load_factor
        self.table_bytes = _lib.gx_join_table_bytes(self.key_size, right.size, load_factor)
        self.table = device_bytes(self.table_bytes)
        valid = right.mask_ptr if right.has_nulls() else None
        if (valid is None and right.size >= (1 << 20)
                and _lib.gx_join_partition_bits(self.key_size, self.table_bytes) > 0):
            # large build side: partition the rows first so the inserts hit L2-resident sub-tables
            _run(_lib.gx_join_build_partitioned, self.key_size, right.data_ptr, right.size, ptr(self.table),
                 self.table_bytes, load_factor)
        else:
            L.check(_lib.gx_join_build(self.key_size, right.data_ptr, valid, right.size, ptr(self.table),
                                       self.table_bytes, load_factor, stream_ptr()), "gx_join_build")

    def _check(self, left: Column) -> Column:
        """type check (hash_join.cu:56-58); returns the probe column in the table's key space"""
        if left.dtype != self.build_dtype:
            raise TypeError("Mismatch in joining column data types")
        return _join_key(left) if left.size else left

    def inner_join_size(self, left: Column) -> int:
        left = self._check(left)
        if left.size == 0 or self.build.size == 0:
            return 0
        cnt = _dev_i64()
        valid = left.mask_ptr if left.has_nulls() else None
        L.check(_lib.gx_join_count(self.key_size, left.data_ptr, valid, left.size, ptr(self.table),
                                   self.table_bytes, ptr(cnt), stream_ptr()), "gx_join_count")
        total = int(cnt.item())
        if self.nulls_equal:
            total += left.null_count * self.build.null_count if left.has_nulls() and self.build.has_nulls() else 0
        return total

    PARTITIONED_MIN_ROWS = 1 << 22

    def _probe(self, left: Column, capacity: int, left_outer: int):
        """left_outer: gx_join_probe's flags (bit 0 left outer, bit 1 null probe rows emit nothing)"""
        lo = Column.empty(np.int32, capacity)
        ro = Column.empty(np.int32, capacity)
        cur = _dev_i64()
        valid = left.mask_ptr if left.has_nulls() else None
        if (valid is None and left.size >= self.PARTITIONED_MIN_ROWS
                and _lib.gx_join_partition_bits(self.key_size, self.table_bytes) > 0):
            # large probe against a table far beyond the L2s: partition the probe rows first
            _run(_lib.gx_join_probe_partitioned, self.key_size, left.data_ptr, left.size, ptr(self.table),
                 self.table_bytes, int(left_outer) & 1, lo.data_ptr, ro.data_ptr, capacity, ptr(cur))
            return lo, ro, int(cur.item())
        L.check(_lib.gx_join_probe(self.key_size, left.data_ptr, valid, left.size, ptr(self.table), self.table_bytes,
                                   int(left_outer), lo.data_ptr, ro.data_ptr, capacity, ptr(cur), stream_ptr()),
                "gx_join_probe")
        return lo, ro, int(cur.item())

    def inner_join(self, left: Column, output_size: Optional[int] = None) -> Tuple[Column, Column]:
        """(left_indices, right_indices), order unspecified (join.hpp:131-134)."""
        left = self._check(left)
        if left.size == 0 or self.build.size == 0:  # trivial joins (hash_join.cu:32-45)
            return Column.empty(np.int32, 0), Column.empty(np.int32, 0)
        # optimistic single pass: with distinct build keys (the common PK-FK case) matches <= probe
        # rows; 288 GB of HBM makes that allocation cheaper than the reference's count pass
        capacity = output_size if output_size is not None else left.size
        lo, ro, total = self._probe(left, capacity, False)
        if total > capacity:  # duplicate build keys blew the guess: size is now known exactly
            lo, ro, total = self._probe(left, total, False)
        lo.size = ro.size = total
        if self.nulls_equal and left.has_nulls() and self.build.has_nulls():
            lo, ro = _append_null_cross(lo, ro, left, self.build)
        return lo, ro

    def left_join(self, left: Column) -> Tuple[Column, Column]:
        left = self._check(left)
        if left.size == 0:
            return Column.empty(np.int32, 0), Column.empty(np.int32, 0)
        # null == null (hash_join.cu:77-84): a null left row matches every null build row instead of (i, JoinNoMatch)
        cross = self.nulls_equal and left.has_nulls() and self.build.has_nulls()
        flags = 3 if cross else 1
        lo, ro, total = self._probe(left, left.size, flags)
        if total > left.size:
            lo, ro, total = self._probe(left, total, flags)
        lo.size = ro.size = total
        if cross:
            lo, ro = _append_null_cross(lo, ro, left, self.build)
        return lo, ro


    def lookup(self, left: Column) -> Column:
        """cudf::distinct_hash_join::left_join (distinct_hash_join.hpp:96-116): for DISTINCT build keys,
        the build row matching each left row, in left order, JoinNoMatch (INT32_MIN) where there is none.
        (With duplicate build keys it returns one of the matching rows.)"""
        left = self._check(left)
        out = Column.empty(np.int32, left.size)
        if left.size == 0:
            return out
        if self.build.size == 0:   # nothing to look up: JoinNoMatch everywhere (a host-built column: no kernel of ours or of torch's)
            return Column.from_numpy(np.full(left.size, -(2 ** 31), np.int32))
        valid = left.mask_ptr if left.has_nulls() else None
        L.check(_lib.gx_join_lookup(self.key_size, left.data_ptr, valid, left.size, ptr(self.table), self.table_bytes,
                                    out.data_ptr, stream_ptr()), "gx_join_lookup")
        if self.nulls_equal and left.has_nulls() and self.build.has_nulls():
            # null == null: every null left row matches the (single, keys are distinct) null build row.  A rare path, patched on the
            # host like the C++ face does (cpp/src/join.cpp: the null x null pairs are composed on the host and copied)
            rv = int(np.nonzero(~self.build.valid_numpy())[0][0])
            o = out.to_numpy()
            o[~left.valid_numpy()] = rv
            out = Column.from_numpy(o)
        return out

    def _filter(self, left: Column, anti: bool) -> Column:
        left = self._check(left)
        out = Column.empty(np.int32, left.size)
        if left.size == 0:
            return out
        if self.build.size == 0:  # nothing can match
            if anti:
                L.check(_lib.gx_sequence_i32(out.data_ptr, left.size, 0, stream_ptr()), "gx_sequence_i32")
            else:
                out.size = 0
            return out
        cnt = _dev_i64()
        valid = left.mask_ptr if left.has_nulls() else None
        null_matches = int(self.nulls_equal and self.build.has_nulls())
        _run(_lib.gx_join_filter, self.key_size, left.data_ptr, valid, left.size, ptr(self.table), self.table_bytes,
             int(anti), null_matches, out.data_ptr, ptr(cnt))
        out.size = int(cnt.item())
        return out

    def semi_join(self, left: Column) -> Column:
        """cudf::filtered_join::semi_join (filtered_join.hpp:96-116): ascending left rows with a match."""
        return self._filter(left, False)

    def anti_join(self, left: Column) -> Column:
        """cudf::filtered_join::anti_join (filtered_join.hpp:118-139): ascending left rows without a match."""
        return self._filter(left, True)


def _append_null_cross(lo: Column, ro: Column, left: Column, right: Column):
    """null_equality::EQUAL for a single nullable key: every null left row matches every null
    right row.  Rare path: the cross product is composed on the HOST from the two validity masks and copied behind the probe's
    pairs -- what the C++ face does (cudf_amd/cpp/src/join.cpp, `cross`); no torch kernel takes part."""
    lv = np.nonzero(~left.valid_numpy())[0].astype(np.int32)
    rv = np.nonzero(~right.valid_numpy())[0].astype(np.int32)
    cross = len(lv) * len(rv)
    n = lo.size + cross
    outs = []
    for src, add in ((lo, np.repeat(lv, len(rv))), (ro, np.tile(rv, len(lv)))):
        out = Column.empty(np.int32, n)
        if lo.size:
            L.check(_lib.gx_copy_bytes(src.data_ptr, out.data_ptr, lo.size * 4, stream_ptr()), "gx_copy_bytes")
        if cross:
            tail = Column.from_numpy(np.ascontiguousarray(add))
            L.check(_lib.gx_copy_bytes(tail.data_ptr, ctypes.c_void_p(out.data.data_ptr() + lo.size * 4), cross * 4, stream_ptr()), "gx_copy_bytes")
            torch.cuda.current_stream().synchronize()   # `tail` may be recycled once the copy has run
        outs.append(out)
    return outs[0], outs[1]


def inner_join(left: Column, right: Column, nulls_equal: bool = True) -> Tuple[Column, Column]:
    """cudf::inner_join (src/join/join.cu:27-60): build on the smaller side, swap the pair back."""
    if left.dtype != right.dtype:
        raise TypeError("Mismatch in joining column data types")
    if right.size > left.size:
        hj = HashJoin(left, nulls_equal)
        r, l = hj.inner_join(right)
        return l, r
    return HashJoin(right, nulls_equal).inner_join(left)


def left_semi_join(left: Column, right: Column, nulls_equal: bool = True) -> Column:
    if left.dtype != right.dtype:
        raise TypeError("Mismatch in joining column data types")
    return HashJoin(right, nulls_equal).semi_join(left)


def left_anti_join(left: Column, right: Column, nulls_equal: bool = True) -> Column:
    if left.dtype != right.dtype:
        raise TypeError("Mismatch in joining column data types")
    return HashJoin(right, nulls_equal).anti_join(left)


def left_join(left: Column, right: Column, nulls_equal: bool = True) -> Tuple[Column, Column]:
    if left.dtype != right.dtype:
        raise TypeError("Mismatch in joining column data types")
    return HashJoin(right, nulls_equal).left_join(left)


def _append_unmatched_right(lo: Column, ro: Column, right_rows: int) -> Tuple[Column, Column]:
    """cudf::full_join's complement step (src/join/join_utils.cu:86-157; gx_join_complement): behind the left-join pairs, one
    (JoinNoMatch, r) pair for every right row r that occurs in no pair.  Returns the grown pair arrays."""
    n0 = lo.size
    ol, orr = Column.empty(np.int32, n0 + right_rows), Column.empty(np.int32, n0 + right_rows)
    if n0:
        L.check(_lib.gx_copy_bytes(lo.data_ptr, ol.data_ptr, n0 * 4, stream_ptr()), "gx_copy_bytes")
        L.check(_lib.gx_copy_bytes(ro.data_ptr, orr.data_ptr, n0 * 4, stream_ptr()), "gx_copy_bytes")
    cur = _dev_i64(n0)
    _run(_lib.gx_join_complement, ro.data_ptr, n0, right_rows, ol.data_ptr, orr.data_ptr, n0 + right_rows, ptr(cur))
    ol.size = orr.size = int(cur.item())
    return ol, orr


def full_join(left: Column, right: Column, nulls_equal: bool = True) -> Tuple[Column, Column]:
    """cudf::full_join (join.hpp:240-246; src/join/hash_join/hash_join.cu:168-199): the left join's pairs, then every right row without
    a partner as (JoinNoMatch, r)."""
    lo, ro = left_join(left, right, nulls_equal)
    return _append_unmatched_right(lo, ro, right.size)


# ------------------------------------------------------------------------------------------------
# multi-column keys: rows -> one fixed-width key  (gx_pack_keys / gx_dense_rank; the reference compares
# whole rows inside its hash tables: detail/row_operator/primitive_row_operators.cuh:207-274)
# ------------------------------------------------------------------------------------------------

def pack_keys(cols: Sequence[Column]) -> Column:
    """Concatenate columns whose widths sum to <= 8 bytes into one uint64 key column (no nulls)."""
    n = cols[0].size
    out = Column.empty(np.uint64, n)
    ptrs = (ctypes.c_void_p * len(cols))(*[c.data_ptr.value or 0 for c in cols])
    dts = (ctypes.c_int * len(cols))(*[c.gx for c in cols])
    L.check(_lib.gx_pack_keys(len(cols), ptrs, dts, n, out.data_ptr, stream_ptr()), "gx_pack_keys")
    return out


def _col_ptrs(cols: Sequence[Column]):
    return ((ctypes.c_void_p * len(cols))(*[c.data_ptr.value or 0 for c in cols]), (ctypes.c_int * len(cols))(*[c.gx for c in cols]))


def hash_rows64(cols: Sequence[Column], seed: int = 0) -> Column:
    """One uint64 hash per row of the key columns (floats normalised: -0.0 == +0.0, NaN == NaN).  Equal rows hash
    equal; a result obtained through the hashes is certified by rows_mismatch_count == 0."""
    n = cols[0].size
    out = Column.empty(np.uint64, n)
    ptrs, dts = _col_ptrs(cols)
    L.check(_lib.gx_hash_rows64(len(cols), ptrs, dts, n, seed, out.data_ptr, stream_ptr()), "gx_hash_rows64")
    return out


def rows_mismatch_count(lcols: Sequence[Column], rcols: Sequence[Column], lidx: Optional[Column], ridx: Optional[Column],
                        npairs: int) -> int:
    """Number of pairs (lidx[i], ridx[i]) -- None = row i, negative = no row -- whose rows differ in some column."""
    lp, dts = _col_ptrs(lcols)
    rp, _ = _col_ptrs(rcols)
    cnt = _dev_i64()
    L.check(_lib.gx_rows_mismatch_count(len(lcols), lp, rp, dts, lidx.data_ptr if lidx is not None else None,
                                        ridx.data_ptr if ridx is not None else None, npairs, ptr(cnt), stream_ptr()),
            "gx_rows_mismatch_count")
    return int(cnt.item())


class RowKeys:
    """ONE 8-byte key per row of a multi-column key table, for the single-key groupby kernels, without sorting:
    the packed column values when their widths sum to <= 8 bytes (exact), else a 64-bit row hash.  Rows holding a
    null key get a null key (they belong to no group: null_policy::EXCLUDE).  key_columns() turns the distinct keys
    of a result back into key columns and -- for hashed keys -- certifies that no two different rows shared a hash."""

    def __init__(self, cols: Sequence[Column]):
        self.cols = list(cols)
        n = self.cols[0].size
        self.bare = [Column(c.data, c.dtype, c.size) for c in self.cols]
        self.exact = sum(c.dtype.itemsize for c in self.cols) <= 8
        self.col = pack_keys(self.bare) if self.exact else hash_rows64(self.bare)
        self.col.mask, self.col.null_count = _and_masks(self.cols, n)

    def key_columns(self, distinct: Column) -> Optional[List[Column]]:
        """Key columns of the groups whose row keys are `distinct` (in that order).  Packed keys are unpacked.  Hashed
        keys: per key column one streaming groupby MIN + MAX by hash; MIN == MAX in every group and column means every
        row of a group carries the same key values (the values returned), i.e. no 64-bit collision; None otherwise
        (the caller then encodes through gx_dense_rank)."""
        g = distinct.size
        if self.exact:
            outs = [Column.empty(c.dtype, g) for c in self.cols]
            ptrs = (ctypes.c_void_p * len(outs))(*[c.data_ptr.value or 0 for c in outs])
            dts = (ctypes.c_int * len(outs))(*[c.gx for c in outs])
            L.check(_lib.gx_unpack_keys(len(outs), ptrs, dts, g, distinct.data_ptr, stream_ptr()), "gx_unpack_keys")
            return outs
        if g == 0:
            return [Column.empty(c.dtype, 0) for c in self.cols]
        mns, mxs = [], []
        for c in self.bare:
            hk, mn, mx, _ = groupby_min_max(self.col, c, max_groups_hint=g)
            if hk.size != g:
                return None
            o = sorted_order(hk)                                   # ascending-hash order
            mns.append(gather(mn, o))
            mxs.append(gather(mx, o))
        if rows_mismatch_count(mns, mxs, None, None, g) != 0:
            return None
        back = sorted_order(sorted_order(distinct))                # ascending-hash position of every entry of `distinct`
        return [gather(m, back) for m in mns]


def dense_rank(col: Column):
    """(ids int32 column, first row of every id, number of ids): equal values share an id, null == null
    has its own id (last), ids ascend with the value."""
    n = col.size
    ids, rep = Column.empty(np.int32, n), Column.empty(np.int32, n)
    ng = _dev_i64()
    _run(_lib.gx_dense_rank, col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, n,
         col.null_count if col.has_nulls() else 0, ids.data_ptr, rep.data_ptr, ptr(ng))
    g = int(ng.item())
    rep.size = g
    return ids, rep, g


def _and_masks(cols: Sequence[Column], n: int):
    """(mask words tensor or None, null count) of the AND of the columns' validity."""
    masks = [c for c in cols if c.has_nulls()]
    if not masks:
        return None, 0
    out = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    arr = (ctypes.c_void_p * len(masks))(*[c.mask_ptr.value for c in masks])
    cnt = _dev_i64()
    L.check(_lib.gx_bitmask_and(arr, len(masks), n, ptr(out), ptr(cnt), stream_ptr()), "gx_bitmask_and")
    return out, n - int(cnt.item())


def concat_columns(a: Column, b: Column) -> Column:
    """cudf::concatenate of two columns of one type (data memcpy + gx_bitmask_copy for the validity)."""
    if a.dtype != b.dtype:
        raise TypeError("Mismatch in joining column data types")
    n = a.size + b.size
    if n > 2**31 - 1:
        raise OverflowError("concatenated key columns exceed cudf::size_type")
    w = a.dtype.itemsize
    out = Column.empty(a.dtype, n, nullable=a.has_nulls() or b.has_nulls())
    out.data[: a.size * w].copy_(a.data[: a.size * w])
    out.data[a.size * w: n * w].copy_(b.data[: b.size * w])
    if out.mask is not None:
        L.check(_lib.gx_bitmask_copy(ptr(out.mask), 0, a.mask_ptr if a.has_nulls() else None, 0, a.size, stream_ptr()),
                "gx_bitmask_copy")
        L.check(_lib.gx_bitmask_copy(ptr(out.mask), a.size, b.mask_ptr if b.has_nulls() else None, 0, b.size,
                                     stream_ptr()), "gx_bitmask_copy")
        out.null_count = a.null_count + b.null_count
    return out


def _slice_rows(col: Column, begin: int, end: int) -> Column:
    """Rows [begin, end) of a column WITHOUT nulls as a new column sharing no storage."""
    w = col.dtype.itemsize
    out = Column.empty(col.dtype, end - begin)
    out.data[: (end - begin) * w].copy_(col.data[begin * w: end * w])
    return out


def encode_rows(tables: Sequence[Sequence[Column]], nulls_equal: bool = True, dense: bool = False):
    """Encode the rows of 1 or 2 tables (same schema) into ONE key column per table such that two rows
    get equal keys iff they compare equal column by column (null == null, NaN == NaN, -0.0 == +0.0).
    Rows holding a null are marked null in the result when nulls_equal is False (they can then match
    nothing).  dense=True (one table): keys are dense int32 ids; also returns (first row per id, #ids).

    Path 1 (widths sum to <= 8 bytes, no nulls): gx_pack_keys, exact, one streaming pass.
    Path 2: every column -> dense ids over the CONCATENATION of the tables (so ids agree across them),
    then (ids so far, next column's ids) pairs are packed and ranked again."""
    ncols = len(tables[0])
    for t in tables[1:]:
        if len(t) != ncols:
            raise ValueError("Mismatch in number of columns to be joined on")
        for a, b in zip(tables[0], t):
            if a.dtype != b.dtype:
                raise TypeError("Mismatch in joining column data types")
    sizes = [t[0].size for t in tables]
    any_nulls = any(c.has_nulls() for t in tables for c in t)
    width = sum(c.dtype.itemsize for c in tables[0])
    if width <= 8 and not any_nulls and not dense:
        return [pack_keys(t) for t in tables]
    # ---- one tall table
    if len(tables) == 2:
        cols = [concat_columns(a, b) for a, b in zip(tables[0], tables[1])]
    else:
        cols = list(tables[0])
    n = cols[0].size
    if width <= 8 and not any_nulls:
        ids, rep, g = dense_rank(pack_keys(cols))
    else:
        def as32(c):  # a column the pair-packing can take as it is: 4 bytes, no nulls, bitwise equality
            return c if (c.dtype.itemsize == 4 and not c.has_nulls() and c.dtype.kind in "iu") else dense_rank(c)[0]
        cur = None
        ids = rep = None
        g = 0
        for k, c in enumerate(cols):
            if cur is None:
                if ncols == 1:
                    ids, rep, g = dense_rank(c)
                cur = as32(c) if ncols > 1 else ids
                continue
            pair = pack_keys([cur, as32(c)])
            if k == ncols - 1 and not dense:
                ids = pair           # the last packing need not be dense
            else:
                ids, rep, g = dense_rank(pair)
                cur = ids
    mask, nulls = (None, 0) if nulls_equal else _and_masks(cols, n)
    outs = []
    begin = 0
    for sz in sizes:
        o = _slice_rows(ids, begin, begin + sz) if len(sizes) > 1 else ids
        if mask is not None:
            words = torch.zeros(bitmask_words(sz), dtype=torch.int32, device="cuda")
            L.check(_lib.gx_bitmask_copy(ptr(words), 0, ptr(mask), begin, sz, stream_ptr()), "gx_bitmask_copy")
            cnt = _dev_i64()
            L.check(_lib.gx_bitmask_count(ptr(words), 0, sz, ptr(cnt), stream_ptr()), "gx_bitmask_count")
            o.mask, o.null_count = words, sz - int(cnt.item())
        outs.append(o)
        begin += sz
    if dense:
        return outs[0], rep, g
    return outs


def _hashed_join(left: Sequence[Column], right: Sequence[Column], nulls_equal: bool, join):
    """Rows wider than 8 bytes: join on a 64-bit row hash (one pass over the key columns per side), then compare the
    real columns of every emitted pair.  Equal rows always hash equal, so no pair is missing; a pair that fails the
    comparison is a 64-bit collision and sends the call to the exact encoding (None).  With nulls the fast path
    needs null != null (a row holding a null matches nothing: its hash is marked null)."""
    if len(left) != len(right):
        raise ValueError("Mismatch in number of columns to be joined on")
    for a, b in zip(left, right):
        if a.dtype != b.dtype:
            raise TypeError("Mismatch in joining column data types")
    width = sum(c.dtype.itemsize for c in left)
    any_nulls = any(c.has_nulls() for c in list(left) + list(right))
    if width <= 8 or (any_nulls and nulls_equal):
        return None
    keys = []
    for t in (left, right):
        bare = [Column(c.data, c.dtype, c.size) for c in t]
        k = hash_rows64(bare)
        k.mask, k.null_count = _and_masks(t, t[0].size)
        keys.append((k, bare))
    (lk, lbare), (rk, rbare) = keys
    l, r = join(lk, rk, False)
    if rows_mismatch_count(lbare, rbare, l, r, l.size) != 0:
        return None
    return l, r


def inner_join_tables(left: Sequence[Column], right: Sequence[Column], nulls_equal: bool = True):
    """cudf::inner_join on key TABLES (join.hpp:160-166): rows are encoded, then the single-key join."""
    if len(left) == 1 and len(right) == 1:
        return inner_join(left[0], right[0], nulls_equal)
    res = _hashed_join(left, right, nulls_equal, inner_join)
    if res is not None:
        return res
    lk, rk = encode_rows([left, right], nulls_equal)
    return inner_join(lk, rk, nulls_equal)


def left_join_tables(left: Sequence[Column], right: Sequence[Column], nulls_equal: bool = True):
    if len(left) == 1 and len(right) == 1:
        return left_join(left[0], right[0], nulls_equal)
    res = _hashed_join(left, right, nulls_equal, left_join)
    if res is not None:
        return res
    lk, rk = encode_rows([left, right], nulls_equal)
    return left_join(lk, rk, nulls_equal)


def full_join_tables(left: Sequence[Column], right: Sequence[Column], nulls_equal: bool = True):
    """cudf::full_join on key tables: the left join of the tables + the unmatched right rows"""
    lo, ro = left_join_tables(left, right, nulls_equal)
    return _append_unmatched_right(lo, ro, right[0].size)


def groupby_keys_tables(keys: Sequence[Column]):
    """Multi-column groupby keys, exact encoding -> (dense int32 id column with the rows holding a null key marked
    null, first row of every id, number of ids): aggregate by id, gather the key columns by first row.  One radix
    sort per key column (gx_dense_rank); the operators use RowKeys (one hash pass) and come here on a collision."""
    ids, rep, g = encode_rows([keys], nulls_equal=False, dense=True)
    return ids, rep, g


# ------------------------------------------------------------------------------------------------
# groupby  (cudf::groupby::groupby::aggregate / scan: groupby.hpp:89-240)
# ------------------------------------------------------------------------------------------------

def groupby_sum_count(keys: Column, values: Column, max_groups_hint: int = 1 << 20):
    """Hash groupby with SUM + COUNT_VALID + COUNT_ALL of one values column.
    Returns (keys, sum, count_valid, count_all) columns in unspecified group order."""
    if keys.size != values.size:
        raise RuntimeError("Size mismatch between request values and groupby keys.")  # groupby.cu:230
    if keys.dtype.itemsize not in (4, 8) or keys.dtype.kind not in "iu":
        raise TypeError("groupby key must be a 32/64-bit integer column")
    n = keys.size
    sum_dt = np.dtype(values.dtype if values.dtype.kind == "f" else np.int64)
    max_groups = max(1, min(n, max_groups_hint))
    while True:
        ok = Column.empty(keys.dtype, max_groups)
        osum = Column.empty(sum_dt, max_groups)
        ocv = Column.empty(np.int32, max_groups)
        oca = Column.empty(np.int32, max_groups)
        ng = _dev_i64()
        _run(_lib.gx_groupby_sum_count, keys.gx, keys.data_ptr, keys.mask_ptr if keys.has_nulls() else None,
             values.gx, values.data_ptr, values.mask_ptr if values.has_nulls() else None, n, max_groups,
             ok.data_ptr, osum.data_ptr, ocv.data_ptr, oca.data_ptr, ptr(ng))
        g = int(ng.item())
        if 0 <= g <= max_groups:
            break
        if max_groups >= n:
            raise RuntimeError("groupby table overflow")
        max_groups = min(n, max_groups * 8)
    for c in (ok, osum, ocv, oca):
        c.size = g
    return ok, osum, ocv, oca


WIDE_GROUPBY_MIN_ROWS = 1 << 18  # below: the partition pass is not worth its 4096 slots
_SIGNED_OF_WIDTH = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _widen_i64(col: Column) -> Column:
    """an integer column as 8-byte words (sign / zero extended): what gx_groupby_sum_count_wide compares"""
    if col.dtype.itemsize == 8:
        return Column(col.data, col.dtype, col.size)
    # any injective map to 8-byte words will do (the words are only hashed and compared): view as the SIGNED type of the same
    # width and sign-extend; narrowing back keeps the low bytes
    t = col.data[: col.size * col.dtype.itemsize].view(_SIGNED_OF_WIDTH[col.dtype.itemsize])
    out = Column.empty(np.int64, col.size)
    out.data[: col.size * 8].view(torch.int64).copy_(t)
    return out


def _groupby_sum_count_wide(keys: Sequence[Column], values: Column, max_groups_hint: int = 1 << 20):
    """groupby on 2..4 integer key columns in ONE partition pass with the rows compared inside the LDS tables
    (gx_groupby_sum_count_wide).  None: not applicable / the device asked for the fallback."""
    n = values.size
    if not (2 <= len(keys) <= 4) or n < WIDE_GROUPBY_MIN_ROWS or values.has_nulls() or values.dtype.kind not in "if" or \
            values.dtype.itemsize not in (4, 8) or any(k.has_nulls() or k.dtype.kind not in "iu" for k in keys):
        return None
    wide = [_widen_i64(k) for k in keys]
    sum_dt = np.dtype(values.dtype if values.dtype.kind == "f" else np.int64)
    max_groups = max(1, min(n, max_groups_hint))
    kp = (ctypes.c_void_p * len(wide))(*[k.data_ptr.value or 0 for k in wide])
    while True:
        outs = [Column.empty(np.int64, max_groups) for _ in wide]
        osum, ocv = Column.empty(sum_dt, max_groups), Column.empty(np.int32, max_groups)
        op = (ctypes.c_void_p * len(outs))(*[o.data_ptr.value or 0 for o in outs])
        ng = _dev_i64()
        _run(_lib.gx_groupby_sum_count_wide, len(wide), kp, values.gx, values.data_ptr, n, max_groups, op, osum.data_ptr, ocv.data_ptr, ptr(ng))
        g = int(ng.item())
        if g == -2:
            return None
        if g >= 0:
            break
        if max_groups >= n:
            raise RuntimeError("groupby table overflow")
        max_groups = min(n, max_groups * 8)
    kcols = []
    for o, k in zip(outs, keys):
        o.size = g
        if k.dtype.itemsize == 8:
            kcols.append(Column(o.data, k.dtype, g))
        else:  # narrow the words back to the column's type
            c = Column.empty(k.dtype, g)
            c.data[: g * k.dtype.itemsize].view(_SIGNED_OF_WIDTH[k.dtype.itemsize]).copy_(o.data[: g * 8].view(torch.int64))
            kcols.append(c)
    osum.size = ocv.size = g
    return kcols, osum, ocv, ocv


def groupby_sum_count_tables(keys: Sequence[Column], values: Column, exact: bool = False):
    """groupby(keys = several columns).agg(SUM, COUNT_VALID, COUNT_ALL): the rows' 8-byte keys (RowKeys: packed values
    or row hash) go through the single-key hash groupby; the key columns come back from the distinct keys.
    exact=True, or a 64-bit collision: dense ids (gx_dense_rank), aggregate by id, gather the key columns by the
    first row of every id.  Returns ([key columns], sum, count_valid, count_all); rows with a null in any key are dropped."""
    if len(keys) == 1 and keys[0].dtype.itemsize in (4, 8) and keys[0].dtype.kind in "iu":
        k, s, cv, ca = groupby_sum_count(keys[0], values)
        return [k], s, cv, ca
    if keys[0].size != values.size:
        raise RuntimeError("Size mismatch between request values and groupby keys.")
    if not exact:
        r = _groupby_sum_count_wide(keys, values)
        if r is not None:
            return r
    if not exact and len(keys) <= 8:
        rk = RowKeys(keys)
        hk, s, cv, ca = groupby_sum_count(rk.col, values)
        kc = rk.key_columns(hk)
        if kc is not None:
            return kc, s, cv, ca
    ids, rep, g = groupby_keys_tables(keys)
    ok, s, cv, ca = groupby_sum_count(ids, values, max_groups_hint=max(g, 1))
    rows = gather(rep, ok)  # id -> its first row
    return [gather(k, rows) for k in keys], s, cv, ca


def groupby_min_max(keys: Column, values: Column, max_groups_hint: int = 1 << 20):
    """Hash groupby MIN + MAX + COUNT_VALID of one values column -> (keys, min, max, count_valid);
    min/max have the values' dtype and are meaningful where count_valid > 0."""
    if keys.size != values.size:
        raise RuntimeError("Size mismatch between request values and groupby keys.")
    if keys.dtype.itemsize not in (4, 8) or keys.dtype.kind not in "iu":
        raise TypeError("groupby key must be a 32/64-bit integer column")
    n = keys.size
    max_groups = max(1, min(n, max_groups_hint))
    while True:
        ok = Column.empty(keys.dtype, max_groups)
        omin, omax = Column.empty(values.dtype, max_groups), Column.empty(values.dtype, max_groups)
        ocv = Column.empty(np.int32, max_groups)
        ng = _dev_i64()
        _run(_lib.gx_groupby_min_max, keys.gx, keys.data_ptr, keys.mask_ptr if keys.has_nulls() else None,
             values.gx, values.data_ptr, values.mask_ptr if values.has_nulls() else None, n, max_groups,
             ok.data_ptr, omin.data_ptr, omax.data_ptr, ocv.data_ptr, ptr(ng))
        g = int(ng.item())
        if 0 <= g <= max_groups:
            break
        if max_groups >= n:
            raise RuntimeError("groupby table overflow")
        max_groups = min(n, max_groups * 8)
    for c in (ok, omin, omax, ocv):
        c.size = g
    return ok, omin, omax, ocv


def _sum_dtype(dt) -> np.dtype:
    return np.dtype(dt if np.dtype(dt).kind == "f" else np.int64)


def groupby_var_std(keys: Column, values: Column, ddof: int = 1):
    """groupby VARIANCE / STD / M2: VAR = M2/(count - ddof), STD = sqrt(VAR) (src/groupby/common/m2_var_std.cu:44-61,153-190).
    Integer values, the way the reference's hash path computes them: SUM, COUNT_VALID and SUM_OF_SQUARES per group in
    wrapping int64, then M2 = sum_sqr - sum^2/count in double (within 8 * 2^-53 * sum_sqr while sum_sqr < 2^53).
    Float values (FLOAT32 is cast to FLOAT64 first): a shifted two-pass, since that formula cancels -- mean = SUM / COUNT_VALID,
    then M2 = the group sums of (x - mean[group of the row])^2 (gx_square_centered over a row -> group lookup).  With u = 2^-53:
    |M2 - exact| <= 16u * exact + 64u^2 * sum x^2, M2 >= 0 and VAR >= 0, STD is never NaN for finite values, and a group holding
    a NaN or an infinity gives a valid NaN for all three.
    Returns (keys, var, std, m2, count_valid) with the groups in ascending key order; var / std are null where
    count - ddof <= 0, m2 of a group without a valid value is 0."""
    n = keys.size
    centred = values.dtype.kind == "f"
    if centred and values.dtype != np.float64:
        values = cast(values, np.float64)
    k, s, cv, _ = groupby_sum_count(keys, values)
    sq = Column(device_bytes(n * _sum_dtype(values.dtype).itemsize), _sum_dtype(values.dtype), n, values.mask,
                values.null_count)
    if centred:
        mean = Column.empty(np.float64, k.size)
        L.check(_lib.gx_mean_from_sum(s.gx, s.data_ptr, cv.data_ptr, k.size, mean.data_ptr, stream_ptr()), "gx_mean_from_sum")
        gid = HashJoin(k).lookup(keys)  # row -> position of its key in k (negative for null keys)
        L.check(_lib.gx_square_centered(values.data_ptr, gid.data_ptr, mean.data_ptr, n, k.size, sq.data_ptr, stream_ptr()),
                "gx_square_centered")
    else:
        L.check(_lib.gx_square(values.gx, values.data_ptr, n, sq.data_ptr, stream_ptr()), "gx_square")
    k2, ss, _, _ = groupby_sum_count(keys, sq)
    o1, o2 = sorted_order(k), sorted_order(k2)  # the two hash passes emit the groups in their own orders
    k, s, cv, ss = gather(k, o1), gather(s, o1), gather(cv, o1), gather(ss, o2)
    g = k.size
    outs = []
    for mode in (1, 2, 0):
        o = Column.empty(np.float64, g, nullable=True)
        cnt = _dev_i64()
        L.check(_lib.gx_var_from_sums(s.gx, ss.data_ptr, None if centred else s.data_ptr, cv.data_ptr, g, int(ddof), mode, o.data_ptr,
                                      o.mask_ptr, ptr(cnt), stream_ptr()), "gx_var_from_sums")
        o.null_count = int(cnt.item())
        outs.append(o)
    return k, outs[0], outs[1], outs[2], cv


def groupby_argmin_argmax(keys: Column, values: Column):
    """groupby ARGMIN / ARGMAX: (keys, argmin, argmax, count_valid); the row index (INT32) of each group's
    MIN / MAX value -- the smallest such row on ties; meaningful where count_valid > 0."""
    k, mn, mx, cv = groupby_min_max(keys, values)
    g = k.size
    amin, amax = Column.empty(np.int32, g), Column.empty(np.int32, g)
    if g == 0:
        return k, amin, amax, cv
    gid = HashJoin(k).lookup(keys)  # row -> position of its key in k (negative for null keys)
    valid = values.mask_ptr if values.has_nulls() else None
    for target, out in ((mn, amin), (mx, amax)):
        L.check(_lib.gx_groupby_arg_select(values.gx, values.data_ptr, valid, gid.data_ptr, keys.size, target.data_ptr, g,
                                           out.data_ptr, stream_ptr()), "gx_groupby_arg_select")
    return k, amin, amax, cv


def groupby_scan(sorted_keys: Column, values: Column, op: str = "sum") -> Column:
    """Segmented inclusive scan over already-sorted keys (groupby::scan's value pass)."""
    opc = {"sum": L.OP_SUM, "min": L.OP_MIN, "max": L.OP_MAX}[op]
    out_dt = (np.int64 if values.dtype.kind in "iub" else values.dtype) if op == "sum" else values.dtype
    out = Column.empty(out_dt, values.size)
    _run(_lib.gx_segmented_scan, sorted_keys.gx, sorted_keys.data_ptr, values.gx, values.data_ptr,
         values.mask_ptr if values.has_nulls() else None, values.size, opc, out.data_ptr)
    return out


# ------------------------------------------------------------------------------------------------
# reduce / scan  (cudf::reduce / cudf::scan: reduction.hpp:60-65,229-235)
# ------------------------------------------------------------------------------------------------
_OPS = {"sum": L.OP_SUM, "product": L.OP_PRODUCT, "min": L.OP_MIN, "max": L.OP_MAX}


def reduce(col: Column, op: str, out_dtype=None):
    """cudf::reduce -> (python scalar, is_valid).  Invalid iff no valid element
    (reductions.cpp; simple.cuh:47-85)."""
    if out_dtype is None:
        if op in ("sum", "product"):
            out_dtype = np.float64 if col.dtype.kind == "f" else (np.uint64 if col.dtype.kind == "u" else np.int64)
        else:
            out_dtype = col.dtype
    out_dtype = np.dtype(out_dtype)
    out = Column.empty(out_dtype, 1)
    cnt = _dev_i64()
    _run(_lib.gx_reduce, col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, col.size, _OPS[op],
         gx_dtype(out_dtype), out.data_ptr, ptr(cnt))
    valid = int(cnt.item()) > 0
    return out.to_numpy()[0], valid


def scan(col: Column, op: str = "sum", inclusive: bool = True, null_include: bool = False) -> Column:
    """cudf::scan; output dtype == input dtype; mask handling of scan_inclusive.cu:198-216."""
    out = Column.empty(col.dtype, col.size)
    valid = col.mask_ptr if col.has_nulls() else None
    _run(_lib.gx_scan, col.gx, col.data_ptr, valid, col.size, _OPS[op], int(inclusive), out.data_ptr)
    if col.mask is not None:  # nullable input -> nullable output, even when no bit happens to be 0
        if null_include:  # everything from the first null on is null (mask_scan :36-61)
            pos = _dev_i64()
            L.check(_lib.gx_bitmask_first_unset(col.mask_ptr, col.size, ptr(pos), stream_ptr()), "first_unset")
            first = min(col.size, int(pos.item()) + (0 if inclusive else 1)) if col.has_nulls() else col.size
            out.mask = torch.zeros(bitmask_words(col.size), dtype=torch.int32, device="cuda")
            L.check(_lib.gx_bitmask_set(ptr(out.mask), 0, first, 1, stream_ptr()), "bitmask_set")
            out.null_count = col.size - first
        else:
            out.mask = col.mask.clone()
            out.null_count = col.null_count
    return out


# ------------------------------------------------------------------------------------------------
# stream compaction  (cudf::apply_boolean_mask / drop_nulls / drop_nans: stream_compaction.hpp; pylibcudf/stream_compaction.pyx)
# A selector writes the plan (one bit per row + chunk starts, gx_compact.hip) and the number of selected rows; every column of
# the table is then compacted from that one plan.  Host reads per call: the count, and once the null counts of all outputs.
# ------------------------------------------------------------------------------------------------

_CMP = {"eq": L.CMP_EQ, "==": L.CMP_EQ, "ne": L.CMP_NE, "!=": L.CMP_NE, "lt": L.CMP_LT, "<": L.CMP_LT,
        "le": L.CMP_LE, "<=": L.CMP_LE, "gt": L.CMP_GT, ">": L.CMP_GT, "ge": L.CMP_GE, ">=": L.CMP_GE}


def _copy_column(col: Column) -> Column:
    out = Column(col.data.clone(), col.dtype, col.size)
    if col.mask is not None:
        out.mask, out.null_count = col.mask.clone(), col.null_count
    return out


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*[p.value if isinstance(p, ctypes.c_void_p) else p for p in ptrs])


def _select_mask(mask: Column):
    """(plan, selected rows) of a BOOL8 mask column: a row is kept where the mask is valid and non-zero"""
    if mask.dtype != np.bool_:
        raise TypeError("Mask must be Boolean type")            # apply_boolean_mask.cu: "Mask must be Boolean type"
    cnt = _dev_i64()
    plan = _run(_lib.gx_select_mask, mask.data_ptr, mask.mask_ptr, 0, mask.size, ptr(cnt))
    return plan, int(cnt.item())


def _compact(cols: Sequence[Column], plan: torch.Tensor, n: int, count: int) -> List[Column]:
    """every column compacted from one plan; a column whose output holds no null comes back without a mask"""
    if count == 0:
        return [Column.empty(c.dtype, 0) for c in cols]
    outs = []
    nulls = torch.zeros(max(len(cols), 1), dtype=torch.int64, device="cuda")
    for k, c in enumerate(cols):
        out = Column.empty(c.dtype, count, nullable=c.mask is not None)
        L.check(_lib.gx_compact_column(c.dtype.itemsize, c.data_ptr, c.mask_ptr, 0, n, ptr(plan), out.data_ptr, out.mask_ptr,
                                       ctypes.c_void_p(nulls.data_ptr() + 8 * k), stream_ptr()), "gx_compact_column")
        outs.append(out)
    if any(c.mask is not None for c in cols):
        host = nulls.cpu().numpy()
        for k, out in enumerate(outs):
            if out.mask is not None:
                out.null_count = int(host[k])
                if out.null_count == 0:
                    out.mask = None
    return outs


def apply_boolean_mask(cols: Sequence[Column], mask: Column) -> List[Column]:
    """cudf::apply_boolean_mask: the rows of the table `cols` where `mask` is true, in row order; a null mask element drops its row."""
    cols = list(cols)
    if mask.dtype != np.bool_:
        raise TypeError("Mask must be Boolean type")
    for c in cols:
        if c.size != mask.size:
            raise ValueError("Column size mismatch")            # apply_boolean_mask.cu: "Column size mismatch"
    if mask.size == 0 or not cols:
        return [_copy_column(c) for c in cols]
    plan, count = _select_mask(mask)
    return _compact(cols, plan, mask.size, count)


def selected_rows(mask: Column) -> Column:
    """the ascending row numbers at which `mask` is true (INT32): the gather map of the selection, np.flatnonzero on the device"""
    if mask.size == 0:
        if mask.dtype != np.bool_:
            raise TypeError("Mask must be Boolean type")
        return Column.empty(np.int32, 0)
    plan, count = _select_mask(mask)
    out = Column.empty(np.int32, count)
    L.check(_lib.gx_compact_indices(mask.size, ptr(plan), out.data_ptr, stream_ptr()), "gx_compact_indices")
    return out


def _keys_of(cols: Sequence[Column], keys: Sequence[int]) -> List[Column]:
    for k in keys:
        if not 0 <= int(k) < len(cols):
            raise IndexError("key column index out of range")   # table_view::select -> std::out_of_range
    if len(keys) > 32:
        raise ValueError("at most 32 key columns")
    return [cols[int(k)] for k in keys]


def drop_nulls(cols: Sequence[Column], keys: Sequence[int], keep_threshold: Optional[int] = None) -> List[Column]:
    """cudf::drop_nulls: the rows with at least keep_threshold (default: all) valid elements among the key columns cols[k], k in
    keys.  Keys without any null return a copy of the input whatever the threshold (drop_nulls.cu)."""
    cols = list(cols)
    kc = _keys_of(cols, keys)
    thr = len(kc) if keep_threshold is None else int(keep_threshold)
    if thr < 0:
        raise ValueError("keep_threshold must not be negative")
    n = cols[0].size if cols else 0
    if n == 0 or not kc or not any(c.has_nulls() for c in kc):
        return [_copy_column(c) for c in cols]
    valids = _ptr_array([c.mask_ptr if c.has_nulls() else None for c in kc])
    cnt = _dev_i64()
    plan = _run(_lib.gx_select_valid_count, len(kc), valids, None, n, thr, ptr(cnt))
    return _compact(cols, plan, n, int(cnt.item()))


def _select_not_nan(kc: Sequence[Column], n: int, thr: int, null_is_missing: bool):
    dts = (ctypes.c_int * len(kc))(*[c.gx for c in kc])
    datas = _ptr_array([c.data_ptr for c in kc])
    valids = _ptr_array([c.mask_ptr if c.has_nulls() else None for c in kc])
    cnt = _dev_i64()
    plan = _run(_lib.gx_select_not_nan, len(kc), dts, datas, valids, None, n, thr, int(null_is_missing), ptr(cnt))
    return plan, int(cnt.item())


def drop_nans(cols: Sequence[Column], keys: Sequence[int], keep_threshold: Optional[int] = None) -> List[Column]:
    """cudf::drop_nans: the rows with at least keep_threshold (default: all) non-NaN elements among the FLOAT32 / FLOAT64 key
    columns; a null element is not a NaN."""
    cols = list(cols)
    kc = _keys_of(cols, keys)
    for c in kc:
        if c.dtype.kind != "f" or c.dtype.itemsize not in (4, 8):
            raise TypeError("Key column is not of floating-point type")    # drop_nans.cu
    thr = len(kc) if keep_threshold is None else int(keep_threshold)
    if thr < 0:
        raise ValueError("keep_threshold must not be negative")
    n = cols[0].size if cols else 0
    if n == 0 or not kc:
        return [_copy_column(c) for c in cols]
    plan, count = _select_not_nan(kc, n, thr, False)
    return _compact(cols, plan, n, count)


def dropna_rows(cols: Sequence[Column], keys: Sequence[int], keep_threshold: int) -> List[Column]:
    """pandas' dropna on a table: the rows with at least keep_threshold elements among the key columns that are neither null nor NaN"""
    cols = list(cols)
    kc = _keys_of(cols, keys)
    n = cols[0].size if cols else 0
    if n == 0 or not kc or not any(c.has_nulls() or c.dtype.kind == "f" for c in kc):
        if kc and n and keep_threshold > len(kc):
            plan, count = _select_not_nan(kc, n, keep_threshold, True)   # nothing can reach the threshold: every row goes
            return _compact(cols, plan, n, count)
        return [_copy_column(c) for c in cols]
    plan, count = _select_not_nan(kc, n, keep_threshold, True)
    return _compact(cols, plan, n, count)


# ---- deduplication (cudf::unique / distinct / stable_distinct / distinct_indices / unique_count / distinct_count: stream_compaction.hpp).
# Two more selectors (gx_distinct.hip): unique compares neighbouring rows, distinct reduces over a lock-free table of row indices.
# Their scratch STARTS with the plan, so _compact / gx_compact_indices take it as it is.

_KEEP = {"any": L.KEEP_ANY, "first": L.KEEP_FIRST, "last": L.KEEP_LAST, "none": L.KEEP_NONE}
_F_NULLS_EQUAL, _F_NANS_EQUAL, _F_NAN_IS_NULL, _F_DROP_NULL_ROWS = 1, 2, 4, 8


def _keep_code(keep: str) -> int:
    if keep not in _KEEP:
        raise ValueError(f"keep must be one of any / first / last / none, not {keep!r}")
    return _KEEP[keep]


def _select_dedup(fn, kc: Sequence[Column], n: int, keep: int, flags: int):
    """(scratch that starts with the plan, selected rows) of gx_select_unique / gx_select_distinct over the key columns kc"""
    if not 1 <= len(kc) <= 32:
        raise ValueError("1 to 32 key columns")
    dts = (ctypes.c_int * len(kc))(*[c.gx for c in kc])
    datas = _ptr_array([c.data_ptr for c in kc])
    valids = _ptr_array([c.mask_ptr if c.has_nulls() else None for c in kc])
    cnt = _dev_i64()
    plan = _run(fn, len(kc), dts, datas, valids, None, n, keep, flags, ptr(cnt))
    return plan, int(cnt.item())


def _dedup(fn, cols: Sequence[Column], keys: Sequence[int], keep: str, flags: int) -> List[Column]:
    cols = list(cols)
    code = _keep_code(keep)
    kc = _keys_of(cols, keys)
    n = cols[0].size if cols else 0
    if n == 0 or not kc:
        return [_copy_column(c) for c in cols]
    plan, count = _select_dedup(fn, kc, n, code, flags)
    return _compact(cols, plan, n, count)


def unique(cols: Sequence[Column], keys: Sequence[int], keep: str = "any", nulls_equal: bool = True) -> List[Column]:
    """cudf::unique: runs of CONSECUTIVE rows that are equal in the key columns cols[k], k in keys, collapse to their first row
    (keep = "first" / "any"), their last ("last"), or vanish unless they are one row long ("none").  Row order is kept; NaNs compare
    equal, -0.0 == +0.0; nulls compare equal unless nulls_equal is False (then a row holding a null equals no row)."""
    return _dedup(_lib.gx_select_unique, cols, keys, keep, (_F_NULLS_EQUAL if nulls_equal else 0) | _F_NANS_EQUAL)


def distinct(cols: Sequence[Column], keys: Sequence[int], keep: str = "any", nulls_equal: bool = True,
             nans_equal: bool = True) -> List[Column]:
    """cudf::distinct == cudf::stable_distinct here: one row per set of rows that are equal in the key columns -- the first of the
    set ("first"), the last ("last"), whichever ("any"), or only the rows without a duplicate ("none") -- in INPUT ORDER (the
    reference leaves distinct's order open).  A row holding a null (a NaN) with nulls_equal (nans_equal) False equals no row and
    is always kept."""
    return _dedup(_lib.gx_select_distinct, cols, keys, keep,
                  (_F_NULLS_EQUAL if nulls_equal else 0) | (_F_NANS_EQUAL if nans_equal else 0))


stable_distinct = distinct


def distinct_indices(key_cols: Sequence[Column], keep: str = "any", nulls_equal: bool = True, nans_equal: bool = True) -> Column:
    """cudf::distinct_indices: the row numbers distinct() keeps when every column of the table is a key (INT32, ascending)"""
    kc = list(key_cols)
    code = _keep_code(keep)
    n = kc[0].size if kc else 0
    if n == 0:
        return Column.empty(np.int32, 0)
    plan, count = _select_dedup(_lib.gx_select_distinct, kc, n, code,
                                (_F_NULLS_EQUAL if nulls_equal else 0) | (_F_NANS_EQUAL if nans_equal else 0))
    out = Column.empty(np.int32, count)
    L.check(_lib.gx_compact_indices(n, ptr(plan), out.data_ptr, stream_ptr()), "gx_compact_indices")
    return out


def _dedup_count(fn, cols_or_col, nulls_equal: bool, null_policy: Optional[str], nan_policy: Optional[str]) -> int:
    """table form (a sequence of key columns): nulls_equal decides, NaNs are equal.  Column form (one Column): null_policy "include"
    / "exclude" and nan_policy "valid" (all NaNs one value) / "null" (a NaN is a null element).  The count word alone is read."""
    if isinstance(cols_or_col, Column):
        np_, nn = null_policy or "include", nan_policy or "valid"
        if np_ not in ("include", "exclude") or nn not in ("valid", "null"):
            raise ValueError("null_policy is include / exclude, nan_policy is valid / null")
        kc = [cols_or_col]
        flags = _F_NULLS_EQUAL | _F_NANS_EQUAL | (_F_NAN_IS_NULL if nn == "null" else 0) | (_F_DROP_NULL_ROWS if np_ == "exclude" else 0)
    else:
        if null_policy is not None or nan_policy is not None:
            raise TypeError("null_policy / nan_policy belong to the column form")
        kc = list(cols_or_col)
        flags = (_F_NULLS_EQUAL if nulls_equal else 0) | _F_NANS_EQUAL
    n = kc[0].size if kc else 0
    if n == 0:
        return 0
    return _select_dedup(fn, kc, n, L.KEEP_ANY, flags)[1]


def distinct_count(cols_or_col, nulls_equal: bool = True, null_policy: Optional[str] = None, nan_policy: Optional[str] = None) -> int:
    """cudf::distinct_count: the number of rows distinct(keep="any") would keep; nothing is compacted"""
    return _dedup_count(_lib.gx_select_distinct, cols_or_col, nulls_equal, null_policy, nan_policy)


def unique_count(cols_or_col, nulls_equal: bool = True, null_policy: Optional[str] = None, nan_policy: Optional[str] = None) -> int:
    """cudf::unique_count: the number of runs of consecutive equal rows.  Column form with null_policy "exclude": a null row is not
    counted, but a row is still compared with the physically previous one ([1, null, 1] -> 2)."""
    return _dedup_count(_lib.gx_select_unique, cols_or_col, nulls_equal, null_policy, nan_policy)


# ---- merging and searching sorted rows (cudf::merge, cudf::lower_bound / upper_bound: merge.hpp, search.hpp; gx_merge.hip).
# The row order is the one of the multi-column sorts: one direction and one null placement per key column.

def _per_key(value, k: int, what: str) -> List[bool]:
    if isinstance(value, (bool, np.bool_)):
        return [bool(value)] * k
    v = [bool(x) for x in value]
    if len(v) != k:
        raise ValueError(f"{what}: one entry per key column")
    return v


def _order_args(k: int, ascending, null_before):
    asc, nb = _per_key(ascending, k, "ascending"), _per_key(null_before, k, "null_before")
    return (ctypes.c_int * k)(*[0 if a else 1 for a in asc]), (ctypes.c_int * k)(*[1 if b else 0 for b in nb])


def _key_side(cols: Sequence[Column]):
    """the host arrays of one side of key columns: data pointers, validity pointers (None = no nulls), rows"""
    n = cols[0].size
    for c in cols:
        if c.size != n:
            raise ValueError("Column size mismatch")
    return _ptr_array([c.data_ptr for c in cols]), _ptr_array([c.mask_ptr if c.has_nulls() else None for c in cols]), n


def _two_sides(x: Sequence[Column], y: Sequence[Column], what: str):
    x, y = list(x), list(y)
    if not 1 <= len(x) <= 32:
        raise ValueError(f"{what}: 1 to 32 key columns")
    if len(x) != len(y) or any(a.dtype != b.dtype for a, b in zip(x, y)):
        raise TypeError(f"{what}: the column counts or types of the two tables differ")
    return x, y, (ctypes.c_int * len(x))(*[c.gx for c in x])


def merge_order(a_keys: Sequence[Column], b_keys: Sequence[Column], ascending=True, null_before=True) -> Column:
    """The map of the stable merge of two sorted key tables (INT32, len(a) + len(b) entries): an entry < len(a) is a row of a, otherwise
    len(a) + a row of b; among equivalent rows a's come first.  Both sides must be sorted under (ascending, null_before)."""
    a, b, dts = _two_sides(a_keys, b_keys, "merge_order")
    desc, nbf = _order_args(len(a), ascending, null_before)
    ad, av, na = _key_side(a)
    bd, bv, nb = _key_side(b)
    if na + nb > 2**31 - 1:
        raise OverflowError("the merged row count exceeds cudf::size_type")
    out = Column.empty(np.int32, na + nb)
    if na + nb:
        _run(_lib.gx_merge_order, len(a), dts, ad, av, None, na, bd, bv, None, nb, desc, nbf, out.data_ptr)
    return out


def _gather2(a: Column, b: Column, gmap: Column, nulls: torch.Tensor, k: int) -> Column:
    nullable = a.has_nulls() or b.has_nulls()
    out = Column.empty(a.dtype, gmap.size, nullable=nullable)
    L.check(_lib.gx_gather2(a.dtype.itemsize, a.data_ptr, a.mask_ptr if a.has_nulls() else None, 0, a.size, b.data_ptr,
                            b.mask_ptr if b.has_nulls() else None, 0, b.size, gmap.data_ptr, gmap.size, out.data_ptr, out.mask_ptr,
                            ctypes.c_void_p(nulls.data_ptr() + 8 * k), stream_ptr()), "gx_gather2")
    return out


def _merge_two(a: List[Column], b: List[Column], keys: Sequence[int], ascending, null_before) -> List[Column]:
    gmap = merge_order([a[k] for k in keys], [b[k] for k in keys], ascending, null_before)
    nulls = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    outs = [_gather2(x, y, gmap, nulls, k) for k, (x, y) in enumerate(zip(a, b))]
    if any(o.mask is not None for o in outs):
        host = nulls.cpu().numpy()
        for k, o in enumerate(outs):
            if o.mask is not None:
                o.null_count = int(host[k])
                if o.null_count == 0:
                    o.mask = None
    return outs


def merge_sorted(tables: Sequence[Sequence[Column]], keys: Sequence[int], ascending=True, null_before=True) -> List[Column]:
    """cudf::merge: the tables (each a list of columns, each sorted on the key columns cols[k], k in keys, under one direction and one
    null placement per key) merged into one sorted table.  Stable: rows that compare equivalent come out by (table index, row).
    Several tables merge as a balanced tree over NEIGHBOURING tables, which keeps that order."""
    tables = [list(t) for t in tables]
    if not tables:
        return []
    ncols = len(tables[0])
    if ncols == 0:
        return []
    for t in tables:
        if len(t) != ncols or any(x.dtype != y.dtype for x, y in zip(t, tables[0])):
            raise TypeError("merge_sorted: the column counts or types of the tables differ")
    if not keys:
        raise ValueError("merge_sorted: no key columns")
    if len(keys) > ncols:
        raise ValueError("merge_sorted: more keys than columns")
    _keys_of(tables[0], keys)
    _order_args(len(keys), ascending, null_before)
    if sum(t[0].size for t in tables if t) > 2**31 - 1:
        raise OverflowError("the merged row count exceeds cudf::size_type")
    level = [t for t in tables if t[0].size > 0]      # (empty tables add nothing; the others keep their relative order)
    if len(level) <= 1:                               # a copy; like a merged column, one without nulls carries no mask
        return [_copy_column(c) if c.has_nulls() else Column(c.data.clone(), c.dtype, c.size) for c in (level[0] if level else tables[0])]
    while len(level) > 1:
        nxt = [_merge_two(level[i], level[i + 1], keys, ascending, null_before) for i in range(0, len(level) - 1, 2)]
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def _bounds(haystack: Sequence[Column], needles: Sequence[Column], ascending, null_before, upper: bool) -> Column:
    h, x, dts = _two_sides(haystack, needles, "upper_bound" if upper else "lower_bound")
    desc, nbf = _order_args(len(h), ascending, null_before)
    hd, hv, nh = _key_side(h)
    xd, xv, nx = _key_side(x)
    out = Column.empty(np.int32, nx)
    if nx:
        L.check(_lib.gx_search_bounds(len(h), dts, hd, hv, None, nh, xd, xv, None, nx, desc, nbf, int(upper), out.data_ptr, stream_ptr()),
                "gx_search_bounds")
    return out


def lower_bound(haystack_cols: Sequence[Column], needle_cols: Sequence[Column], ascending=True, null_before=True) -> Column:
    """cudf::lower_bound: for every needle row the number of haystack rows that compare strictly less (INT32): the first insertion
    point that keeps the haystack, sorted under (ascending, null_before), sorted."""
    return _bounds(haystack_cols, needle_cols, ascending, null_before, False)


def upper_bound(haystack_cols: Sequence[Column], needle_cols: Sequence[Column], ascending=True, null_before=True) -> Column:
    """cudf::upper_bound: the number of haystack rows that compare less than or equal: the last such insertion point."""
    return _bounds(haystack_cols, needle_cols, ascending, null_before, True)


# ------------------------------------------------------------------------------------------------
# rolling windows  (cudf::rolling_window / grouped_rolling_window: include/cudf/rolling.hpp)
# ------------------------------------------------------------------------------------------------

_ROLLING_OPS = {"sum": L.OP_SUM, "min": L.OP_MIN, "max": L.OP_MAX, "mean": L.OP_MEAN, "count_valid": L.OP_COUNT_VALID,
                "count_all": L.OP_COUNT_ALL}


def _rolling_out_dtype(dt: np.dtype, op: str) -> np.dtype:
    if op in ("count_valid", "count_all"):
        return np.dtype(np.int32)
    if op == "mean":
        return np.dtype(np.float64)
    if op == "sum" and dt.kind != "f":
        return np.dtype(np.uint64 if dt == np.uint64 else np.int64)
    return dt


def group_runs(key_cols: Sequence[Column]):
    """(labels, offsets) of the runs of equal key rows, as gx_group_offsets writes them: gx_group_heads per key column (nulls equal
    to nulls, NaNs to NaNs), ORed together."""
    n = key_cols[0].size
    heads = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    for k, c in enumerate(key_cols):
        if c.size != n:
            raise ValueError("group keys of different lengths")
        L.check(_lib.gx_group_heads(c.gx, c.data_ptr, c.mask_ptr if c.has_nulls() else None, None, n, int(k > 0), ptr(heads), stream_ptr()),
                "gx_group_heads")
    labels = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    _run(_lib.gx_group_offsets, ptr(heads), n, ptr(labels), ptr(offsets), None, ptr(_dev_i64()))
    return labels, offsets


def rolling_window(col: Column, preceding, following, min_periods: int, op: str, group_keys: Optional[Sequence[Column]] = None) -> Column:
    """cudf::rolling_window / grouped_rolling_window: op ("sum", "min", "max", "mean", "count_valid", "count_all") over the rows
    [i - preceding + 1, i + following] of every row i (preceding counts the row itself), cut to the column or, with group_keys (a
    sequence of key Columns: groups are runs of equal key rows), to the row's group.  preceding / following: two ints, or two INT32
    Columns without nulls (one window per row).  A value is valid iff its window holds max(min_periods, 1) valid values, a count iff
    its window has min_periods rows (include/cudf_amd/gx.h); the mask is kept only when a row is null."""
    if op not in _ROLLING_OPS:
        raise ValueError(f"rolling_window: unsupported aggregation {op!r}")
    if min_periods < 0:
        raise ValueError("min_periods must be non-negative")
    per_row = isinstance(preceding, Column) or isinstance(following, Column)
    if per_row:
        if group_keys:
            raise ValueError("rolling_window: per-row windows and group keys do not combine")
        for w in (preceding, following):
            if not isinstance(w, Column) or w.dtype != np.int32 or w.mask is not None or w.size != col.size:
                raise ValueError("rolling_window: window columns must be INT32 Columns without a mask, one row per input row")
    if col.dtype not in (np.dtype(t) for t in ("i1", "i2", "i4", "i8", "u1", "u2", "u4", "u8", "f4", "f8", "bool")):
        raise TypeError(f"unsupported dtype {col.dtype}")
    n = col.size
    out = Column.empty(_rolling_out_dtype(col.dtype, op), n, nullable=True)
    if n == 0:
        out.mask = None
        return out
    labels = offsets = None
    if group_keys:
        for c in group_keys:
            if c.size != n:
                raise ValueError("rolling_window: the group keys must have one row per input row")
        labels, offsets = group_runs(list(group_keys))
    nulls = _dev_i64()
    L.check(_lib.gx_rolling_window(col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, 0, n,
                                   0 if per_row else int(preceding), 0 if per_row else int(following),
                                   preceding.data_ptr if per_row else None, following.data_ptr if per_row else None,
                                   ptr(labels), ptr(offsets), int(min_periods), _ROLLING_OPS[op], out.data_ptr, out.mask_ptr, ptr(nulls),
                                   stream_ptr()), "gx_rolling_window")
    k = int(nulls.item())
    if k:
        out.null_count = k
    else:
        out.mask = None
    return out


# ------------------------------------------------------------------------------------------------
# row movement  (cudf::concatenate: include/cudf/concatenate.hpp; scatter / copy_if_else: include/cudf/copying.hpp)
# ------------------------------------------------------------------------------------------------

def concatenate(cols: Sequence[Column]) -> Column:
    """cudf::concatenate: the rows of cols[0], then cols[1], ... in ONE launch (gx_concatenate: data, validity words and any
    number of inputs).  The result has a mask only if an input has nulls; its null count is the sum of the inputs'."""
    cols = list(cols)
    if not cols:
        raise ValueError("concatenate: no columns")
    dt = cols[0].dtype
    gx_dtype(dt)
    for c in cols:
        if c.dtype != dt:
            raise TypeError("Type mismatch in columns to concatenate.")
    n = sum(c.size for c in cols)
    if n > 2**31 - 1:
        raise OverflowError("Total number of concatenated rows exceeds the column size limit")
    with_mask = any(c.has_nulls() for c in cols)
    out = Column.empty(dt, n, nullable=with_mask and n > 0)
    if n == 0:
        return out
    k = len(cols)
    ptrs = (ctypes.c_void_p * k)(*[c.data.data_ptr() for c in cols])
    rows = (ctypes.c_int64 * k)(*[c.size for c in cols])
    valid = (ctypes.c_void_p * k)(*[c.mask.data_ptr() if c.has_nulls() else None for c in cols])
    _run(_lib.gx_concatenate, dt.itemsize, k, ptrs, rows, valid, None, out.data_ptr, out.mask_ptr, None)
    if with_mask:
        out.null_count = sum(c.null_count for c in cols)
    return out


def concatenate_tables(tables: Sequence[Sequence[Column]]) -> List[Column]:
    """cudf::concatenate of tables (each a sequence of Columns): column by column"""
    tables = [list(t) for t in tables]
    if not tables:
        raise ValueError("concatenate: no tables")
    nc = len(tables[0])
    for t in tables:
        if len(t) != nc:
            raise ValueError("Mismatch in table columns to concatenate.")
        if len({c.size for c in t}) > 1:
            raise ValueError("Column size mismatch")
    for k in range(nc):
        for t in tables:
            if t[k].dtype != tables[0][k].dtype:
                raise TypeError("Type mismatch in columns to concatenate.")
    return [concatenate([t[k] for t in tables]) for k in range(nc)]


def _check_scatter_map(m: Column, what: str):
    if not isinstance(m, Column) or m.dtype != np.int32:
        raise TypeError(f"{what} must be an INT32 Column")
    if m.mask is not None:
        raise ValueError(f"{what} contains nulls")


def _scatter_into(target: Column, src_ptr, src_mask_ptr, scalar_valid, is_scalar: bool, src_may_be_null: bool, smap: Column) -> Column:
    """a copy of `target` with the rows of smap written in place by gx_scatter; the mask is kept only when a row ends up null"""
    n = target.size
    out = Column(target.data.clone(), target.dtype, n)
    if target.has_nulls() or src_may_be_null:
        out.mask = target.mask.clone() if target.has_nulls() else torch.full((bitmask_words(n),), -1, dtype=torch.int32, device="cuda")
    if smap.size:
        L.check(_lib.gx_scatter(target.dtype.itemsize, src_ptr, src_mask_ptr, 0, ptr(scalar_valid), int(is_scalar), smap.data_ptr, smap.size,
                                out.data_ptr, out.mask_ptr, n, stream_ptr()), "gx_scatter")
    if out.mask is not None:
        out.null_count = n - bitmask_count(out.mask, n)
        if out.null_count == 0:
            out.mask = None
    return out


def scatter(source_cols: Sequence[Column], scatter_map: Column, target_cols: Sequence[Column]) -> List[Column]:
    """cudf::scatter: copies of the target columns with target[scatter_map[i]] = source[i]; a negative index counts from the end,
    indices outside [-n, n) are undefined behaviour (not checked).  scatter_map: an INT32 Column without a mask, no longer than the
    source.  A map that repeats a row leaves it with one of its candidates."""
    source_cols, target_cols = list(source_cols), list(target_cols)
    if len(source_cols) != len(target_cols):
        raise ValueError("Number of columns in source and target not equal")
    _check_scatter_map(scatter_map, "scatter_map")
    for s, t in zip(source_cols, target_cols):
        if s.dtype != t.dtype:
            raise TypeError("Column types do not match between source and target")
        gx_dtype(t.dtype)
        if scatter_map.size > s.size:
            raise ValueError("Size of scatter map must be equal to or less than source rows")
    if len({t.size for t in target_cols}) > 1 or len({s.size for s in source_cols}) > 1:
        raise ValueError("Column size mismatch")
    return [_scatter_into(t, s.data_ptr, s.mask_ptr if s.has_nulls() else None, None, False, s.has_nulls(), scatter_map)
            for s, t in zip(source_cols, target_cols)]


def _device_scalar(value, dt: np.dtype, valid: bool = True):
    """(one element of dt, its validity byte) in device memory, as cudf::scalar keeps them; None is the invalid scalar (value 0); an
    invalid scalar with a value keeps it, as the reference's does"""
    host = np.zeros(1, dtype=dt)
    if value is not None:
        host[0] = value                      # numpy raises OverflowError for an integer the dtype cannot hold
        if dt.kind in "iub" and host[0] != value:
            raise TypeError(f"{value!r} is not representable as {dt}")
    ok = int(valid and value is not None)
    return torch.from_numpy(host.view(np.uint8).copy()).cuda(), torch.full((1,), ok, dtype=torch.uint8, device="cuda")


def scatter_scalar(values: Sequence, valids: Optional[Sequence[bool]], indices: Column, target_cols: Sequence[Column]) -> List[Column]:
    """cudf::scatter with one scalar per column: target[indices[i]] = values[k] in column k; valids[k] false (or values[k] None)
    writes nulls.  valids None = all valid."""
    values, target_cols = list(values), list(target_cols)
    valids = [True] * len(values) if valids is None else list(valids)
    if len(values) != len(target_cols) or len(valids) != len(values):
        raise ValueError("Number of scalars and table columns mismatch")
    _check_scatter_map(indices, "indices")
    for t in target_cols:
        gx_dtype(t.dtype)
    if len({t.size for t in target_cols}) > 1:
        raise ValueError("Column size mismatch")
    outs = []
    for v, ok, t in zip(values, valids, target_cols):
        val, vb = _device_scalar(v, t.dtype, bool(ok))
        outs.append(_scatter_into(t, ptr(val), None, vb, True, (v is None or not ok) and indices.size > 0, indices))
    return outs


def copy_if_else(lhs, rhs, mask: Column) -> Column:
    """cudf::copy_if_else: out[i] = lhs[i] where mask[i] is valid and true, else rhs[i] (a null mask element takes rhs).  lhs / rhs:
    a Column of mask.size rows, or a Python scalar (None: the invalid scalar) standing for a column of equal rows.  The validity
    of a row is the chosen side's; the mask is kept only when a row is null."""
    if not isinstance(mask, Column) or mask.dtype != np.bool_:
        raise TypeError("Boolean mask column must be of type BOOL8")
    sides = (lhs, rhs)
    cols = [s for s in sides if isinstance(s, Column)]
    if len(cols) == 2 and lhs.dtype != rhs.dtype:
        raise TypeError("Both inputs must be of the same type")
    if cols:
        dt = cols[0].dtype
    else:
        known = [s for s in sides if s is not None]
        if not known:
            raise TypeError("copy_if_else: two invalid scalars have no type")
        dt = np.asarray(known[0]).dtype
    gx_dtype(dt)
    for c in cols:
        if c.size != mask.size:
            raise ValueError("Boolean mask column must be the same size as lhs and rhs columns")
    n = mask.size
    keep = []                                # device scalars stay alive until the launch is queued
    args = []
    may_be_null = False
    for s in sides:
        if isinstance(s, Column):
            args += [s.data_ptr, s.mask_ptr if s.has_nulls() else None, 0, None, 0]
            may_be_null |= s.has_nulls()
        else:
            if n:
                val, vb = _device_scalar(s, dt)
                keep.append((val, vb))
                args += [ptr(val), None, 0, ptr(vb), 1]
            may_be_null |= s is None
    out = Column.empty(dt, n, nullable=may_be_null and n > 0)
    if n == 0:
        return out
    nulls = _dev_i64() if may_be_null else None
    L.check(_lib.gx_copy_if_else(dt.itemsize, *args, mask.data_ptr, mask.mask_ptr if mask.has_nulls() else None, 0, n, out.data_ptr,
                                 out.mask_ptr, ptr(nulls), stream_ptr()), "gx_copy_if_else")
    if may_be_null:
        out.null_count = int(nulls.item())
        if out.null_count == 0:
            out.mask = None
    return out


def compare_scalar(col: Column, op: str, value) -> Column:
    """BOOL8 column of col[i] <op> value, op in eq / ne / lt / le / gt / ge (or ==, !=, <, <=, >, >=); it shares the input's validity
    (a null row stays null).  NaN compares false except under ne.  The scalar must be representable in the column's dtype."""
    if op not in _CMP:
        raise ValueError(f"unknown comparison {op!r}")
    dt = col.dtype
    if dt.kind in "iu":
        info = np.iinfo(dt)
        if int(value) != value or not info.min <= int(value) <= info.max:
            raise OverflowError(f"{value!r} is not representable as {dt}")
        raw = np.array([int(value)], dtype=dt)
    else:
        raw = np.array([value]).astype(dt)
    sc = np.zeros(8, dtype=np.uint8)
    sc[: dt.itemsize] = raw.view(np.uint8)
    bits = int(sc.view(np.uint64)[0])
    out = Column.empty(np.bool_, col.size)
    L.check(_lib.gx_compare_scalar(col.gx, col.data_ptr, col.mask_ptr, col.size, _CMP[op], ctypes.c_uint64(bits), out.data_ptr,
                                   stream_ptr()), "gx_compare_scalar")
    if col.mask is not None:
        out.mask, out.null_count = col.mask, col.null_count
    return out


# ------------------------------------------------------------------------------------------------
# element-wise operations  (cudf::binary_operation / unary_operation / cast: binaryop.hpp, unary.hpp; gx_elementwise.hip)
# ------------------------------------------------------------------------------------------------

def _op_code(op, table, what: str) -> int:
    if isinstance(op, str):
        if op.upper() not in table:
            raise ValueError(f"unknown {what} {op!r}")
        return table[op.upper()]
    return int(op)


def binary_operation(lhs, rhs, op, out_dtype, scalar_dtype=None) -> Column:
    """cudf::binary_operation: out[i] = cast<out_dtype>(lhs[i] op rhs[i]), op a name of cudf::binary_operator ("ADD", "LESS", ...).
    One side may be a Python / NumPy scalar, or None for the invalid scalar; it is held in scalar_dtype, or else in the dtype NumPy's
    promotion gives it beside the column (np.result_type(column dtype, scalar): a Python scalar is weak; None: the column's dtype).
    The operands are converted to the common type of C++ (int32 o uint32 -> uint32, ...: include/cudf_amd/gx.h), not to NumPy's.
    A row is null where a side is (the NULL_* operators have their own rules); the mask is kept only when a row is null."""
    code = _op_code(op, L.BINOP, "binary operator")
    sides = (lhs, rhs)
    cols = [s for s in sides if isinstance(s, Column)]
    if not cols:
        raise TypeError("binary_operation: one side must be a Column")
    if len(cols) == 2 and lhs.size != rhs.size:
        raise ValueError("Column sizes don't match")
    out_dt = np.dtype(out_dtype)
    n = cols[0].size
    dts = []
    for s in sides:
        if isinstance(s, Column):
            dts.append(s.dtype)
        elif scalar_dtype is not None:
            dts.append(np.dtype(scalar_dtype))
        elif s is None:
            dts.append(cols[0].dtype)
        else:
            dts.append(np.result_type(cols[0].dtype, s))
    if not _lib.gx_binary_op_supported(code, gx_dtype(dts[0]), gx_dtype(dts[1]), gx_dtype(out_dt)):
        raise TypeError(f"binary operator {op!r} is not supported for {dts[0]} and {dts[1]}")
    keep, args = [], []                      # device scalars stay alive until the launch is queued
    may_be_null = False
    for s, dt in zip(sides, dts):
        if isinstance(s, Column):
            args += [s.gx, s.data_ptr, s.mask_ptr if s.has_nulls() else None, 0, None, 0]
            may_be_null |= s.has_nulls()
        else:
            val, vb = _device_scalar(s, dt) if n else (None, None)
            keep.append((val, vb))
            args += [gx_dtype(dt), ptr(val), None, 0, ptr(vb), 1]
            may_be_null |= s is None
    out = Column.empty(out_dt, n, nullable=may_be_null and n > 0)
    if n == 0:
        return out
    nulls = _dev_i64() if may_be_null else None
    L.check(_lib.gx_binary_op(code, *args, n, out.gx, out.data_ptr, out.mask_ptr, ptr(nulls), stream_ptr()), "gx_binary_op")
    if may_be_null:
        out.null_count = int(nulls.item())
        if out.null_count == 0:
            out.mask = None
    return out


def _share_validity(out: Column, col: Column) -> Column:
    if col.mask is not None:
        out.mask, out.null_count = col.mask, col.null_count
    return out


def unary_operation(col: Column, op) -> Column:
    """cudf::unary_operation (SQRT, CEIL, FLOOR, ABS, RINT, BIT_INVERT, NOT, NEGATE) and IS_NAN / IS_NOT_NAN: the result has the
    input's dtype (NOT and the NaN predicates: bool) and shares its validity."""
    code = _op_code(op, L.UNOP, "unary operator")
    out_dt = np.dtype(np.bool_) if code in (L.UNOP["NOT"], L.UNOP["IS_NAN"], L.UNOP["IS_NOT_NAN"]) else col.dtype
    if not _lib.gx_unary_op_supported(code, col.gx, gx_dtype(out_dt)):
        raise TypeError(f"unary operator {op!r} is not supported for {col.dtype}")
    out = Column.empty(out_dt, col.size)
    L.check(_lib.gx_unary_op(code, col.gx, col.data_ptr, col.size, out.gx, out.data_ptr, stream_ptr()), "gx_unary_op")
    return _share_validity(out, col)


def cast(col: Column, dtype) -> Column:
    """cudf::cast: static_cast of every element (to bool: x != 0; float -> integer truncates toward zero); shares the validity"""
    gx_dtype(dtype), gx_dtype(col.dtype)     # TypeError before anything is allocated
    out = Column.empty(np.dtype(dtype), col.size)
    L.check(_lib.gx_cast(col.gx, col.data_ptr, col.size, out.gx, out.data_ptr, stream_ptr()), "gx_cast")
    return _share_validity(out, col)


def _validity_as_bool(col: Column, invert: bool) -> Column:
    out = Column.empty(np.bool_, col.size)
    L.check(_lib.gx_bitmask_to_bool8(col.mask_ptr if col.has_nulls() else None, 0, col.size, int(invert), out.data_ptr, stream_ptr()),
            "gx_bitmask_to_bool8")
    return out


def is_null(col: Column) -> Column:
    """cudf::is_null: a bool column without nulls, true where the row is null"""
    return _validity_as_bool(col, True)


def is_valid(col: Column) -> Column:
    return _validity_as_bool(col, False)


def is_nan(col: Column) -> Column:
    """cudf::is_nan: a float column -> bool, true where the value is a NaN; a null row stays null"""
    return unary_operation(col, "IS_NAN")


def is_not_nan(col: Column) -> Column:
    return unary_operation(col, "IS_NOT_NAN")


# ------------------------------------------------------------------------------------------------
# expressions  (cudf::compute_column: transform.hpp, ast/expressions.hpp; gx_expression.hip)
# ------------------------------------------------------------------------------------------------

_GX2NP = {L.INT8: np.int8, L.INT16: np.int16, L.INT32: np.int32, L.INT64: np.int64, L.UINT8: np.uint8, L.UINT16: np.uint16,
          L.UINT32: np.uint32, L.UINT64: np.uint64, L.FLOAT32: np.float32, L.FLOAT64: np.float64, L.BOOL8: np.bool_}


def _expression_args(columns: Sequence[Column], expr):
    """the node array of an expression over `columns`, the table columns it reads and its literals, checked against the table"""
    from . import ast as A
    columns = list(columns)
    nodes, used, literals = A.flatten(expr)
    for i in used:
        if i >= len(columns):
            raise IndexError(f"column reference {i} is out of range for a table of {len(columns)} columns")
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    return node_arr, [columns[i] for i in used], literals


def _expression_dtype(node_arr, cols: Sequence[Column], literals) -> np.dtype:
    cd = (ctypes.c_int32 * max(len(cols), 1))(*[c.gx for c in cols])
    ld = (ctypes.c_int32 * max(len(literals), 1))(*[gx_dtype(l.dtype) for l in literals])
    rc = _lib.gx_expr_result_dtype(node_arr, len(node_arr), cd, len(cols), ld, len(literals))
    if rc == -2:
        raise TypeError("the expression has a type error: operands of different dtypes, or an operator that does not take the dtype")
    if rc <= 0:
        raise ValueError("the expression is malformed or beyond the limits of gx_expr_limits")
    return np.dtype(_GX2NP[rc])


def expression_result_dtype(columns: Sequence[Column], expr) -> np.dtype:
    """the dtype ops.compute_column gives for `expr` over `columns` (gx_expr_result_dtype): TypeError for a type error"""
    node_arr, cols, literals = _expression_args(columns, expr)
    return _expression_dtype(node_arr, cols, literals)


def compute_column(columns: Sequence[Column], expr) -> Column:
    """cudf::compute_column: the expression tree `expr` (cudf_amd.ast) over the columns of a table, in one launch and without
    intermediate columns.  A row is null where an operand of a node is (IS_NULL, NULL_EQUAL and NULL_LOGICAL_* have their own
    rules); a mask is allocated when a column the expression reads has nulls or a literal is invalid, and kept when a row is null."""
    node_arr, cols, literals = _expression_args(columns, expr)
    out_dt = _expression_dtype(node_arr, cols, literals)
    if len({c.size for c in columns}) > 1:
        raise ValueError("Column sizes don't match")
    if not len(columns):
        raise ValueError("compute_column needs a table with at least one column")
    n = columns[0].size
    may_be_null = any(c.has_nulls() for c in cols) or any(l.value is None for l in literals)
    out = Column.empty(out_dt, n, nullable=may_be_null and n > 0)
    if n == 0:
        return out
    keep = [_device_scalar(l.value, l.dtype) for l in literals]   # device scalars stay alive until the launch is queued
    col_arr = (L.ExprColumn * max(len(cols), 1))(*[L.ExprColumn(c.data.data_ptr(), c.mask.data_ptr() if c.has_nulls() else None, 0, c.gx, 0)
                                                   for c in cols])
    lit_arr = (L.ExprLiteral * max(len(literals), 1))(*[L.ExprLiteral(val.data_ptr(), vb.data_ptr(), gx_dtype(l.dtype), 0)
                                                       for l, (val, vb) in zip(literals, keep)])
    nulls = _dev_i64() if may_be_null else None
    L.check(_lib.gx_compute_column(node_arr, len(node_arr), col_arr, len(cols), lit_arr, len(literals), n, out.gx, out.data_ptr, out.mask_ptr,
                                   ptr(nulls), stream_ptr()), "gx_compute_column")
    if may_be_null:
        out.null_count = int(nulls.item())
        if out.null_count == 0:
            out.mask = None
    return out


# ------------------------------------------------------------------------------------------------
# conditional joins  (cudf::conditional_*_join: join/conditional_join.hpp; gx_conditional_join.hip)
# ------------------------------------------------------------------------------------------------
CONDITIONAL_JOIN_KINDS = {"inner": 0, "left": 1, "full": 2, "leftsemi": 3, "leftanti": 4}
JOIN_NO_MATCH = -2**31


class _ConditionalJoin:
    """the arguments of one conditional join over the C ABI: count() runs the size pass, write() the output pass"""

    def __init__(self, left_cols: Sequence[Column], right_cols: Sequence[Column], predicate, kind: str):
        from . import ast as A
        if kind not in CONDITIONAL_JOIN_KINDS:
            raise ValueError(f"unknown conditional join kind {kind!r}: one of {sorted(CONDITIONAL_JOIN_KINDS)}")
        self.kind = CONDITIONAL_JOIN_KINDS[kind]
        sides = {"left": list(left_cols), "right": list(right_cols)}
        for name, cols in sides.items():
            if len({c.size for c in cols}) > 1:
                raise ValueError(f"Column sizes of the {name} table don't match")
        self.n_left = sides["left"][0].size if sides["left"] else 0
        self.n_right = sides["right"][0].size if sides["right"] else 0
        nodes, used, self.literals = A.flatten_pair(predicate)
        for table, i in used:
            if i >= len(sides[table]):
                raise IndexError(f"column reference {i} is out of range for the {table} table of {len(sides[table])} columns")
        self.cols = [sides[table][i] for table, i in used]
        self.node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
        max_cols = ctypes.c_int(0)
        _lib.gx_expr_limits(None, ctypes.byref(max_cols), None, None)
        if len(self.cols) > max_cols.value:
            raise ValueError("the expression is malformed or beyond the limits of gx_expr_limits")
        if _expression_dtype(self.node_arr, self.cols, self.literals) != np.bool_:
            raise TypeError("the predicate of a conditional join must be a BOOL8 expression")
        self.keep = [_device_scalar(l.value, l.dtype) for l in self.literals]
        self.col_arr = (L.ExprColumn * max(len(self.cols), 1))(*[
            L.ExprColumn(c.data.data_ptr(), c.mask.data_ptr() if c.has_nulls() else None, 0, c.gx, int(table == "right"))
            for c, (table, _) in zip(self.cols, used)])
        self.lit_arr = (L.ExprLiteral * max(len(self.literals), 1))(*[L.ExprLiteral(val.data_ptr(), vb.data_ptr(), gx_dtype(l.dtype), 0)
                                                                     for l, (val, vb) in zip(self.literals, self.keep)])
        self.tmp = None

    def _head(self):
        return (self.node_arr, len(self.node_arr), self.col_arr, len(self.cols), self.lit_arr, len(self.literals), self.n_left, self.n_right,
                self.kind)

    def count(self) -> Tuple[int, int]:
        """(rows of the result, rows of its left-join part): exact in 64 bits"""
        nbytes = ctypes.c_size_t(0)
        L.check(_lib.gx_conditional_join_count(*self._head(), None, None, ctypes.byref(nbytes), stream_ptr()), "gx_conditional_join_count")
        self.tmp = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
        L.check(_lib.gx_conditional_join_count(*self._head(), ptr(sizes), ptr(self.tmp), ctypes.byref(nbytes), stream_ptr()),
                "gx_conditional_join_count")
        total, left_total = (int(v) for v in sizes.tolist())
        return total, left_total

    def write(self, total: int, left_total: int, pairs: bool):
        if total > 2**31 - 1:
            raise OverflowError(f"the conditional join has {total} rows: more than 2^31 - 1")
        out_l = Column.empty(np.int32, total)
        out_r = Column.empty(np.int32, total) if pairs else None
        L.check(_lib.gx_conditional_join_write(*self._head(), total, left_total, ptr(self.tmp), out_l.data_ptr,
                                               out_r.data_ptr if pairs else None, stream_ptr()), "gx_conditional_join_write")
        return (out_l, out_r) if pairs else out_l


def _conditional_join(left_cols, right_cols, predicate, kind: str):
    j = _ConditionalJoin(left_cols, right_cols, predicate, kind)
    total, left_total = j.count()
    return j.write(total, left_total, pairs=j.kind <= 2)


def conditional_inner_join(left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> Tuple[Column, Column]:
    """cudf::conditional_inner_join: the (left row, right row) pairs where `predicate` (cudf_amd.ast over both tables:
    ColumnReference(i, "left" / "right")) is valid and true, ascending by (left, right)."""
    return _conditional_join(left_cols, right_cols, predicate, "inner")


def conditional_left_join(left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> Tuple[Column, Column]:
    """cudf::conditional_left_join: the inner pairs, with (i, JOIN_NO_MATCH) in the place of a left row i without a match."""
    return _conditional_join(left_cols, right_cols, predicate, "left")


def conditional_full_join(left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> Tuple[Column, Column]:
    """cudf::conditional_full_join: the left join, then (JOIN_NO_MATCH, r) for the unmatched right rows, r ascending."""
    return _conditional_join(left_cols, right_cols, predicate, "full")


def conditional_left_semi_join(left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> Column:
    """cudf::conditional_left_semi_join: the left rows with at least one match, ascending."""
    return _conditional_join(left_cols, right_cols, predicate, "leftsemi")


def conditional_left_anti_join(left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> Column:
    """cudf::conditional_left_anti_join: the left rows without a match, ascending."""
    return _conditional_join(left_cols, right_cols, predicate, "leftanti")


def conditional_join_size(kind: str, left_cols: Sequence[Column], right_cols: Sequence[Column], predicate) -> int:
    """cudf::conditional_*_join_size: the rows the join of `kind` ("inner", "left", "full", "leftsemi", "leftanti") returns; the
    count pass alone, exact beyond 2^31 - 1."""
    return _ConditionalJoin(left_cols, right_cols, predicate, kind).count()[0]


# ------------------------------------------------------------------------------------------------
# null and value replacement  (cudf::replace_nulls / replace_nans / clamp / find_and_replace_all: replace.hpp; gx_replace.hip)
# ------------------------------------------------------------------------------------------------

def _check_scalar(value, dt: np.dtype):
    """host check of a scalar against the column's dtype: no promotion; a value the dtype cannot hold is a TypeError"""
    host = np.zeros(1, dtype=dt)
    try:
        host[0] = value
    except OverflowError:
        raise TypeError(f"{value!r} is not representable as {dt}") from None
    if dt.kind in "iub" and host[0] != value:
        raise TypeError(f"{value!r} is not representable as {dt}")


def _typed_scalar(value, dt: np.dtype):
    """(value, validity byte) in device memory of a valid scalar cast to the column's dtype"""
    _check_scalar(value, dt)
    return _device_scalar(value, dt)


def _counted(out: Column, nulls) -> Column:
    """the null count of a launch that wrote out.mask; a mask that nulls nothing is dropped"""
    if nulls is not None:
        out.null_count = int(nulls.item())
        if out.null_count == 0:
            out.mask = None
    return out


def _replace_from(fn, what: str, first, col: Column, replacement, nulls_in_both: bool) -> Column:
    """shared by replace_nulls and replace_nans: the replacement is a Column of equal rows and dtype, or a valid scalar"""
    n = col.size
    if isinstance(replacement, Column):
        if replacement.dtype != col.dtype:
            raise TypeError("Data type mismatch")
        if replacement.size != n:
            raise ValueError("Column size mismatch")
        r_null = replacement.has_nulls()
        keep = None
        rargs = [replacement.data_ptr, replacement.mask_ptr if r_null else None, 0, None, 0]
    else:
        r_null = False
        keep = _typed_scalar(replacement, col.dtype)
        rargs = [ptr(keep[0]), None, 0, None, 1]
    may_be_null = (col.has_nulls() and r_null) if nulls_in_both else (col.has_nulls() or r_null)
    out = Column.empty(col.dtype, n, nullable=may_be_null and n > 0)
    if n == 0:
        return out
    nulls = _dev_i64() if may_be_null else None
    L.check(fn(first, col.data_ptr, col.mask_ptr if col.has_nulls() else None, 0, *rargs, n, out.data_ptr, out.mask_ptr, ptr(nulls),
               stream_ptr()), what)
    return _counted(out, nulls)


def replace_nulls(col: Column, replacement) -> Column:
    """cudf::replace_nulls.  replacement: a Column of equal rows and dtype (a row stays null where both are), a Python / NumPy scalar
    (cast to the column's dtype), None (the invalid scalar: nothing is replaced), or "preceding" / "following": a null takes the
    nearest valid value before / after it, rows without one stay null.  A column without nulls comes back as a copy."""
    gx_dtype(col.dtype)
    if isinstance(replacement, str):
        if replacement not in ("preceding", "following"):
            raise ValueError(f"unknown replace policy {replacement!r}")
        if not col.has_nulls():
            return _copy_column(col)
        n = col.size
        out = Column.empty(col.dtype, n, nullable=True)
        nulls = _dev_i64()
        args = (col.dtype.itemsize, col.data_ptr, col.mask_ptr, 0, n, int(replacement == "following"), out.data_ptr, out.mask_ptr, ptr(nulls))
        nb = ctypes.c_size_t(0)
        L.check(_lib.gx_replace_nulls_policy(*args, None, ctypes.byref(nb), None), "gx_replace_nulls_policy")
        tmp = device_bytes(nb.value)
        L.check(_lib.gx_replace_nulls_policy(*args, ptr(tmp), ctypes.byref(nb), stream_ptr()), "gx_replace_nulls_policy")
        return _counted(out, nulls)
    if isinstance(replacement, Column) and replacement.dtype != col.dtype:
        raise TypeError("Data type mismatch")
    if isinstance(replacement, Column) and replacement.size != col.size:
        raise ValueError("Column size mismatch")
    if not isinstance(replacement, Column) and replacement is not None:
        _check_scalar(replacement, col.dtype)    # the value is checked even where nothing is replaced
    if replacement is None or not col.has_nulls():
        return _copy_column(col)
    return _replace_from(_lib.gx_replace_nulls, "gx_replace_nulls", col.dtype.itemsize, col, replacement, True)


def replace_nans(col: Column, replacement) -> Column:
    """cudf::replace_nans: a valid NaN row of a float column takes the replacement's value and validity (a Column of equal rows and
    dtype, a scalar, or None: nothing is replaced); every other row, a null row with NaN bits included, is kept."""
    if col.dtype.kind != "f":
        raise TypeError("replace_nans takes a floating-point column")
    if replacement is None:
        return _copy_column(col)
    return _replace_from(_lib.gx_replace_nans, "gx_replace_nans", col.gx, col, replacement, False)


def clamp(col: Column, lo, hi, lo_replace=None, hi_replace=None) -> Column:
    """cudf::clamp: out[i] = x < lo ? lo_replace : (x > hi ? hi_replace : x) in the column's own dtype; lo / hi None does not bound;
    lo_replace / hi_replace None is the bound itself.  NaN passes through; the result shares the input's validity."""
    gx_dtype(col.dtype)
    if lo is None and hi is None:
        return _copy_column(col)
    dt = col.dtype
    for v in (lo, hi, lo_replace, hi_replace):
        if v is not None:
            _check_scalar(v, dt)             # every value before the first allocation
    lo_v = _typed_scalar(lo, dt)[0] if lo is not None else None
    hi_v = _typed_scalar(hi, dt)[0] if hi is not None else None
    lo_r = _typed_scalar(lo_replace, dt)[0] if lo is not None and lo_replace is not None else None
    hi_r = _typed_scalar(hi_replace, dt)[0] if hi is not None and hi_replace is not None else None
    out = Column.empty(dt, col.size)
    L.check(_lib.gx_clamp(col.gx, col.data_ptr, col.size, ptr(lo_v), None, ptr(lo_r), ptr(hi_v), None, ptr(hi_r), out.data_ptr, stream_ptr()),
            "gx_clamp")
    return _share_validity(out, col)


def find_and_replace_all(col: Column, values_to_replace: Column, replacement_values: Column) -> Column:
    """cudf::find_and_replace_all: out[i] = replacement_values[j] for the first j with col[i] == values_to_replace[j], else col[i]
    (NaN matches nothing, -0.0 matches +0.0).  A null row stays null; a replaced row takes its replacement's validity.  The cost is
    rows x list length comparisons: meant for short lists."""
    gx_dtype(col.dtype)
    if values_to_replace.dtype != col.dtype or replacement_values.dtype != col.dtype:
        raise TypeError("Columns type mismatch")
    if values_to_replace.size != replacement_values.size:
        raise ValueError("values_to_replace and replacement_values size mismatch")
    if values_to_replace.has_nulls():
        raise ValueError("values_to_replace must not have nulls")
    n, m = col.size, values_to_replace.size
    if m == 0:
        return _copy_column(col)
    may_be_null = col.has_nulls() or replacement_values.has_nulls()
    out = Column.empty(col.dtype, n, nullable=may_be_null and n > 0)
    if n == 0:
        return out
    nulls = _dev_i64() if may_be_null else None
    L.check(_lib.gx_find_and_replace(col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, 0, n, values_to_replace.data_ptr,
                                     replacement_values.data_ptr, replacement_values.mask_ptr if replacement_values.has_nulls() else None,
                                     0, m, out.data_ptr, out.mask_ptr, ptr(nulls), stream_ptr()), "gx_find_and_replace")
    return _counted(out, nulls)


def normalize_nans_and_zeros(col: Column) -> Column:
    """cudf::normalize_nans_and_zeros: every NaN becomes the positive quiet NaN, -0.0 becomes +0.0; shares the input's validity"""
    if col.dtype.kind != "f":
        raise TypeError("normalize_nans_and_zeros takes a floating-point column")
    out = Column.empty(col.dtype, col.size)
    L.check(_lib.gx_normalize_nans_and_zeros(col.gx, col.data_ptr, col.size, out.data_ptr, stream_ptr()), "gx_normalize_nans_and_zeros")
    return _share_validity(out, col)


# ------------------------------------------------------------------------------------------------
# making and reshaping columns  (cudf::fill / repeat / sequence: filling.hpp; interleave_columns / tile: reshape.hpp; transpose:
# transpose.hpp; gx_reshape.hip).  Every argument check comes before the first device call.
# ------------------------------------------------------------------------------------------------

_SIZE_MAX = 2**31 - 1


def _same_table(cols: Sequence[Column], what: str, same_type: bool) -> List[Column]:
    cols = list(cols)
    for c in cols:
        if not isinstance(c, Column):
            raise TypeError(f"{what}: expected Columns")
        gx_dtype(c.dtype)
    if len({c.size for c in cols}) > 1:
        raise ValueError("Column size mismatch")
    if same_type and len({c.dtype for c in cols}) > 1:
        raise TypeError(f"{what}: the columns differ in dtype")
    return cols


def interleave_columns(cols: Sequence[Column]) -> Column:
    """cudf::interleave_columns: out[i * k + j] = cols[j][i] for k columns of one dtype and length (gx_interleave: an LDS-staged
    transpose).  The result has a mask only if it holds a null."""
    cols = _same_table(cols, "interleave_columns", True)
    if not cols:
        raise ValueError("interleave_columns: the table has no columns")
    k, n, dt = len(cols), cols[0].size, cols[0].dtype
    if n * k > _SIZE_MAX:
        raise OverflowError("interleave_columns: the result exceeds the column size limit")
    with_mask = any(c.has_nulls() for c in cols) and n > 0
    out = Column.empty(dt, n * k, nullable=with_mask)
    if n == 0:
        return out
    ptrs = (ctypes.c_void_p * k)(*[c.data.data_ptr() for c in cols])
    valid = (ctypes.c_void_p * k)(*[c.mask.data_ptr() if c.has_nulls() else None for c in cols])
    nulls = _dev_i64() if with_mask else None
    _run(_lib.gx_interleave, dt.itemsize, k, ptrs, valid, None, n, out.data_ptr, out.mask_ptr, ptr(nulls))
    return _counted(out, nulls)


def transpose(cols: Sequence[Column]) -> List[Column]:
    """cudf::transpose: the table on its side -- len(cols[0]) result columns of len(cols) rows each, result[i][j] = cols[j][i].  One
    interleave moves the data; the result columns are cut out of it.  A table without columns or rows gives []."""
    cols = _same_table(cols, "transpose", True)
    if not cols or cols[0].size == 0:
        return []
    k, n, dt = len(cols), cols[0].size, cols[0].dtype
    whole = interleave_columns(cols)
    nulls = np.zeros(n, dtype=np.int64)
    if whole.has_nulls():
        nulls = (~whole.valid_numpy()).reshape(n, k).sum(axis=1)
    row_bytes = k * dt.itemsize
    out = []
    for i in range(n):
        c = Column(whole.data[i * row_bytes:(i + 1) * row_bytes].clone(), dt, k)
        if nulls[i]:
            c.mask = torch.zeros(bitmask_words(k), dtype=torch.int32, device="cuda")
            c.null_count = int(nulls[i])
            L.check(_lib.gx_bitmask_copy(c.mask_ptr, 0, whole.mask_ptr, i * k, k, stream_ptr()), "gx_bitmask_copy")
        out.append(c)
    return out


def _tile_or_repeat(fn, what: str, cols, count: int):
    single = isinstance(cols, Column)
    cols = _same_table([cols] if single else cols, what, False)
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)):
        raise TypeError(f"{what}: count must be an integer")
    if count < 0:
        raise ValueError(f"{what}: count cannot be negative")
    n = cols[0].size if cols else 0
    if n * int(count) > _SIZE_MAX:
        raise OverflowError(f"{what}: the result exceeds the column size limit")
    total = n * int(count)
    outs = []
    for c in cols:
        with_mask = c.has_nulls() and total > 0
        out = Column.empty(c.dtype, total, nullable=with_mask)
        if total:
            nulls = _dev_i64() if with_mask else None
            L.check(fn(c.dtype.itemsize, c.data_ptr, c.mask_ptr if with_mask else None, 0, n, int(count), out.data_ptr, out.mask_ptr,
                       ptr(nulls), stream_ptr()), what)
            _counted(out, nulls)
        outs.append(out)
    return outs[0] if single else outs


def tile(cols, count: int):
    """cudf::tile: the rows of the table laid down `count` times (one streaming launch per column: gx_tile).  cols: a Column or a
    list of Columns; the result has the same shape."""
    return _tile_or_repeat(_lib.gx_tile, "tile", cols, count)


def repeat(cols, repeats):
    """cudf::repeat: every row repeated `repeats` times -- an int (gx_repeat_each), or an integer Column of per-row counts without
    nulls (cast and scanned in int64; one expansion map from gx_repeat_map, then gx_gather per column).  Negative entries of a count
    Column are undefined behaviour, as in the reference.  cols: a Column or a list of Columns; the result has the same shape."""
    if not isinstance(repeats, Column):
        return _tile_or_repeat(_lib.gx_repeat_each, "repeat", cols, repeats)
    single = isinstance(cols, Column)
    cols = _same_table([cols] if single else cols, "repeat", False)
    if repeats.dtype.kind not in "iu":
        raise ValueError("repeat: count must be an integral Column")
    if repeats.has_nulls():
        raise ValueError("repeat: count cannot have nulls")
    n = cols[0].size if cols else 0
    if repeats.size != n:
        raise ValueError("repeat: count and the table differ in length")
    if n == 0:
        outs = [Column.empty(c.dtype, 0) for c in cols]
        return outs[0] if single else outs
    # counts as int64 with one 0 behind them: the exclusive scan of n + 1 entries ends in the total
    counts = Column(torch.zeros((n + 1) * 8, dtype=torch.uint8, device="cuda"), np.int64, n + 1)
    L.check(_lib.gx_cast(repeats.gx, repeats.data_ptr, n, L.INT64, counts.data_ptr, stream_ptr()), "gx_cast")
    offsets64 = scan(counts, "sum", inclusive=False)
    total = int(offsets64.data.view(torch.int64)[n].item())      # the one host read: it sizes the result
    if total > _SIZE_MAX:
        raise OverflowError("repeat: the result exceeds the column size limit")
    offsets = cast(offsets64, np.int32)
    gmap = Column.empty(np.int32, total)
    if total:
        _run(_lib.gx_repeat_map, offsets.data_ptr, n, total, gmap.data_ptr)
    outs = []
    for c in cols:
        out = gather(c, gmap) if total else Column.empty(c.dtype, 0)
        if out.mask is not None and out.null_count == 0:
            out.mask = None
        outs.append(out)
    return outs[0] if single else outs


def _sequence_dtype(dtype) -> np.dtype:
    dt = np.dtype(dtype)
    gx_dtype(dt)
    if dt.kind not in "iuf":
        raise TypeError(f"sequence: {dt} is not a numeric type")
    return dt


def sequence(size: int, init, step=None, dtype=None) -> Column:
    """cudf::sequence: out[i] = init + i * step in `dtype` (default: NumPy's type of init), step None = 1.  Integers wrap; floats round
    the product and then the sum, as NumPy's init + arange(size).astype(dtype) * step does."""
    if init is None:
        raise ValueError("sequence: init must be a valid scalar")
    dt = _sequence_dtype(np.asarray(init).dtype if dtype is None else dtype)
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)):
        raise TypeError("sequence: size must be an integer")
    if size < 0:
        raise ValueError("sequence: size cannot be negative")
    if size > _SIZE_MAX:
        raise OverflowError("sequence: size exceeds the column size limit")
    _check_scalar(init, dt)
    if step is not None:
        _check_scalar(step, dt)
    out = Column.empty(dt, int(size))
    if size == 0:
        return out
    init_dev = _device_scalar(init, dt)[0]
    step_dev = _device_scalar(step, dt)[0] if step is not None else None
    L.check(_lib.gx_sequence(out.gx, out.data_ptr, int(size), ptr(init_dev), ptr(step_dev), stream_ptr()), "gx_sequence")
    return out


def fill(col: Column, begin: int, end: int, value) -> Column:
    """cudf::fill: a copy of col with rows [begin, end) set to `value` (cast to the column's dtype; None: the invalid scalar, the rows
    become null).  Outside the range values and validity are the input's; begin == end is a copy."""
    gx_dtype(col.dtype)
    if begin < 0 or end > col.size or begin > end:
        raise IndexError("fill: range out of bounds")
    if value is not None:
        _check_scalar(value, col.dtype)
    out = _copy_column(col)
    if begin == end:
        return out
    n = col.size
    if value is not None:
        val = _device_scalar(value, col.dtype)[0]
        L.check(_lib.gx_fill_range(col.dtype.itemsize, out.data_ptr, begin, end, ptr(val), stream_ptr()), "gx_fill_range")
    old_nulls = 0
    if col.has_nulls():
        cnt = _dev_i64()
        L.check(_lib.gx_bitmask_count(col.mask_ptr, begin, end, ptr(cnt), stream_ptr()), "gx_bitmask_count")
        old_nulls = (end - begin) - int(cnt.item())
    else:
        out.mask = None
    if value is None and out.mask is None:
        out.mask = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
        L.check(_lib.gx_bitmask_set(out.mask_ptr, 0, n, 1, stream_ptr()), "gx_bitmask_set")
    if out.mask is not None:
        L.check(_lib.gx_bitmask_set(out.mask_ptr, begin, end, int(value is not None), stream_ptr()), "gx_bitmask_set")
        out.null_count = col.null_count - old_nulls + (0 if value is not None else end - begin)
        if out.null_count == 0:
            out.mask = None
    return out


# ------------------------------------------------------------------------------------------------
# quantiles  (cudf::quantile / quantiles: quantiles.hpp; the MEDIAN / QUANTILE aggregations) -- gx_quantile.hip
# ------------------------------------------------------------------------------------------------
QUANTILE_MAX_Q = 64  # quantiles of one gx_quantile / gx_quantile_lookup call


def _quantile_args(col: Column, q, interpolation: str, what: str):
    if col.dtype.kind not in "iuf" or col.dtype.itemsize not in (1, 2, 4, 8) or (col.dtype.kind == "f" and col.dtype.itemsize == 2):
        raise TypeError(f"{what}: {col.dtype} is not a numeric type")  # cudf::data_type_error
    qs = [float(x) for x in (list(q) if np.ndim(q) else [q])]
    if any(x != x for x in qs):
        raise ValueError(f"{what}: a quantile is NaN")
    if len(qs) > QUANTILE_MAX_Q:
        raise ValueError(f"{what}: at most {QUANTILE_MAX_Q} quantiles per call")
    if interpolation not in L.INTERP:
        raise ValueError(f"{what}: interpolation must be one of {sorted(L.INTERP)}")
    return qs, L.INTERP[interpolation]


def quantile_index(count: int, q: float):
    """(lower, higher, nearest, frac) of quantile q over `count` >= 1 rows: the one index rule of the kernels (gx_quantile_index)"""
    lo, hi, ne = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    fr = ctypes.c_double(0.0)
    L.check(_lib.gx_quantile_index(int(count), float(q), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)),
            "gx_quantile_index")
    return lo.value, hi.value, ne.value, fr.value


def _all_null(dtype, n: int) -> Column:
    out = Column.empty(dtype, n, nullable=True)
    out.null_count = n
    if n == 0:
        out.mask = None
    return out


def quantile(col: Column, q, interpolation: str = "linear", exact: bool = True, mode: str = "auto", return_info: bool = False):
    """Quantiles of an UNSORTED column, nulls excluded (what Series.quantile and cudf::reduce MEDIAN / QUANTILE ask for): gx_quantile
    -- three streaming passes and a sort of the few candidate rows ("select"), or a sort of the valid rows ("sort"); "auto" picks.
    Returns a Column of len(q) rows: FLOAT64, or with exact=False the column's dtype (linear / midpoint: the double cast to it; else
    the element itself); every row null when the column has no valid row.  return_info=True: (Column, {"path", "nvalid", "elems"})
    with elems = the (lower, higher) elements per quantile as a NumPy array of shape (len(q), 2)."""
    qs, interp = _quantile_args(col, q, interpolation, "quantile")
    if mode not in L.QUANTILE_MODE:
        raise ValueError(f"quantile: mode must be one of {sorted(L.QUANTILE_MODE)}")
    nq = len(qs)
    out_dt = np.dtype(np.float64) if exact else col.dtype
    if nq == 0:
        out = Column.empty(out_dt, 0)
        return (out, {"path": None, "nvalid": None, "elems": np.zeros((0, 2), col.dtype)}) if return_info else out
    f64 = Column.empty(np.float64, nq)
    elems = device_bytes(2 * nq * col.dtype.itemsize)
    nv = _dev_i64()
    path = ctypes.c_int(0)
    qarr = (ctypes.c_double * nq)(*qs)
    tmp = _run(_lib.gx_quantile, col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, 0, col.size, qarr, nq, interp,
                    L.QUANTILE_MODE[mode], f64.data_ptr, ptr(elems), ptr(nv), ctypes.byref(path))
    st = ctypes.c_int(0)
    if _lib.gx_quantile_status(ptr(tmp), ctypes.byref(st), stream_ptr()) != 0:
        raise L.GxError(f"gx_quantile: device-side bounds check failed (status {st.value})")
    nvalid = int(nv.item())
    e = elems[: 2 * nq * col.dtype.itemsize].cpu().numpy().view(col.dtype).reshape(nq, 2).copy()
    if nvalid == 0:
        out = _all_null(out_dt, nq)
    elif exact:
        out = f64
    elif interpolation in ("linear", "midpoint"):
        out = cast(f64, col.dtype)
    else:
        pick = []
        for j, x in enumerate(qs):
            lo, _, ne, _ = quantile_index(nvalid, x)
            pick.append(e[j, 0] if interpolation == "lower" or (interpolation == "nearest" and ne == lo) else e[j, 1])
        out = Column.from_numpy(np.array(pick, dtype=col.dtype))
    return (out, {"path": L.QUANTILE_PATH.get(path.value), "nvalid": nvalid, "elems": e}) if return_info else out


def _lookup(col: Column, order_ptr, nseg: int, offsets: torch.Tensor, counts_ptr, qs, interp: int, exact: bool) -> Column:
    nq = len(qs)
    out = Column.empty(np.float64 if exact else col.dtype, nseg * nq, nullable=True)
    nulls = _dev_i64()
    qarr = (ctypes.c_double * nq)(*qs)
    L.check(_lib.gx_quantile_lookup(col.gx, col.data_ptr, col.mask_ptr if col.has_nulls() else None, 0, order_ptr, nseg, ptr(offsets),
                                    counts_ptr, qarr, nq, interp, int(exact), out.data_ptr, out.mask_ptr, ptr(nulls), stream_ptr()),
            "gx_quantile_lookup")
    return _counted(out, nulls)


def quantile_sorted(col: Column, q, interpolation: str = "linear", ordered_indices: Optional[Column] = None, exact: bool = True) -> Column:
    """cudf::quantile: the quantiles of a column in its EXISTING order, or in the order of `ordered_indices` (an INT32 map of
    col.size rows) -- nothing is sorted.  count = col.size, nulls included; a result is null when a row it reads is null (both
    neighbours for linear / midpoint).  An empty column gives len(q) nulls, an empty q an empty column."""
    qs, interp = _quantile_args(col, q, interpolation, "quantile_sorted")
    out_dt = np.dtype(np.float64) if exact else col.dtype
    if ordered_indices is not None and ordered_indices.size == 0 and col.size > 0:
        ordered_indices = None
    if ordered_indices is not None and (ordered_indices.dtype != np.int32 or ordered_indices.size != col.size or ordered_indices.has_nulls()):
        raise ValueError("quantile_sorted: ordered_indices must be an INT32 column of the input's size")  # std::invalid_argument
    if not qs:
        return Column.empty(out_dt, 0)
    if col.size == 0:
        return _all_null(out_dt, len(qs))
    offsets = torch.tensor([0, col.size], dtype=torch.int32, device="cuda")
    return _lookup(col, ordered_indices.data_ptr if ordered_indices is not None else None, 1, offsets, None, qs, interp, exact)


def _stable_order(cols: Sequence[Column], ascending: Sequence[bool], null_before: Sequence[bool]) -> Column:
    order = None
    for c, a, nb in reversed(list(zip(cols, ascending, null_before))):
        order = sorted_order(c, a, nb) if order is None else gather(order, sorted_order(gather(c, order), a, nb))
    return order


def quantiles(cols: Sequence[Column], q, interpolation: str = "nearest", is_sorted: bool = False, ascending=True,
              null_before=True) -> List[Column]:
    """cudf::quantiles: whole ROWS of a table at the quantiles of its lexicographic order (sorted here unless is_sorted).  The
    interpolation must pick a row: "lower", "higher" or "nearest"."""
    cols = list(cols)
    if not cols:
        raise ValueError("quantiles: no columns")
    if interpolation in ("linear", "midpoint"):
        raise ValueError("quantiles: the interpolation must be non-arithmetic (lower, higher or nearest)")
    if interpolation not in L.INTERP:
        raise ValueError(f"quantiles: interpolation must be one of {sorted(L.INTERP)}")
    n = cols[0].size
    if any(c.size != n for c in cols):
        raise ValueError("quantiles: columns of different lengths")
    if n == 0:
        raise ValueError("quantiles: the table has no rows")
    qs = [float(x) for x in (list(q) if np.ndim(q) else [q])]
    if any(x != x for x in qs):
        raise ValueError("quantiles: a quantile is NaN")
    idx = np.array([dict(zip(("lower", "higher", "nearest"), quantile_index(n, x)[:3]))[interpolation] for x in qs], dtype=np.int32)
    gmap = Column.from_numpy(idx)
    if not is_sorted:
        asc, nb = _per_key(ascending, len(cols), "ascending"), _per_key(null_before, len(cols), "null_before")
        gmap = gather(_stable_order(cols, asc, nb), gmap)
    return [gather(c, gmap) for c in cols]


def groupby_quantile(keys: Column, values: Column, q, interpolation: str = "linear"):
    """groupby QUANTILE (MEDIAN = q 0.5, linear) of one values column by one key column: the rows ordered by (key, value) with null
    values behind their group's valid ones (two stable argsorts), the group offsets, the valid count per group, then
    gx_quantile_lookup: FLOAT64, len(q) results per group, group-major, null for a group without a valid value.
    Returns (group keys in ascending order -- rows with a null key are dropped --, results, number of groups)."""
    qs, interp = _quantile_args(values, q, interpolation, "groupby_quantile")
    if keys.size != values.size:
        raise RuntimeError("Size mismatch between request values and groupby keys.")
    if not qs:
        raise ValueError("groupby_quantile: no quantiles")
    n = keys.size
    if n == 0:
        return Column.empty(keys.dtype, 0), Column.empty(np.float64, 0), 0
    o1 = sorted_order(values, True, False)
    order = gather(o1, sorted_order(gather(keys, o1), True, False))
    ks, vs = gather(keys, order), gather(values, order)
    heads = torch.empty(n, dtype=torch.uint8, device="cuda")
    L.check(_lib.gx_group_heads(ks.gx, ks.data_ptr, ks.mask_ptr if ks.has_nulls() else None, None, n, 0, ptr(heads), stream_ptr()),
            "gx_group_heads")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ng = _dev_i64()
    _run(_lib.gx_group_offsets, ptr(heads), n, ptr(labels), ptr(offsets), None, ptr(ng))
    g = int(ng.item())
    counts = None
    if vs.has_nulls():
        counts = torch.zeros(g, dtype=torch.int32, device="cuda")
        _run(_lib.gx_segmented_reduce, vs.gx, vs.data_ptr, vs.mask_ptr, ptr(heads), ptr(labels), n, L.OP_COUNT_VALID, None, ptr(counts))
    if ks.has_nulls():
        g -= 1  # nulls sort behind every key: their group is the last one
    if g == 0:
        return Column.empty(keys.dtype, 0), Column.empty(np.float64, 0), 0
    res = _lookup(vs, None, g, offsets, ptr(counts), qs, interp, True)
    starts = Column(offsets[:g].contiguous().view(torch.uint8), np.int32, g)
    gk = gather(ks, starts)
    gk.mask, gk.null_count = None, 0
    return gk, res, g


# ------------------------------------------------------------------------------------------------
# synthetic data / checks (bench + tests)
# ------------------------------------------------------------------------------------------------

def random_column(dtype, n: int, seed: int, lo: int = 0, hi: int = 0) -> Column:
    out = Column.empty(dtype, n)
    L.check(_lib.gx_fill_random(out.gx, out.data_ptr, n, seed, lo, hi, stream_ptr()), "gx_fill_random")
    return out


def checksum(col: Column, descending: bool = False):
    """(sum, xor, sortedness violations) computed on the device."""
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    L.check(_lib.gx_checksum(col.gx, col.data_ptr, col.size, int(descending), ptr(res), stream_ptr()), "gx_checksum")
    r = res.cpu().numpy().view(np.uint64)
    return int(r[0]), int(r[1]), int(r[2])
