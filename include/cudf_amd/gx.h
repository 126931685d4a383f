/*
 * gx.h -- the C ABI of libcudf_amd (MI355X / gfx950 kernel layer).
 *
 * This is the drop-in boundary for the cudf hot path: plain pointers and sizes, no C++ types,
 * no torch types.  Everything above it (include/cudf/ C++ API mirror, the Python ctypes
 * wrapper) only allocates, validates and throws; everything below it is hand-written HIP.
 *
 * Conventions (all entry points):
 *   - return 0 on success, a positive hipError_t value on a runtime failure, a negative
 *     GX_E* code on misuse;
 *   - every pointer is a DEVICE pointer unless the parameter is documented "host";
 *   - work is enqueued on `stream` and is asynchronous w.r.t. the host unless the entry point
 *     returns a host value (documented per function);
 *   - entry points never allocate: scratch comes from the caller through the cub-style query
 *     convention (tmp == NULL  ->  *tmp_bytes is set to the required size and nothing runs),
 *     mirroring the reference's call sites, e.g. cpp/src/sort/sort_radix.cu:67-71;
 *   - row counts are int64_t here; the cudf::size_type (int32) limit is enforced one layer up
 *     (cpp/include/cudf/types.hpp:76).
 *
 * Each declaration cites the reference interface it replaces (paths relative to
 * /root/reference/cpp).
 */
#ifndef CUDF_AMD_GX_H
#define CUDF_AMD_GX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* gx_stream_t; /* == hipStream_t */

/* element types: numeric values match cudf::type_id (include/cudf/types.hpp:184-216) */
enum gx_dtype {
  GX_INT8    = 1,
  GX_INT16   = 2,
  GX_INT32   = 3,
  GX_INT64   = 4,
  GX_UINT8   = 5,
  GX_UINT16  = 6,
  GX_UINT32  = 7,
  GX_UINT64  = 8,
  GX_FLOAT32 = 9,
  GX_FLOAT64 = 10,
  GX_BOOL8   = 11
};

enum gx_error {
  GX_SUCCESS       = 0,
  GX_EINVAL        = -1, /* bad argument (null pointer, negative size, aliasing) */
  GX_EDTYPE        = -2, /* dtype not supported by this entry point */
  GX_ETMP          = -3, /* scratch buffer too small */
  GX_EINTERNAL     = -4, /* device-side protocol failure reported by gx_sort_status */
  GX_EOVERFLOW     = -5  /* output does not fit the caller's capacity */
};

/* reduce / scan / groupby operator codes: match cudf::aggregation::Kind for the kinds we
 * implement (include/cudf/aggregation.hpp:84-130) */
enum gx_op {
  GX_OP_SUM         = 0,
  GX_OP_PRODUCT     = 1,
  GX_OP_MIN         = 2,
  GX_OP_MAX         = 3,
  GX_OP_COUNT_VALID = 4,
  GX_OP_COUNT_ALL   = 5,
  GX_OP_COUNT_NONZERO = 6, /* gx_reduce only: valid elements != 0 (NaN counts); cudf::reduce ANY / ALL (reductions/any.cu, all.cu) */
  GX_OP_MEAN        = 10
};

const char* gx_version(void);
/* size in bytes of one element of `dtype`, 0 if unknown */
int gx_dtype_size(int dtype);

/* ------------------------------------------------------------------------------------------
 * Radix sort.
 * Replaces cub::DeviceRadixSort::SortKeys[Descending] as called at src/sort/sort_radix.cu:69-76
 * (and the float path :80-119): stable LSD radix sort of a fixed-width column without nulls,
 * begin_bit = 0, end_bit = 8*sizeof(T).  Floats: -0.0 == +0.0 (input order kept), NaNs after
 * +Inf in input order (descending: NaNs first, reverse input order -- the composite-key rule of
 * sort_radix.cu:36-45).  `in` and `out` must not alias.
 * ------------------------------------------------------------------------------------------ */
int gx_sort_keys(int dtype, const void* in, void* out, int64_t n, int descending,
                 void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* Replaces cub::DeviceRadixSort::SortPairs[Descending] as called at
 * src/sort/sorted_order_radix.cu:83-94,125-135.  vals_in == NULL means iota (what
 * thrust::sequence writes at :70-73).  keys_out may be NULL (sorted keys are then kept only in
 * scratch, as the reference discards them: :67). */
int gx_sort_pairs(int key_dtype, const void* keys_in, void* keys_out, const int32_t* vals_in,
                  int32_t* vals_out, int64_t n, int descending, void* tmp, size_t* tmp_bytes,
                  gx_stream_t stream);

/* cudf::sorted_order / stable_sorted_order of one column (include/cudf/sorting.hpp:44-64;
 * src/sort/sort_column.cu:22-44, stable_sort_column.cu:22-46, sort_column_impl.cuh:35-57).
 * valid == NULL: radix path above.  Otherwise `valid` is an Arrow validity bitmap (LSB-first,
 * 1 = valid, bit 0 = row 0): null rows are placed first when (nulls_before XOR descending) --
 * the flip of sort_column_impl.cuh:42-45 -- in input order, valid rows are radix sorted (stable,
 * NaN greater than every number and equivalent to each other in BOTH directions: the comparator
 * path, include/cudf/detail/row_operator/common_utils.cuh:157-169).  null_count is the host-side
 * null count the column_view carries (include/cudf/column/column_view.hpp null_count()). */
int gx_sorted_order(int dtype, const void* keys, const uint32_t* valid, int64_t n, int64_t null_count,
                    int descending, int nulls_before, int32_t* out_indices, void* tmp, size_t* tmp_bytes,
                    gx_stream_t stream);

/* cudf::sorted_order / stable_sorted_order of a TABLE of 1 <= ncols <= 8 numeric columns without nulls: replaces thrust::sort /
 * thrust::stable_sort of the row indices under the lexicographic row comparator (src/sort/sort_impl.cuh:61-93; src/sort/sort.cu:22-50).
 * cols[c] / dtypes[c] / descending[c] (NULL = all ascending) are HOST arrays of ncols entries; the columns are device buffers of n rows.
 * Stable (ties of the whole tuple in row order); NaN equivalent to each other and greater than every number in both directions,
 * -0.0 == +0.0 (include/cudf/detail/row_operator/common_utils.cuh:157-169).  One keys-only word sort on a nested rank of the tuple plus
 * a pass over the runs of equal ranks (gx_order.hip); gx_sort_status(tmp) reports the word sort's status. */
int gx_sorted_order_table(int ncols, const int* dtypes, const void* const* cols, const int* descending, int64_t n, int32_t* out_indices,
                          void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* Copies the device-side status word of the last sort that used `tmp` to *status_host (0 = ok).  Synchronises `stream`.
 * 5: a look-back wait made no progress for 30 s of wall-clock time (gx_sort_set_spin_limit_ms) and was abandoned -- the output is
 * NOT sorted (every write stayed inside it); 3: a bookkeeping mismatch of the hybrid path, the LSD passes produced the output. */
int gx_sort_status(const void* tmp, int* status_host, gx_stream_t stream);
/* The same copy, queued on `stream` and NOT waited for: *status_host_pinned (host memory the device can write, e.g.
 * hipHostMalloc) holds the status once everything queued on `stream` so far has run.  The asynchronous form the
 * C++ surface uses so that cudf::sort returns without a host round trip (reference: sort.cu:52-89 is asynchronous). */
int gx_sort_status_async(const void* tmp, int* status_host_pinned, gx_stream_t stream);
/* What an abandoned look-back wait does, for the sorts the CALLING THREAD issues from now on: 0 (default) = __builtin_trap -- loud, fatal
 * for the process' HIP context: right for a caller that never reads the status word; 1 = the recoverable form: status 5, every write
 * inside the output, the caller MUST read the word (gx_sort_status / gx_sort_status_async) before it trusts the result. */
void gx_sort_set_fault_mode(int recoverable);



/* ------------------------------------------------------------------------------------------
 * The two halves of the sort, for a SHARDED sort whose exchange sits between the sort's own two partition levels (gxd_sort;
 * the reference's shape is sample -> boundaries -> shuffle -> local sort: python/cudf_polars/cudf_polars/streaming/
 * actor_graph/collectives/sort.py, with cub::DeviceRadixSort as the local sort, cpp/src/sort/sort_radix.cu:52-161).
 * INT64 / UINT64 / INT32 / UINT32 keys, ascending, keys only.  One scratch blob serves all calls of a sort: query its size with
 * gx_sortx_sample(tmp = NULL); n = this rank's rows, recv_rows_max = the most rows it is prepared to receive.
 *   gx_sortx_sample   varying-bit masks of a sample of the shard            -> gx_sortx_masks reads {OR, NOR} (sortable form)
 *   gx_sortx_level0   level 0 (256 bins on the 8 bits below the highest bit that varies in masks2 = the OR over ALL ranks of
 *                     what gx_sortx_masks returned) into padded (bin, input range) slots of the level-0 buffer
 *   gx_sortx_tables   cur0[r * 256 + bin] = keys in slot (range r, bin), slot0[...] = its first key in the level-0 buffer (slots
 *                     are laid out bin-major: the 8 slots of a bin are neighbours, bins ascend), slot_total = rows in use,
 *                     state = 3 when level 0 succeeded (anything else: take another path)
 *   gx_sortx_level0_buffer   the level-0 buffer: own_rows keys of this rank's slots, the rest (up to total_rows) is the
 *                     receive area the caller fills with the spans its peers send
 *   gx_sortx_finish   level 1 + cell sort over `nreg` regions {first key in the level-0 buffer, keys, level-0 bucket}, given in
 *                     bucket order; n = their total; `out` receives the n sorted keys
 *   gx_sortx_status   1 when the sorted output is valid (0: a device-side check failed -- take another path)
 * masks, tables, status synchronise the stream (they return host values). */
int gx_sortx_sample(int dtype, const void* keys, int64_t n, int64_t recv_rows_max, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_sortx_masks(const void* tmp, uint64_t* masks2_host, gx_stream_t stream);
int gx_sortx_level0(int dtype, const void* keys, int64_t n, int64_t recv_rows_max, const uint64_t* masks2_host, void* tmp, gx_stream_t stream);
int gx_sortx_tables(const void* tmp, uint32_t* cur0_host, uint32_t* slot0_host, uint32_t* slot_total_host, int32_t* state_host, gx_stream_t stream);
void* gx_sortx_level0_buffer(int dtype, void* tmp, int64_t n, int64_t recv_rows_max, int64_t* own_rows, int64_t* total_rows);
int gx_sortx_finish(int dtype, int64_t n_send, int64_t recv_rows_max, int64_t n, const uint64_t* masks2_host, const uint32_t* reg_start_host,
                    const uint32_t* reg_count_host, const uint32_t* reg_bucket_host, int nreg, void* out, void* tmp, gx_stream_t stream);
int gx_sortx_status(const void* tmp, int32_t* ok_host, gx_stream_t stream);

/* info8_host (host, 8 x int32) = {hybrid attempted, hybrid used, d1, shift2, bits2, LDS passes,
 * largest cell, active LSD passes (-1 when the hybrid path produced the output)} of the last sort
 * that used `tmp`.  Synchronises `stream`. */
int gx_sort_info(const void* tmp, int32_t* info8_host, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gather.  Replaces cudf::detail::gather for fixed-width columns
 * (include/cudf/detail/gather.cuh:108-131 data, :506-577 validity): out[i] = in[map[i]].
 * elem_size in {1,2,4,8}.  map entries must be in [0, src_rows) (bounds_policy::DONT_CHECK);
 * entries equal to INT32_MIN (JoinNoMatch) produce a null/zero row when nullify_oob != 0.
 * src_valid/out_valid may be NULL (no validity handled).
 * ------------------------------------------------------------------------------------------ */
int gx_gather(int elem_size, const void* src, const uint32_t* src_valid, int64_t src_rows,
              const int32_t* map, int64_t n, int nullify_oob, void* out, uint32_t* out_valid,
              gx_stream_t stream);
/* Sharded joins: out[j] = rows[idx[j]] + seg_bases[s], s = the segment of the receive buffer position idx[j] falls
 * into (segment k holds seg_counts[k] entries; nseg <= 16 ranks; counts and bases are HOST arrays).  Turns the
 * (int32 local row) a rank received next to each key into the global int64 row id of a join pair in one gather
 * (the per-rank split of cudf_polars' shuffle carries the same information as a partition id). */
int gx_gather_global_rows(const int32_t* rows, int64_t nrows, const int32_t* idx, int64_t n, int nseg,
                          const int64_t* seg_counts_host, const int64_t* seg_bases_host, int64_t* out, gx_stream_t stream);

/* The same with the segment table in DEVICE memory and any number of segments (the chunked exchange of gxd.h leaves
 * chunks x ranks segments): segtab_dev = [nseg + 1] int64 segment starts followed by [nseg] int64 bases. */
int gx_gather_global_rows_dev(const int32_t* rows, int64_t nrows, const int32_t* idx, int64_t n, int nseg, const int64_t* segtab_dev,
                              int64_t* out, gx_stream_t stream);
/* The sharded join's pairs without a gather: a row travels as enc = (source rank << shift) | row (the payload of the *_pl entry
 * points below) and is decoded in one streaming pass: out[j] = bases_dev[src] + row, plus chunk(j) * chunk_rows_dev[src] when
 * the row was counted inside its sender's CHUNK -- chunk(j) = the c with snap_dev[c] <= j < snap_dev[c + 1], snap_dev = the
 * pair positions at which the probe of each received chunk started (nchunks + 1 device int64; nchunks <= 1024). */
int gx_decode_global_rows(const int32_t* enc, int64_t n, int shift, const int64_t* bases_dev, const int64_t* chunk_rows_dev,
                          const int64_t* snap_dev, int nchunks, int64_t* out, gx_stream_t stream);
/* out[i] = in[i] as int64 (row indices / counts leaving the int32 world of cudf::size_type) */
int gx_widen_i32_i64(const int32_t* in, int64_t n, int64_t* out, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Validity bitmaps.  Replace src/bitmask/null_mask.cu:152 (set), :339-409 (count),
 * include/cudf/detail/null_mask.cuh:68 (bitmask_and).
 * ------------------------------------------------------------------------------------------ */
int gx_bitmask_set(uint32_t* mask, int64_t begin_bit, int64_t end_bit, int valid, gx_stream_t stream);
/* *count_dev (device int64) = number of set bits in [begin_bit, end_bit) */
int gx_bitmask_count(const uint32_t* mask, int64_t begin_bit, int64_t end_bit, int64_t* count_dev,
                     gx_stream_t stream);
/* dst bits [dst_begin_bit, +nbits) = src bits [src_begin_bit, +nbits); src == NULL writes 1s.  The
 * building block of cudf::copy_bitmask (src/bitmask/null_mask.cu:357-390) and concatenate_masks
 * (src/copying/concatenate.cu:111-170); bits of dst outside the range are preserved. */
int gx_bitmask_copy(uint32_t* dst, int64_t dst_begin_bit, const uint32_t* src, int64_t src_begin_bit,
                    int64_t nbits, gx_stream_t stream);
/* out = AND of `nmasks` bitmaps (host array of device pointers; NULL entries = all valid),
 * nbits bits each; *count_dev (optional) = set bits of the result */
int gx_bitmask_and(const uint32_t* const* masks_host, int nmasks, int64_t nbits, uint32_t* out,
                   int64_t* count_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Ordered stream compaction (row filtering).  Replaces thrust::copy_if / cudf::detail::copy_if behind
 * cudf::apply_boolean_mask, drop_nulls and drop_nans (src/stream_compaction/apply_boolean_mask.cu, drop_nulls.cu,
 * drop_nans.cu; include/cudf/detail/copy_if.cuh).  Two steps:
 *   a SELECTOR writes the plan into `sel_tmp` -- one bit per row as uint64 ballot words, the number of selected rows before
 *   every 4096-row chunk -- and the number of selected rows to *count_dev (device int64, optional).  cub-style query:
 *   sel_tmp == NULL -> *tmp_bytes = gx_compact_plan_bytes(n) = align256(8 * (ceil(n / 64) + 1)) + align256(8 * (ceil(n / 4096) + 1));
 *   gx_compact_column / gx_compact_indices read the plan, once per column: the selected elements in row order.  One plan
 *   serves every column of a table of n rows (`n` must be the n the plan was made for).
 * Bitmaps are Arrow validity bitmaps read from a begin bit on (sliced views), as in gx_bitmask_copy.  n < 2^31.
 *
 * gx_select_mask: selected = mask[i] != 0 and (mask_valid == NULL or its bit is set): a null mask element drops the row.
 * gx_select_valid_count: selected = (number of the nkeys <= 32 bitmaps whose bit is set) >= keep_threshold; a NULL entry of
 *   valid_ptrs_host is a column without nulls.  valid_ptrs_host / begin_bits_host (NULL = zeros) are HOST arrays.
 * gx_select_not_nan: null_is_missing == 0 (cudf::drop_nans): selected = (number of keys that are not a VALID NaN) >=
 *   keep_threshold -- a null element is not a NaN; every dtype must be FLOAT32 / FLOAT64, else GX_EDTYPE.
 *   null_is_missing != 0 (pandas dropna): a key counts when it is valid AND not NaN; keys of other dtypes are allowed, their
 *   validity alone decides (cols_host[k] is not read for them).
 * gx_compact_column: elem_size in {1,2,4,8} (else GX_EDTYPE).  in_valid != NULL: out_valid (REQUIRED then, zeroed by the
 *   caller, (selected + 31) / 32 words) receives bit j = validity of the j-th selected row, *out_null_count_dev (device
 *   int64, optional) the number of selected null rows.
 * gx_compact_indices: out_idx[j] = row number of the j-th selected row (the gather map of the selection).
 * gx_compare_scalar: out_bool8[i] = in[i] <cmp> scalar (gx_cmp; the scalar's bits in the column's type sit in the low bytes of
 *   scalar_bits); NaN compares false except under GX_CMP_NE; a null row (in_valid bit 0) gets 0 -- the result column shares
 *   the input's bitmap.  One grid-stride kernel; what makes a mask on the device.
 * ------------------------------------------------------------------------------------------ */
enum gx_cmp { GX_CMP_EQ = 0, GX_CMP_NE = 1, GX_CMP_LT = 2, GX_CMP_LE = 3, GX_CMP_GT = 4, GX_CMP_GE = 5 };
size_t gx_compact_plan_bytes(int64_t n); /* 0 for n outside [0, 2^31) */
int gx_select_mask(const uint8_t* mask_bool8, const uint32_t* mask_valid, int64_t mask_valid_begin_bit, int64_t n,
                   int64_t* count_dev, void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_select_valid_count(int nkeys, const uint32_t* const* valid_ptrs_host, const int64_t* begin_bits_host, int64_t n,
                          int keep_threshold, int64_t* count_dev, void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_select_not_nan(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                      const int64_t* begin_bits_host, int64_t n, int keep_threshold, int null_is_missing, int64_t* count_dev,
                      void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_compact_column(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_valid_begin_bit, int64_t n,
                      const void* sel_tmp, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_compact_indices(int64_t n, const void* sel_tmp, int32_t* out_idx, gx_stream_t stream);
int gx_compare_scalar(int dtype, const void* in, const uint32_t* in_valid, int64_t n, int cmp, uint64_t scalar_bits,
                      uint8_t* out_bool8, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Deduplicating selectors (cudf_amd/csrc/gx_distinct.hip).  Replace the reduction over a set of row indices behind
 * cudf::distinct / stable_distinct / distinct_indices / distinct_count (src/stream_compaction/distinct.cu,
 * stable_distinct.cu, distinct_helpers.cu, distinct_count.cu) and the adjacent-row predicate behind cudf::unique /
 * unique_count (src/stream_compaction/unique.cu, unique_count.cu).  Both are SELECTORS of the block above: same scratch
 * query, same *count_dev, and the plan sits at the START of sel_tmp, so gx_compact_column / gx_compact_indices take the
 * same pointer (whatever else a selector needs lies behind the plan).
 * Key row = the nkeys (1..32) fixed-width columns cols_host[k] of dtypes_host[k], validity valid_ptrs_host[k] (NULL = no
 * nulls) read from bit begin_bits_host[k] on (begin_bits_host == NULL = zeros); all three are HOST arrays.
 * Element equality: both null and flag 1, or both valid and equal values; floats: -0.0 == +0.0, NaN == NaN (any sign,
 * any payload) iff flag 2.  A null element's bytes are never read.  Rows are equal when all their elements are.
 * flags: 1 nulls equal; 2 NaNs equal; 4 a NaN element counts as a null element; 8 a row holding a null key (a NaN under
 *   flag 4 included) is not selected at all.  Without flag 1 (2) a row holding a null (a NaN) equals no row, itself
 *   included in no class: it is always selected, under GX_KEEP_NONE as well.
 * gx_select_unique: runs of CONSECUTIVE equal rows.  KEEP_ANY / KEEP_FIRST select the first row of a run, KEEP_LAST the
 *   last, KEEP_NONE the runs of length 1.  Under flag 8 a row is compared with its physical neighbour all the same
 *   ([1, null, 1] selects rows 0 and 2).
 * gx_select_distinct: equality classes over all rows.  KEEP_FIRST selects the smallest row of a class, KEEP_LAST the
 *   largest, KEEP_NONE the classes of one row, KEEP_ANY one row per class (whichever claimed the class's slot first).
 *   Scratch: plan + 4 * capacity bytes of table (capacity = the power of two >= 2 n, >= 64); every keep but KEEP_ANY adds
 *   4 n bytes of slot numbers + n / 8 of bits, KEEP_NONE another 4 * capacity: query with the `keep` of the call.
 * Errors, before any launch: GX_EINVAL n outside [0, 2^31), nkeys outside [1, 32], keep outside gx_keep, flags outside
 *   [0, 15], a negative begin bit, tmp_bytes == NULL, null array / column pointers with n > 0 and sel_tmp != NULL;
 *   GX_EDTYPE an unknown dtype; GX_ETMP short scratch.  n == 0: *count_dev = 0, nothing else runs.
 * ------------------------------------------------------------------------------------------ */
enum gx_keep { GX_KEEP_ANY = 0, GX_KEEP_FIRST = 1, GX_KEEP_LAST = 2, GX_KEEP_NONE = 3 };
int gx_select_unique(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                     const int64_t* begin_bits_host, int64_t n, int keep, int flags, int64_t* count_dev, void* sel_tmp,
                     size_t* tmp_bytes, gx_stream_t stream);
int gx_select_distinct(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                       const int64_t* begin_bits_host, int64_t n, int keep, int flags, int64_t* count_dev, void* sel_tmp,
                       size_t* tmp_bytes, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Merging and searching sorted rows (cudf_amd/csrc/gx_merge.hip).  Replace thrust::merge over the tagged row comparator
 * behind cudf::merge (cpp/src/merge/merge.cu) and thrust::lower_bound / upper_bound over the row comparator behind
 * cudf::lower_bound / upper_bound (cpp/src/search/search_ordered.cu).
 * Key rows as in the selector block: nkeys (1..32) fixed-width columns per side, HOST arrays of device pointers, validity
 * NULL = no nulls, read from the begin bit on (begin bits NULL = zeros); both sides share dtypes_host, descending_host
 * (NULL = all ascending) and null_before_host (NULL = nulls before, everywhere).  Row order: the lexicographic comparator of
 * the multi-column sorts -- nulls equivalent and first iff null_before != descending, NaN == NaN greater than every number,
 * -0.0 == +0.0; a null element's bytes are never read.
 * gx_merge_order: A (na rows) and B (nb rows), each sorted under that order; out_map (na + nb entries) = the STABLE merge:
 *   entry < na is a row of A, otherwise na + a row of B; among equivalent rows all of A's precede all of B's, each side in
 *   row order.  Scratch query through tmp == NULL.  Unsorted input: an unspecified map whose entries are all inside
 *   [0, na + nb) (without bitmaps: a permutation), and no read outside the columns.
 * gx_gather2: out[i] = map[i] < na ? a[map[i]] : b[map[i] - na], elem_size in {1,2,4,8} (else GX_EDTYPE); out_valid
 *   (ceil(n / 32) words, every word written) is REQUIRED when either side has a bitmap, a side without one is all valid;
 *   *out_null_count_dev (optional, device int64) = nulls written.  A map entry outside [0, na + nb) reads nothing: a zero
 *   element, null where there is a bitmap.
 * gx_search_bounds: out[i] (INT32) = the number of haystack rows that compare < needle i (upper == 0: lower_bound) or
 *   <= needle i (upper != 0: upper_bound); the haystack sorted under the same order, the needles in any order.
 * gx_merge_tile_rows: output rows per workgroup of the merge-path tile kernel (tests size their cases from it).
 * Errors, before any launch: GX_EINVAL negative or >= 2^31 row counts (merge, gather: the sum), nkeys outside [1, 32], no
 *   dtypes, a negative begin bit, tmp_bytes == NULL, null array / column / output pointers where the call would launch and
 *   the side has rows; GX_EDTYPE; GX_ETMP.  No rows to write: nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int gx_merge_tile_rows(void);
int gx_merge_order(int nkeys, const int* dtypes_host, const void* const* a_cols_host, const uint32_t* const* a_valid_ptrs_host,
                   const int64_t* a_begin_bits_host, int64_t na, const void* const* b_cols_host,
                   const uint32_t* const* b_valid_ptrs_host, const int64_t* b_begin_bits_host, int64_t nb,
                   const int* descending_host, const int* null_before_host, int32_t* out_map, void* tmp, size_t* tmp_bytes,
                   gx_stream_t stream);
int gx_gather2(int elem_size, const void* a, const uint32_t* a_valid, int64_t a_begin_bit, int64_t na, const void* b,
               const uint32_t* b_valid, int64_t b_begin_bit, int64_t nb, const int32_t* map, int64_t n, void* out,
               uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_search_bounds(int nkeys, const int* dtypes_host, const void* const* hay_cols_host,
                     const uint32_t* const* hay_valid_ptrs_host, const int64_t* hay_begin_bits_host, int64_t n_hay,
                     const void* const* needle_cols_host, const uint32_t* const* needle_valid_ptrs_host,
                     const int64_t* needle_begin_bits_host, int64_t n_needles, const int* descending_host,
                     const int* null_before_host, int upper, int32_t* out, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Rolling windows (cudf_amd/csrc/gx_rolling.hip).  Replace the per-row window loop behind cudf::rolling_window and
 * cudf::grouped_rolling_window (cpp/include/cudf/rolling.hpp; rolling_detail.cuh, grouped_rolling.cu of the reference).
 * gx_rolling_window: out[i] = op over the rows [i - preceding + 1, i + following] of `in` (n rows; `preceding` counts row i
 *   itself), cut to [0, n) -- or, with labels / offsets (both or neither; as gx_group_offsets writes them: labels[i] = group
 *   of row i, offsets[g] = its first row, offsets[ngroups] = n), to the row's group.  Negative values are legal: such a window
 *   does not hold row i and may be empty.  Bounds are computed in 64 bits.  preceding_col / following_col (both or neither,
 *   INT32, n rows) give one window per row; the two scalars are then ignored.
 *   op: GX_OP_SUM (integers and BOOL8 -> INT64, wrapping mod 2^64, UINT64 -> UINT64 with the same bits; floats keep their
 *   type, FLOAT32 accumulated in double and rounded once), GX_OP_MIN / GX_OP_MAX (input type), GX_OP_MEAN (FLOAT64; integers
 *   summed exactly in 64 bits, then divided), GX_OP_COUNT_VALID / GX_OP_COUNT_ALL (INT32).
 *   Validity: out_valid is REQUIRED, (n + 31) / 32 words, every word written; *out_null_count_dev (optional, device int64) =
 *   nulls written.  SUM / MIN / MAX / MEAN: row i is valid iff its window holds at least max(min_periods, 1) valid values -- a
 *   window without a valid value is NULL, never an identity, also at min_periods == 0 (a deliberate choice: the reference's
 *   handling of min_periods == 0 is not copied).  The two counts: row i is valid iff its cut window has at least min_periods
 *   ROWS.  in_valid (NULL = no nulls) is read from in_begin_bit on; a null's bytes are never read; a null row of `out` is 0.
 *   Floats: +-inf, NaN and overflow follow plain addition over the window's values (nothing is subtracted anywhere); MIN / MAX
 *   in the order of the sorts: NaN greater than every number, -0.0 == +0.0 (which zero comes back is unspecified).
 *   Cost: fixed windows whose halo max(preceding - 1, 0) + max(following, 0) is at most gx_rolling_max_span() and that hold a
 *   row (preceding + following >= 1) take the tile kernel: constant work per row whatever the window.  Per-row windows, wider
 *   halos, preceding + following <= 0 -- and windows of up to 8 rows, where it is the faster of the two -- take one thread per
 *   row looping over its window: O(window) per row.  No scratch.
 * gx_rolling_tile_rows: output rows per workgroup of the tile kernel (tests size their cases from it).
 * gx_rolling_max_span: the largest halo (rows before + rows after) the tile kernel takes.
 * Errors, before any launch: GX_EINVAL n outside [0, 2^31), min_periods < 0, only one of the two window columns, only one of
 *   labels / offsets, null in / out / out_valid with n > 0, a negative begin bit; GX_EDTYPE an unknown dtype or op.
 *   n == 0: nothing is launched.
 * ------------------------------------------------------------------------------------------ */
int gx_rolling_tile_rows(void);
int gx_rolling_max_span(void);
int gx_rolling_window(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, int64_t preceding,
                      int64_t following, const int32_t* preceding_col, const int32_t* following_col, const int32_t* labels,
                      const int32_t* offsets, int min_periods, int op, void* out, uint32_t* out_valid,
                      int64_t* out_null_count_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Row movement (cudf_amd/csrc/gx_copying.hip).  Replace fused_concatenate_kernel / concatenate_masks (concatenate.cu), the
 * thrust::scatter + scatter_bitmask pair (detail/scatter.cuh) and copy_if_else_kernel (detail/copy_if_else.cuh) of the
 * reference.  elem_size is the element width in bytes, 1 / 2 / 4 / 8 (values move as bits: NaN payloads and -0.0 survive).
 * Validity bitmaps are Arrow bitmaps read from a begin bit on (a sliced view needs no re-based copy); row counts lie in
 * [0, 2^31).  Every argument check comes before the first device call; with no rows nothing is launched.
 * gx_concatenate: out = the rows of input 0, then input 1, ... (ninputs >= 1; cols_host / rows_host / valid_ptrs_host /
 *   begin_bits_host are HOST arrays of ninputs entries; valid_ptrs_host may be NULL, as may any entry: an input without nulls;
 *   begin_bits_host NULL = all 0).  One launch: a workgroup takes a tile of gx_concat_tile_rows() output rows, finds the inputs
 *   that cover it, copies each piece with the widest access that source and destination address share (16 bytes down to 1), and
 *   -- with out_valid, (rows + 31) / 32 words, every word written, bits behind the last row 0 -- composes the tile's validity
 *   words from the inputs' bitmaps; a tile owns whole words, so nothing is merged with atomics.  *out_null_count_dev
 *   (optional, device int64) = nulls written (0 without out_valid).  A tile fed by more than 16 inputs copies row by row.
 *   out == NULL with out_valid: the validity alone (cudf::concatenate_masks); cols_host is then not read.
 *   Scratch (cub-style query: tmp == NULL -> *tmp_bytes) holds the input descriptors; they reach it as kernel arguments, 64
 *   per small launch, so the host arrays are not read after the call returns and the stream is not waited for.
 *   GX_EINVAL: ninputs < 1, a NULL host array (cols, rows), a negative row count or begin bit, a row total of 2^31 or more,
 *   a NULL input with rows, NULL out and out_valid with rows; GX_ETMP: scratch too small.
 * gx_scatter: in place on a target the caller has filled: target[wrap(map[i])] = src[i] for i in [0, n), src[0] with
 *   src_is_scalar; wrap(m) = m < 0 ? m + target_rows : m.  Entries outside [-target_rows, target_rows) are undefined behaviour
 *   (the reference's DONT_CHECK).  With target_valid the bit of every written row is set or cleared atomically on its word
 *   (src_valid read from src_begin_bit on, NULL = no nulls; a scalar's validity is the device byte *src_scalar_valid_dev, NULL =
 *   valid); bits of other rows stay.  A map that repeats a target row leaves it with the value AND validity of one of its
 *   candidates, which one is unspecified: where the source has nulls the bits are written by a second pass, by the rows whose
 *   value the target holds.  GX_EINVAL: n or target_rows outside [0, 2^31), a negative begin bit, NULL src / map / target or
 *   target_rows == 0 with n > 0.
 * gx_copy_if_else: out[i] = (mask_bool8[i] != 0 and the mask's bit set) ? lhs[i] : rhs[i]; a side with *_is_scalar is one
 *   element in device memory with its validity byte (NULL = valid).  With out_valid ((n + 31) / 32 words, every word written)
 *   the validity is the chosen side's, and *out_null_count_dev (optional) the nulls written.  One streaming pass, no scratch.
 *   GX_EINVAL: n outside [0, 2^31), a negative begin bit, NULL lhs / rhs / mask / out with n > 0.
 * ------------------------------------------------------------------------------------------ */
int gx_concat_tile_rows(void);
int gx_concatenate(int elem_size, int ninputs, const void* const* cols_host, const int64_t* rows_host,
                   const uint32_t* const* valid_ptrs_host, const int64_t* begin_bits_host, void* out, uint32_t* out_valid,
                   int64_t* out_null_count_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_scatter(int elem_size, const void* src, const uint32_t* src_valid, int64_t src_begin_bit,
               const uint8_t* src_scalar_valid_dev, int src_is_scalar, const int32_t* map, int64_t n, void* target,
               uint32_t* target_valid, int64_t target_rows, gx_stream_t stream);
int gx_copy_if_else(int elem_size, const void* lhs, const uint32_t* lhs_valid, int64_t lhs_begin_bit,
                    const uint8_t* lhs_scalar_valid_dev, int lhs_is_scalar, const void* rhs, const uint32_t* rhs_valid,
                    int64_t rhs_begin_bit, const uint8_t* rhs_scalar_valid_dev, int rhs_is_scalar, const uint8_t* mask_bool8,
                    const uint32_t* mask_valid, int64_t mask_begin_bit, int64_t n, void* out, uint32_t* out_valid,
                    int64_t* out_null_count_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise operations (cudf_amd/csrc/gx_elementwise.hip).  Replace the type-dispatched functors and the JIT of the
 * reference's cpp/src/binaryop and the kernels of cpp/src/unary.  All eleven gx_dtype are taken on every operand and on the
 * output; no scratch, no host synchronisation, everything is stream-ordered; row counts lie in [0, 2^31).
 * gx_binary_op: out[i] = cast<Out>( f( cast<C>(lhs[i]), cast<C>(rhs[i]) ) ).  C is the type the usual arithmetic conversions of
 *   C++ give for L op R: anything narrower than 32 bits, and BOOL8, computes in int32; else C is uint32, int64, uint64, float or
 *   double (int32 o uint32 -> uint32, int64 o uint64 -> uint64, integer o float -> float, anything o double -> double).  Integer
 *   results wrap modulo 2^width of C.  A BOOL8 load takes any nonzero byte as 1, a BOOL8 store writes 0 or 1 (x != 0).
 *   Operators (gx_binop, the values of cudf::binary_operator):
 *     ADD SUB MUL in C; DIV '/' in C (integers truncate); TRUE_DIV double(x) / double(y);
 *     FLOOR_DIV integers: exact floor division; floats: NumPy's floor_divide -- floor of (x - fmod(x, y)) / y, corrected as
 *       npy_divmod does, which is floor(x / y) wherever that quotient is exact, NaN for an infinite x, -1 for finite x / -inf of
 *       opposite signs, and a zero that carries the sign of x / y;
 *     MOD '%' (sign of the dividend) / fmod; PMOD and PYMOD on signed integers ((x % y) + y) % y computed without the overflow of
 *       the inner sum, on unsigned x % y; PMOD on floats r = fmod(x, y), r < 0: r = fmod(r + y, y); PYMOD on floats NumPy's
 *       remainder (r = fmod(x, y); r != 0: r += y when the signs of r and y differ; else r = copysign(0, y));
 *     POW pow(double(x), double(y)), powf when C is float; INT_POW (integer C) by squaring, wrapping, 0 for a negative exponent;
 *     BITWISE_AND / OR / XOR, SHIFT_LEFT, SHIFT_RIGHT (integer C; arithmetic for signed C), SHIFT_RIGHT_UNSIGNED a logical shift
 *       of the left operand as the unsigned type of ITS OWN width (an int8 -1 by 1 is 127);
 *     LOGICAL_AND / OR on x != 0, y != 0; EQUAL ... GREATER_EQUAL in C (NaN compares false except under NOT_EQUAL);
 *     NULL_EQUALS / NULL_NOT_EQUALS, NULL_MAX / NULL_MIN ((x < y) ? y : x, (y < x) ? y : x), NULL_LOGICAL_AND / OR: below.
 *     LOG_BASE, ATAN2 and GENERIC_BINARY are not built (gx_binary_op_supported = 0).
 *   Unspecified, as where the reference has C++ undefined behaviour -- integer division or modulo by zero, INT_MIN / -1, shift
 *   counts outside [0, width), a float -> integer cast out of range, the data of a null output row -- but none of them faults,
 *   traps or hangs the kernel.
 *   A side with *_is_scalar is one element in device memory with its validity byte (NULL = valid), as in gx_copy_if_else; the
 *   bitmaps are read from their own begin bits.  out_valid == NULL: no bitmap is read or written (neither side can be null).
 *   Else every one of the (n + 31) / 32 words is written, bits behind the last row 0: ordinary operators lhs bit AND rhs bit (an
 *   invalid scalar makes every row null); NULL_EQUALS / NULL_NOT_EQUALS always valid (both null: true / false, one null: false /
 *   true); NULL_MAX / NULL_MIN valid when either side is, the value that side's when only one is; NULL_LOGICAL_AND / OR Kleene
 *   logic (a valid false / true on either side decides the row, otherwise it is null if either side is).
 *   *out_null_count_dev (optional) = null rows (0 without out_valid).  A workgroup owns gx_elementwise_tile_rows() consecutive
 *   rows per trip (a multiple of 32: one writer per word, no atomics) and at most gx_elementwise_grid_cap() workgroups are
 *   launched; a thread moves 16 bytes per access on the widest of lhs, rhs and out.
 *   GX_EINVAL: n outside [0, 2^31), a negative begin bit, NULL lhs / rhs / out with n > 0, an op outside gx_binop;
 *   GX_EDTYPE: an unknown dtype or a combination gx_binary_op_supported rejects.  n == 0 returns 0 and reads no pointer.
 * gx_unary_op (gx_unop, the values of cudf::unary_operator; IS_NAN / IS_NOT_NAN beside them): ABS (identity on unsigned), NEGATE
 *   (numeric dtypes), SQRT CEIL FLOOR RINT (floats; RINT rounds half to even), BIT_INVERT (integers, not BOOL8): out_dtype ==
 *   in_dtype; NOT: x == 0 into BOOL8 from any dtype; IS_NAN / IS_NOT_NAN: a float into BOOL8.  The transcendental operators,
 *   CBRT and BIT_COUNT are not built.  gx_cast: static_cast between any two dtypes (to BOOL8: x != 0).  Neither touches a
 *   bitmap: the caller copies or shares the input's.  Errors as gx_binary_op.
 * gx_bitmask_to_bool8: out[i] = bit begin_bit + i of valid (NULL: every bit set), inverted with invert != 0.
 * ------------------------------------------------------------------------------------------ */
enum gx_binop {
  GX_BINOP_ADD = 0, GX_BINOP_SUB = 1, GX_BINOP_MUL = 2, GX_BINOP_DIV = 3, GX_BINOP_TRUE_DIV = 4, GX_BINOP_FLOOR_DIV = 5,
  GX_BINOP_MOD = 6, GX_BINOP_PMOD = 7, GX_BINOP_PYMOD = 8, GX_BINOP_POW = 9, GX_BINOP_INT_POW = 10, GX_BINOP_LOG_BASE = 11,
  GX_BINOP_ATAN2 = 12, GX_BINOP_SHIFT_LEFT = 13, GX_BINOP_SHIFT_RIGHT = 14, GX_BINOP_SHIFT_RIGHT_UNSIGNED = 15,
  GX_BINOP_BITWISE_AND = 16, GX_BINOP_BITWISE_OR = 17, GX_BINOP_BITWISE_XOR = 18, GX_BINOP_LOGICAL_AND = 19,
  GX_BINOP_LOGICAL_OR = 20, GX_BINOP_EQUAL = 21, GX_BINOP_NOT_EQUAL = 22, GX_BINOP_LESS = 23, GX_BINOP_GREATER = 24,
  GX_BINOP_LESS_EQUAL = 25, GX_BINOP_GREATER_EQUAL = 26, GX_BINOP_NULL_EQUALS = 27, GX_BINOP_NULL_NOT_EQUALS = 28,
  GX_BINOP_NULL_MAX = 29, GX_BINOP_NULL_MIN = 30, GX_BINOP_GENERIC_BINARY = 31, GX_BINOP_NULL_LOGICAL_AND = 32,
  GX_BINOP_NULL_LOGICAL_OR = 33
};
enum gx_unop {
  GX_UNOP_SIN = 0, GX_UNOP_COS = 1, GX_UNOP_TAN = 2, GX_UNOP_ARCSIN = 3, GX_UNOP_ARCCOS = 4, GX_UNOP_ARCTAN = 5, GX_UNOP_SINH = 6,
  GX_UNOP_COSH = 7, GX_UNOP_TANH = 8, GX_UNOP_ARCSINH = 9, GX_UNOP_ARCCOSH = 10, GX_UNOP_ARCTANH = 11, GX_UNOP_EXP = 12,
  GX_UNOP_LOG = 13, GX_UNOP_SQRT = 14, GX_UNOP_CBRT = 15, GX_UNOP_CEIL = 16, GX_UNOP_FLOOR = 17, GX_UNOP_ABS = 18,
  GX_UNOP_RINT = 19, GX_UNOP_BIT_COUNT = 20, GX_UNOP_BIT_INVERT = 21, GX_UNOP_NOT = 22, GX_UNOP_NEGATE = 23,
  GX_UNOP_IS_NAN = 100, GX_UNOP_IS_NOT_NAN = 101
};
int gx_binary_op(int op, int lhs_dtype, const void* lhs, const uint32_t* lhs_valid, int64_t lhs_begin_bit,
                 const uint8_t* lhs_scalar_valid_dev, int lhs_is_scalar, int rhs_dtype, const void* rhs, const uint32_t* rhs_valid,
                 int64_t rhs_begin_bit, const uint8_t* rhs_scalar_valid_dev, int rhs_is_scalar, int64_t n, int out_dtype, void* out,
                 uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_unary_op(int op, int in_dtype, const void* in, int64_t n, int out_dtype, void* out, gx_stream_t stream);
int gx_cast(int in_dtype, const void* in, int64_t n, int out_dtype, void* out, gx_stream_t stream);
int gx_bitmask_to_bool8(const uint32_t* valid, int64_t begin_bit, int64_t n, int invert, uint8_t* out, gx_stream_t stream);
int gx_binary_op_supported(int op, int lhs_dtype, int rhs_dtype, int out_dtype); /* host only: 1 / 0 */
int gx_unary_op_supported(int op, int in_dtype, int out_dtype);                  /* host only: 1 / 0 */
int gx_elementwise_tile_rows(void);                                              /* rows one workgroup owns per trip */
int gx_elementwise_grid_cap(void);                                               /* most workgroups of one launch */

/* ------------------------------------------------------------------------------------------
 * Expressions (cudf_amd/csrc/gx_expression.hip): cudf::compute_column.  One launch evaluates a whole expression tree over the
 * columns of a table, row by row, with the per-value operators, compute classes and validity rules of the element-wise block
 * above (one copy: csrc/gx_elementwise_ops.hpp): no intermediate column is written.  Conventions as above: raw device pointers,
 * stream-ordered, no host synchronisation, n in [0, 2^31), n == 0 returns 0 and reads no pointer.
 * The expression is a flat post-order array of gx_expr_node: COLUMN (lhs = index into cols), LITERAL (lhs = index into lits), UNARY
 *   (op, lhs = child node), BINARY (op, lhs / rhs = child nodes).  A child's index is below its parent's, the last node is the
 *   root, a node may be the child of several parents (it is then evaluated once per parent).  A literal is one element in device
 *   memory with a device validity byte (NULL = valid), as the scalar sides of gx_binary_op.
 * Types.  C(T) is the compute class of T as a dtype: INT32 for BOOL8 and everything narrower than 32 bits, else T.  The two
 *   operands of a binary node must have the same dtype (no promotion: the caller inserts CAST_TO_*).  gx_ast_op carries the values
 *   of cudf::ast::ast_operator:
 *     ADD SUB MUL DIV MOD PYMOD -> C(T), gx_binary_op's operators in class C(T);  TRUE_DIV -> FLOAT64, double(a) / double(b);
 *     FLOOR_DIV -> FLOAT64, floor(double(a) / double(b)) (not gx_binary_op's integer FLOOR_DIV);  POW -> FLOAT32 on FLOAT32, else
 *     FLOAT64;  BITWISE_AND / OR / XOR -> C(T), integers only;  EQUAL ... GREATER_EQUAL, LOGICAL_AND / OR -> BOOL8;
 *     NULL_EQUAL -> BOOL8, always valid;  NULL_LOGICAL_AND / OR -> BOOL8, Kleene validity;
 *     IDENTITY -> T;  IS_NULL -> BOOL8, always valid;  NOT -> BOOL8 (x == 0);  ABS, BIT_INVERT -> C(T), computed in the class (ABS of
 *     an INT8 -128 is 128), on the dtypes gx_unary_op takes them on;  SQRT CEIL FLOOR RINT -> T, floats;  CAST_TO_INT64 / UINT64 /
 *     FLOAT64 -> the target, gx_cast's conversion.  The transcendental operators and CBRT are not built: GX_EDTYPE.
 *   Every other node is null where an operand is; the data of a null row and the undefined cases of gx_binary_op are unspecified and
 *   do not fault.  a * b + c is two roundings.  out_dtype must equal gx_expr_result_dtype: there is no cast on the final store.
 * gx_compute_column: out_valid (optional) gets every one of the (n + 31) / 32 words, bits behind the last row 0, and nothing behind
 *   them; *out_null_count_dev (optional) the null rows (0 without out_valid).  The bitmaps of the columns are read from their own
 *   begin bits whether or not out_valid is given (IS_NULL and the NULL_* operators see them).  A workgroup owns
 *   gx_expression_tile_rows() consecutive rows per trip (a multiple of 32: one writer per word, no atomics), at most
 *   gx_expression_grid_cap() workgroups are launched, and a thread moves 16 bytes per access on the widest column the expression
 *   reads or the output.  One launch per call; spill slots are LDS; a program without the division family, TRUE_DIV / FLOOR_DIV
 *   and POW runs a variant of the kernel built without them (fewer registers, more waves).
 * gx_expr_plan: the linear program of the accumulator machine the kernel runs, for a model on the host.  Instructions
 *   (gx_expr_instr): LOAD acc = src;  BINARY acc = acc op src;  BINARY_REV acc = src op acc;  UNARY acc = op(acc);  SPILL slot
 *   src_index = acc.  src is a column, a literal or a spill slot; in_dtype is the dtype of the operands (of src for LOAD), out_dtype
 *   that of the accumulator afterwards.  The heavier child of a node runs first, so only a node with two non-leaf children spills,
 *   and *n_slots never exceeds the Strahler number of the tree.  GX_EOVERFLOW when capacity is too small (*n_instructions is set).
 * gx_expr_limits: at most 32 nodes, 16 columns, 16 literals, 4 spill slots; a program has at most 64 instructions (what a tree of 32
 *   nodes can need; shared nodes count once per parent).  Beyond any of them every entry point returns GX_EINVAL.
 * Errors: GX_EINVAL n outside [0, 2^31), a child index not below its parent, a column / literal index out of range, an operator
 *   outside gx_ast_op or of the other arity, a column whose `table` is not 0 (gx_compute_column has one table), NULL where a
 *   pointer is needed with n > 0, a negative begin bit, a limit exceeded;
 *   GX_EDTYPE an unknown dtype, operands of different dtypes, an operator that does not take the dtype, out_dtype != the result's.
 * ------------------------------------------------------------------------------------------ */
enum gx_ast_op {
  GX_AST_ADD = 0, GX_AST_SUB = 1, GX_AST_MUL = 2, GX_AST_DIV = 3, GX_AST_TRUE_DIV = 4, GX_AST_FLOOR_DIV = 5, GX_AST_MOD = 6,
  GX_AST_PYMOD = 7, GX_AST_POW = 8, GX_AST_EQUAL = 9, GX_AST_NULL_EQUAL = 10, GX_AST_NOT_EQUAL = 11, GX_AST_LESS = 12,
  GX_AST_GREATER = 13, GX_AST_LESS_EQUAL = 14, GX_AST_GREATER_EQUAL = 15, GX_AST_BITWISE_AND = 16, GX_AST_BITWISE_OR = 17,
  GX_AST_BITWISE_XOR = 18, GX_AST_LOGICAL_AND = 19, GX_AST_NULL_LOGICAL_AND = 20, GX_AST_LOGICAL_OR = 21,
  GX_AST_NULL_LOGICAL_OR = 22, /* unary from here on */
  GX_AST_IDENTITY = 23, GX_AST_IS_NULL = 24, GX_AST_SIN = 25, GX_AST_COS = 26, GX_AST_TAN = 27, GX_AST_ARCSIN = 28,
  GX_AST_ARCCOS = 29, GX_AST_ARCTAN = 30, GX_AST_SINH = 31, GX_AST_COSH = 32, GX_AST_TANH = 33, GX_AST_ARCSINH = 34,
  GX_AST_ARCCOSH = 35, GX_AST_ARCTANH = 36, GX_AST_EXP = 37, GX_AST_LOG = 38, GX_AST_SQRT = 39, GX_AST_CBRT = 40, GX_AST_CEIL = 41,
  GX_AST_FLOOR = 42, GX_AST_ABS = 43, GX_AST_RINT = 44, GX_AST_BIT_INVERT = 45, GX_AST_NOT = 46, GX_AST_CAST_TO_INT64 = 47,
  GX_AST_CAST_TO_UINT64 = 48, GX_AST_CAST_TO_FLOAT64 = 49
};
enum gx_expr_node_kind { GX_EXPR_COLUMN = 0, GX_EXPR_LITERAL = 1, GX_EXPR_UNARY = 2, GX_EXPR_BINARY = 3 };
enum gx_expr_instr_kind { GX_EXPR_LOAD = 0, GX_EXPR_APPLY = 1, GX_EXPR_APPLY_REV = 2, GX_EXPR_APPLY_UNARY = 3, GX_EXPR_SPILL = 4 };
enum gx_expr_src_kind { GX_EXPR_SRC_COLUMN = 0, GX_EXPR_SRC_LITERAL = 1, GX_EXPR_SRC_SLOT = 2 };
typedef struct gx_expr_node {
  int32_t kind; /* gx_expr_node_kind */
  int32_t op;   /* gx_ast_op of UNARY / BINARY */
  int32_t lhs;  /* column index, literal index, or the (left) child's node index */
  int32_t rhs;  /* BINARY: the right child's node index */
} gx_expr_node;
typedef struct gx_expr_column {
  const void* data;
  const uint32_t* valid; /* NULL: no nulls */
  int64_t begin_bit;     /* row i is bit begin_bit + i of valid */
  int32_t dtype;
  int32_t table; /* 0 = LEFT (the table of gx_compute_column), 1 = RIGHT: the conditional joins below */
} gx_expr_column;
typedef struct gx_expr_literal {
  const void* value;    /* one element, device memory */
  const uint8_t* valid; /* device byte, NULL: valid */
  int32_t dtype;
  int32_t reserved;
} gx_expr_literal;
typedef struct gx_expr_instr {
  uint8_t kind;      /* gx_expr_instr_kind */
  uint8_t op;        /* gx_ast_op of APPLY / APPLY_REV / APPLY_UNARY */
  uint8_t src_kind;  /* gx_expr_src_kind of LOAD / APPLY / APPLY_REV */
  uint8_t src_index; /* column, literal or slot; the slot written by SPILL */
  uint8_t in_dtype;  /* dtype of the operands (LOAD: of src; SPILL: of the accumulator) */
  uint8_t out_dtype; /* dtype of the accumulator afterwards */
  uint8_t family;    /* for the kernel: operator family and the operator of that family (gx_binop / gx_unop) */
  uint8_t family_op;
} gx_expr_instr;
int gx_compute_column(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits,
                      int n_lits, int64_t n, int out_dtype, void* out, uint32_t* out_valid, int64_t* out_null_count_dev,
                      gx_stream_t stream);
/* host only: the root's dtype (> 0) or a gx_error */
int gx_expr_result_dtype(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes,
                         int n_lits);
int gx_expr_plan(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes, int n_lits,
                 gx_expr_instr* out_instructions, int capacity, int* n_instructions, int* n_slots); /* host only */
void gx_expr_limits(int* max_nodes, int* max_columns, int* max_literals, int* max_slots);           /* host only */
int gx_expression_tile_rows(void); /* rows one workgroup owns per trip */
int gx_expression_grid_cap(void);  /* most workgroups of one launch */

/* ------------------------------------------------------------------------------------------
 * Conditional joins (cudf_amd/csrc/gx_conditional_join.hip): cudf::conditional_inner / left / full / left_semi / left_anti_join and
 * their sizes (cpp/include/cudf/join/conditional_join.hpp, cpp/src/join/conditional_join_kernels.cuh).  The predicate is an
 * expression of the block above over the columns of TWO tables: gx_expr_column::table says which (0 LEFT, 1 RIGHT), `cols` holds
 * the columns of both sides in any order (16 together), row i of a LEFT column pairs with every row j of a RIGHT column.  The pair
 * kernel runs the same program gx_compute_column runs (gx_expr_plan gives it, whichever side a column comes from).
 * Contract.
 *   The predicate's result dtype must be BOOL8, else GX_EDTYPE.  A pair matches iff the result is VALID and TRUE: a null result is
 *   no match.  Column validity is read from each column's own begin bit; IS_NULL, NULL_EQUAL, NULL_LOGICAL_* and literals behave
 *   as in gx_compute_column.
 *   Order (fixed here; the reference leaves it open): INNER pairs ascending by (left, right); LEFT the same with (i, INT32_MIN) in
 *   the place of a row i without a match; FULL = LEFT, then (INT32_MIN, r) for the unmatched right rows, r ascending; SEMI / ANTI
 *   left rows ascending.
 *   n_left, n_right in [0, 2^31).  An empty side is not read (its columns' pointers may be NULL): n_left == 0 gives nothing (FULL:
 *   every right row), n_right == 0 gives nothing for INNER / SEMI and every left row for LEFT / FULL / ANTI.
 *   Limits are the expression's (gx_expr_limits; 16 columns over both tables): beyond them GX_EINVAL.
 * Two calls, stream-ordered, no host synchronisation inside; every argument is checked before anything is launched.
 * gx_conditional_join_count: evaluates every pair once.  sizes_dev (device int64[2]): [0] the rows of the result (FULL: the tail
 *   included), [1] the rows of its left-join part (== [0] except for FULL).  Both are tallied in 64 bits and exact beyond 2^31 - 1.
 *   cub-style scratch query (tmp == NULL -> *tmp_bytes, host arithmetic on kind and the row counts, monotone in both); the scratch
 *   then holds what the write pass needs -- INNER / LEFT / FULL: the exclusive scan of the counts per (left row, segment of the right
 *   table), row-major, which IS the output position of that cell's first pair (LEFT / FULL: a row without a match in any segment gets
 *   one place and a byte that says so), FULL: the bitmap of the unmatched right rows (the count pass clears a matched row's bit, one LDS atomic
 *   per wave and matched row, one global atomic per workgroup, chunk and word) and its selection plan; SEMI / ANTI: one bit per left
 *   row and its selection plan (gx_select_valid_count).  The size functions of the reference are this call alone.
 * gx_conditional_join_write: total / left_total are the host's copies of sizes_dev[0] / [1], tmp the scratch of the count call with
 *   the same arguments.  total > 2^31 - 1: GX_EOVERFLOW, before anything is launched.  INNER / LEFT / FULL evaluate the predicate
 *   again (the reference's design) and store a left row's matches in ascending right row from its offset on; out_left / out_right
 *   get `total` rows each.  SEMI / ANTI: out_left gets `total` rows (gx_compact_indices), out_right is not used.
 * The kernel: a workgroup owns a tile of left rows (gx_conditional_join_tile: at most *left_rows; 128 or 64 where the tables are
 *   short) and one segment of the right table (whole chunks of *right_rows rows; as many segments as fill the device when the left
 *   tiles alone do not -- host arithmetic on the two row counts), a thread one left row; the columns the program reads are staged
 *   as 64-bit payloads in LDS per tile and per chunk, and one run of the program evaluates gx_conditional_join_pairs_per_run()
 *   pairs per thread.  At most gx_conditional_join_grid_cap() workgroups per segment are launched.
 *   gx_conditional_join_set_shape (measurement knob; 0 = default): pairs per run in {2, 4, 8}, left rows in {64, 128, 256}
 *   (0: by the device), right rows in {64, 128, 256}; else GX_EINVAL.
 * Errors: GX_EINVAL as gx_compute_column, an unknown kind, `table` outside {0, 1}, total / left_total inconsistent; GX_EDTYPE as
 *   gx_compute_column, a predicate that is not BOOL8; GX_EOVERFLOW see above; GX_ETMP scratch too small.
 * ------------------------------------------------------------------------------------------ */
enum gx_cj_kind { GX_CJ_INNER = 0, GX_CJ_LEFT = 1, GX_CJ_FULL = 2, GX_CJ_SEMI = 3, GX_CJ_ANTI = 4 };
int gx_conditional_join_count(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits,
                              int n_lits, int64_t n_left, int64_t n_right, int kind, int64_t* sizes_dev, void* tmp, size_t* tmp_bytes,
                              gx_stream_t stream);
int gx_conditional_join_write(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits,
                              int n_lits, int64_t n_left, int64_t n_right, int kind, int64_t total, int64_t left_total, const void* tmp,
                              int32_t* out_left, int32_t* out_right, gx_stream_t stream);
void gx_conditional_join_tile(int* left_rows, int* right_rows); /* host only */
int gx_conditional_join_grid_cap(void);                         /* most workgroups of one launch */
int gx_conditional_join_pairs_per_run(void);                    /* R: pairs per thread and run of the program */
int gx_conditional_join_set_shape(int pairs_per_run, int left_rows, int right_rows);

/* ------------------------------------------------------------------------------------------
 * Null and value replacement (cudf_amd/csrc/gx_replace.hip).  Replace the kernels of the reference's cpp/src/replace (nulls.cu,
 * nans.cu, clamp.cu, replace.cu).  All eleven gx_dtype (the functions that compare nothing take the element width in bytes, 1 / 2 /
 * 4 / 8); row counts lie in [0, 2^31).  Bitmaps are Arrow bitmaps read from their own begin bit on (a sliced view needs no
 * re-based copy); every one of the (n + 31) / 32 words of out_valid is written, bits behind the last row 0; *out_null_count_dev
 * (optional, device int64) = nulls written (0 without out_valid).  Values move as bits wherever no comparison is needed: NaN
 * payloads and -0.0 survive.  Every argument check comes before the first device call; n == 0 launches nothing and reads no
 * pointer.  A workgroup owns gx_replace_tile_rows() consecutive rows per trip (a multiple of 64: whole validity words, no atomics
 * on words) and a thread moves 16 bytes per access on the value streams (the policy fill: one row).  Except where noted `out` must
 * not overlap an input.  GX_EINVAL: n outside [0, 2^31), a negative begin bit, a NULL pointer that is needed with n > 0;
 * GX_EDTYPE: an element width or dtype the function does not take; GX_ETMP: scratch too small.
 * gx_replace_nulls: out[i] = bit(in, i) ? in[i] : repl[i], repl[0] with repl_is_scalar: one element in device memory with its
 *   validity byte (NULL = valid), as in gx_copy_if_else.  in_valid NULL = no nulls (a copy).  Output bit = input bit OR
 *   replacement bit; out_valid may be NULL when the caller knows the result has no nulls.  One streaming pass, no scratch; the
 *   replacement is read only where a thread's rows hold a null.
 * gx_replace_nulls_policy: replace_policy PRECEDING (backward == 0) / FOLLOWING: a null row takes the value of the nearest valid
 *   row before / after it and becomes valid; rows without one stay null, their data is unspecified.  in_valid and out_valid are
 *   required.  No workgroup waits for another (no look-back, no tickets), because the source row of every null is a function of
 *   the bitmap: (1) a pass over the bitmap alone writes, per tile of gx_replace_tile_rows() rows, the tile's last (first) valid
 *   row or -1; (2) an exclusive running max over that table, two small launches of fixed depth, gives every tile the nearest
 *   valid row strictly before (after) it; (3) one streaming pass per tile reads the tile's 64 validity words into a per-word
 *   LDS table and resolves each null's source from its own word (clz / ctz), the table, or the carried row, then does one load
 *   in[source] and one store per row, and writes the validity words.  HBM traffic: the column once in and once out plus the
 *   bitmap twice.  Scratch (cub-style query: tmp == NULL -> *tmp_bytes) holds the carry table only: 4 bytes per tile.
 * gx_replace_nans (GX_FLOAT32 / GX_FLOAT64): a valid NaN row takes the replacement's value and validity (column or scalar, as
 *   above); every other row keeps its own value and validity -- a null row stays null whatever its data bits.  out_valid may be
 *   NULL only when neither side can be null (no in_valid, no repl_valid / scalar validity byte): otherwise GX_EINVAL.
 * gx_clamp: out[i] = x < lo ? lo_replace : (x > hi ? hi_replace : x) compared in the column's own dtype (64-bit integers as
 *   integers; BOOL8 as x != 0, a row inside the bounds keeps its byte); a float NaN compares false both ways and passes.  lo, hi,
 *   lo_replace, hi_replace are device scalars of the dtype; *lo_valid_dev / *hi_valid_dev (NULL = valid) == 0, or a NULL bound,
 *   does not bound; a NULL replacement is the bound itself.  Reads and writes no bitmap: the caller copies or shares the
 *   input's, as for gx_unary_op.
 * gx_find_and_replace: out[i] = new_vals[j] for the smallest j in [0, m) with in[i] == old_vals[j], else in[i]; == is the
 *   dtype's (integers and BOOL8: equal bits; floats: NaN matches nothing, -0.0 matches +0.0).  A null input row stays null and
 *   is not compared; a replaced row takes bit new_begin_bit + j of new_valid (NULL = valid).  old_vals is staged through LDS
 *   gx_find_and_replace_chunk() values at a time, the earliest match across chunks wins, so any m in [0, 2^31) works; the cost is
 *   O(n * m) comparisons, like the reference's thrust::find per row: meant for short lists.  m == 0 copies.  out_valid may be
 *   NULL only without in_valid and new_valid.
 * gx_normalize_nans_and_zeros (floats): every NaN becomes the positive quiet NaN 0x7FC00000 / 0x7FF8000000000000, -0.0 becomes
 *   +0.0, everything else is copied bit for bit.  out may equal in.
 * ------------------------------------------------------------------------------------------ */
int gx_replace_tile_rows(void);
int gx_find_and_replace_chunk(void);
int gx_replace_nulls(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, const void* repl,
                     const uint32_t* repl_valid, int64_t repl_begin_bit, const uint8_t* repl_scalar_valid_dev, int repl_is_scalar,
                     int64_t n, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_replace_nulls_policy(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, int backward,
                            void* out, uint32_t* out_valid, int64_t* out_null_count_dev, void* tmp, size_t* tmp_bytes,
                            gx_stream_t stream);
int gx_replace_nans(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, const void* repl,
                    const uint32_t* repl_valid, int64_t repl_begin_bit, const uint8_t* repl_scalar_valid_dev, int repl_is_scalar,
                    int64_t n, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_clamp(int dtype, const void* in, int64_t n, const void* lo, const uint8_t* lo_valid_dev, const void* lo_replace,
             const void* hi, const uint8_t* hi_valid_dev, const void* hi_replace, void* out, gx_stream_t stream);
int gx_find_and_replace(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, const void* old_vals,
                        const void* new_vals, const uint32_t* new_valid, int64_t new_begin_bit, int64_t m, void* out,
                        uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_normalize_nans_and_zeros(int dtype, const void* in, int64_t n, void* out, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Making and reshaping columns (cudf_amd/csrc/gx_reshape.hip).  Replace the kernels of the reference's cpp/src/reshape
 * (interleave_columns.cu, tile.cu), cpp/src/transpose/transpose.cu and cpp/src/filling (fill.cu, repeat.cu, sequence.cu).  The
 * conventions of the row-movement section hold: elem_size is the element width in bytes, 1 / 2 / 4 / 8, and values move as bits;
 * bitmaps are Arrow bitmaps read from a begin bit on; row counts (of inputs AND of the result) lie in [0, 2^31); every argument
 * check comes before the first device call; with no rows nothing is launched; host pointer arrays are not read after the call
 * returns and the stream is not waited for.  With out_valid every one of its (result rows + 31) / 32 words is written exactly once,
 * by one owner and without atomics on words, bits behind the last row 0, nothing behind the last word touched;
 * *out_null_count_dev (optional, device int64) = nulls written.
 * gx_interleave: out[i * ncols + j] = col_j[i]: cudf::interleave_columns, and the whole data movement of cudf::transpose.
 *   cols_host / valid_ptrs_host / begin_bits_host are HOST arrays of ncols entries (valid_ptrs_host NULL or a NULL entry = no
 *   nulls; begin_bits_host NULL = all 0).  A workgroup owns the tile gx_interleave_tile() reports: rows x cols.  Up to 32 columns
 *   the tile holds all of them for a band of rows: each column's stretch is read with 16-byte loads where the addresses allow
 *   (a tile with a column off a 16-byte boundary, and a ragged last band, element by element), laid out in LDS in output order,
 *   and the band leaves as one contiguous run of 16-byte stores.
 *   Above 32 columns the tile is two-dimensional (64 rows x 32 columns): column-wise coalesced reads, row-wise runs of 32
 *   elements on the way out.  The LDS image is padded by one word per 32 and per 1024 words, so the column-strided writes into
 *   it do not fall on one bank.  ncols == 1 is a plain copy.  The validity is composed in a pass of its own, one thread per output
 *   word.  Scratch (cub-style query: tmp == NULL -> *tmp_bytes) holds the column descriptors; they reach it as kernel arguments.
 *   GX_EINVAL: ncols < 1, nrows or nrows * ncols outside [0, 2^31), NULL tmp_bytes / cols_host / out or a NULL column with
 *   rows, a negative begin bit; GX_ETMP: scratch too small.
 * gx_interleave_tile (host only): the tile of gx_interleave for this width and column count; GX_EDTYPE / GX_EINVAL as above.
 * gx_tile: out[r * nrows + i] = in[i] for r in [0, count): the column laid down count times, in one streaming launch whatever
 *   count is; the validity words of the result wrap around the input bitmap (several times inside a word when nrows < 32).
 * gx_repeat_each: out[i * count + k] = in[i] for k in [0, count).  Streaming, no scratch, validity composed per output word.
 *   Both: a workgroup owns gx_reshape_tile_rows() result rows per trip (whole validity words).  GX_EINVAL: nrows, count or
 *   nrows * count outside [0, 2^31), a negative begin bit, NULL in / out with result rows.
 * gx_repeat_map: out_map[e] = the source row of result row e of a per-row repeat, from offsets_dev: the exclusive prefix sum of
 *   the counts as int32, nrows + 1 entries, the last equal to total (the caller has read it to size the result).  A workgroup owns
 *   gx_reshape_tile_rows() result rows: it finds its first source row by binary search, marks in LDS where each source row
 *   with a count begins inside the tile (rows of count 0 share a position with the row behind them, which is the one marked:
 *   the largest row number wins), turns the marks into row numbers with a max-scan and writes them with 16-byte stores.  No
 *   workgroup waits for another; a source row that spans many tiles costs each one binary search.  The values and bitmaps then
 *   go through gx_gather with this map.  No scratch is needed (the query answers 0).  GX_EINVAL: nrows or total outside [0, 2^31),
 *   total > 0 with nrows == 0, NULL tmp_bytes / offsets_dev / out_map with total > 0.
 * gx_fill_range: data[i] = *value_dev (a device scalar of elem_size bytes) for i in [begin, end): elements up to the first
 *   16-byte boundary, 16-byte stores, elements behind the last.  The validity side of cudf::fill is gx_bitmask_set / _copy.
 *   GX_EINVAL: begin < 0, end < begin, end >= 2^31, NULL data / value_dev with begin < end.
 * gx_sequence: out[i] = init + i * step in the column's own type, every numeric gx_dtype (GX_BOOL8: GX_EDTYPE); init_dev /
 *   step_dev are device scalars of the dtype, step_dev NULL = 1.  Integers wrap modulo 2^w.  Floats round twice, the product
 *   T(i) * step and then the sum, as NumPy evaluates init + arange(n).astype(T) * step: no fused multiply-add.
 *   GX_EINVAL: n outside [0, 2^31), NULL out / init_dev with n > 0.
 * ------------------------------------------------------------------------------------------ */
int gx_reshape_tile_rows(void);
int gx_interleave_tile(int elem_size, int ncols, int* rows, int* cols);
int gx_interleave(int elem_size, int ncols, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                  const int64_t* begin_bits_host, int64_t nrows, void* out, uint32_t* out_valid, int64_t* out_null_count_dev,
                  void* tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_tile(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count, void* out,
            uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_repeat_each(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count,
                   void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);
int gx_repeat_map(const int32_t* offsets_dev, int64_t nrows, int64_t total, int32_t* out_map, void* tmp, size_t* tmp_bytes,
                  gx_stream_t stream);
int gx_fill_range(int elem_size, void* data, int64_t begin, int64_t end, const void* value_dev, gx_stream_t stream);
int gx_sequence(int dtype, void* out, int64_t n, const void* init_dev, const void* step_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Quantiles (cudf_amd/csrc/gx_quantile.hip).  Replace the kernels behind cudf::quantile / quantiles (cpp/src/quantiles/quantile.cu,
 * quantiles.cu), the MEDIAN / QUANTILE reductions (cpp/src/reductions/quantile.cu) and the groupby aggregations of the same name
 * (cpp/src/groupby/sort/group_quantiles.cu).  The index and interpolation rules (pos = q * (count - 1); lower / higher / nearest;
 * LINEAR and MIDPOINT without fused multiply-add) are stated once, in the header comment of gx_quantile.hip; gx_interp has the values
 * of cudf::interpolation.  The order is that of the sorts (NaN greatest, -0.0 == +0.0, ties in input order); the ten numeric dtypes
 * are taken, GX_BOOL8 is GX_EDTYPE.  1 <= nq <= 64; q_host is a HOST array, each q clamped to [0, 1], a NaN is GX_EINVAL.
 * gx_quantile: order statistics of an UNSORTED column, nulls (bitmap read from valid_begin_bit on; NULL = none) excluded.
 *   out_f64_dev[nq] = the interpolated results; out_elems_dev[2 * nq] (optional) = the elements at `lower` and `higher` of every q in
 *   the column's own dtype, the very bytes of gx_sort_keys(valid rows)[rank]; *nvalid_dev (device int64) = valid rows: when it is 0
 *   the outputs are unspecified and the caller makes the result null.  n in [0, 2^31).
 *   mode (gx_quantile_mode): FORCE_SELECT = three streaming passes (range, 2048-bin histogram on the top 11 bits of the span, collect
 *   of the rows in the wanted bins) + a sort of the candidates only; FORCE_SORT = valid rows compacted, gx_sort_keys, ranks read;
 *   AUTO = SORT when n < min_rows, else the plan of the select path decides: SORT when candidates > max_share * n
 *   (gx_quantile_set_thresholds, gx_knobs.h), else SELECT.  *path_host (optional, host) = what ran (gx_quantile_path): SELECT_DIRECT when
 *   the span is below 2048 (a bin is a value; also one distinct value, and no valid row on the select side): no collect pass.
 *   HOST ROUND TRIP: the call reads the plan's head (valid count, candidate count, shift) back once and waits for `stream` there --
 *   except FORCE_SORT / AUTO below min_rows without a bitmap, which wait for nothing.  cub-style scratch query (tmp == NULL); the
 *   scratch holds a candidate / compaction buffer and a sorted copy of n elements each beside the sort's own scratch.
 *   GX_EINVAL: n outside [0, 2^31), nq outside [1, 64], NULL q_host / tmp_bytes, a NaN q, unknown interp / mode, a negative begin
 *   bit; with tmp: NULL out_f64_dev / nvalid_dev, NULL data with rows; GX_ETMP.  All before anything touches the device.
 * gx_quantile_status: the status word of the last gx_quantile on `tmp` (0 = ok; a non-zero word -- an index of the collect pass or
 *   of the rank read-out met its bound, nothing was written out of bounds -- also returns GX_EINTERNAL).  Synchronises `stream`.
 * gx_quantile_tile_rows (host): rows one workgroup handles per trip of the streaming passes.
 * gx_quantile_index (host): the shared index helper: lower / higher / nearest / frac for `count` >= 1 rows.
 * gx_quantile_lookup: quantiles of data whose order is KNOWN: out[s * nq + j] for segment s = rows [offsets[s], offsets[s + 1]) of
 *   `order` (int32 map, NULL = the rows themselves), count = seg_counts_dev[s] (NULL = the segment's size): the rows in front of the
 *   segment that take part (groupby: the valid ones, sorted with nulls after).  A whole column is nseg = 1, offsets {0, n}.
 *   exact != 0: out is FLOAT64; else the input dtype (LINEAR / MIDPOINT: static_cast of the double; otherwise the element's bits).
 *   An output is valid when the rows it reads are valid (both neighbours for LINEAR / MIDPOINT, the one row otherwise) and its
 *   count is not 0.  out_valid (optional): (nseg * nq + 31) / 32 words, every one written; *out_null_count_dev (optional).
 *   One thread per output, no scratch.  GX_EINVAL: nseg < 0, nseg * nq >= 2^31, nq outside [1, 64], NULL q_host, NaN q, unknown
 *   interp, negative begin bit, NULL offsets_dev / out with segments.
 * ------------------------------------------------------------------------------------------ */
enum gx_interp { GX_INTERP_LINEAR = 0, GX_INTERP_LOWER = 1, GX_INTERP_HIGHER = 2, GX_INTERP_MIDPOINT = 3, GX_INTERP_NEAREST = 4 };
enum gx_quantile_mode { GX_QUANTILE_AUTO = 0, GX_QUANTILE_FORCE_SELECT = 1, GX_QUANTILE_FORCE_SORT = 2 };
enum gx_quantile_path { GX_QUANTILE_PATH_SELECT = 1, GX_QUANTILE_PATH_SELECT_DIRECT = 2, GX_QUANTILE_PATH_SORT = 3 };
int gx_quantile_tile_rows(void);
int gx_quantile_index(int64_t count, double q, int64_t* lower, int64_t* higher, int64_t* nearest, double* frac);
int gx_quantile(int dtype, const void* data, const uint32_t* valid, int64_t valid_begin_bit, int64_t n, const double* q_host, int nq,
                int interp, int mode, double* out_f64_dev, void* out_elems_dev, int64_t* nvalid_dev, int* path_host, void* tmp,
                size_t* tmp_bytes, gx_stream_t stream);
int gx_quantile_status(const void* tmp, int* status_host, gx_stream_t stream);
int gx_quantile_lookup(int dtype, const void* data, const uint32_t* valid, int64_t begin_bit, const int32_t* order, int64_t nseg,
                       const int32_t* offsets_dev, const int32_t* seg_counts_dev, const double* q_host, int nq, int interp, int exact,
                       void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Hashing / partitioning.
 * gx_murmur3_32: cudf::hashing::detail::MurmurHash3_x86_32<T>
 * (include/cudf/hashing/detail/murmurhash3_x86_32.cuh:22-67), null -> UINT32_MAX, and the
 * column fold of primitive_row_operators.cuh:247-268: combine == 0 writes out[i] = hash(x[i]),
 * combine != 0 writes out[i] = hash_combine(out[i], hash(x[i])) (hashing.hpp:83-86).
 * ------------------------------------------------------------------------------------------ */
int gx_murmur3_32(int dtype, const void* in, const uint32_t* valid, int64_t n, uint32_t seed,
                  int combine, uint32_t* out, gx_stream_t stream);

/* IdentityHash<T> of cudf::hash_partition(..., hash_id::HASH_IDENTITY) (src/partitioning/partitioning.cu:852-872): the element
 * cast to uint32 (static_cast<uint32_t>(key); floating point truncated toward zero, NaN / negative -> 0, >= 2^32 -> UINT32_MAX as
 * the device conversion does), null -> UINT32_MAX, the same column fold as gx_murmur3_32 (combine).  Also what turns a
 * cudf::partition map of any integral type (partitioning.cu:780-842, is_index_type) into the uint32 ids gx_hash_partition_map takes. */
int gx_identity_hash_32(int dtype, const void* in, const uint32_t* valid, int64_t n, int combine,
                        uint32_t* out, gx_stream_t stream);

/* cudf::hash_partition (include/cudf/partitioning.hpp:103-110; src/partitioning/partitioning.cu:
 * 53-92,120-360,568-660) reduced to its index form: from row hashes, a stable gather map that
 * groups rows by partition (hash % num_partitions) plus num_partitions+1 int32 offsets.
 * The caller gathers every column through the map (gx_gather). */
int gx_hash_partition_map(const uint32_t* row_hash, int64_t n, int num_partitions,
                          int32_t* out_map, int32_t* out_offsets, void* tmp, size_t* tmp_bytes,
                          gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Row-key encoding for multi-column join / groupby keys.  The reference hashes and compares whole
 * rows inside its tables (include/cudf/detail/row_operator/primitive_row_operators.cuh:95-163,
 * 207-274); here a row is encoded into ONE fixed-width key first (cf. the reference's own
 * include/cudf/join/key_remapping.hpp) and the single-key kernels below do the rest.
 *
 * gx_pack_keys: out[i] = the ncols (<= 8) column values of row i concatenated into a uint64 (column 0
 *   most significant; widths must sum to <= 8 bytes, else GX_EINVAL).  FLOAT32/64 columns are
 *   normalised (-0.0 -> +0.0, every NaN -> one NaN): the row comparator's equality classes
 *   (detail/row_operator/common_utils.cuh:215-220).  `cols` / `dtypes` are HOST arrays.
 * gx_dense_rank: out_ids[i] in [0, G) with equal values sharing an id (null == null has its own id,
 *   floats compared as above), ids ascending with the value, nulls last; out_rep[g] (optional, n
 *   entries) = the smallest row of id g; *out_ngroups_dev = G.  sorted_order + adjacent difference +
 *   scan + scatter.  cub-style scratch query.
 * ------------------------------------------------------------------------------------------ */
int gx_pack_keys(int ncols, const void* const* cols, const int* dtypes, int64_t n, uint64_t* out,
                 gx_stream_t stream);
/* gx_unpack_keys: the inverse of gx_pack_keys -- out_cols[k][i] = column k of packed[i] (float columns come back
 * normalised: +0.0 for either zero, one NaN).  Turns the distinct packed keys of a groupby back into key columns. */
int gx_unpack_keys(int ncols, void* const* out_cols, const int* dtypes, int64_t n, const uint64_t* packed,
                   gx_stream_t stream);
/* Rows wider than 8 bytes: hash-and-verify.  gx_hash_rows64: out[i] = a 64-bit hash of the ncols (<= 8) column
 *   values of row i (floats normalised as in gx_pack_keys; equal rows hash equal); the single-key join / groupby
 *   kernels then run on the hashes, one pass over the key columns instead of one radix sort per column -- the
 *   reference hashes the row once too (detail/row_operator/primitive_row_operators.cuh:247-268).
 * gx_rows_mismatch_count: *mismatch_dev = the number of pairs (lidx[i], ridx[i]) -- NULL index array = row i
 *   itself, a negative index = no row, skipped -- whose rows differ in some column (the row equality the reference
 *   evaluates inside its probe, primitive_row_operators.cuh:95-163).  0 certifies a result obtained through the
 *   hashes as exact; otherwise (a 64-bit collision) the caller re-runs through gx_dense_rank. */
int gx_hash_rows64(int ncols, const void* const* cols, const int* dtypes, int64_t n, uint64_t seed, uint64_t* out,
                   gx_stream_t stream);
int gx_rows_mismatch_count(int ncols, const void* const* lcols, const void* const* rcols, const int* dtypes,
                           const int32_t* lidx, const int32_t* ridx, int64_t npairs, int64_t* mismatch_dev,
                           gx_stream_t stream);
int gx_dense_rank(int dtype, const void* keys, const uint32_t* valid, int64_t n, int64_t null_count,
                  int32_t* out_ids, int32_t* out_rep, int64_t* out_ngroups_dev, void* tmp,
                  size_t* tmp_bytes, gx_stream_t stream);
/* data[i] = value_bits (low elem_size bytes) for every row whose validity bit is 0 -- cudf::replace_nulls
 * with a scalar (src/replace/nulls.cu), in place; valid == NULL: no-op. */
int gx_fill_nulls(int elem_size, void* data, const uint32_t* valid, int64_t n, uint64_t value_bits,
                  gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Hash join (single fixed-width key column of 4 or 8 bytes; multi-column keys are packed or
 * hashed by the layer above -- see include/cudf/join/).
 * Replaces cudf::detail::hash_join build (src/join/hash_join/hash_join.cu:62-99,112-148 ->
 * cuco::static_multiset::insert) and probe (src/join/hash_join/retrieve_impl.cuh:28-113,
 * size_impl.cuh:26-62 -> cuco count / retrieve).
 *
 * The table is an open-addressing multiset of {key, row} slots followed by one 4-bit tag per slot
 * (0 = empty, else hash bits; the partitioned probe walks chains on the tags in LDS), sized by
 * gx_join_table_bytes = 256 + slots * (slot bytes + 1/2);
 * build rows whose validity bit is 0 are skipped (null_equality::UNEQUAL semantics of
 * hash_join.cu:77-84; for EQUAL the caller maps nulls to a reserved key -- see DESIGN.md).
 * ------------------------------------------------------------------------------------------ */
size_t gx_join_table_bytes(int key_size, int64_t build_rows, double load_factor);
int gx_join_build(int key_size, const void* build_keys, const uint32_t* build_valid,
                  int64_t build_rows, void* table, size_t table_bytes, double load_factor,
                  gx_stream_t stream);
/* Number of matches: *count_dev (device int64).  probe_valid NULL = all valid. */
int gx_join_count(int key_size, const void* probe_keys, const uint32_t* probe_valid,
                  int64_t probe_rows, const void* table, size_t table_bytes, int64_t* count_dev,
                  gx_stream_t stream);
/* Emits pairs (probe_idx, build_idx) in unspecified order (include/cudf/join/join.hpp:131-134)
 * through a device cursor *cursor_dev (must be zeroed by the caller); pairs beyond `capacity`
 * are counted but not written (caller compares the cursor with capacity).
 * left_outer bit 0: probe rows without a match emit (probe_idx, INT32_MIN) -- cudf::left_join
 * (src/join/join.cu:62-85).  left_outer bit 1 (with bit 0): NULL probe rows emit nothing -- under
 * null_equality::EQUAL with null build rows present their partners are those rows, which the caller appends
 * (hash_join.cu:77-84). */
int gx_join_probe(int key_size, const void* probe_keys, const uint32_t* probe_valid,
                  int64_t probe_rows, const void* table, size_t table_bytes, int left_outer,
                  int32_t* out_probe_idx, int32_t* out_build_idx, int64_t capacity,
                  int64_t* cursor_dev, gx_stream_t stream);

/* Partitioned form of gx_join_probe for large probes (no probe nulls) against tables far beyond the
 * L2s: the probe rows are radix-partitioned on the table's top hash bits (one streaming pass), then
 * probed partition by partition with XCD-affine scheduling so that each ~2 MiB sub-table is L2
 * resident while it is probed.  Same outputs and cursor convention as gx_join_probe (pair order
 * unspecified).  cub-style scratch query.  GX_EINVAL when the table is too small to partition
 * (gx_join_partition_bits() == 0): use gx_join_probe. */
int gx_join_probe_partitioned(int key_size, const void* probe_keys, int64_t probe_rows, const void* table,
                              size_t table_bytes, int left_outer, int32_t* out_probe_idx,
                              int32_t* out_build_idx, int64_t capacity, int64_t* cursor_dev, void* tmp,
                              size_t* tmp_bytes, gx_stream_t stream);
/* Partitioned form of gx_join_build for large build sides without nulls: the rows are radix-
 * partitioned on the table's top hash bits, then inserted partition by partition so that the CAS
 * and slot writes of concurrently running workgroups fall into one L2-resident ~2 MiB sub-table.
 * Produces the same table as gx_join_build (slot positions may differ among equal hashes).
 * cub-style scratch query.  GX_EINVAL when the table is too small to partition. */
int gx_join_build_partitioned(int key_size, const void* build_keys, int64_t build_rows, void* table,
                              size_t table_bytes, double load_factor, void* tmp, size_t* tmp_bytes,
                              gx_stream_t stream);
/* Matches per probe row: counts[i] = max(min_count, number of build rows whose key equals probe key i); null probe
 * rows count 0.  The per-row form of gx_join_count behind cudf::hash_join::*_join_match_context
 * (cpp/include/cudf/join/hash_join.hpp:259-340; cpp/src/join/hash_join/size_impl.cuh:26-62). */
int gx_join_count_rows(int key_size, const void* probe_keys, const uint32_t* probe_valid, int64_t probe_rows,
                       const void* table, size_t table_bytes, int32_t min_count, int32_t* counts, gx_stream_t stream);
/* data[i] += value wherever data[i] != INT32_MIN (JoinNoMatch): re-bases the probe indices of a chunk of a
 * partitioned join (hash_join.hpp:352-440) onto the whole left table. */
int gx_add_i32(int32_t* data, int64_t n, int32_t value, gx_stream_t stream);
/* One-pass partition of rows into `nparts` <= 16 contiguous groups (histogram + LDS-ranked scatter, the partition pass
 * of the partitioned join): out_keys = the keys grouped by destination (order inside a group unspecified), out_rows
 * (optional) = their row indices, offsets_dev[nparts + 1] = group starts (device int64).  What a rank runs before the
 * all-to-all of the distributed operators (cudf::hash_partition, cpp/src/partitioning/partitioning.cu:568-660, feeding
 * the shuffle of cpp/libcudf_streaming/src/partition_utils.cpp:72-117):
 *   mode 0  destination = the top 32 bits of a multiplicative hash independent of the join table's slot bits, scaled into
 *           [0, nparts) by a multiply-shift (any nparts; for a power of two these are the hash's top bits);
 *           key_dtype any 4- or 8-byte type (bit patterns are hashed);
 *   mode 1  destination = number of splitters <= key in cudf sort order; splitters_host = nparts - 1 ascending keys
 *           of key_dtype in HOST memory (INT32/UINT32/FLOAT32/INT64/UINT64/FLOAT64).
 * cub-style scratch query. */
int gx_partition_rows(int key_dtype, const void* keys, int64_t n, int mode, int nparts, const void* splitters_host,
                      void* out_keys, int32_t* out_rows, int64_t* offsets_dev, void* tmp, size_t* tmp_bytes,
                      gx_stream_t stream);
/* The same pass over a CHUNK of a shard: out_rows[i] = row_base + (index inside `keys`), so that chunks of one column can be
 * partitioned (and exchanged) one after the other while the row ids stay those of the whole shard. */
int gx_partition_rows_at(int key_dtype, const void* keys, int64_t n, int32_t row_base, int mode, int nparts, const void* splitters_host,
                         void* out_keys, int32_t* out_rows, int64_t* offsets_dev, void* tmp, size_t* tmp_bytes,
                         gx_stream_t stream);
/* The SPECULATIVE form (cap_rows > 0): no histogram pass.  Group g owns the fixed slot [g, g + 1) * cap_rows of out_keys /
 * out_rows (which hold nparts * cap_rows elements); offsets_dev[g] receives the ROWS of group g (not a start), offsets_dev[nparts]
 * is non-zero when some group outgrew its slot -- its surplus rows were dropped and the caller must partition this input again
 * with the exact form.  What the sharded operators run per chunk before an exchange: one read of the keys instead of two. */
int gx_partition_rows_spec_at(int key_dtype, const void* keys, int64_t n, int32_t row_base, int mode, int nparts, const void* splitters_host,
                              int64_t cap_rows, void* out_keys, int32_t* out_rows, int64_t* offsets_dev, void* tmp, size_t* tmp_bytes,
                              gx_stream_t stream);
/* gx_join_probe_partitioned for a chunk of the probe side: the probe indices written are row_base + (index inside probe_keys);
 * pairs are appended at *cursor_dev (which the caller zeroes once, before the first chunk). */
int gx_join_probe_partitioned_at(int key_size, const void* probe_keys, int64_t probe_rows, int32_t row_base, const void* table,
                                 size_t table_bytes, int left_outer, int32_t* out_probe_idx, int32_t* out_build_idx,
                                 int64_t capacity, int64_t* cursor_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
/* PAYLOAD forms: a build / probe row is represented by payload[i] (int32 >= 0) instead of its row number i -- what the table
 * slots store and what the pair arrays receive.  The sharded join puts encoded global rows there (gx_decode_global_rows). */
int gx_join_build_pl(int key_size, const void* build_keys, const int32_t* payload, const uint32_t* build_valid, int64_t build_rows,
                     void* table, size_t table_bytes, double load_factor, gx_stream_t stream);
int gx_join_build_partitioned_pl(int key_size, const void* build_keys, const int32_t* payload, int64_t build_rows, void* table,
                                 size_t table_bytes, double load_factor, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_join_probe_partitioned_pl(int key_size, const void* probe_keys, const int32_t* payload, int64_t probe_rows, int32_t row_base,
                                 const void* table, size_t table_bytes, int left_outer, int32_t* out_probe_idx, int32_t* out_build_idx,
                                 int64_t capacity, int64_t* cursor_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
/* log2 of the number of partitions the partitioned probe uses for this table; 0 = not partitionable */
int gx_join_partition_bits(int key_size, size_t table_bytes);

/* out_build_idx[i] = the first build row whose key equals probe key i, or INT32_MIN (JoinNoMatch) --
 * the left join against DISTINCT build keys, in probe order and without an output reservation:
 * cudf::distinct_hash_join::left_join (include/cudf/join/distinct_hash_join.hpp:111-116,
 * src/join/distinct_hash_join.cu).  Null probe rows (validity bit 0) get JoinNoMatch. */
int gx_join_lookup(int key_size, const void* probe_keys, const uint32_t* probe_valid, int64_t probe_rows,
                   const void* table, size_t table_bytes, int32_t* out_build_idx, gx_stream_t stream);
/* Left semi (anti == 0) / left anti (anti != 0) join: the ASCENDING list of probe rows that have
 * (have no) match in the table, *count_dev = its length -- the contains map + stable copy_if of
 * cudf::filtered_join::semi_join / anti_join (src/join/filtered_join/filtered_join.cu:124-156).
 * Null probe rows count as matching iff null_matches != 0 (null_equality::EQUAL and the build side
 * holds a null).  out_probe_idx needs room for probe_rows entries.  cub-style scratch query. */
int gx_join_filter(int key_size, const void* probe_keys, const uint32_t* probe_valid, int64_t probe_rows,
                   const void* table, size_t table_bytes, int anti, int null_matches,
                   int32_t* out_probe_idx, int64_t* count_dev, void* tmp, size_t* tmp_bytes,
                   gx_stream_t stream);

/* cudf::full_join's complement step (src/join/join_utils.cu:86-157): appends (JoinNoMatch, r) for
 * every build row r in [0, build_rows) that does not occur in build_idx[0..n) to the pair arrays,
 * starting at *cursor_dev (device int64: pairs already present, updated to the new total; pairs
 * beyond `capacity` are counted but not written).  tmp: cub-style query. */
int gx_join_complement(const int32_t* build_idx, int64_t n, int64_t build_rows, int32_t* out_probe_idx,
                       int32_t* out_build_idx, int64_t capacity, int64_t* cursor_dev, void* tmp,
                       size_t* tmp_bytes, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Groupby, hash path (single int32/int64 key column; values int32/int64/float32/float64).
 * Replaces src/groupby/hash/compute_groupby.cu:50-155 + compute_global_memory_aggs.cuh:123-157:
 * distinct keys (unspecified order) and per-group SUM / COUNT_VALID / COUNT_ALL / MIN / MAX.
 * float sums are accumulated in 128-bit fixed point (exact, order independent, bit-reproducible)
 * and rounded once: see DESIGN.md "groupby".  Outputs have capacity `max_groups`; *ngroups_dev
 * (device int64) receives the group count.  Rows with key validity 0 are dropped
 * (null_policy::EXCLUDE, compute_groupby.cu:62-66).
 * ------------------------------------------------------------------------------------------ */
int gx_groupby_sum_count(int key_dtype, const void* keys, const uint32_t* keys_valid,
                         int val_dtype, const void* vals, const uint32_t* vals_valid, int64_t n,
                         int64_t max_groups, void* out_keys, void* out_sum /* f64 or i64 */,
                         int32_t* out_count_valid, int32_t* out_count_all, int64_t* ngroups_dev,
                         void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* Groupby SUM + COUNT on SEVERAL key columns, rows compared inside the table (the reference hashes a row once and
 * compares rows in its probe: include/cudf/detail/row_operator/primitive_row_operators.cuh:95-163, 247-268).
 * key_cols: nkeys (2..4) HOST array of device pointers to columns of 8-byte words (int64 / uint64 columns as they are;
 * narrower integer columns widened by the caller); out_key_cols: nkeys device columns of capacity max_groups that
 * receive the groups' key words.  No nulls (nullable inputs take gx_hash_rows64 + gx_groupby_sum_count).  Groups come
 * out in unspecified order.  *ngroups_dev: the group count; -1: more than max_groups groups (retry with a larger bound);
 * -2: keys skewed beyond the partition slots / more groups per partition than an LDS table holds -- the caller takes the
 * single-key path over row hashes instead (nothing usable was written). */
int gx_groupby_sum_count_wide(int nkeys, const void* const* key_cols, int val_dtype, const void* vals, int64_t n,
                              int64_t max_groups, void* const* out_key_cols, void* out_sum /* f64 or i64 */,
                              int32_t* out_count, int64_t* ngroups_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* Groupby MIN / MAX of one value column (src/groupby/hash/global_memory_aggregator.cuh:18-238):
 * same conventions as gx_groupby_sum_count; out_min / out_max have the VALUE dtype (either may be
 * NULL); a group without a valid value has count 0 and an unspecified min/max (the caller nulls it).
 * Floats: -0.0 == +0.0, NaN greater than every number (the row comparator's order). */
int gx_groupby_min_max(int key_dtype, const void* keys, const uint32_t* keys_valid, int val_dtype,
                       const void* vals, const uint32_t* vals_valid, int64_t n, int64_t max_groups,
                       void* out_keys, void* out_min, void* out_max, int32_t* out_count_valid,
                       int64_t* ngroups_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* Compound groupby aggregations on top of gx_groupby_sum_count / gx_groupby_min_max.
 * gx_square: out[i] = in[i]^2 in the SUM accumulator type of `dtype` (integers -> int64 wrapping mod
 *   2^64, FLOAT32/64 keep their type): the values of the reference's single-pass SUM_OF_SQUARES
 *   (include/cudf/detail/aggregation/aggregation.hpp:944-954), summed by gx_groupby_sum_count.
 * gx_square_centered: out[i] = (in[i] - mean[group_of_row[i]])^2 in FLOAT64, 0 where group_of_row[i] is
 *   outside [0, num_groups) (a row whose key is null).  The second pass of the float VARIANCE / STD / M2:
 *   mean = gx_mean_from_sum of the SUM pass, the squares are summed by the same SUM pass as the values.
 * gx_var_from_sums: mode 0 M2 (valid for every group), 1 VARIANCE = M2/(count-ddof),
 *   2 STD = sqrt(VARIANCE); null where count == 0 or count - ddof <= 0
 *   (src/groupby/common/m2_var_std.cu:44-61,153-190; hash_compound_agg_finalizer.cu:135-186).
 *   sum != NULL (integer values, sum_dtype GX_INT64; also GX_FLOAT64): M2 = sum_sqr - sum^2/count in double.
 *   sum == NULL (float values, sum_dtype GX_FLOAT64): sum_sqr is the sum of gx_square_centered and M2 is that
 *   sum, with a negative one raised to 0 and a NaN kept.
 *   mask_out holds ceil(n/32) words; *null_count_dev = nulls.
 * gx_groupby_arg_select: ARGMIN / ARGMAX (global_memory_aggregator.cuh: ARGMIN/ARGMAX updates): out_rows[g] =
 *   the smallest row i with group_of_row[i] == g, a valid value and vals[i] == target[g] (target = the
 *   group's MIN or MAX; floats NaN == NaN); 0x7F7F7F7F where the group has no valid value. */
int gx_square(int dtype, const void* in, int64_t n, void* out, gx_stream_t stream);
int gx_square_centered(const double* in, const int32_t* group_of_row, const double* mean, int64_t n,
                       int64_t num_groups, double* out, gx_stream_t stream);
int gx_var_from_sums(int sum_dtype, const void* sum_sqr, const void* sum, const int32_t* count, int64_t n,
                     int ddof, int mode, double* out, uint32_t* mask_out, int64_t* null_count_dev,
                     gx_stream_t stream);
int gx_groupby_arg_select(int val_dtype, const void* vals, const uint32_t* vals_valid,
                          const int32_t* group_of_row, int64_t n, const void* target, int64_t num_groups,
                          int32_t* out_rows, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sort-based groupby building blocks: rows that are (or have been brought, through `order`) in key order.
 * Replace compute_group_offsets / label_segments (cpp/src/groupby/sort/sort_helper.cu:151-214),
 * thrust::reduce_by_key of the sort-path aggregations (sort/group_single_pass_reduction_util.cuh:133-200,
 * sort/group_count.cu:25-89), segmented_shift (groupby.cu:306-346), group_replace_nulls
 * (sort/group_replace_nulls.cu) and the rank scans of cpp/src/sort/rank.cu:60-330.
 *
 * gx_group_heads: heads[i] = 1 iff row order[i] differs from row order[i - 1] in this column (order NULL =
 *   identity; heads[0] = 1; null == null, NaN == NaN, -0.0 == +0.0); combine != 0 ORs into `heads`, so a key
 *   TABLE is one call per column.
 * gx_group_offsets: labels[i] = group of sorted row i, offsets[g] = first sorted row of group g,
 *   offsets[ngroups] = n (capacity n + 1), sizes (optional, capacity n) = rows per group; *ngroups_dev.
 * gx_segmented_reduce: one value per group at out[label] -- op GX_OP_SUM / PRODUCT (integers -> INT64, floats
 *   keep their type; float SUM in double-double: <= 1 ulp, order-independent), MIN / MAX (input type),
 *   COUNT_VALID (out NULL); out_count_valid (optional) = valid values per group.  `vals` are in sorted order.
 * gx_segmented_shift: out[i] = in[i - offset] when that row is in the same group, else the fill value
 *   (fill_valid == 0: null); out_valid (optional) holds ceil(n/64)*2 words.
 * gx_segmented_fill_nulls: replace_policy PRECEDING (backward == 0) / FOLLOWING: a null takes the nearest valid
 *   value of its group before / after it, or stays null.
 * gx_rank_from_groups: scatter ranks to out[order[i]]: method 0 FIRST, 1 AVERAGE, 2 MIN, 3 MAX, 4 DENSE
 *   (rank_method, cpp/include/cudf/aggregation.hpp:91-98); scale > 0 = percentage (rank / scale, or
 *   (rank - 1) / (scale - 1) when one_normalized); exactly one of out_i32 / out_f64.
 * ------------------------------------------------------------------------------------------ */
int gx_group_heads(int dtype, const void* col, const uint32_t* valid, const int32_t* order, int64_t n, int combine,
                   uint8_t* heads, gx_stream_t stream);
int gx_group_offsets(const uint8_t* heads, int64_t n, int32_t* labels, int32_t* offsets, int32_t* sizes,
                     int64_t* ngroups_dev, void* tmp, size_t* tmp_bytes, gx_stream_t stream);
int gx_segmented_reduce(int val_dtype, const void* vals, const uint32_t* vals_valid, const uint8_t* heads,
                        const int32_t* labels, int64_t n, int op, void* out, int32_t* out_count_valid, void* tmp,
                        size_t* tmp_bytes, gx_stream_t stream);
int gx_segmented_shift(int elem_size, const void* in, const uint32_t* in_valid, const int32_t* labels, int64_t n,
                       int64_t offset, uint64_t fill_bits, int fill_valid, void* out, uint32_t* out_valid,
                       gx_stream_t stream);
int gx_segmented_fill_nulls(int elem_size, const void* in, const uint32_t* in_valid, const uint8_t* heads, int64_t n,
                            int backward, void* out, uint32_t* out_valid, void* tmp, size_t* tmp_bytes,
                            gx_stream_t stream);
int gx_rank_from_groups(const int32_t* order, const int32_t* labels, const int32_t* offsets, int64_t n, int method,
                        double scale, int one_normalized, int32_t* out_i32, double* out_f64, gx_stream_t stream);
/* Segment id of every row for cudf::segmented_sorted_order (cpp/src/sort/segmented_sort_impl.cuh:178-203): rows of
 * segment [offsets[j], offsets[j+1]) get offsets[j+1]; rows outside every segment get unique ascending ids. */
int gx_segment_ids(const int32_t* offsets, int64_t num_offsets, int64_t num_rows, int32_t* ids, gx_stream_t stream);


/* Result finalizers of cudf::groupby::aggregate: (a) validity bitmap of SUM / MEAN results from
 * COUNT_VALID -- a group without a valid value is null (src/groupby/hash/output_utils.cu:68-70);
 * *null_count_dev (device int64) receives the number of null groups; mask_out needs
 * (n + 31) / 32 words.  (b) MEAN = SUM / COUNT_VALID computed in double
 * (src/groupby/hash/hash_compound_agg_finalizer.cu:92-133); sum_dtype in {INT64, FLOAT64, FLOAT32}. */
int gx_valid_from_counts(const int32_t* counts, int64_t n, uint32_t* mask_out, int64_t* null_count_dev,
                         gx_stream_t stream);
int gx_mean_from_sum(int sum_dtype, const void* sum, const int32_t* count, int64_t n, double* out,
                     gx_stream_t stream);

/* Segmented inclusive scan over sorted group labels: replaces thrust::inclusive_scan_by_key at
 * src/groupby/sort/group_scan_util.cuh:109-130 (groupby::scan SUM/MIN/MAX).  keys are the
 * (already sorted) key column; out[i] = op over the rows of the same key run up to i.
 * Null values (vals_valid bit 0) contribute the identity. Integer SUM accumulates in int64.
 * op GX_OP_COUNT_VALID / GX_OP_COUNT_ALL (sort/group_count_scan.cu:24-62): out is INT32, out[i] = valid rows (all
 * rows) of the run up to and including i; `vals` is not read and may be NULL. */
int gx_segmented_scan(int key_dtype, const void* sorted_keys, int val_dtype, const void* vals,
                      const uint32_t* vals_valid, int64_t n, int op, void* out, void* tmp,
                      size_t* tmp_bytes, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Column reduce / scan.
 * gx_reduce replaces cub::DeviceReduce::Reduce at include/cudf/reduction/detail/reduction.cuh:
 * 46-83 (cudf::reduce SUM/MIN/MAX/PRODUCT; nulls skipped).  Result written to *out_dev in
 * `out_dtype` (GX_INT64, GX_UINT64 or GX_FLOAT64 for SUM/PRODUCT; in_dtype for MIN/MAX; an integer type for
 * GX_OP_COUNT_NONZERO, the number of valid elements != 0 -- ANY = count > 0, ALL = count == valid count);
 * *valid_count_dev (device int64, optional) = number of valid inputs.
 * gx_scan replaces thrust::inclusive_scan / exclusive_scan at
 * src/reductions/scan/scan_inclusive.cu:76-89 and scan_exclusive.cu; output dtype == input
 * dtype (ints wrap); nulls contribute the identity (null_policy handling of the mask is done by
 * the caller: scan_inclusive.cu:198-216).
 * Float MIN / MAX -- here, in gx_segmented_scan and in gx_segmented_reduce -- use the order of the sorts and of the hash
 * groupby: every NaN is one value above +inf (and equal to every other NaN), -0.0 == +0.0 (which zero comes back is
 * unspecified), nulls never take part.  MIN is the smallest non-NaN valid value and NaN only when every valid value is NaN;
 * MAX is NaN once a valid value is NaN; a running MIN is NaN until the first non-NaN valid value.  The result does not depend
 * on where the rows sit.  Row 0 of an exclusive scan (and every row with no valid value before it) holds +inf / -inf.
 * ------------------------------------------------------------------------------------------ */
int gx_reduce(int in_dtype, const void* in, const uint32_t* valid, int64_t n, int op,
              int out_dtype, void* out_dev, int64_t* valid_count_dev, void* tmp, size_t* tmp_bytes,
              gx_stream_t stream);
int gx_scan(int dtype, const void* in, const uint32_t* valid, int64_t n, int op, int inclusive,
            void* out, void* tmp, size_t* tmp_bytes, gx_stream_t stream);

/* index of the first 0 bit in [0,nbits) or nbits: *pos_dev (device int64).  Used for the
 * null_policy::INCLUDE scan mask (scan_inclusive.cu:44-53 thrust::find_if_not). */
int gx_bitmask_first_unset(const uint32_t* mask, int64_t nbits, int64_t* pos_dev, gx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Synthetic data (bench / tests): counter-based generator so that 1e9-row inputs never cross
 * PCIe.  out[i] = splitmix64(seed + i) mapped to the dtype; `lo`,`hi` bound integer outputs
 * when hi > lo (uniform in [lo, hi)), floats are uniform in [0,1).
 * ------------------------------------------------------------------------------------------ */
int gx_fill_random(int dtype, void* out, int64_t n, uint64_t seed, int64_t lo, int64_t hi,
                   gx_stream_t stream);
/* data[i] = mix64(data[i]) in place, mix64 = the splitmix64 FINALIZER (a bijection of the 64-bit integers): ids j in [0, m)
 * become m distinct keys that look random in every bit -- the join benchmarks' key sets (distinct random build keys,
 * a probe side that hits them with a chosen probability; cpp/benchmarks/join/generate_input_tables.cu:24-103). */
int gx_mix64_inplace(uint64_t* data, int64_t n, gx_stream_t stream);
/* device-to-device copy as a KERNEL on `stream` (16-byte lanes): what a rank does with the part of an exchange that stays
 * on it.  hipMemcpyAsync picks the SDMA engines when other queues are busy -- 32 GB/s for an intra-device copy on this
 * part, measured (profiles/r3_xp_distributed_single_rank.txt: 252 ms for 8 GB in chunks, 4 ms as one kernel). */
int gx_copy_bytes(const void* src, void* dst, size_t bytes, gx_stream_t stream);
/* iota: out[i] = start + i (int32) */
int gx_sequence_i32(int32_t* out, int64_t n, int32_t start, gx_stream_t stream);
/* order-independent 64-bit checksum of a column (sum and xor of splitmix64(element)) and a
 * sortedness violation count in the column's cudf order: res_dev[0]=sum, [1]=xor, [2]=violations */
int gx_checksum(int dtype, const void* in, int64_t n, int descending, uint64_t* res_dev,
                gx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CUDF_AMD_GX_H */
