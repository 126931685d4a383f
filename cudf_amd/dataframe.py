"""Thin pandas-like wrapper over the hot path (the cudf.DataFrame surface of the reference, reduced
to the methods that land on it): sort_values, merge, groupby(...).agg, rolling(...), df[mask], dropna, drop_duplicates, where, mask;
concat(frames) beside it.

reference: python/cudf/cudf/core/dataframe.py (sort_values -> core/_internals/sorting.py ->
pylibcudf.sorting.sorted_order + gather; merge -> core/join/join.py -> pylibcudf.join.inner_join /
left_join / full_join / left_semi_join / left_anti_join + gather; groupby(...).agg -> core/groupby/groupby.py -> pylibcudf.groupby.aggregate).
Columns are fixed-width numeric; data moves host<->device only in from_pandas / to_pandas.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from . import ops
from .column import Column, bitmask_words, ptr, stream_ptr

_lib = L.lib


class DataFrame:
    def __init__(self, data: Optional[Dict[str, Union[Column, np.ndarray, Sequence]]] = None):
        self._cols: Dict[str, Column] = {}
        for name, v in (data or {}).items():
            self[name] = v

    # ---- construction / export
    @classmethod
    def from_pandas(cls, pdf) -> "DataFrame":
        df = cls()
        for name in pdf.columns:
            s = pdf[name]
            if s.isna().any():
                valid = ~s.isna().to_numpy()
                vals = s.fillna(0).to_numpy()
                df._cols[str(name)] = Column.from_numpy(vals, valid)
            else:
                df._cols[str(name)] = Column.from_numpy(s.to_numpy())
        return df

    def to_pandas(self):
        import pandas as pd
        out = {}
        for name, c in self._cols.items():
            v = c.to_numpy()
            if c.has_nulls():
                m = c.valid_numpy()
                v = v.astype(np.float64) if v.dtype.kind != "f" else v.copy()
                v[~m] = np.nan
            out[name] = v
        return pd.DataFrame(out)

    # ---- dict-like
    def __setitem__(self, name: str, value):
        col = value if isinstance(value, Column) else Column.from_numpy(np.asarray(value))
        if self._cols and len(col) != len(self):
            raise ValueError("Length of values does not match length of index")
        self._cols[name] = col

    def __getitem__(self, key):
        """df["name"] -> the column; df[mask] -> the rows where a bool Column / NumPy bool array of len(df) is true, in row order
        (a null mask element drops its row)"""
        if isinstance(key, str):
            return self._cols[key]
        if isinstance(key, np.ndarray):
            if key.dtype != np.bool_:
                raise TypeError("a row mask must be a bool array")
            key = Column.from_numpy(key)
        if not isinstance(key, Column):
            raise TypeError(f"unsupported key type {type(key).__name__}")
        if key.dtype != np.bool_:
            raise TypeError("a row mask must be a bool Column")
        if key.size != len(self):
            raise ValueError(f"Item wrong length {key.size} instead of {len(self)}.")
        return self._from_columns(ops.apply_boolean_mask(list(self._cols.values()), key))

    def eval(self, text: str) -> Column:
        """pandas' DataFrame.eval for one expression over the columns: names, numeric literals, + - * / // % **, comparisons,
        & | ~, and / or / not, parentheses (cudf_amd.ast.parse_eval has the typing rules).  The whole expression is one launch
        (ops.compute_column); the Column operators stay eager."""
        from .ast import parse_eval
        expr, _ = parse_eval(text, {name: c.dtype for name, c in self._cols.items()})
        return ops.compute_column(list(self._cols.values()), expr)

    def query(self, text: str) -> "DataFrame":
        """pandas' DataFrame.query: the rows where the bool expression `text` is true, in row order (a null drops its row)"""
        mask = self.eval(text)
        if mask.dtype != np.bool_:
            raise ValueError(f"query: {text!r} is a {mask.dtype} expression, not a bool one")
        return self._from_columns(ops.apply_boolean_mask(list(self._cols.values()), mask))

    def _from_columns(self, cols: Sequence[Column]) -> "DataFrame":
        out = DataFrame()
        for name, c in zip(self._cols, cols):
            out._cols[name] = c
        return out

    def dropna(self, subset: Optional[Union[str, Sequence[str]]] = None, how: Optional[str] = None,
               thresh: Optional[int] = None) -> "DataFrame":
        """pandas' DataFrame.dropna(axis=0): a null or a NaN counts as missing.  how="any" (default) drops a row with any missing
        value among `subset` (default: every column), how="all" one whose values are all missing; thresh keeps the rows with at
        least that many values present.  Row order is kept."""
        if how is not None and thresh is not None:
            raise TypeError("You cannot set both the how and thresh arguments at the same time.")
        if how not in (None, "any", "all"):
            raise ValueError(f"invalid how option: {how}")
        names = list(self._cols) if subset is None else ([subset] if isinstance(subset, str) else list(subset))
        for k in names:
            if k not in self._cols:
                raise KeyError(k)
        order = list(self._cols)
        keys = [order.index(k) for k in names]
        need = int(thresh) if thresh is not None else (1 if how == "all" else len(keys))
        return self._from_columns(ops.dropna_rows(list(self._cols.values()), keys, need))

    def drop_duplicates(self, subset: Optional[Union[str, Sequence[str]]] = None, keep: Union[str, bool] = "first") -> "DataFrame":
        """pandas' DataFrame.drop_duplicates: of the rows that are equal in `subset` (default: every column) keep the first
        (keep="first"), the last ("last") or none (False).  Row order is kept; nulls are equal to nulls and NaNs to NaNs, as in pandas."""
        if keep not in ("first", "last", False):
            raise ValueError('keep must be either "first", "last" or False')
        names = list(self._cols) if subset is None else ([subset] if isinstance(subset, str) else list(subset))
        for k in names:
            if k not in self._cols:
                raise KeyError(k)
        order = list(self._cols)
        keys = [order.index(k) for k in names]
        return self._from_columns(ops.distinct(list(self._cols.values()), keys, keep=keep or "none"))

    def __len__(self) -> int:
        return next(iter(self._cols.values())).size if self._cols else 0

    @property
    def columns(self) -> List[str]:
        return list(self._cols)

    def _take(self, gather_map: Column, nullify: bool = False) -> "DataFrame":
        out = DataFrame()
        for name, c in self._cols.items():
            out._cols[name] = ops.gather(c, gather_map, nullify_out_of_bounds=nullify)
        return out

    # ---- the hot path
    def sort_values(self, by: Union[str, Sequence[str]], ascending: Union[bool, Sequence[bool]] = True,
                    na_position: str = "last") -> "DataFrame":
        """Stable sort by one or more key columns (pandas semantics: NaN/nulls last by default).
        Several keys = LSD over the key columns with stable sorts, as cudf::sorted_order does."""
        keys = [by] if isinstance(by, str) else list(by)
        asc = [ascending] * len(keys) if isinstance(ascending, bool) else list(ascending)
        if len(asc) != len(keys):
            raise ValueError("Length of ascending must match the number of sort keys")
        if na_position not in ("first", "last"):
            raise ValueError("invalid na_position")
        order = _table_order([self._cols[k] for k in keys], asc)   # several numeric keys without nulls: one word sort on the tuple
        if order is not None:
            return self._take(order)
        for name, a in reversed(list(zip(keys, asc))):
            col = self._cols[name] if order is None else ops.gather(self._cols[name], order)
            # NullOrder mapping of core/_internals/sorting.py:83-90: null_before = asc ^ (na == "last")
            null_before = a ^ (na_position == "last")
            if len(keys) >= 2 and not a and col.dtype.kind == "f" and not col.has_nulls():
                # a DESCENDING float key without nulls: the comparator order (NaN rows tied, in row order), not the single-column radix
                # argsort, whose NaN block comes out in reverse row order and would undo the less significant keys' order among them
                perm = ops.sorted_order_table([col], [a])
            else:
                perm = ops.sorted_order(col, ascending=a, null_before=null_before)
            order = perm if order is None else ops.gather(order, perm)
        return self._take(order)

    def searchsorted(self, values, side: str = "left", ascending: Union[bool, Sequence[bool]] = True, na_position: str = "last") -> Column:
        """cudf's DataFrame.searchsorted: the frame, sorted on ALL its columns (lexicographically, one direction per column, nulls
        and NaNs at na_position), is the haystack; `values` -- a DataFrame or dict with the same columns, a sequence of one array /
        Column per column, or a plain array for a frame of one column -- are the needle rows.  Returns the insertion points (INT32):
        side="left" the first position that keeps the frame sorted (cudf::lower_bound), "right" the last (cudf::upper_bound)."""
        if side not in ("left", "right"):
            raise ValueError("side must be 'left' or 'right'")
        if na_position not in ("first", "last"):
            raise ValueError("invalid na_position")
        names = list(self._cols)
        if not names:
            raise ValueError("searchsorted on a frame without columns")
        asc = [ascending] * len(names) if isinstance(ascending, (bool, np.bool_)) else [bool(a) for a in ascending]
        if len(asc) != len(names):
            raise ValueError("Length of ascending must match the number of columns")
        if isinstance(values, DataFrame):
            values = values._cols
        if isinstance(values, dict):
            if list(values) != names:
                raise ValueError("values must have the columns of the frame")
            parts = [values[k] for k in names]
        elif isinstance(values, Column) or (isinstance(values, np.ndarray) and values.ndim == 1):
            parts = [values]
        else:
            parts = list(values)
        if len(parts) != len(names):
            raise ValueError("values must have one entry per column of the frame")
        hay = [self._cols[k] for k in names]
        needles = [p if isinstance(p, Column) else Column.from_numpy(np.asarray(p, dtype=h.dtype)) for p, h in zip(parts, hay)]
        # NullOrder mapping of sort_values: null_before = asc ^ (na == "last")
        null_before = [a ^ (na_position == "last") for a in asc]
        fn = ops.lower_bound if side == "left" else ops.upper_bound
        return fn(hay, needles, asc, null_before)

    def merge(self, right: "DataFrame", on: Union[str, Sequence[str]], how: str = "inner",
              suffixes=("_x", "_y")) -> "DataFrame":
        """Equi-join on one or several key columns; how in {"inner", "left", "right", "outer", "leftsemi", "leftanti"}
        (python/cudf/cudf/core/dataframe.py `merge`; null keys match nothing, as pandas' NaN keys do not on this path).
        Row order is unspecified for inner / left / right / outer (as in cudf); leftsemi / leftanti keep the left order.
        Columns: the keys, then the left frame's other columns, then the right frame's (suffixes where names collide)."""
        if how not in ("inner", "left", "right", "outer", "leftsemi", "leftanti"):
            raise NotImplementedError(f"merge(how={how!r}) is not on this path yet")
        on = [on] if isinstance(on, str) else list(on)
        lt, rt = [self._cols[k] for k in on], [right._cols[k] for k in on]
        if how in ("leftsemi", "leftanti"):
            if len(on) == 1:
                lk, rk = lt[0], rt[0]
            else:
                lk, rk = ops.encode_rows([lt, rt], nulls_equal=False)
            fn = ops.left_semi_join if how == "leftsemi" else ops.left_anti_join
            return self._take(fn(lk, rk, nulls_equal=False))
        if how == "inner":
            li, ri = ops.inner_join_tables(lt, rt, nulls_equal=False)
        elif how == "left":
            li, ri = ops.left_join_tables(lt, rt, nulls_equal=False)
        elif how == "right":   # the left join of the swapped frames: every right row appears, li = JoinNoMatch where it has no partner
            ri, li = ops.left_join_tables(rt, lt, nulls_equal=False)
        else:                  # outer: the left join's pairs, then (JoinNoMatch, r) for every right row without a partner
            li, ri = ops.left_join_tables(lt, rt, nulls_equal=False)
            n0 = li.size           # pairs of the left join; the unmatched right rows come behind them
            li, ri = ops._append_unmatched_right(li, ri, len(right))
        null_l, null_r = how in ("right", "outer"), how in ("left", "outer")
        out = DataFrame()
        for k, lc, rc in zip(on, lt, rt):
            if how == "right":
                out._cols[k] = ops.gather(rc, ri)
            elif how == "outer":
                # the key of a pair is the left row's where there is one, else the right row's: unmatched right rows sit BEHIND the
                # left join's pairs (one per left row or match), so the column is two gathers side by side
                head = ops.gather(lc, _head(li, n0))
                tail = ops.gather(rc, _tail(ri, n0))
                out._cols[k] = ops.concat_columns(head, tail)
            else:
                out._cols[k] = ops.gather(lc, li)
        for name, c in self._cols.items():
            if name not in on:
                out._cols[name + (suffixes[0] if name in right._cols else "")] = ops.gather(c, li, nullify_out_of_bounds=null_l)
        for name, c in right._cols.items():
            if name not in on:
                out._cols[name + (suffixes[1] if name in self._cols else "")] = ops.gather(c, ri, nullify_out_of_bounds=null_r)
        return out

    def join_where(self, other: "DataFrame", predicate, how: str = "inner", suffixes=("_x", "_y")) -> "DataFrame":
        """Conditional (non-equi) join: the pairs of a row of this frame and a row of `other` for which `predicate` is true
        (cudf::conditional_*_join; a null predicate is no match).  how in {"inner", "left", "outer", "leftsemi", "leftanti"}.
        `predicate` is a cudf_amd.ast expression over both tables (ColumnReference(i, "left" / "right")) or a string in the grammar of
        DataFrame.eval: left.name / right.name name a column of one frame, a bare name must occur in exactly one frame (in both:
        ValueError).  Rows: ascending by (left row, right row); an unmatched left row keeps its place, unmatched right rows
        (how="outer") come last.  Columns: this frame's, then `other`'s (suffixes where names collide; leftsemi / leftanti: this
        frame's only); the side without a partner is null."""
        kinds = {"inner": "inner", "left": "left", "outer": "full", "leftsemi": "leftsemi", "leftanti": "leftanti"}
        if how not in kinds:
            raise ValueError(f"join_where(how={how!r}): how must be one of {sorted(kinds)}")
        if isinstance(predicate, str):
            from .ast import parse_eval
            predicate, dt = parse_eval(predicate, {name: c.dtype for name, c in self._cols.items()},
                                       {name: c.dtype for name, c in other._cols.items()})
            if dt != np.bool_:
                raise ValueError(f"join_where: the predicate is a {dt} expression, not a bool one")
        lcols, rcols = list(self._cols.values()), list(other._cols.values())
        if how in ("leftsemi", "leftanti"):
            fn = ops.conditional_left_semi_join if how == "leftsemi" else ops.conditional_left_anti_join
            return self._take(fn(lcols, rcols, predicate))
        fn = {"inner": ops.conditional_inner_join, "left": ops.conditional_left_join, "outer": ops.conditional_full_join}[how]
        li, ri = fn(lcols, rcols, predicate)
        out = DataFrame()
        for name, c in self._cols.items():
            out._cols[name + (suffixes[0] if name in other._cols else "")] = ops.gather(c, li, nullify_out_of_bounds=how == "outer")
        for name, c in other._cols.items():
            out._cols[name + (suffixes[1] if name in self._cols else "")] = ops.gather(c, ri, nullify_out_of_bounds=how != "inner")
        return out

    def groupby(self, by: Union[str, Sequence[str]]) -> "GroupBy":
        return GroupBy(self, by)

    def _select(self, cond: Column, other, keep_where_true: bool) -> "DataFrame":
        if not isinstance(cond, Column) or cond.dtype != np.bool_:
            raise TypeError("cond must be a bool Column")
        if cond.size != len(self):
            raise ValueError(f"cond has {cond.size} rows instead of {len(self)}")
        if isinstance(other, DataFrame):
            if other.columns != self.columns or len(other) != len(self):
                raise ValueError("other must have the columns and the rows of the frame")
            for name, c in self._cols.items():
                if other._cols[name].dtype != c.dtype:
                    raise TypeError(f"column {name!r}: other has dtype {other._cols[name].dtype}, the frame {c.dtype}")
        elif isinstance(other, Column) or (other is not None and np.ndim(other) != 0):
            raise TypeError("other must be a scalar, None or a DataFrame")
        out = DataFrame()
        for name, c in self._cols.items():
            o = other._cols[name] if isinstance(other, DataFrame) else other
            out._cols[name] = ops.copy_if_else(c, o, cond) if keep_where_true else ops.copy_if_else(o, c, cond)
        return out

    def where(self, cond: Column, other=None) -> "DataFrame":
        """pandas' DataFrame.where for a row condition: every column keeps its value where cond (a bool Column of len(df) rows) is
        true and takes `other` elsewhere -- a scalar representable in every column's dtype (no upcast: TypeError otherwise), None
        (the row becomes null, where pandas has NaN) or a DataFrame with the same columns, dtypes and rows.  A null cond element
        counts as false."""
        return self._select(cond, other, True)

    def mask(self, cond: Column, other=None) -> "DataFrame":
        """pandas' DataFrame.mask: the complement of where -- `other` where cond is true, the frame's value elsewhere (also where
        cond is null)"""
        return self._select(cond, other, False)

    def _each(self, f) -> "DataFrame":
        out = DataFrame()
        for name, c in self._cols.items():
            out._cols[name] = f(name, c)
        return out

    def fillna(self, value=None, method: Optional[str] = None) -> "DataFrame":
        """pandas' DataFrame.fillna: the nulls of every column take `value` -- a scalar cast to each column's dtype (no upcast:
        TypeError where it does not fit) or a dict per column name (columns it does not name are kept) -- or, with method "ffill" /
        "bfill", the nearest valid value before / after them; rows without one stay null."""
        if isinstance(value, dict):
            if method is not None:
                raise ValueError("Cannot specify both 'value' and 'method'")
            for k in value:
                if k not in self._cols:
                    raise KeyError(k)
            return self._each(lambda name, c: c.fillna(value[name]) if name in value else c)
        return self._each(lambda name, c: c.fillna(value, method))

    def ffill(self) -> "DataFrame":
        return self.fillna(method="ffill")

    def bfill(self) -> "DataFrame":
        return self.fillna(method="bfill")

    def clip(self, lower=None, upper=None) -> "DataFrame":
        """pandas' DataFrame.clip with scalar bounds, each cast to every column's dtype; None does not bound"""
        return self._each(lambda name, c: c.clip(lower, upper))

    def replace(self, to_replace, value) -> "DataFrame":
        """pandas' DataFrame.replace for a scalar pair or two lists of equal length, in every column"""
        return self._each(lambda name, c: c.replace(to_replace, value))

    # ---- reshaping (ops.repeat / interleave_columns / transpose)
    def repeat(self, repeats) -> "DataFrame":
        """cudf's DataFrame.repeat: every row `repeats` times -- an int, or an integer Column of per-row counts"""
        return self._from_columns(ops.repeat(list(self._cols.values()), repeats))

    def interleave_columns(self) -> Column:
        """cudf's DataFrame.interleave_columns: one Column, row 0 of every column, then row 1, ...; the columns must share a dtype"""
        return ops.interleave_columns(list(self._cols.values()))

    def transpose(self) -> "DataFrame":
        """cudf's DataFrame.transpose: row i becomes the column named str(i).  The columns must share a dtype: TypeError otherwise
        (no upcast to a common type)"""
        out = DataFrame()
        for i, c in enumerate(ops.transpose(list(self._cols.values()))):
            out._cols[str(i)] = c
        return out

    @property
    def T(self) -> "DataFrame":
        return self.transpose()

    def quantile(self, q=0.5, interpolation: str = "linear") -> "DataFrame":
        """pandas' DataFrame.quantile over the numeric columns (bool columns are left out): one FLOAT64 row per quantile -- a scalar q
        gives one row, where pandas gives a Series over the columns.  Nulls are skipped; a column without a valid row gives nulls."""
        qs = list(q) if np.ndim(q) else [q]
        if any(not 0.0 <= float(x) <= 1.0 for x in qs):
            raise ValueError("percentiles should all be in the interval [0, 1]")
        out = DataFrame()
        for name, c in self._cols.items():
            if c.dtype.kind in "iuf":
                out._cols[name] = ops.quantile(c, qs, interpolation)
        return out

    def median(self) -> "DataFrame":
        """pandas' DataFrame.median over the numeric columns, as one row"""
        return self.quantile(0.5)

    def rolling(self, window: int, min_periods: Optional[int] = None, center: bool = False) -> "Rolling":
        """pandas' DataFrame.rolling(window, min_periods, center) over the rows: .sum() / .min() / .max() / .mean() of every column"""
        return Rolling(self, window, min_periods, center)


def concat(frames: Sequence[DataFrame]) -> DataFrame:
    """pandas' concat(frames, ignore_index=True) for frames with the same columns (names, order) and dtypes: the rows of frames[0],
    then frames[1], ...; every column is one fused launch (ops.concatenate).  ValueError: no frames, differing columns; TypeError:
    differing dtypes (no upcast)."""
    frames = list(frames)
    if not frames:
        raise ValueError("No objects to concatenate")
    for f in frames:
        if not isinstance(f, DataFrame):
            raise TypeError("concat takes DataFrames")
        if f.columns != frames[0].columns:
            raise ValueError("concat: the frames must have the same columns")
    for name, c in frames[0]._cols.items():
        for f in frames:
            if f._cols[name].dtype != c.dtype:
                raise TypeError(f"concat: column {name!r} has dtypes {c.dtype} and {f._cols[name].dtype}")
    out = DataFrame()
    for name in frames[0].columns:
        out._cols[name] = ops.concatenate([f._cols[name] for f in frames])
    return out


def _head(col: Column, n: int) -> Column:
    return ops._slice_rows(col, 0, n)


def _tail(col: Column, n: int) -> Column:
    return ops._slice_rows(col, n, col.size)


def _valid_from_counts(counts: Column):
    """(validity words, null count) of per-group results from COUNT_VALID: a group without a valid value is null
    (src/groupby/hash/output_utils.cu:68-70); None when every group has one"""
    n = counts.size
    words = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    L.check(_lib.gx_valid_from_counts(counts.data_ptr, n, ptr(words), ptr(nulls), stream_ptr()), "gx_valid_from_counts")
    k = int(nulls.item())
    return (words, k) if k else (None, 0)


_TABLE_PATH_MIN_ROWS = 1 << 18   # as cudf::sorted_order(table_view) of this tree (cudf_amd/cpp/src/sorting.cpp)


def _table_order(cols: Sequence[Column], asc: Sequence[bool]) -> Optional[Column]:
    """2 - 8 numeric key columns without nulls from 2^18 rows: the lexicographic stable order in ONE word sort on a nested rank of the
    tuple (ops.sorted_order_table -> gx_sorted_order_table; 2 x int64 at 1e9 rows: 32 ms against ~90 for the per-column loop); None
    where that path does not apply.  Same result as the loop: without nulls na_position has nothing to place, and NaN is the greatest
    value of a column on both paths (sort_impl.cuh:61-93)."""
    if not 2 <= len(cols) <= 8 or cols[0].size < _TABLE_PATH_MIN_ROWS:
        return None
    for c in cols:
        if c.has_nulls() or c.dtype.kind not in "iufb" or c.dtype.itemsize not in (1, 2, 4, 8) or (c.dtype.kind == "f" and c.dtype.itemsize == 2):
            return None
    return ops.sorted_order_table(list(cols), list(asc))


def _lexicographic_order(cols: Sequence[Column]) -> Column:
    """stable order of the rows by (cols[0], cols[1], ...): one word sort where _table_order applies, else LSD over the columns with
    the stable radix argsort"""
    order = _table_order(cols, [True] * len(cols))
    if order is not None:
        return order
    for c in reversed(list(cols)):
        if order is None:
            order = ops.sorted_order(c)
        else:
            order = ops.gather(order, ops.sorted_order(ops.gather(c, order)))
    return order


class Rolling:
    """A fixed window of `window` rows ending at each row (center=True: centred on it, the extra row of an even window before it).
    min_periods (default: window) = the valid values a window needs for a result; below it the result is null, where pandas has NaN.
    There is no count: pandas' count has a min_periods rule of its own."""

    def __init__(self, df: DataFrame, window: int, min_periods: Optional[int] = None, center: bool = False):
        if not isinstance(window, (int, np.integer)) or window < 0:
            raise ValueError("window must be an integer 0 or greater")
        if min_periods is not None and min_periods > window:
            raise ValueError(f"min_periods {min_periods} must be <= window {window}")
        if min_periods is not None and min_periods < 0:
            raise ValueError("min_periods must be >= 0")
        self._df = df
        self._following = (int(window) - 1) // 2 if center else 0
        self._preceding = int(window) - self._following
        self._min_periods = int(window) if min_periods is None else int(min_periods)

    def _all(self, op: str) -> DataFrame:
        out = DataFrame()
        for name, c in self._df._cols.items():
            out._cols[name] = ops.rolling_window(c, self._preceding, self._following, self._min_periods, op)
        return out

    def sum(self) -> DataFrame:
        return self._all("sum")

    def min(self) -> DataFrame:
        return self._all("min")

    def max(self) -> DataFrame:
        return self._all("max")

    def mean(self) -> DataFrame:
        return self._all("mean")


class GroupBy:
    _SUPPORTED = ("sum", "count", "mean", "min", "max", "var", "std", "median")

    def __init__(self, df: DataFrame, by: Union[str, Sequence[str]]):
        self._df, self._by = df, ([by] if isinstance(by, str) else list(by))

    def _all(self, fn: str) -> DataFrame:
        """fn over every column that is not a key (python/cudf/cudf/core/groupby/groupby.py: GroupBy.sum / mean / ... = agg(fn))"""
        vals = [c for c in self._df.columns if c not in self._by]
        if not vals:
            raise ValueError("groupby: no value columns to aggregate")
        return self.agg({c: fn for c in vals})

    def sum(self) -> DataFrame:
        return self._all("sum")

    def count(self) -> DataFrame:
        return self._all("count")

    def mean(self) -> DataFrame:
        return self._all("mean")

    def min(self) -> DataFrame:
        return self._all("min")

    def max(self) -> DataFrame:
        return self._all("max")

    def var(self) -> DataFrame:
        return self._all("var")

    def std(self) -> DataFrame:
        return self._all("std")

    def median(self) -> DataFrame:
        return self._all("median")

    def quantile(self, q: float = 0.5, interpolation: str = "linear") -> DataFrame:
        """pandas' GroupBy.quantile for a scalar q: per group and value column, the quantile of the valid values (FLOAT64; null for a
        group without one)"""
        if np.ndim(q):
            raise NotImplementedError("groupby quantile: one quantile per call")
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError("percentiles should all be in the interval [0, 1]")
        return self._all(("quantile", float(q), interpolation))

    def agg(self, spec: Dict[str, Union[str, Sequence[str]]], _exact: bool = False) -> DataFrame:
        """{value column: "sum" | "count" | "mean" | "min" | "max" | "var" | "std" | "median" | [..]} -> one row per group, sorted by key
        (pandas' default sort=True).  Null keys are dropped (dropna=True), null values are skipped."""
        by = self._by
        k0 = self._df[by[0]]
        rep = rk = None
        if len(by) == 1 and k0.dtype.kind in "iu" and k0.dtype.itemsize in (4, 8):
            keys = k0
        elif _exact or len(by) > 8:  # exact encoding: dense row ids, one radix sort per key column
            keys, rep, _ = ops.groupby_keys_tables([self._df[b] for b in by])
        else:  # several key columns / floats / narrow types: one 8-byte row key (packed values or row hash)
            rk = ops.RowKeys([self._df[b] for b in by])
            keys = rk.col
        out = DataFrame()
        first = True
        for name, fns in spec.items():
            fns = [fns] if isinstance(fns, (str, tuple)) else list(fns)
            for f in fns:
                if f not in self._SUPPORTED and not (isinstance(f, tuple) and f[0] == "quantile"):
                    raise NotImplementedError(f"groupby aggregation {f!r} is not on this path yet")
            k, s, cv, _ = ops.groupby_sum_count(keys, self._df[name])
            order = ops.sorted_order(k)
            if first:
                kk = ops.gather(k, order)
                if rk is not None:
                    kc = rk.key_columns(kk)
                    if kc is None:  # two different rows shared a 64-bit hash: start over with the exact encoding
                        return self.agg(spec, _exact=True)
                    for b, c in zip(by, kc):
                        out._cols[b] = c
                elif rep is None:
                    out._cols[by[0]] = kk
                else:
                    rows = ops.gather(rep, kk)
                    for b in by:
                        out._cols[b] = ops.gather(self._df[b], rows)
                first = False
            s, cv = ops.gather(s, order), ops.gather(cv, order)
            mn = mx = None
            if any(f in ("min", "max") for f in fns):
                k2, mn, mx, cv2 = ops.groupby_min_max(keys, self._df[name])
                o2 = ops.sorted_order(k2)
                mn, mx, cv2 = ops.gather(mn, o2), ops.gather(mx, o2), ops.gather(cv2, o2)
                mn.mask, mn.null_count = _valid_from_counts(cv2)    # a group without a valid value is null
                mx.mask, mx.null_count = mn.mask, mn.null_count
            var = std = None
            if any(f in ("var", "std") for f in fns):  # ddof = 1, groups come back in ascending key order
                _, var, std, _, _ = ops.groupby_var_std(keys, self._df[name])
            for f in fns:
                label = name if len(fns) == 1 and len(spec) >= 1 and all(isinstance(v, (str, tuple)) for v in spec.values()) else f"{name}_{f}"
                if f == "median" or isinstance(f, tuple):  # the sort path: rows ordered by (key, value), one lookup per result
                    qv, how = (0.5, "linear") if f == "median" else (f[1], f[2])
                    _, out._cols[label], _ = ops.groupby_quantile(keys, self._df[name], [qv], how)
                elif f == "sum":
                    out._cols[label] = s
                elif f == "count":
                    out._cols[label] = cv
                elif f == "min":
                    out._cols[label] = mn
                elif f == "max":
                    out._cols[label] = mx
                elif f == "var":
                    out._cols[label] = var
                elif f == "std":
                    out._cols[label] = std
                else:  # MEAN = SUM / COUNT_VALID in double, on the device (hash_compound_agg_finalizer.cu:92-133)
                    m = Column.empty(np.float64, s.size)
                    L.check(_lib.gx_mean_from_sum(s.gx, s.data_ptr, cv.data_ptr, s.size, m.data_ptr, stream_ptr()), "gx_mean_from_sum")
                    m.mask, m.null_count = _valid_from_counts(cv)
                    out._cols[label] = m
        if (rep is not None or rk is not None) and len(out._cols):
            # results are in row-key order, pandas sorts by the key columns: order the (few) groups once
            perm = _lexicographic_order([out._cols[b] for b in by])
            for name in list(out._cols):
                out._cols[name] = ops.gather(out._cols[name], perm)
        return out
