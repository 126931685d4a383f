"""Device column = Arrow-layout buffers in HBM (data + optional validity bitmap).

Mirrors the data model of cudf::column / cudf::column_view
(cpp/include/cudf/column/column.hpp:36-331, column_view.hpp): a typed data buffer, an optional
LSB-first validity bitmap in uint32 words padded to 64 bytes (cpp/include/cudf/null_mask.hpp:55)
and a host-side null count.  PyTorch is used only as the device allocator / stream provider.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib as L

_NP2GX = {
    np.dtype("int8"): L.INT8, np.dtype("int16"): L.INT16, np.dtype("int32"): L.INT32,
    np.dtype("int64"): L.INT64, np.dtype("uint8"): L.UINT8, np.dtype("uint16"): L.UINT16,
    np.dtype("uint32"): L.UINT32, np.dtype("uint64"): L.UINT64, np.dtype("float32"): L.FLOAT32,
    np.dtype("float64"): L.FLOAT64, np.dtype("bool"): L.BOOL8,
}


def gx_dtype(dt) -> int:
    try:
        return _NP2GX[np.dtype(dt)]
    except KeyError:
        raise TypeError(f"unsupported dtype {dt}") from None  # cudf::data_type_error -> TypeError


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_bytes(nbytes: int) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")


def ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bitmask_words(nbits: int) -> int:
    """uint32 words of a validity bitmap, allocation padded to 64 B (null_mask.hpp:55)."""
    return ((nbits + 511) // 512) * 16


def pack_mask(valid: np.ndarray) -> np.ndarray:
    """bool array -> LSB-first uint32 words (padded)."""
    n = len(valid)
    bits = np.zeros(bitmask_words(n) * 32, dtype=np.uint8)
    bits[:n] = np.asarray(valid, dtype=np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint32)


def unpack_mask(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


class Column:
    """Owning device column."""

    __slots__ = ("data", "dtype", "size", "mask", "null_count")

    def __init__(self, data: torch.Tensor, dtype, size: int, mask: Optional[torch.Tensor] = None,
                 null_count: int = 0):
        self.data = data          # uint8 tensor, size*itemsize bytes (at least)
        self.dtype = np.dtype(dtype)
        self.size = int(size)
        self.mask = mask          # int32 tensor of bitmask words or None
        self.null_count = int(null_count) if mask is not None else 0

    # -------- construction / export (host <-> device, Arrow layout)
    @classmethod
    def from_numpy(cls, values: np.ndarray, valid: Optional[np.ndarray] = None) -> "Column":
        v = np.ascontiguousarray(values)
        if v.size > 2**31 - 1:
            raise OverflowError("column size exceeds cudf::size_type")  # column.hpp:78-81
        raw = torch.from_numpy(v.view(np.uint8).reshape(-1).copy()) if v.size else torch.empty(0, dtype=torch.uint8)
        data = device_bytes(v.nbytes)
        if v.size:
            data[: v.nbytes].copy_(raw)
        mask = None
        nulls = 0
        if valid is not None:
            valid = np.asarray(valid, dtype=bool)
            nulls = int((~valid).sum())
            words = pack_mask(valid)
            mask = torch.from_numpy(words.view(np.int32).copy()).cuda()
        return cls(data, v.dtype, v.size, mask, nulls)

    @classmethod
    def empty(cls, dtype, size: int, nullable: bool = False) -> "Column":
        dt = np.dtype(dtype)
        data = device_bytes(size * dt.itemsize)
        mask = torch.zeros(bitmask_words(size), dtype=torch.int32, device="cuda") if nullable else None
        return cls(data, dt, size, mask, 0)

    @classmethod
    def arange(cls, start, stop=None, step=1, dtype=None) -> "Column":
        """numpy.arange on the device (ops.sequence): start + i * step for i in [0, ceil((stop - start) / step)); one argument is the
        stop.  dtype defaults to NumPy's for the arguments (int64 / float64).  Floats round the product, then the sum."""
        from . import ops
        if stop is None:
            start, stop = 0, start
        if step == 0:
            raise ValueError("arange: step cannot be zero")
        dt = np.dtype(dtype) if dtype is not None else np.result_type(start, stop, step)
        if dt.kind not in "iuf":
            raise TypeError(f"arange: {dt} is not a numeric type")
        n = max(0, int(np.ceil((stop - start) / step)))
        return ops.sequence(n, start, step, dt)

    def repeat(self, repeats) -> "Column":
        """pandas' Series.repeat: every row `repeats` times -- an int, or an integer Column of per-row counts (ops.repeat)"""
        from . import ops
        return ops.repeat(self, repeats)

    def quantile(self, q=0.5, interpolation: str = "linear"):
        """pandas' Series.quantile: nulls are skipped.  A scalar q gives a Python float (None when no row is valid), a list a FLOAT64
        Column (ops.quantile)."""
        from . import ops
        qs = list(q) if np.ndim(q) else [q]
        if any(not 0.0 <= float(x) <= 1.0 for x in qs):
            raise ValueError("percentiles should all be in the interval [0, 1]")
        out = ops.quantile(self, qs, interpolation)
        if np.ndim(q):
            return out
        return None if out.null_count else float(out.to_numpy()[0])

    def median(self):
        """pandas' Series.median: the 0.5 quantile, linear"""
        return self.quantile(0.5)

    def to_numpy(self) -> np.ndarray:
        nbytes = self.size * self.dtype.itemsize
        return self.data[:nbytes].cpu().numpy().view(self.dtype).copy()

    def valid_numpy(self) -> Optional[np.ndarray]:
        if self.mask is None:
            return None
        return unpack_mask(self.mask.cpu().numpy().view(np.uint32), self.size)

    # -------- raw pointers for the C ABI
    @property
    def gx(self) -> int:
        return gx_dtype(self.dtype)

    @property
    def data_ptr(self):
        return ctypes.c_void_p(self.data.data_ptr())

    @property
    def mask_ptr(self):
        return ctypes.c_void_p(self.mask.data_ptr()) if self.mask is not None else None

    def has_nulls(self) -> bool:
        return self.mask is not None and self.null_count > 0

    def __len__(self):
        return self.size

    # -------- element-wise operators (ops.binary_operation / unary_operation / cast).  The result dtype is NumPy's:
    # np.result_type of the operands (a Python scalar is weak), float64 for / on integers, bool for comparisons.  Where NumPy
    # promotes further than the common type of C++ the operands are cast first (int32 o uint32 -> int64, int64 o uint64 -> float64).
    # __eq__ / __ne__ are NOT defined: columns are compared and hashed by identity; use .eq() / .ne().
    def _binop(self, other, kind: str, reflected: bool = False) -> "Column":
        from . import ops
        if isinstance(other, Column):
            odt = other.dtype
            rt = np.result_type(self.dtype, odt)
        elif isinstance(other, (bool, int, float, np.generic)):
            rt = np.result_type(self.dtype, other)
            odt = other.dtype if isinstance(other, np.generic) else rt
        else:
            return NotImplemented
        integral = rt.kind in "iub"
        if kind in ("and", "or", "xor", "lshift", "rshift") and not integral:
            raise TypeError(f"operator {kind!r} is not supported for {rt}")
        if kind in ("lshift", "rshift") and rt.kind == "b":
            rt = np.dtype(np.int8)           # NumPy shifts bools as int8
        name = {"add": "ADD", "sub": "SUB", "mul": "MUL", "floordiv": "FLOOR_DIV", "mod": "PYMOD", "and": "BITWISE_AND",
                "or": "BITWISE_OR", "xor": "BITWISE_XOR", "lshift": "SHIFT_LEFT", "rshift": "SHIFT_RIGHT", "lt": "LESS",
                "le": "LESS_EQUAL", "gt": "GREATER", "ge": "GREATER_EQUAL", "eq": "EQUAL", "ne": "NOT_EQUAL",
                "truediv": "TRUE_DIV" if integral else "DIV", "pow": "INT_POW" if integral else "POW"}[kind]
        if kind in ("lt", "le", "gt", "ge", "eq", "ne"):
            out = np.dtype(np.bool_)
        elif kind == "truediv" and integral:
            out = np.dtype(np.float64)
        else:
            out = rt
        # the compute class of the kernel (everything below 32 bits computes in int32) against the class of NumPy's type
        cls = lambda dt: {"u4": 1, "i8": 2, "u8": 3, "f4": 4, "f8": 5}.get(np.dtype(dt).str[1:], 0)  # noqa: E731
        lhs = self
        if max(cls(self.dtype), cls(odt)) != cls(rt):
            lhs = ops.cast(self, rt) if self.dtype != rt else self
            if isinstance(other, Column):
                other = ops.cast(other, rt) if other.dtype != rt else other
            odt = rt
        sdt = None if isinstance(other, Column) else odt
        if reflected:
            return ops.binary_operation(other, lhs, name, out, scalar_dtype=sdt)
        return ops.binary_operation(lhs, other, name, out, scalar_dtype=sdt)

    def __add__(self, o): return self._binop(o, "add")
    def __radd__(self, o): return self._binop(o, "add", True)
    def __sub__(self, o): return self._binop(o, "sub")
    def __rsub__(self, o): return self._binop(o, "sub", True)
    def __mul__(self, o): return self._binop(o, "mul")
    def __rmul__(self, o): return self._binop(o, "mul", True)
    def __truediv__(self, o): return self._binop(o, "truediv")
    def __rtruediv__(self, o): return self._binop(o, "truediv", True)
    def __floordiv__(self, o): return self._binop(o, "floordiv")
    def __rfloordiv__(self, o): return self._binop(o, "floordiv", True)
    def __mod__(self, o): return self._binop(o, "mod")
    def __rmod__(self, o): return self._binop(o, "mod", True)
    def __pow__(self, o): return self._binop(o, "pow")
    def __rpow__(self, o): return self._binop(o, "pow", True)
    def __and__(self, o): return self._binop(o, "and")
    def __rand__(self, o): return self._binop(o, "and", True)
    def __or__(self, o): return self._binop(o, "or")
    def __ror__(self, o): return self._binop(o, "or", True)
    def __xor__(self, o): return self._binop(o, "xor")
    def __rxor__(self, o): return self._binop(o, "xor", True)
    def __lshift__(self, o): return self._binop(o, "lshift")
    def __rlshift__(self, o): return self._binop(o, "lshift", True)
    def __rshift__(self, o): return self._binop(o, "rshift")
    def __rrshift__(self, o): return self._binop(o, "rshift", True)
    def __lt__(self, o): return self._binop(o, "lt")
    def __le__(self, o): return self._binop(o, "le")
    def __gt__(self, o): return self._binop(o, "gt")
    def __ge__(self, o): return self._binop(o, "ge")

    def eq(self, o) -> "Column":
        """element-wise ==, a bool column (== itself compares columns by identity)"""
        return self._binop(o, "eq")

    def ne(self, o) -> "Column":
        return self._binop(o, "ne")

    def __neg__(self):
        from . import ops
        return ops.unary_operation(self, "NEGATE")

    def __abs__(self):
        from . import ops
        return ops.unary_operation(self, "ABS")

    def __invert__(self):
        from . import ops
        return ops.unary_operation(self, "NOT" if self.dtype == np.bool_ else "BIT_INVERT")

    def astype(self, dtype) -> "Column":
        from . import ops
        return ops.cast(self, dtype)

    def isnull(self) -> "Column":
        from . import ops
        return ops.is_null(self)

    def notnull(self) -> "Column":
        from . import ops
        return ops.is_valid(self)

    # -------- null and value replacement (ops.replace_nulls / clamp / find_and_replace_all).  Scalars are cast to the column's dtype:
    # there is no promotion, a value the dtype cannot hold is a TypeError.
    def fillna(self, value=None, method: Optional[str] = None) -> "Column":
        """pandas' Series.fillna: nulls take `value` (a scalar, or a Column of equal rows and dtype), or with method "ffill" / "bfill"
        the nearest valid value before / after them (rows without one stay null)"""
        from . import ops
        if (value is None) == (method is None):
            raise ValueError("Must specify a fill 'value' or 'method'" if value is None else "Cannot specify both 'value' and 'method'")
        if method is not None:
            if method not in ("ffill", "bfill"):
                raise ValueError(f"invalid fill method {method!r}: expected 'ffill' or 'bfill'")
            return ops.replace_nulls(self, "preceding" if method == "ffill" else "following")
        if isinstance(value, str):
            raise TypeError(f"{value!r} is not representable as {self.dtype}")
        return ops.replace_nulls(self, value)

    def ffill(self) -> "Column":
        return self.fillna(method="ffill")

    def bfill(self) -> "Column":
        return self.fillna(method="bfill")

    def clip(self, lower=None, upper=None) -> "Column":
        """pandas' Series.clip: values below `lower` become lower, values above `upper` become upper; None does not bound"""
        from . import ops
        return ops.clamp(self, lower, upper)

    def replace(self, to_replace, value) -> "Column":
        """pandas' Series.replace for a scalar pair or two lists of equal length: a row equal to to_replace[j] becomes value[j] (the
        first j that matches; None in `value` makes the row null).  Null rows stay null; NaN matches nothing."""
        from . import ops
        olds = list(to_replace) if np.ndim(to_replace) else [to_replace]
        news = list(value) if np.ndim(value) else [value] * len(olds)      # one value for a whole list, as in pandas
        if len(olds) != len(news):
            raise ValueError(f"Replacement lists must match in length. Expecting {len(olds)} got {len(news)}")
        for v in olds + [w for w in news if w is not None]:
            ops._check_scalar(v, self.dtype)
        valid = np.array([w is not None for w in news], dtype=bool)
        new_np = np.array([0 if w is None else w for w in news]).astype(self.dtype) if news else np.zeros(0, self.dtype)
        old_np = np.array(olds).astype(self.dtype) if olds else np.zeros(0, self.dtype)
        return ops.find_and_replace_all(self, Column.from_numpy(old_np), Column.from_numpy(new_np, None if valid.all() else valid))
