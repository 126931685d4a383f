"""Columns that tell a wrong route through the dtype table (cudf_amd/csrc/gx_dtype.hpp) from the right one.

A host dispatch picks a kernel instantiation by a dtype's value type, unsigned word, kind (unsigned / signed / float) and is_bool.
Both the right and a wrong instantiation exist in the library, so only values can tell them apart: a negative value for a signed
type and a value >= 2^(w-1) for an unsigned one (a signed / unsigned mix-up reorders them), -0.0, NaN and the infinities for floats
(a float sent down an integer route compares their bits), and for BOOL8 -- where asked for -- bytes other than 0 and 1, which mean
`true` (a BOOL8 sent down the UINT8 route sees 2 and 255).  ROWS = 65 is one wave and a tail row."""
import numpy as np

DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
ROWS = 65


def route_values(dtype, seed=0, nan=True, raw_bool=False, n=ROWS):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dt.kind == "b":
        if not raw_bool:
            return rng.integers(0, 2, n).astype(bool)
        raw = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
        raw[:4] = [2, 0, 255, 1]
        return raw.view(bool)
    if dt.kind == "f":
        v = np.round(rng.standard_normal(n) * 100, 1).astype(dt)
        v[[1, 20, 21, 40, 64]] = [-0.0, 0.0, -np.inf, np.inf, -0.0]
        if nan:
            v[[5, 33]] = [np.nan, -np.nan]
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    v[[0, 7, 64]] = [info.max, info.min, info.max // 2 + 1 if dt.kind == "u" else -1]  # the last: 2^(w-1), or -1
    return v
