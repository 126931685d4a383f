// gx_elementwise_ops.hpp -- the per-value layer of the element-wise kernels: the six compute classes, the typed loads and stores of
// R rows per access, the operators on one pair of values and the validity rule of an operator (out_bits).  Shared by
// gx_elementwise.hip (one operator per launch) and gx_expression.hip (a whole expression per launch): one copy of every rule.
#pragma once
#include "gx_common.hpp"

#include <type_traits>

// results are compared bit for bit with a host that does not fuse: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace gx {

enum { KIND_BASIC = 0, KIND_DIV = 1, KIND_REAL = 2, KIND_UNARY = 3 };
enum { CLS_I32 = 0, CLS_U32 = 1, CLS_I64 = 2, CLS_U64 = 3, CLS_F32 = 4, CLS_F64 = 5 };
constexpr int UNOP_CAST = -1;  // the identity of the UNARY family: gx_cast

// compute class of one dtype: everything narrower than 32 bits, and BOOL8, is promoted to int; the class of L op R is the larger
// of the two codes, which is what the usual arithmetic conversions give on an LP64 target (int32 o uint32 -> uint32,
// int64 o uint32 -> int64, int64 o uint64 -> uint64, integer o float -> float, anything o double -> double)
__host__ __device__ constexpr int class_of_dtype(int dtype)
{
  switch (dtype) {
    case GX_UINT32: return CLS_U32;
    case GX_INT64: return CLS_I64;
    case GX_UINT64: return CLS_U64;
    case GX_FLOAT32: return CLS_F32;
    case GX_FLOAT64: return CLS_F64;
    default: return CLS_I32;
  }
}
template <typename T> struct class_of { static constexpr int value = CLS_I32; };
template <> struct class_of<uint32_t> { static constexpr int value = CLS_U32; };
template <> struct class_of<int64_t> { static constexpr int value = CLS_I64; };
template <> struct class_of<uint64_t> { static constexpr int value = CLS_U64; };
template <> struct class_of<float> { static constexpr int value = CLS_F32; };
template <> struct class_of<double> { static constexpr int value = CLS_F64; };

static inline bool dtype_ok(int d) { return d >= GX_INT8 && d <= GX_BOOL8; }

// R consecutive elements moved as one access of R * sizeof(T) <= 16 bytes where the column's first row is aligned to that size
// (row0 is a multiple of R, so the base decides for every access: a wave-uniform choice); a sliced view that starts elsewhere is
// read and written element by element.
template <typename T, int R>
using Pack = T __attribute__((ext_vector_type(R)));
template <typename T, int R>
__device__ __forceinline__ bool pack_aligned(const void* base)
{
  return (reinterpret_cast<uintptr_t>(base) & (sizeof(Pack<T, R>) - 1)) == 0;
}

template <typename C, typename T, int R, bool ISBOOL>
__device__ __forceinline__ void load_as(const void* p, int64_t row0, int cnt, int is_scalar, C (&v)[R])
{
  // an operand's class never exceeds the class of the operation, and R * sizeof(T) never exceeds 16: other pairs are not built
  if constexpr (class_of<T>::value <= class_of<C>::value && sizeof(T) * R <= 16) {
    const T* tp = static_cast<const T*>(p);
    if (is_scalar) {
      const T s = tp[0];
      const C x = ISBOOL ? C(s != 0) : C(s);
#pragma unroll
      for (int k = 0; k < R; ++k) v[k] = x;
    } else if (cnt == R && pack_aligned<T, R>(p)) {
      const Pack<T, R> pk = *reinterpret_cast<const Pack<T, R>*>(tp + row0);
#pragma unroll
      for (int k = 0; k < R; ++k) v[k] = ISBOOL ? C(pk[k] != 0) : C(pk[k]);
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        v[k] = C(1);  // a row that does not exist: any value that divides
        if (k < cnt) {
          const T s = tp[row0 + k];
          v[k]      = ISBOOL ? C(s != 0) : C(s);
        }
      }
    }
  }
}

template <typename C, int R>
__device__ __forceinline__ void load_rows(int dtype, const void* p, int64_t row0, int cnt, int is_scalar, C (&v)[R])
{
  switch (dtype) {
    case GX_INT8: load_as<C, int8_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_INT16: load_as<C, int16_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_INT32: load_as<C, int32_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_INT64: load_as<C, int64_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_UINT8: load_as<C, uint8_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_UINT16: load_as<C, uint16_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_UINT32: load_as<C, uint32_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_UINT64: load_as<C, uint64_t, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_FLOAT32: load_as<C, float, R, false>(p, row0, cnt, is_scalar, v); break;
    case GX_FLOAT64: load_as<C, double, R, false>(p, row0, cnt, is_scalar, v); break;
    default: load_as<C, uint8_t, R, true>(p, row0, cnt, is_scalar, v); break;  // BOOL8: any nonzero byte is 1
  }
}

template <typename S, typename T, int R, bool ISBOOL>
__device__ __forceinline__ void store_as(void* p, int64_t row0, int cnt, const S (&v)[R])
{
  if constexpr (sizeof(T) * R <= 16) {
    T* tp = static_cast<T*>(p);
    Pack<T, R> pk;
#pragma unroll
    for (int k = 0; k < R; ++k) pk[k] = ISBOOL ? T(v[k] != S(0)) : T(v[k]);
    if (cnt == R && pack_aligned<T, R>(p)) {
      *reinterpret_cast<Pack<T, R>*>(tp + row0) = pk;
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k)
        if (k < cnt) tp[row0 + k] = pk[k];
    }
  }
}

template <typename S, int R>
__device__ __forceinline__ void store_rows(int dtype, void* p, int64_t row0, int cnt, const S (&v)[R])
{
  switch (dtype) {
    case GX_INT8: store_as<S, int8_t, R, false>(p, row0, cnt, v); break;
    case GX_INT16: store_as<S, int16_t, R, false>(p, row0, cnt, v); break;
    case GX_INT32: store_as<S, int32_t, R, false>(p, row0, cnt, v); break;
    case GX_INT64: store_as<S, int64_t, R, false>(p, row0, cnt, v); break;
    case GX_UINT8: store_as<S, uint8_t, R, false>(p, row0, cnt, v); break;
    case GX_UINT16: store_as<S, uint16_t, R, false>(p, row0, cnt, v); break;
    case GX_UINT32: store_as<S, uint32_t, R, false>(p, row0, cnt, v); break;
    case GX_UINT64: store_as<S, uint64_t, R, false>(p, row0, cnt, v); break;
    case GX_FLOAT32: store_as<S, float, R, false>(p, row0, cnt, v); break;
    case GX_FLOAT64: store_as<S, double, R, false>(p, row0, cnt, v); break;
    default: store_as<S, uint8_t, R, true>(p, row0, cnt, v); break;  // BOOL8: 0 or 1
  }
}

// ---------------------------------------------------------------- the operators on one pair of values of class C
template <typename C>
struct cls {
  static constexpr bool is_float = std::is_floating_point<C>::value;
  using U = typename std::conditional<is_float, C, typename std::make_unsigned<typename std::conditional<is_float, int, C>::type>::type>::type;
  static constexpr int bits = (int)sizeof(C) * 8;
};

// integer results wrap modulo 2^width of C: the arithmetic runs on the unsigned type
template <typename C> __device__ __forceinline__ C w_add(C a, C b) { using U = typename cls<C>::U; return C(U(a) + U(b)); }
template <typename C> __device__ __forceinline__ C w_sub(C a, C b) { using U = typename cls<C>::U; return C(U(a) - U(b)); }
template <typename C> __device__ __forceinline__ C w_mul(C a, C b) { using U = typename cls<C>::U; return C(U(a) * U(b)); }

template <typename C>
__device__ __forceinline__ C op_floor_div(C a, C b)
{
  if constexpr (cls<C>::is_float) {
    // NumPy's floor_divide (npy_divmod): floor(a / b) without the quotient's rounding error, NaN for an infinite dividend
    if (b == C(0)) return a / b;
    C mod = fmod(a, b);
    C div = (a - mod) / b;
    if (mod != C(0)) {
      if ((b < C(0)) != (mod < C(0))) div -= C(1);
    }
    if (div != C(0)) {
      C fl = floor(div);
      if (div - fl > C(0.5)) fl += C(1);
      return fl;
    }
    return copysign(C(0), a / b);
  } else if constexpr (std::is_signed<C>::value) {
    C q       = a / b;
    const C r = a % b;
    if (r != 0 && ((r < 0) != (b < 0))) --q;
    return q;
  } else {
    return a / b;
  }
}
template <typename C>
__device__ __forceinline__ C op_mod(C a, C b)
{
  if constexpr (cls<C>::is_float) return fmod(a, b); else return a % b;
}
// ((a % b) + b) % b without the overflow of the inner sum: the remainder moves by one divisor when its sign is not the divisor's
template <typename C>
__device__ __forceinline__ C int_pymod(C a, C b)
{
  C r = a % b;
  if constexpr (std::is_signed<C>::value) {
    if (r != 0 && ((r < 0) != (b < 0))) r += b;
  }
  return r;
}
template <typename C>
__device__ __forceinline__ C op_pmod(C a, C b)
{
  if constexpr (cls<C>::is_float) {
    C r = fmod(a, b);
    if (r < C(0)) r = fmod(r + b, b);
    return r;
  } else {
    return int_pymod(a, b);
  }
}
template <typename C>
__device__ __forceinline__ C op_pymod(C a, C b)
{
  if constexpr (cls<C>::is_float) {
    C r = fmod(a, b);
    if (r != C(0)) {
      if ((b < C(0)) != (r < C(0))) r += b;
    } else {
      r = copysign(C(0), b);
    }
    return r;
  } else {
    return int_pymod(a, b);
  }
}
template <typename C>
__device__ __forceinline__ C op_int_pow(C a, C b)
{
  if constexpr (cls<C>::is_float) {
    return C(0);
  } else {
    using U = typename cls<C>::U;
    if constexpr (std::is_signed<C>::value) {
      if (b < 0) return C(0);
    }
    U base = U(a), e = U(b), r = 1;
    while (e) {  // at most `bits` rounds
      if (e & 1) r *= base;
      base *= base;
      e >>= 1;
    }
    return C(r);
  }
}

#define EW_EACH(expr)                                         \
  {                                                           \
    _Pragma("unroll") for (int k = 0; k < R; ++k)             \
    {                                                         \
      const C a = x[k], b = y[k];                             \
      const bool lv = (lb >> k) & 1u, rv = (rb >> k) & 1u;    \
      (void)a; (void)b; (void)lv; (void)rv;                   \
      out[k] = (expr);                                        \
    }                                                         \
  }                                                           \
  break;

// BASIC and DIV: the result of every row in C (a truth value as 0 / 1, which casts like the bool it stands for)
template <typename C, int R, int KIND>
__device__ __forceinline__ void apply_rows(int op, const C (&x)[R], const C (&y)[R], uint32_t lb, uint32_t rb, int lhs_bits, C (&out)[R])
{
  using U = typename cls<C>::U;
  constexpr bool F = cls<C>::is_float;
  constexpr int SM = cls<C>::bits - 1;  // shift counts outside [0, width) are unspecified: they are taken modulo the width
  if constexpr (KIND == KIND_BASIC) {
    switch (op) {
      case GX_BINOP_ADD: EW_EACH(w_add(a, b))
      case GX_BINOP_SUB: EW_EACH(w_sub(a, b))
      case GX_BINOP_MUL: EW_EACH(w_mul(a, b))
      case GX_BINOP_EQUAL: EW_EACH(C(a == b))
      case GX_BINOP_NOT_EQUAL: EW_EACH(C(a != b))
      case GX_BINOP_LESS: EW_EACH(C(a < b))
      case GX_BINOP_GREATER: EW_EACH(C(a > b))
      case GX_BINOP_LESS_EQUAL: EW_EACH(C(a <= b))
      case GX_BINOP_GREATER_EQUAL: EW_EACH(C(a >= b))
      case GX_BINOP_LOGICAL_AND: EW_EACH(C(a != C(0) && b != C(0)))
      case GX_BINOP_LOGICAL_OR: EW_EACH(C(a != C(0) || b != C(0)))
      case GX_BINOP_NULL_EQUALS: EW_EACH(C((lv && rv) ? a == b : lv == rv))
      case GX_BINOP_NULL_NOT_EQUALS: EW_EACH(C((lv && rv) ? a != b : lv != rv))
      case GX_BINOP_NULL_MAX: EW_EACH((lv && rv) ? (a < b ? b : a) : (lv ? a : b))
      case GX_BINOP_NULL_MIN: EW_EACH((lv && rv) ? (b < a ? b : a) : (lv ? a : b))
      // Kleene: a null side counts as "unknown", which the valid side alone decides or not (the validity: out_bits)
      case GX_BINOP_NULL_LOGICAL_AND: EW_EACH(C((!lv || a != C(0)) && (!rv || b != C(0))))
      case GX_BINOP_NULL_LOGICAL_OR: EW_EACH(C((lv && a != C(0)) || (rv && b != C(0))))
      default:
        if constexpr (!F) {
          switch (op) {
            case GX_BINOP_BITWISE_AND: EW_EACH(C(U(a) & U(b)))
            case GX_BINOP_BITWISE_OR: EW_EACH(C(U(a) | U(b)))
            case GX_BINOP_BITWISE_XOR: EW_EACH(C(U(a) ^ U(b)))
            case GX_BINOP_SHIFT_LEFT: EW_EACH(C(U(a) << (int(b) & SM)))
            case GX_BINOP_SHIFT_RIGHT: EW_EACH(C(a >> (int(b) & SM)))  // arithmetic for signed C
            // the left operand as the unsigned type of its own width: the bits above it are the sign extension of the load
            case GX_BINOP_SHIFT_RIGHT_UNSIGNED:
              EW_EACH(C((lhs_bits >= cls<C>::bits ? U(a) : U(U(a) & ((U(1) << lhs_bits) - U(1)))) >> (int(b) & SM)))
            default: break;
          }
        }
        break;
    }
  } else {
    switch (op) {
      case GX_BINOP_DIV: EW_EACH(a / b)
      case GX_BINOP_FLOOR_DIV: EW_EACH(op_floor_div(a, b))
      case GX_BINOP_MOD: EW_EACH(op_mod(a, b))
      case GX_BINOP_PMOD: EW_EACH(op_pmod(a, b))
      case GX_BINOP_PYMOD: EW_EACH(op_pymod(a, b))
      case GX_BINOP_INT_POW: EW_EACH(op_int_pow(a, b))
      default: break;
    }
  }
}

// REAL: TRUE_DIV is a division of doubles in every class; POW is pow on doubles, powf in the float class
template <typename C, int R>
__device__ __forceinline__ void apply_real(int op, const C (&x)[R], const C (&y)[R], double (&out)[R])
{
  const uint32_t lb = 0, rb = 0;
  if (op == GX_BINOP_TRUE_DIV) {
    do { EW_EACH(double(a) / double(b)) } while (0);
  } else if constexpr (std::is_same<C, float>::value) {
    do { EW_EACH(double(powf(a, b))) } while (0);
  } else {
    do { EW_EACH(pow(double(a), double(b))) } while (0);
  }
}

template <typename C, int R>
__device__ __forceinline__ void apply_unary(int op, const C (&x)[R], C (&out)[R])
{
  using U = typename cls<C>::U;
  constexpr bool F = cls<C>::is_float;
  const C(&y)[R]   = x;
  const uint32_t lb = 0, rb = 0;
  switch (op) {
    case GX_UNOP_ABS:
      if constexpr (F) { EW_EACH(fabs(a)) } else if constexpr (std::is_signed<C>::value) { EW_EACH(a < 0 ? C(U(0) - U(a)) : a) } else { EW_EACH(a) }
    case GX_UNOP_NEGATE:
      if constexpr (F) { EW_EACH(-a) } else { EW_EACH(C(U(0) - U(a))) }
    case GX_UNOP_NOT: EW_EACH(C(a == C(0)))
    case GX_UNOP_SQRT:
      if constexpr (F) { EW_EACH(sqrt(a)) } else break;
    case GX_UNOP_CEIL:
      if constexpr (F) { EW_EACH(ceil(a)) } else break;
    case GX_UNOP_FLOOR:
      if constexpr (F) { EW_EACH(floor(a)) } else break;
    case GX_UNOP_RINT:
      if constexpr (F) { EW_EACH(rint(a)) } else break;  // round half to even
    case GX_UNOP_IS_NAN:
      if constexpr (F) { EW_EACH(C(a != a)) } else break;
    case GX_UNOP_IS_NOT_NAN:
      if constexpr (F) { EW_EACH(C(a == a)) } else break;
    case GX_UNOP_BIT_INVERT:
      if constexpr (!F) { EW_EACH(C(~U(a))) } else break;
    default: EW_EACH(a)  // UNOP_CAST
  }
}
#undef EW_EACH

// the validity of the R rows of a thread from the validity of its operands (bits above the live rows are masked by the caller)
template <typename C, int R>
__device__ __forceinline__ uint32_t out_bits(int op, const C (&x)[R], const C (&y)[R], uint32_t lb, uint32_t rb)
{
  switch (op) {
    case GX_BINOP_NULL_EQUALS:
    case GX_BINOP_NULL_NOT_EQUALS: return ~0u;
    case GX_BINOP_NULL_MAX:
    case GX_BINOP_NULL_MIN: return lb | rb;
    case GX_BINOP_NULL_LOGICAL_AND:
    case GX_BINOP_NULL_LOGICAL_OR: {
      uint32_t tx = 0, ty = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        tx |= (x[k] != C(0) ? 1u : 0u) << k;
        ty |= (y[k] != C(0) ? 1u : 0u) << k;
      }
      // a valid false decides AND, a valid true decides OR
      if (op == GX_BINOP_NULL_LOGICAL_AND) return (lb & rb) | (lb & ~tx) | (rb & ~ty);
      return (lb & rb) | (lb & tx) | (rb & ty);
    }
    default: return lb & rb;
  }
}

}  // namespace gx
