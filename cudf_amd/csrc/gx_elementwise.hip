// gx_elementwise.hip -- the element-wise kernels behind <cudf/binaryop.hpp> and <cudf/unary.hpp>: binary operations between two
// columns or a column and a scalar, unary operations, casts and the expansion of a validity bitmap into BOOL8.
// reference: cpp/src/binaryop (binaryop.cpp, compiled/binary_ops.cuh, compiled/operation.cuh), cpp/src/unary (math_ops.cu,
// cast_ops.cu, null_ops.cu, nan_ops.cu).  The reference instantiates a functor per (lhs, rhs, out, operator) through a type
// dispatcher; here the value model out = cast<Out>(f(cast<C>(lhs), cast<C>(rhs))) has six compute classes C, and the operand and
// output dtypes are runtime, wave-uniform choices around them.  A kernel is instantiated per (C, rows per access, operator family):
//   rows per access R = 16 / (the widest of lhs, rhs and out), so a thread moves 16 bytes per access on the widest operand;
//   families: BASIC (add / sub / mul, bits, shifts, logic, comparisons, NULL_*), DIV (the division family and INT_POW),
//   REAL (TRUE_DIV and POW, carried as double), UNARY (one operand, casts included).
// All of them are pure streaming kernels: no scratch, no host synchronisation, LDS only for the null count of a workgroup.
#include "gx_common.hpp"

#include <type_traits>

// results are compared bit for bit with a host that does not fuse: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace gx {

constexpr int EW_BT       = 256;
constexpr int EW_ROWS     = 16;               // rows of one thread per trip: 16 / R accesses of R rows
constexpr int EW_TILE     = EW_BT * EW_ROWS;  // rows one workgroup owns per trip: a multiple of 32, so it owns whole validity words
constexpr int EW_GRID_CAP = 2048;             // 8 workgroups on each of 256 CUs; further tiles are further trips
constexpr int64_t EW_MAX_ROWS = (int64_t(1) << 31) - 1;

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

struct Operand : ValueSrc {
  int dtype;
};

// A workgroup owns tiles of EW_TILE consecutive output rows; in a tile a thread makes 16 / R accesses of R rows, access j of
// thread t at row (j * 256 + t) * R of the tile, so that a wave's access is one contiguous run of 64 * R rows (whole validity
// words).  With out_valid every thread takes the R bits of each operand at that operand's own begin bit, and the lanes that
// share an output word (32 / R of them) merge their bits across the wave: one writer per word, no atomics.
template <typename C, int R, int KIND>
__global__ void __launch_bounds__(EW_BT) k_elementwise(int op, Operand lhs, Operand rhs, int64_t n, int out_dtype, void* __restrict__ out,
                                                       uint32_t* __restrict__ out_valid, unsigned long long* __restrict__ null_count,
                                                       int lhs_bits)
{
  using S = typename std::conditional<KIND == KIND_REAL, double, C>::type;
  constexpr int NJ    = EW_ROWS / R;
  constexpr int GROUP = 32 / R;  // lanes that share a validity word
  __shared__ unsigned long long s_nulls;
  const unsigned t    = threadIdx.x;
  const unsigned lane = lane_id();
  const bool l_ok     = lhs.scalar_ok(), r_ok = rhs.scalar_ok();
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  const int64_t tiles = div_up(n, EW_TILE);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * EW_TILE;
#pragma unroll 1
    for (int j = 0; j < NJ; ++j) {
      const int64_t row0 = t0 + ((int64_t)j * EW_BT + t) * R;
      if (row0 - (int64_t)lane * R >= n) break;  // the whole wave is behind the last row, in this access and in the later ones
      const int cnt     = row0 >= n ? 0 : (n - row0 < R ? (int)(n - row0) : R);
      const uint32_t lm = (1u << cnt) - 1u;      // cnt <= 16
      uint32_t lb = lm, rb = lm;
      if (out_valid && cnt > 0) {
        // (spelled out, not a member of ValueSrc: behind any wrapper k_elementwise<float, 2, REAL> takes a 101st SGPR and loses its 8th wave)
        lb = lhs.valid ? bits_from(lhs.valid, lhs.begin_bit + row0, cnt) : (l_ok ? lm : 0u);
        if (KIND != KIND_UNARY) rb = rhs.valid ? bits_from(rhs.valid, rhs.begin_bit + row0, cnt) : (r_ok ? lm : 0u);
      }
      uint32_t ob = 0;
      if (cnt > 0) {
        C x[R];
        S res[R];
        load_rows<C, R>(lhs.dtype, lhs.data, row0, cnt, lhs.is_scalar, x);
        if constexpr (KIND == KIND_UNARY) {
          apply_unary<C, R>(op, x, res);
          ob = lb;
        } else {
          C y[R];
          load_rows<C, R>(rhs.dtype, rhs.data, row0, cnt, rhs.is_scalar, y);
          if constexpr (KIND == KIND_REAL) apply_real<C, R>(op, x, y, res); else apply_rows<C, R, KIND>(op, x, y, lb, rb, lhs_bits, res);
          ob = out_bits<C, R>(op, x, y, lb, rb) & lm;
        }
        store_rows<S, R>(out_dtype, out, row0, cnt, res);
      }
      if (out_valid) {  // every lane of the wave is here
        uint32_t w = ob << ((lane % GROUP) * R);
#pragma unroll
        for (int d = 1; d < GROUP; d <<= 1) w |= (uint32_t)__shfl_xor((int)w, d, GX_WAVE);
        if (lane % GROUP == 0 && row0 < n) out_valid[row0 >> 5] = w;
        nulls += (unsigned long long)__builtin_popcount(~ob & lm);
      }
    }
  }
  if (null_count) tally_end(&s_nulls, wave_reduce(nulls, SumOp()), null_count);
}

// out[i] = bit (begin_bit + i) of valid, inverted on request; 16 rows = one 16-byte store per thread
__global__ void __launch_bounds__(EW_BT) k_bitmask_to_bool8(const uint32_t* __restrict__ valid, int64_t begin_bit, int64_t n, int invert,
                                                            uint8_t* __restrict__ out)
{
  const int64_t stride = (int64_t)gridDim.x * EW_BT * 16;
  for (int64_t row0 = ((int64_t)blockIdx.x * EW_BT + threadIdx.x) * 16; row0 < n; row0 += stride) {
    const int cnt = n - row0 < 16 ? (int)(n - row0) : 16;
    uint32_t b    = valid ? bits_from(valid, begin_bit + row0, cnt) : 0xFFFFu;
    if (invert) b = ~b;
    Pack<uint8_t, 16> pk;
#pragma unroll
    for (int k = 0; k < 16; ++k) pk[k] = (b >> k) & 1u;
    if (cnt == 16 && pack_aligned<uint8_t, 16>(out)) {
      *reinterpret_cast<Pack<uint8_t, 16>*>(out + row0) = pk;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < cnt) out[row0 + k] = pk[k];
    }
  }
}

// ---------------------------------------------------------------- host: operator tables and launches
static inline int binop_kind(int op)
{
  switch (op) {
    case GX_BINOP_ADD: case GX_BINOP_SUB: case GX_BINOP_MUL:
    case GX_BINOP_SHIFT_LEFT: case GX_BINOP_SHIFT_RIGHT: case GX_BINOP_SHIFT_RIGHT_UNSIGNED:
    case GX_BINOP_BITWISE_AND: case GX_BINOP_BITWISE_OR: case GX_BINOP_BITWISE_XOR:
    case GX_BINOP_LOGICAL_AND: case GX_BINOP_LOGICAL_OR:
    case GX_BINOP_EQUAL: case GX_BINOP_NOT_EQUAL: case GX_BINOP_LESS: case GX_BINOP_GREATER: case GX_BINOP_LESS_EQUAL:
    case GX_BINOP_GREATER_EQUAL:
    case GX_BINOP_NULL_EQUALS: case GX_BINOP_NULL_NOT_EQUALS: case GX_BINOP_NULL_MAX: case GX_BINOP_NULL_MIN:
    case GX_BINOP_NULL_LOGICAL_AND: case GX_BINOP_NULL_LOGICAL_OR: return KIND_BASIC;
    case GX_BINOP_DIV: case GX_BINOP_FLOOR_DIV: case GX_BINOP_MOD: case GX_BINOP_PMOD: case GX_BINOP_PYMOD:
    case GX_BINOP_INT_POW: return KIND_DIV;
    case GX_BINOP_TRUE_DIV: case GX_BINOP_POW: return KIND_REAL;
    default: return -1;  // LOG_BASE, ATAN2, GENERIC_BINARY: not built
  }
}
static inline bool binop_known(int op) { return op >= GX_BINOP_ADD && op <= GX_BINOP_NULL_LOGICAL_OR; }
static inline bool binop_integer_only(int op)
{
  switch (op) {
    case GX_BINOP_INT_POW: case GX_BINOP_SHIFT_LEFT: case GX_BINOP_SHIFT_RIGHT: case GX_BINOP_SHIFT_RIGHT_UNSIGNED:
    case GX_BINOP_BITWISE_AND: case GX_BINOP_BITWISE_OR: case GX_BINOP_BITWISE_XOR: return true;
    default: return false;
  }
}
static inline bool unop_known(int op)
{
  return (op >= GX_UNOP_SIN && op <= GX_UNOP_NEGATE) || op == GX_UNOP_IS_NAN || op == GX_UNOP_IS_NOT_NAN;
}

template <typename C, int R, int KIND>
int ew_launch(int op, const Operand& l, const Operand& r, int64_t n, int out_dtype, void* out, uint32_t* out_valid, int64_t* nulls,
              int lhs_bits, hipStream_t s)
{
  hipLaunchKernelGGL((k_elementwise<C, R, KIND>), dim3(capped_grid(n, EW_TILE, EW_GRID_CAP)), dim3(EW_BT), 0, s, op, l, r, n, out_dtype, out, out_valid,
                     reinterpret_cast<unsigned long long*>(nulls), lhs_bits);
  GX_LAUNCH_CHECK();
  return 0;
}

// the (class, R) pairs that exist: R = 16 / widest operand, and a class of 4 (8) bytes has an operand of 4 (8) bytes
template <int KIND>
int ew_dispatch(int c, int widest, int op, const Operand& l, const Operand& r, int64_t n, int out_dtype, void* out, uint32_t* out_valid,
                int64_t* nulls, int lhs_bits, hipStream_t s)
{
#define EW_GO(C, R) return ew_launch<C, R, KIND>(op, l, r, n, out_dtype, out, out_valid, nulls, lhs_bits, s)
  switch (c) {
    case CLS_I32:
      switch (widest) {
        case 1: EW_GO(int32_t, 16);
        case 2: EW_GO(int32_t, 8);
        case 4: EW_GO(int32_t, 4);
        default: EW_GO(int32_t, 2);
      }
    case CLS_U32:
      if (widest == 4) EW_GO(uint32_t, 4);
      EW_GO(uint32_t, 2);
    case CLS_F32:
      if (widest == 4) EW_GO(float, 4);
      EW_GO(float, 2);
    case CLS_I64: EW_GO(int64_t, 2);
    case CLS_U64: EW_GO(uint64_t, 2);
    default: EW_GO(double, 2);
  }
#undef EW_GO
}

static inline int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

static int unary_launch(int op, int in_dtype, const void* in, int64_t n, int out_dtype, void* out, hipStream_t s)
{
  const Operand l{{in, nullptr, 0, nullptr, 0}, in_dtype};
  const int widest = gx_dtype_size(in_dtype) > gx_dtype_size(out_dtype) ? gx_dtype_size(in_dtype) : gx_dtype_size(out_dtype);
  return ew_dispatch<KIND_UNARY>(class_of_dtype(in_dtype), widest, op, l, l, n, out_dtype, out, nullptr, nullptr, 0, s);
}

}  // namespace gx

extern "C" {

int gx_elementwise_tile_rows(void) { return gx::EW_TILE; }
int gx_elementwise_grid_cap(void) { return gx::EW_GRID_CAP; }

int gx_binary_op_supported(int op, int lhs_dtype, int rhs_dtype, int out_dtype)
{
  if (!gx::dtype_ok(lhs_dtype) || !gx::dtype_ok(rhs_dtype) || !gx::dtype_ok(out_dtype)) return 0;
  if (gx::binop_kind(op) < 0) return 0;
  const int cl = gx::class_of_dtype(lhs_dtype), cr = gx::class_of_dtype(rhs_dtype);
  const int c  = cl > cr ? cl : cr;
  if (gx::binop_integer_only(op) && c >= gx::CLS_F32) return 0;
  return 1;
}

int gx_unary_op_supported(int op, int in_dtype, int out_dtype)
{
  if (!gx::dtype_ok(in_dtype) || !gx::dtype_ok(out_dtype)) return 0;
  const bool is_float = in_dtype == GX_FLOAT32 || in_dtype == GX_FLOAT64;
  const bool is_bool  = in_dtype == GX_BOOL8;
  switch (op) {
    case GX_UNOP_ABS:
    case GX_UNOP_NEGATE: return !is_bool && out_dtype == in_dtype;
    case GX_UNOP_SQRT:
    case GX_UNOP_CEIL:
    case GX_UNOP_FLOOR:
    case GX_UNOP_RINT: return is_float && out_dtype == in_dtype;
    case GX_UNOP_BIT_INVERT: return !is_float && !is_bool && out_dtype == in_dtype;
    case GX_UNOP_NOT: return out_dtype == GX_BOOL8;
    case GX_UNOP_IS_NAN:
    case GX_UNOP_IS_NOT_NAN: return is_float && out_dtype == GX_BOOL8;
    default: return 0;  // the transcendental operators, CBRT and BIT_COUNT are not built
  }
}

int gx_binary_op(int op, int lhs_dtype, const void* lhs, const uint32_t* lhs_valid, int64_t lhs_begin_bit,
                 const uint8_t* lhs_scalar_valid_dev, int lhs_is_scalar, int rhs_dtype, const void* rhs, const uint32_t* rhs_valid,
                 int64_t rhs_begin_bit, const uint8_t* rhs_scalar_valid_dev, int rhs_is_scalar, int64_t n, int out_dtype, void* out,
                 uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  if (!gx::binop_known(op)) return GX_EINVAL;
  if (n < 0 || n > gx::EW_MAX_ROWS || lhs_begin_bit < 0 || rhs_begin_bit < 0) return GX_EINVAL;
  if (!gx_binary_op_supported(op, lhs_dtype, rhs_dtype, out_dtype)) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!lhs || !rhs || !out) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  const gx::Operand l{{lhs, lhs_is_scalar ? nullptr : lhs_valid, lhs_begin_bit, lhs_scalar_valid_dev, lhs_is_scalar}, lhs_dtype};
  const gx::Operand r{{rhs, rhs_is_scalar ? nullptr : rhs_valid, rhs_begin_bit, rhs_scalar_valid_dev, rhs_is_scalar}, rhs_dtype};
  const int cl = gx::class_of_dtype(lhs_dtype), cr = gx::class_of_dtype(rhs_dtype);
  const int c  = cl > cr ? cl : cr;
  const int widest   = gx::max3(gx_dtype_size(lhs_dtype), gx_dtype_size(rhs_dtype), gx_dtype_size(out_dtype));
  const int lhs_bits = gx_dtype_size(lhs_dtype) * 8;
  int64_t* nulls     = out_valid ? out_null_count_dev : nullptr;  // without a bitmap there are no nulls: the count stays 0
  switch (gx::binop_kind(op)) {
    case gx::KIND_BASIC: return gx::ew_dispatch<gx::KIND_BASIC>(c, widest, op, l, r, n, out_dtype, out, out_valid, nulls, lhs_bits, s);
    case gx::KIND_DIV: return gx::ew_dispatch<gx::KIND_DIV>(c, widest, op, l, r, n, out_dtype, out, out_valid, nulls, lhs_bits, s);
    default: return gx::ew_dispatch<gx::KIND_REAL>(c, widest, op, l, r, n, out_dtype, out, out_valid, nulls, lhs_bits, s);
  }
}

int gx_unary_op(int op, int in_dtype, const void* in, int64_t n, int out_dtype, void* out, gx_stream_t s)
{
  if (!gx::unop_known(op)) return GX_EINVAL;
  if (n < 0 || n > gx::EW_MAX_ROWS) return GX_EINVAL;
  if (!gx_unary_op_supported(op, in_dtype, out_dtype)) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!in || !out) return GX_EINVAL;
  return gx::unary_launch(op, in_dtype, in, n, out_dtype, out, s);
}

int gx_cast(int in_dtype, const void* in, int64_t n, int out_dtype, void* out, gx_stream_t s)
{
  if (n < 0 || n > gx::EW_MAX_ROWS) return GX_EINVAL;
  if (!gx::dtype_ok(in_dtype) || !gx::dtype_ok(out_dtype)) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!in || !out) return GX_EINVAL;
  return gx::unary_launch(gx::UNOP_CAST, in_dtype, in, n, out_dtype, out, s);
}

int gx_bitmask_to_bool8(const uint32_t* valid, int64_t begin_bit, int64_t n, int invert, uint8_t* out, gx_stream_t s)
{
  if (n < 0 || n > gx::EW_MAX_ROWS || begin_bit < 0) return GX_EINVAL;
  if (n == 0) return 0;
  if (!out) return GX_EINVAL;
  hipLaunchKernelGGL(gx::k_bitmask_to_bool8, dim3(gx::capped_grid(n, gx::EW_TILE, gx::EW_GRID_CAP)), dim3(gx::EW_BT), 0, s, valid, begin_bit, n, invert, out);
  GX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
