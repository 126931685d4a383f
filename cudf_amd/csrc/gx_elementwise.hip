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
#include "gx_elementwise_ops.hpp"  // classes, loads / stores, apply_*, out_bits: shared with gx_expression.hip

// results are compared bit for bit with a host that does not fuse: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace gx {

constexpr int EW_BT       = 256;
constexpr int EW_ROWS     = 16;               // rows of one thread per trip: 16 / R accesses of R rows
constexpr int EW_TILE     = EW_BT * EW_ROWS;  // rows one workgroup owns per trip: a multiple of 32, so it owns whole validity words
constexpr int EW_GRID_CAP = 2048;             // 8 workgroups on each of 256 CUs; further tiles are further trips
constexpr int64_t EW_MAX_ROWS = (int64_t(1) << 31) - 1;

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
