// gx_expression.hip -- cudf::compute_column: a whole expression tree over the columns of a table in ONE launch.
// reference: cpp/include/cudf/ast/expressions.hpp, cpp/include/cudf/transform.hpp (compute_column), cpp/src/ast (expression_parser,
// the device expression evaluator with its per-thread intermediate storage).  Here the host linearises the tree into the program of
// an accumulator machine (below) and the kernel runs that program on R rows per thread and access, with the per-value operators,
// compute classes and validity rules of gx_elementwise_ops.hpp: what gx_binary_op / gx_unary_op / gx_cast compute node by node,
// without the intermediate columns.
//
// The machine.  One accumulator: R rows of 64-bit payload (the value in the compute class of the accumulator's dtype; 32-bit classes
// use the low word) and R validity bits.  Instructions: LOAD acc = src; APPLY acc = acc op src; APPLY_REV acc = src op acc;
// APPLY_UNARY acc = op(acc); SPILL slot k = acc.  src is a column, a literal or a spill slot.  The planner evaluates the heavier
// child of a binary node first, takes a leaf operand as src, and spills only under a node with two non-leaf children: a chain never
// leaves the registers.  Every index into the accumulator is a compile-time constant (the row loops are unrolled, the program
// counter only selects code), so nothing lives in scratch; spill slots are LDS, [slot][row][thread] payloads behind [slot][thread]
// validity words, sized by the plan's slot count.  The program, the column and the literal descriptors travel as one by-value
// kernel argument: every switch on them is wave-uniform.
#include "gx_common.hpp"
#include "gx_elementwise_ops.hpp"

// results are compared bit for bit with a host that does not fuse: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace gx {

constexpr int EX_BT        = 256;
constexpr int EX_ROWS      = 16;               // rows of one thread per trip: 16 / R accesses of R rows
constexpr int EX_TILE      = EX_BT * EX_ROWS;  // a multiple of 32: a workgroup owns whole validity words
constexpr int EX_GRID_CAP  = 2048;
constexpr int64_t EX_MAX_ROWS = (int64_t(1) << 31) - 1;
constexpr int EX_MAX_NODES = 32, EX_MAX_COLS = 16, EX_MAX_LITS = 16, EX_MAX_SLOTS = 4, EX_MAX_INSTR = 64;
constexpr int EX_SLOT_BITS_BYTES = EX_MAX_SLOTS * EX_BT * (int)sizeof(uint32_t);  // the validity words, in front of the payloads

// operator families of an instruction (gx_expr_instr::family); family_op is the gx_binop / gx_unop the family applies
enum { FAM_BASIC = 0, FAM_DIV = 1, FAM_REAL = 2, FAM_REAL_FLOOR = 3, FAM_UNARY = 4, FAM_NOT = 5, FAM_IS_NULL = 6, FAM_IDENTITY = 7, FAM_CAST = 8 };

struct ExprArgs {
  gx_expr_instr ins[EX_MAX_INSTR];
  gx_expr_column cols[EX_MAX_COLS];
  gx_expr_literal lits[EX_MAX_LITS];
  int n_instr;
  int out_dtype;
};

template <typename T>
using class_t = typename std::conditional<(sizeof(T) < 4), int32_t, T>::type;

template <typename C>
__device__ __forceinline__ C from_payload(uint64_t p)
{
  C c;
  if constexpr (sizeof(C) == 4) {
    const uint32_t w = (uint32_t)p;
    __builtin_memcpy(&c, &w, 4);
  } else {
    __builtin_memcpy(&c, &p, 8);
  }
  return c;
}
template <typename C>
__device__ __forceinline__ uint64_t to_payload(C c)
{
  if constexpr (sizeof(C) == 4) {
    uint32_t w;
    __builtin_memcpy(&w, &c, 4);
    return w;
  } else {
    uint64_t p;
    __builtin_memcpy(&p, &c, 8);
    return p;
  }
}

#define EX_EACH_DTYPE(X)                                                                                                     \
  X(GX_INT8, int8_t, false) X(GX_INT16, int16_t, false) X(GX_INT32, int32_t, false) X(GX_INT64, int64_t, false)              \
  X(GX_UINT8, uint8_t, false) X(GX_UINT16, uint16_t, false) X(GX_UINT32, uint32_t, false) X(GX_UINT64, uint64_t, false)      \
  X(GX_FLOAT32, float, false) X(GX_FLOAT64, double, false) X(GX_BOOL8, uint8_t, true)

// R rows of a column from row0 on, as payloads of the dtype's class (rows behind cnt: a value that divides)
template <int R>
__device__ __forceinline__ void fetch_column(int dtype, const void* p, int64_t row0, int cnt, uint64_t (&s)[R])
{
  switch (dtype) {
#define EX_LD(DT, T, ISB)                                   \
  case DT: {                                                \
    using C = class_t<T>;                                   \
    C v[R];                                                 \
    load_as<C, T, R, ISB>(p, row0, cnt, 0, v);              \
    _Pragma("unroll") for (int k = 0; k < R; ++k) s[k] = to_payload<C>(v[k]); \
  } break;
    EX_EACH_DTYPE(EX_LD)
#undef EX_LD
    default: break;
  }
}
// a literal in every row (its width does not bound R: it is one scalar load)
template <int R>
__device__ __forceinline__ void fetch_literal(int dtype, const void* p, uint64_t (&s)[R])
{
  uint64_t x = 0;
  switch (dtype) {
#define EX_LIT(DT, T, ISB)                                  \
  case DT: {                                                \
    using C   = class_t<T>;                                 \
    const T v = *static_cast<const T*>(p);                  \
    x         = to_payload<C>(ISB ? C(v != 0) : C(v));      \
  } break;
    EX_EACH_DTYPE(EX_LIT)
#undef EX_LIT
    default: break;
  }
#pragma unroll
  for (int k = 0; k < R; ++k) s[k] = x;
}
template <int R>
__device__ __forceinline__ void store_result(int dtype, void* out, int64_t row0, int cnt, const uint64_t (&acc)[R])
{
  switch (dtype) {
#define EX_ST(DT, T, ISB)                                   \
  case DT: {                                                \
    using C = class_t<T>;                                   \
    C v[R];                                                 \
    _Pragma("unroll") for (int k = 0; k < R; ++k) v[k] = from_payload<C>(acc[k]); \
    store_as<C, T, R, ISB>(out, row0, cnt, v);              \
  } break;
    EX_EACH_DTYPE(EX_ST)
#undef EX_ST
    default: break;
  }
}

#define EX_EACH_CLASS(c, BODY)                                            \
  switch (c) {                                                            \
    case CLS_I32: { using C = int32_t; BODY } break;                      \
    case CLS_U32: { using C = uint32_t; BODY } break;                     \
    case CLS_I64: { using C = int64_t; BODY } break;                      \
    case CLS_U64: { using C = uint64_t; BODY } break;                     \
    case CLS_F32: { using C = float; BODY } break;                        \
    default: { using C = double; BODY } break;                            \
  }

// acc = lhs op rhs in class C; lb / rb the operands' validity bits, lm the rows that exist.  HEAVY: the division family, TRUE_DIV and
// POW are built in (64-bit integer division and pow() set the register count of the whole kernel: a program without them runs the
// variant without them, at twice the waves per SIMD)
template <typename C, int R, bool HEAVY>
__device__ __forceinline__ void apply_binary(const gx_expr_instr& in, const uint64_t (&lp)[R], const uint64_t (&rp)[R], uint32_t lb, uint32_t rb,
                                             uint32_t lm, uint64_t (&acc)[R], uint32_t& ab)
{
  C x[R], y[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    x[k] = from_payload<C>(lp[k]);
    y[k] = from_payload<C>(rp[k]);
  }
  const int fop = in.family_op;
  if (HEAVY && (in.family == FAM_REAL || in.family == FAM_REAL_FLOOR)) {
    double o[R];
    apply_real<C, R>(fop, x, y, o);
    if (in.family == FAM_REAL_FLOOR) {
#pragma unroll
      for (int k = 0; k < R; ++k) o[k] = floor(o[k]);
    }
    if (in.out_dtype == GX_FLOAT32) {
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<float>(float(o[k]));
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<double>(o[k]);
    }
    ab = lb & rb & lm;
  } else {
    C o[R];
    if (!HEAVY || in.family == FAM_BASIC) apply_rows<C, R, KIND_BASIC>(fop, x, y, lb, rb, cls<C>::bits, o); else apply_rows<C, R, KIND_DIV>(fop, x, y, lb, rb, cls<C>::bits, o);
    ab = out_bits<C, R>(fop, x, y, lb, rb) & lm;
    if (in.out_dtype == GX_BOOL8) {  // a truth value, 0 / 1 in C: BOOL8 lives in the int class
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<int32_t>(int32_t(o[k]));
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<C>(o[k]);
    }
  }
}

template <typename C, int R>
__device__ __forceinline__ void apply_unary_instr(const gx_expr_instr& in, uint64_t (&acc)[R])
{
  C x[R];
#pragma unroll
  for (int k = 0; k < R; ++k) x[k] = from_payload<C>(acc[k]);
  if (in.family == FAM_CAST) {
    switch (in.out_dtype) {
      case GX_INT64:
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = to_payload<int64_t>(int64_t(x[k]));
        break;
      case GX_UINT64:
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = to_payload<uint64_t>(uint64_t(x[k]));
        break;
      default:
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = to_payload<double>(double(x[k]));
        break;
    }
  } else {
    C o[R];
    apply_unary<C, R>(in.family_op, x, o);
    if (in.family == FAM_NOT) {
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<int32_t>(int32_t(o[k]));
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) acc[k] = to_payload<C>(o[k]);
    }
  }
}

// Rows, tiles, the merge of the validity word across the lanes that share it, the null count and the capped grid are k_elementwise's.
template <int R, bool HEAVY>
__global__ void __launch_bounds__(EX_BT) k_expression(const ExprArgs a, int64_t n, void* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                      unsigned long long* __restrict__ null_count)
{
  constexpr int NJ    = EX_ROWS / R;
  constexpr int GROUP = 32 / R;  // lanes that share a validity word
  extern __shared__ uint64_t ex_lds[];
  __shared__ unsigned long long s_nulls;
  uint32_t* slot_bits    = reinterpret_cast<uint32_t*>(ex_lds);
  uint64_t* slot_payload = ex_lds + EX_SLOT_BITS_BYTES / sizeof(uint64_t);
  const unsigned t    = threadIdx.x;
  const unsigned lane = lane_id();
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  const int64_t tiles = div_up(n, EX_TILE);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * EX_TILE;
#pragma unroll 1
    for (int j = 0; j < NJ; ++j) {
      const int64_t row0 = t0 + ((int64_t)j * EX_BT + t) * R;
      if (row0 - (int64_t)lane * R >= n) break;  // the whole wave is behind the last row, in this access and in the later ones
      const int cnt     = row0 >= n ? 0 : (n - row0 < R ? (int)(n - row0) : R);
      const uint32_t lm = (1u << cnt) - 1u;      // cnt <= 16
      uint32_t ab = 0;
      if (cnt > 0) {
        uint64_t acc[R];
#pragma unroll
        for (int k = 0; k < R; ++k) acc[k] = 0;
#pragma unroll 1
        for (int ip = 0; ip < a.n_instr; ++ip) {
          const gx_expr_instr in = a.ins[ip];
          if (in.kind == GX_EXPR_SPILL) {
            slot_bits[in.src_index * EX_BT + t] = ab;
#pragma unroll
            for (int k = 0; k < R; ++k) slot_payload[(in.src_index * R + k) * EX_BT + t] = acc[k];
            continue;
          }
          if (in.kind == GX_EXPR_APPLY_UNARY) {
            if (in.family == FAM_IS_NULL) {
#pragma unroll
              for (int k = 0; k < R; ++k) acc[k] = ((ab >> k) & 1u) ^ 1u;
              ab = lm;
            } else if (in.family != FAM_IDENTITY) {
              EX_EACH_CLASS(class_of_dtype(in.in_dtype), (apply_unary_instr<C, R>(in, acc));)
            }
            continue;
          }
          uint64_t src[R];
          uint32_t sb;
          if (in.src_kind == GX_EXPR_SRC_COLUMN) {
            const gx_expr_column c = a.cols[in.src_index];
            fetch_column<R>(c.dtype, c.data, row0, cnt, src);
            sb = c.valid ? bits_from(c.valid, c.begin_bit + row0, cnt) : lm;
          } else if (in.src_kind == GX_EXPR_SRC_LITERAL) {
            const gx_expr_literal l = a.lits[in.src_index];
            fetch_literal<R>(l.dtype, l.value, src);
            sb = (l.valid == nullptr || *l.valid != 0) ? lm : 0u;
          } else {
            sb = slot_bits[in.src_index * EX_BT + t];
#pragma unroll
            for (int k = 0; k < R; ++k) src[k] = slot_payload[(in.src_index * R + k) * EX_BT + t];
          }
          if (in.kind == GX_EXPR_LOAD) {
#pragma unroll
            for (int k = 0; k < R; ++k) acc[k] = src[k];
            ab = sb;
            continue;
          }
          const bool rev = in.kind == GX_EXPR_APPLY_REV;
          uint64_t lp[R], rp[R];
#pragma unroll
          for (int k = 0; k < R; ++k) {
            lp[k] = rev ? src[k] : acc[k];
            rp[k] = rev ? acc[k] : src[k];
          }
          const uint32_t lb = rev ? sb : ab, rb = rev ? ab : sb;
          EX_EACH_CLASS(class_of_dtype(in.in_dtype), (apply_binary<C, R, HEAVY>(in, lp, rp, lb, rb, lm, acc, ab));)
        }
        store_result<R>(a.out_dtype, out, row0, cnt, acc);
      }
      if (out_valid) {  // every lane of the wave is here
        uint32_t w = ab << ((lane % GROUP) * R);
#pragma unroll
        for (int d = 1; d < GROUP; d <<= 1) w |= (uint32_t)__shfl_xor((int)w, d, GX_WAVE);
        if (lane % GROUP == 0 && row0 < n) out_valid[row0 >> 5] = w;
        nulls += (unsigned long long)__builtin_popcount(~ab & lm);
      }
    }
  }
  if (null_count) tally_end(&s_nulls, wave_reduce(nulls, SumOp()), null_count);
}

// ---------------------------------------------------------------- host: types, the planner, the launch
struct NodeType {
  int dtype;
  int slots;  // spill slots its evaluation into the accumulator needs
  bool leaf;
  int family, family_op, in_dtype;
};

static inline int class_dtype(int d)
{
  switch (d) {
    case GX_UINT32: case GX_INT64: case GX_UINT64: case GX_FLOAT32: case GX_FLOAT64: return d;
    default: return GX_INT32;
  }
}

// the gx_binop an AST binary operator maps to (FLOOR_DIV: TRUE_DIV, floored), its family and result; -1: not a binary operator
static inline int binary_rule(int op, int t, int* family, int* result)
{
  const int c = class_dtype(t);
  switch (op) {
    case GX_AST_ADD: *family = FAM_BASIC; *result = c; return GX_BINOP_ADD;
    case GX_AST_SUB: *family = FAM_BASIC; *result = c; return GX_BINOP_SUB;
    case GX_AST_MUL: *family = FAM_BASIC; *result = c; return GX_BINOP_MUL;
    case GX_AST_DIV: *family = FAM_DIV; *result = c; return GX_BINOP_DIV;
    case GX_AST_MOD: *family = FAM_DIV; *result = c; return GX_BINOP_MOD;
    case GX_AST_PYMOD: *family = FAM_DIV; *result = c; return GX_BINOP_PYMOD;
    case GX_AST_TRUE_DIV: *family = FAM_REAL; *result = GX_FLOAT64; return GX_BINOP_TRUE_DIV;
    case GX_AST_FLOOR_DIV: *family = FAM_REAL_FLOOR; *result = GX_FLOAT64; return GX_BINOP_TRUE_DIV;
    case GX_AST_POW: *family = FAM_REAL; *result = t == GX_FLOAT32 ? GX_FLOAT32 : GX_FLOAT64; return GX_BINOP_POW;
    case GX_AST_BITWISE_AND: *family = FAM_BASIC; *result = c; return GX_BINOP_BITWISE_AND;
    case GX_AST_BITWISE_OR: *family = FAM_BASIC; *result = c; return GX_BINOP_BITWISE_OR;
    case GX_AST_BITWISE_XOR: *family = FAM_BASIC; *result = c; return GX_BINOP_BITWISE_XOR;
    case GX_AST_EQUAL: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_EQUAL;
    case GX_AST_NULL_EQUAL: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_NULL_EQUALS;
    case GX_AST_NOT_EQUAL: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_NOT_EQUAL;
    case GX_AST_LESS: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_LESS;
    case GX_AST_GREATER: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_GREATER;
    case GX_AST_LESS_EQUAL: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_LESS_EQUAL;
    case GX_AST_GREATER_EQUAL: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_GREATER_EQUAL;
    case GX_AST_LOGICAL_AND: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_LOGICAL_AND;
    case GX_AST_NULL_LOGICAL_AND: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_NULL_LOGICAL_AND;
    case GX_AST_LOGICAL_OR: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_LOGICAL_OR;
    case GX_AST_NULL_LOGICAL_OR: *family = FAM_BASIC; *result = GX_BOOL8; return GX_BINOP_NULL_LOGICAL_OR;
    default: return -1;
  }
}

// 0, or GX_EDTYPE: family, the family's operator and the result of a unary operator on dtype t
static inline int unary_rule(int op, int t, int* family, int* family_op, int* result)
{
  const int c = class_dtype(t);
  *family_op  = 0;
  switch (op) {
    case GX_AST_IDENTITY: *family = FAM_IDENTITY; *result = t; return 0;
    case GX_AST_IS_NULL: *family = FAM_IS_NULL; *result = GX_BOOL8; return 0;
    case GX_AST_NOT: *family = FAM_NOT; *family_op = GX_UNOP_NOT; *result = GX_BOOL8; return gx_unary_op_supported(GX_UNOP_NOT, t, GX_BOOL8) ? 0 : GX_EDTYPE;
    case GX_AST_ABS: *family = FAM_UNARY; *family_op = GX_UNOP_ABS; *result = c; return gx_unary_op_supported(GX_UNOP_ABS, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_BIT_INVERT: *family = FAM_UNARY; *family_op = GX_UNOP_BIT_INVERT; *result = c; return gx_unary_op_supported(GX_UNOP_BIT_INVERT, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_SQRT: *family = FAM_UNARY; *family_op = GX_UNOP_SQRT; *result = t; return gx_unary_op_supported(GX_UNOP_SQRT, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_CEIL: *family = FAM_UNARY; *family_op = GX_UNOP_CEIL; *result = t; return gx_unary_op_supported(GX_UNOP_CEIL, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_FLOOR: *family = FAM_UNARY; *family_op = GX_UNOP_FLOOR; *result = t; return gx_unary_op_supported(GX_UNOP_FLOOR, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_RINT: *family = FAM_UNARY; *family_op = GX_UNOP_RINT; *result = t; return gx_unary_op_supported(GX_UNOP_RINT, t, t) ? 0 : GX_EDTYPE;
    case GX_AST_CAST_TO_INT64: *family = FAM_CAST; *result = GX_INT64; return 0;
    case GX_AST_CAST_TO_UINT64: *family = FAM_CAST; *result = GX_UINT64; return 0;
    case GX_AST_CAST_TO_FLOAT64: *family = FAM_CAST; *result = GX_FLOAT64; return 0;
    default: return GX_EDTYPE;  // the transcendental operators and CBRT are not built
  }
}

// structure first (GX_EINVAL), then types (GX_EDTYPE): ty[i] for every node
static int infer(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes, int n_lits, NodeType* ty)
{
  if (!nodes || n_nodes < 1 || n_nodes > EX_MAX_NODES || n_cols < 0 || n_cols > EX_MAX_COLS || n_lits < 0 || n_lits > EX_MAX_LITS) return GX_EINVAL;
  if ((n_cols > 0 && !col_dtypes) || (n_lits > 0 && !lit_dtypes)) return GX_EINVAL;
  for (int i = 0; i < n_nodes; ++i) {
    const gx_expr_node& nd = nodes[i];
    switch (nd.kind) {
      case GX_EXPR_COLUMN:
        if (nd.lhs < 0 || nd.lhs >= n_cols) return GX_EINVAL;
        break;
      case GX_EXPR_LITERAL:
        if (nd.lhs < 0 || nd.lhs >= n_lits) return GX_EINVAL;
        break;
      case GX_EXPR_UNARY:
        if (nd.lhs < 0 || nd.lhs >= i || nd.op < GX_AST_IDENTITY || nd.op > GX_AST_CAST_TO_FLOAT64) return GX_EINVAL;
        break;
      case GX_EXPR_BINARY:
        if (nd.lhs < 0 || nd.lhs >= i || nd.rhs < 0 || nd.rhs >= i || nd.op < GX_AST_ADD || nd.op > GX_AST_NULL_LOGICAL_OR) return GX_EINVAL;
        break;
      default: return GX_EINVAL;
    }
  }
  for (int i = 0; i < n_nodes; ++i) {
    const gx_expr_node& nd = nodes[i];
    NodeType& t            = ty[i];
    t = NodeType{0, 0, false, 0, 0, 0};
    if (nd.kind == GX_EXPR_COLUMN || nd.kind == GX_EXPR_LITERAL) {
      t.dtype = nd.kind == GX_EXPR_COLUMN ? col_dtypes[nd.lhs] : lit_dtypes[nd.lhs];
      t.leaf  = true;
      if (!dtype_ok(t.dtype)) return GX_EDTYPE;
    } else if (nd.kind == GX_EXPR_UNARY) {
      const NodeType& c = ty[nd.lhs];
      t.in_dtype        = c.dtype;
      t.slots           = c.slots;
      if (int rc = unary_rule(nd.op, c.dtype, &t.family, &t.family_op, &t.dtype); rc != 0) return rc;
    } else {
      const NodeType &l = ty[nd.lhs], &r = ty[nd.rhs];
      if (l.dtype != r.dtype) return GX_EDTYPE;
      t.in_dtype  = l.dtype;
      t.family_op = binary_rule(nd.op, l.dtype, &t.family, &t.dtype);
      if (!gx_binary_op_supported(t.family_op, l.dtype, l.dtype, t.dtype)) return GX_EDTYPE;
      if (l.leaf || r.leaf) t.slots = l.leaf ? r.slots : l.slots;
      else t.slots = l.slots == r.slots ? l.slots + 1 : (l.slots > r.slots ? l.slots : r.slots);
    }
  }
  return 0;
}

struct Planner {
  const gx_expr_node* nodes;
  const NodeType* ty;
  gx_expr_instr* ins;  // EX_MAX_INSTR of them
  int count;           // may run past EX_MAX_INSTR: only the first EX_MAX_INSTR are stored
  int slots;

  void emit(int kind, int op, int src_kind, int src_index, int in_dtype, int out_dtype, int family, int family_op)
  {
    if (count < EX_MAX_INSTR)
      ins[count] = gx_expr_instr{(uint8_t)kind, (uint8_t)op, (uint8_t)src_kind, (uint8_t)src_index, (uint8_t)in_dtype, (uint8_t)out_dtype, (uint8_t)family, (uint8_t)family_op};
    ++count;
  }
  static int src_kind_of(const gx_expr_node& nd) { return nd.kind == GX_EXPR_COLUMN ? GX_EXPR_SRC_COLUMN : GX_EXPR_SRC_LITERAL; }
  // node i into the accumulator; `depth` slots are live
  void eval(int i, int depth)
  {
    if (count > EX_MAX_INSTR) return;  // a shared subtree can unfold without bound: the caller reports the overflow
    const gx_expr_node& nd = nodes[i];
    const NodeType& t      = ty[i];
    if (t.leaf) {
      emit(GX_EXPR_LOAD, 0, src_kind_of(nd), nd.lhs, t.dtype, t.dtype, 0, 0);
    } else if (nd.kind == GX_EXPR_UNARY) {
      eval(nd.lhs, depth);
      emit(GX_EXPR_APPLY_UNARY, nd.op, 0, 0, t.in_dtype, t.dtype, t.family, t.family_op);
    } else {
      const NodeType &l = ty[nd.lhs], &r = ty[nd.rhs];
      if (r.leaf) {  // acc = l, then acc op r
        eval(nd.lhs, depth);
        emit(GX_EXPR_APPLY, nd.op, src_kind_of(nodes[nd.rhs]), nodes[nd.rhs].lhs, t.in_dtype, t.dtype, t.family, t.family_op);
      } else if (l.leaf) {  // acc = r, then l op acc
        eval(nd.rhs, depth);
        emit(GX_EXPR_APPLY_REV, nd.op, src_kind_of(nodes[nd.lhs]), nodes[nd.lhs].lhs, t.in_dtype, t.dtype, t.family, t.family_op);
      } else {  // the heavier side first, into slot `depth`; the other side runs with one more slot live
        const bool left_first = l.slots >= r.slots;
        eval(left_first ? nd.lhs : nd.rhs, depth);
        emit(GX_EXPR_SPILL, 0, GX_EXPR_SRC_SLOT, depth, t.in_dtype, t.in_dtype, 0, 0);
        if (depth + 1 > slots) slots = depth + 1;
        eval(left_first ? nd.rhs : nd.lhs, depth + 1);
        emit(left_first ? GX_EXPR_APPLY_REV : GX_EXPR_APPLY, nd.op, GX_EXPR_SRC_SLOT, depth, t.in_dtype, t.dtype, t.family, t.family_op);
      }
    }
  }
};

// the program of an expression: 0, GX_EINVAL (malformed, or beyond a limit), GX_EDTYPE
static int plan(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes, int n_lits,
                gx_expr_instr* ins, int* n_instr, int* n_slots, int* result_dtype)
{
  NodeType ty[EX_MAX_NODES];
  if (int rc = infer(nodes, n_nodes, col_dtypes, n_cols, lit_dtypes, n_lits, ty); rc != 0) return rc;
  if (ty[n_nodes - 1].slots > EX_MAX_SLOTS) return GX_EINVAL;
  Planner p{nodes, ty, ins, 0, 0};
  p.eval(n_nodes - 1, 0);
  if (p.count > EX_MAX_INSTR) return GX_EINVAL;
  *n_instr      = p.count;
  *n_slots      = p.slots;
  *result_dtype = ty[n_nodes - 1].dtype;
  return 0;
}

template <int R, bool HEAVY>
static int ex_launch_as(const ExprArgs& a, int n_slots, int64_t n, void* out, uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  const dim3 grid(capped_grid(n, EX_TILE, EX_GRID_CAP)), block(EX_BT);
  unsigned long long* nc = reinterpret_cast<unsigned long long*>(nulls);
  if (n_slots == 0) {
    hipLaunchKernelGGL((k_expression<R, HEAVY>), grid, block, 0, s, a, n, out, out_valid, nc);
  } else {
    Device dev;
    GX_HIP_TRY(device(&dev));
    const size_t lds = (size_t)EX_SLOT_BITS_BYTES + (size_t)n_slots * R * EX_BT * sizeof(uint64_t);
    GX_HIP_TRY(launch_lds(dev, k_expression<R, HEAVY>, grid, block, lds, s, a, n, out, out_valid, nc));
  }
  GX_LAUNCH_CHECK();
  return 0;
}
template <int R>
static int ex_launch(const ExprArgs& a, int n_slots, int64_t n, void* out, uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  bool heavy = false;
  for (int ip = 0; ip < a.n_instr; ++ip) {
    const gx_expr_instr& in = a.ins[ip];
    if (in.kind == GX_EXPR_APPLY || in.kind == GX_EXPR_APPLY_REV) heavy = heavy || in.family == FAM_DIV || in.family == FAM_REAL || in.family == FAM_REAL_FLOOR;
  }
  return heavy ? ex_launch_as<R, true>(a, n_slots, n, out, out_valid, nulls, s) : ex_launch_as<R, false>(a, n_slots, n, out, out_valid, nulls, s);
}

}  // namespace gx

extern "C" {

int gx_expression_tile_rows(void) { return gx::EX_TILE; }
int gx_expression_grid_cap(void) { return gx::EX_GRID_CAP; }

void gx_expr_limits(int* max_nodes, int* max_columns, int* max_literals, int* max_slots)
{
  if (max_nodes) *max_nodes = gx::EX_MAX_NODES;
  if (max_columns) *max_columns = gx::EX_MAX_COLS;
  if (max_literals) *max_literals = gx::EX_MAX_LITS;
  if (max_slots) *max_slots = gx::EX_MAX_SLOTS;
}

int gx_expr_result_dtype(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes, int n_lits)
{
  gx_expr_instr ins[gx::EX_MAX_INSTR];
  int n_instr = 0, n_slots = 0, dtype = 0;
  if (int rc = gx::plan(nodes, n_nodes, col_dtypes, n_cols, lit_dtypes, n_lits, ins, &n_instr, &n_slots, &dtype); rc != 0) return rc;
  return dtype;
}

int gx_expr_plan(const gx_expr_node* nodes, int n_nodes, const int32_t* col_dtypes, int n_cols, const int32_t* lit_dtypes, int n_lits,
                 gx_expr_instr* out_instructions, int capacity, int* n_instructions, int* n_slots)
{
  gx_expr_instr ins[gx::EX_MAX_INSTR];
  int n_instr = 0, slots = 0, dtype = 0;
  if (!n_instructions || !n_slots || capacity < 0 || (capacity > 0 && !out_instructions)) return GX_EINVAL;
  if (int rc = gx::plan(nodes, n_nodes, col_dtypes, n_cols, lit_dtypes, n_lits, ins, &n_instr, &slots, &dtype); rc != 0) return rc;
  *n_instructions = n_instr;
  *n_slots        = slots;
  if (capacity < n_instr) return GX_EOVERFLOW;
  for (int i = 0; i < n_instr; ++i) out_instructions[i] = ins[i];
  return 0;
}

int gx_compute_column(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits, int n_lits,
                      int64_t n, int out_dtype, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  if (n < 0 || n > gx::EX_MAX_ROWS) return GX_EINVAL;
  if (n_cols < 0 || n_cols > gx::EX_MAX_COLS || n_lits < 0 || n_lits > gx::EX_MAX_LITS) return GX_EINVAL;
  if ((n_cols > 0 && !cols) || (n_lits > 0 && !lits)) return GX_EINVAL;
  int32_t col_dtypes[gx::EX_MAX_COLS], lit_dtypes[gx::EX_MAX_LITS];
  for (int i = 0; i < n_cols; ++i) {
    col_dtypes[i] = cols[i].dtype;
    if (cols[i].begin_bit < 0) return GX_EINVAL;
  }
  for (int i = 0; i < n_lits; ++i) lit_dtypes[i] = lits[i].dtype;
  gx::ExprArgs a;
  int n_slots = 0, dtype = 0;
  if (int rc = gx::plan(nodes, n_nodes, col_dtypes, n_cols, lit_dtypes, n_lits, a.ins, &a.n_instr, &n_slots, &dtype); rc != 0) return rc;
  if (!gx::dtype_ok(out_dtype) || out_dtype != dtype) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!out) return GX_EINVAL;
  // only what the program reads needs a pointer, and only that bounds the rows per access
  int widest = gx_dtype_size(out_dtype);
  for (int ip = 0; ip < a.n_instr; ++ip) {
    const gx_expr_instr& in = a.ins[ip];
    if (in.kind == GX_EXPR_SPILL || in.kind == GX_EXPR_APPLY_UNARY) continue;
    if (in.src_kind == GX_EXPR_SRC_COLUMN) {
      if (!cols[in.src_index].data) return GX_EINVAL;
      const int w = gx_dtype_size(cols[in.src_index].dtype);
      if (w > widest) widest = w;
    } else if (in.src_kind == GX_EXPR_SRC_LITERAL) {
      if (!lits[in.src_index].value) return GX_EINVAL;
    }
  }
  for (int i = 0; i < n_cols; ++i) a.cols[i] = cols[i];
  for (int i = 0; i < n_lits; ++i) a.lits[i] = lits[i];
  a.out_dtype = out_dtype;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  int64_t* nulls = out_valid ? out_null_count_dev : nullptr;  // without a bitmap there are no nulls: the count stays 0
  switch (widest) {
    case 1: return gx::ex_launch<16>(a, n_slots, n, out, out_valid, nulls, s);
    case 2: return gx::ex_launch<8>(a, n_slots, n, out, out_valid, nulls, s);
    case 4: return gx::ex_launch<4>(a, n_slots, n, out, out_valid, nulls, s);
    default: return gx::ex_launch<2>(a, n_slots, n, out, out_valid, nulls, s);
  }
}

}  // extern "C"
