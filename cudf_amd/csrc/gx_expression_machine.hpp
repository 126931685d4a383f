// gx_expression_machine.hpp -- the accumulator machine of cudf::ast expressions, shared by the kernels that run its programs:
// gx_expression.hip (one row per value: compute_column) and gx_conditional_join.hip (one row PAIR per value: the conditional joins).
// Device side: the by-value arguments, the payload conversions, the sources of a value, the operators on R values.  Host side: type
// inference, the planner and plan().  One copy, as gx_elementwise_ops.hpp is for the per-value operators.
#pragma once
#include "gx_common.hpp"
#include "gx_elementwise_ops.hpp"

// results are compared bit for bit with a host that does not fuse: a * b + c stays two roundings
#pragma clang fp contract(off)

namespace gx {

constexpr int64_t EX_MAX_ROWS = (int64_t(1) << 31) - 1;
constexpr int EX_MAX_NODES = 32, EX_MAX_COLS = 16, EX_MAX_LITS = 16, EX_MAX_SLOTS = 4, EX_MAX_INSTR = 64;

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

// ---------------------------------------------------------------- host: types and the planner
// a program with the division family, TRUE_DIV / FLOOR_DIV or POW runs the HEAVY variant of a kernel
static inline bool program_is_heavy(const gx_expr_instr* ins, int n_instr)
{
  bool heavy = false;
  for (int ip = 0; ip < n_instr; ++ip) {
    const gx_expr_instr& in = ins[ip];
    if (in.kind == GX_EXPR_APPLY || in.kind == GX_EXPR_APPLY_REV) heavy = heavy || in.family == FAM_DIV || in.family == FAM_REAL || in.family == FAM_REAL_FLOOR;
  }
  return heavy;
}
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

}  // namespace gx
