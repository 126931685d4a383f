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
#include "gx_expression_machine.hpp"

namespace gx {

constexpr int EX_BT        = 256;
constexpr int EX_ROWS      = 16;               // rows of one thread per trip: 16 / R accesses of R rows
constexpr int EX_TILE      = EX_BT * EX_ROWS;  // a multiple of 32: a workgroup owns whole validity words
constexpr int EX_GRID_CAP  = 2048;
constexpr int EX_SLOT_BITS_BYTES = EX_MAX_SLOTS * EX_BT * (int)sizeof(uint32_t);  // the validity words, in front of the payloads

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

// ---------------------------------------------------------------- host: the launch
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
  return program_is_heavy(a.ins, a.n_instr) ? ex_launch_as<R, true>(a, n_slots, n, out, out_valid, nulls, s) : ex_launch_as<R, false>(a, n_slots, n, out, out_valid, nulls, s);
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
    if (cols[i].begin_bit < 0 || cols[i].table != 0) return GX_EINVAL;  // one table: a RIGHT column belongs to the conditional joins
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
