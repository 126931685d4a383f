// gx_conditional_join.hip -- cudf::conditional_*_join: an AST predicate over every (left row, right row) pair.
// reference: cpp/include/cudf/join/conditional_join.hpp, cpp/src/join/conditional_join.cu, conditional_join_kernels.cuh (one thread per
// left row walks the right table twice: a size pass and a write pass; a pair matches when the predicate is valid and true).
// Here the pair kernel runs the program of the accumulator machine (gx_expression_machine.hpp) that compute_column runs, with two
// kinds of column source.
//
// The pair walk.  A workgroup owns a tile of TL = blockDim.x left rows, a thread one left row, and one segment of the right table (the
// grid's y: as many segments as fill the device when the left tiles alone do not), which it walks in chunks of TR rows.  The columns the program reads are converted once per tile (left) and once per chunk (right) into 64-bit payloads
// in LDS, [column][row]; validity: the left row's column bits stay in a register, the right rows' are [column][row / 32] words
// behind the payloads.  In the pair loop a LEFT source is then a per-lane LDS read at stride 1 and a RIGHT source a read of one
// address by the whole wave (a broadcast); a literal is a broadcast too: no global load sits in the pair loop.  One run of the
// program evaluates R pairs per thread, one left row against R consecutive right rows, as acc[R] with compile-time indices: the
// instruction fetch and the wave-uniform switches of the interpreter are paid once per R pairs.  Where the rows of a pair come
// from is decided in one place, PairSource below (a later pair-list mode replaces it).
//
// Passes.  The pair order is fixed -- ascending (left, right) -- so the output position of a left row's matches is the exclusive
// scan of the counts per (left row, segment), row-major: COUNT writes them (and, for FULL, clears the bit of every matched right row
// in a bitmap that starts all ones), k_outer_fix gives an unmatched row of LEFT / FULL its one place, the scan runs in place, WRITE
// evaluates the predicate again and stores each cell's matches from its offset on, as the reference does.  MARK (semi / anti) sets
// (clears) one bit per matched left row and leaves the chunk loop as soon as every row of the tile has
// matched (a wave leaves the pair loop as soon as every one of its rows has); the existing selectors turn that bitmap, and FULL's
// bitmap of unmatched right rows, into ascending row lists.
#include "gx_expression_machine.hpp"
#include "gx_scan.hpp"

#include <atomic>

namespace gx {

constexpr int CJ_TL       = 256;  // the widest left tile: the most threads of a workgroup
constexpr int CJ_TR       = 256;  // right rows per chunk
constexpr int CJ_R        = 8;    // pairs per thread and run of the program (measured: 8 beats 4 beats 2 on every arm)
constexpr int CJ_GRID_CAP = 2048;
constexpr int CJ_SRC_RIGHT = 3;   // src_kind of a staged RIGHT column (GX_EXPR_SRC_COLUMN: a staged LEFT column); kernel-internal
enum { CJ_COUNT = 0, CJ_WRITE = 1, CJ_MARK = 2 };
enum { CJ_LEFT_OUTER = 1, CJ_FULL = 2, CJ_INVERT = 4 };  // flags of a launch

// what the kernel gets by value: the program with its column sources renumbered to the staged columns of their side
struct PairArgs {
  gx_expr_instr ins[EX_MAX_INSTR];
  gx_expr_column lcols[EX_MAX_COLS], rcols[EX_MAX_COLS];  // the columns the program reads, per side
  gx_expr_literal lits[EX_MAX_LITS];
  int n_instr, n_l, n_r, n_lits, n_slots;
};

// byte offsets of the LDS image: 8-byte arrays first
struct PairLds {
  int lit_p, l_p, r_p, slot_p, r_v, slot_b, lit_v, r_hit, total;
};
__host__ __device__ static inline PairLds pair_lds(int tl, int tr, int n_l, int n_r, int n_slots, int r)
{
  PairLds o;
  int at   = 0;
  o.lit_p  = at; at += EX_MAX_LITS * 8;
  o.l_p    = at; at += n_l * tl * 8;
  o.r_p    = at; at += n_r * tr * 8;
  o.slot_p = at; at += n_slots * r * tl * 8;
  o.r_v    = at; at += (n_r > 0 ? n_r : 1) * (tr / 32) * 4;
  o.slot_b = at; at += n_slots * tl * 4;
  o.lit_v  = at; at += EX_MAX_LITS * 4;
  o.r_hit  = at; at += (tr / 32) * 4;
  o.total  = at;
  return o;
}

// The rows of a pair: thread t of tile `tile` owns left row tile * TL + t, the chunk at c0 holds right rows c0 .. c0 + TR - 1.
// The right table is cut into n_seg segments of seg_rows rows (whole chunks): workgroup (x, y) walks segment y only.
struct PairSource {
  int64_t n_left, n_right, seg_rows;
  int n_seg;
  __device__ __forceinline__ int64_t left_row(int64_t tile, int tl, unsigned t) const { return tile * tl + t; }
  __device__ __forceinline__ int64_t right_row(int64_t c0, int r) const { return c0 + r; }
};

// what a pass writes (and WRITE's offsets); a pass touches only its own members
struct PairOut {
  int32_t* counts;                 // COUNT: matches per (left row, segment), [row][segment]
  unsigned long long* total;       // COUNT: their sum
  uint32_t* right_unmatched;       // COUNT of FULL: all ones on entry
  const int32_t* offsets;          // WRITE: the exclusive scan of counts (k_outer_fix gave an unmatched row of LEFT / FULL one place)
  const uint8_t* lone;             // WRITE of LEFT / FULL: 1 for a left row without a match
  int32_t *out_l, *out_r;          // WRITE
  uint32_t* left_bits;             // MARK: zeroes on entry (SEMI: matched rows are set), ones under CJ_INVERT (ANTI: they are cleared)
};

__device__ __forceinline__ uint32_t valid_bit(const gx_expr_column& c, int64_t row)
{
  if (!c.valid) return 1u;
  const int64_t b = c.begin_bit + row;
  return (c.valid[b >> 5] >> (b & 31)) & 1u;
}

template <int R, bool HEAVY>
__global__ void __launch_bounds__(CJ_TL) k_pairs(const PairArgs a, const PairSource ps, int mode, int flags, int tr, const PairOut po)
{
  extern __shared__ uint64_t cj_lds[];
  const int tl     = (int)blockDim.x;
  const PairLds o  = pair_lds(tl, tr, a.n_l, a.n_r, a.n_slots, R);
  char* base       = reinterpret_cast<char*>(cj_lds);
  uint64_t* lit_p  = reinterpret_cast<uint64_t*>(base + o.lit_p);
  uint64_t* l_p    = reinterpret_cast<uint64_t*>(base + o.l_p);
  uint64_t* r_p    = reinterpret_cast<uint64_t*>(base + o.r_p);
  uint64_t* slot_payload = reinterpret_cast<uint64_t*>(base + o.slot_p);
  uint32_t* r_v    = reinterpret_cast<uint32_t*>(base + o.r_v);
  uint32_t* slot_bits = reinterpret_cast<uint32_t*>(base + o.slot_b);
  uint32_t* lit_v  = reinterpret_cast<uint32_t*>(base + o.lit_v);
  uint32_t* r_hit  = reinterpret_cast<uint32_t*>(base + o.r_hit);
  const unsigned t    = threadIdx.x;
  const unsigned lane = lane_id();
  const int rwords    = tr / 32;
  const bool full     = (flags & CJ_FULL) != 0;

  if ((int)t < a.n_lits) {  // the literals, once: read before the first pair loop's barrier
    const gx_expr_literal l = a.lits[t];
    uint64_t s[1];
    fetch_literal<1>(l.dtype, l.value, s);
    lit_p[t] = s[0];
    lit_v[t] = (l.valid == nullptr || *l.valid != 0) ? 1u : 0u;
  }
  unsigned long long tally = 0;
  const int seg        = (int)blockIdx.y;
  const int64_t seg_lo = seg * ps.seg_rows;
  const int64_t seg_hi = seg_lo + ps.seg_rows < ps.n_right ? seg_lo + ps.seg_rows : ps.n_right;
  const int64_t tiles = div_up(ps.n_left, (int64_t)tl);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = ps.left_row(tile, tl, t);
    const bool live = i < ps.n_left;
    // the left tile: a thread converts its own row and is the only reader of it
    uint32_t lv = 0;
    for (int c = 0; c < a.n_l; ++c) {
      const gx_expr_column col = a.lcols[c];
      uint64_t s[1];
      fetch_column<1>(col.dtype, col.data, i, live ? 1 : 0, s);
      l_p[c * tl + t] = s[0];
      if (live) lv |= valid_bit(col, i) << c;
    }
    int32_t cnt        = 0;
    const int32_t pos0 = (mode == CJ_WRITE && live) ? po.offsets[i * ps.n_seg + seg] : 0;
    int32_t pos        = pos0;
    bool matched       = false;
    for (int64_t c0 = seg_lo; c0 < seg_hi; c0 += tr) {
      const int rc = seg_hi - c0 < tr ? (int)(seg_hi - c0) : tr;
      // the previous chunk is consumed; MARK: a tile whose rows have all matched is done
      if (mode == CJ_MARK) {
        if (__syncthreads_and(matched || !live)) break;
      } else {
        __syncthreads();
      }
      for (int r = (int)t; r < tr; r += tl) {  // tr and tl are multiples of 64: whole waves take every trip
        const int64_t row = ps.right_row(c0, r);
        const bool ex     = r < rc;
        for (int c = 0; c < a.n_r; ++c) {
          const gx_expr_column col = a.rcols[c];
          uint64_t s[1];
          fetch_column<1>(col.dtype, col.data, row, ex ? 1 : 0, s);  // a row behind the table: a value that divides, null
          r_p[c * tr + r] = s[0];
          const unsigned long long b = __ballot(ex && valid_bit(col, row) != 0u);
          if (lane == 0) {
            r_v[c * rwords + (r >> 5)]     = (uint32_t)b;
            r_v[c * rwords + (r >> 5) + 1] = (uint32_t)(b >> 32);
          }
        }
      }
      if (full && (int)t < rwords) r_hit[t] = 0u;
      __syncthreads();
      if (live) {
#pragma unroll 1
        for (int r0 = 0; r0 < rc; r0 += R) {
          if (mode == CJ_MARK && __all(matched)) break;  // every live row of this wave has a match
          const int ex      = rc - r0 < R ? rc - r0 : R;
          const uint32_t lm = (1u << ex) - 1u;
          uint64_t acc[R];
          uint32_t ab = 0;
#pragma unroll
          for (int k = 0; k < R; ++k) acc[k] = 0;
#pragma unroll 1
          for (int ip = 0; ip < a.n_instr; ++ip) {
            const gx_expr_instr in = a.ins[ip];
            if (in.kind == GX_EXPR_SPILL) {
              slot_bits[in.src_index * tl + t] = ab;
#pragma unroll
              for (int k = 0; k < R; ++k) slot_payload[(in.src_index * R + k) * tl + t] = acc[k];
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
            if (in.src_kind == GX_EXPR_SRC_COLUMN) {  // LEFT: this thread's row in every pair
              const uint64_t v = l_p[in.src_index * tl + t];
#pragma unroll
              for (int k = 0; k < R; ++k) src[k] = v;
              sb = ((lv >> in.src_index) & 1u) ? lm : 0u;
            } else if (in.src_kind == CJ_SRC_RIGHT) {  // RIGHT: rows r0 .. r0 + R - 1, one address per wave
#pragma unroll
              for (int k = 0; k < R; ++k) src[k] = r_p[in.src_index * tr + r0 + k];
              sb = (r_v[in.src_index * rwords + (r0 >> 5)] >> (r0 & 31)) & lm;  // R divides 32
            } else if (in.src_kind == GX_EXPR_SRC_LITERAL) {
              const uint64_t v = lit_p[in.src_index];
#pragma unroll
              for (int k = 0; k < R; ++k) src[k] = v;
              sb = lit_v[in.src_index] ? lm : 0u;
            } else {
              sb = slot_bits[in.src_index * tl + t];
#pragma unroll
              for (int k = 0; k < R; ++k) src[k] = slot_payload[(in.src_index * R + k) * tl + t];
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
          // a pair matches when the BOOL8 result (0 / 1 in the low word) is valid and true
          uint32_t m = 0;
#pragma unroll
          for (int k = 0; k < R; ++k) m |= ((uint32_t)acc[k] != 0u ? 1u : 0u) << k;
          m &= ab & lm;
          if (mode == CJ_MARK) {
            matched = matched || m != 0u;
          } else if (mode == CJ_COUNT) {
            cnt += __builtin_popcount(m);
            if (full && __any(m != 0u)) {  // one LDS atomic per wave and matched right row at most
#pragma unroll
              for (int k = 0; k < R; ++k) {
                const unsigned long long b = __ballot((m >> k) & 1u);
                if (b != 0ull && lane == (unsigned)__builtin_ctzll(b)) atomicOr(&r_hit[(r0 + k) >> 5], 1u << ((r0 + k) & 31));
              }
            }
          } else {
#pragma unroll
            for (int k = 0; k < R; ++k) {
              if ((m >> k) & 1u) {
                po.out_l[pos] = (int32_t)i;
                po.out_r[pos] = (int32_t)ps.right_row(c0, r0 + k);
                ++pos;
              }
            }
          }
        }
      }
      if (full && mode == CJ_COUNT) {  // the chunk's matched right rows leave the bitmap of the unmatched ones
        __syncthreads();
        if ((int)t < rwords && r_hit[t] != 0u) atomicAnd(&po.right_unmatched[(c0 >> 5) + t], ~r_hit[t]);
      }
    }
    if (mode == CJ_COUNT) {
      if (live) {
        po.counts[i * ps.n_seg + seg] = cnt;
        tally += (unsigned long long)cnt;
      }
    } else if (mode == CJ_WRITE) {
      if (live && seg == 0 && (flags & CJ_LEFT_OUTER) && po.lone[i]) {  // no segment found a match: the one place of the row
        po.out_l[pos0] = (int32_t)i;
        po.out_r[pos0] = INT32_MIN;
      }
    } else {  // every lane of the wave is here: 64 rows, two whole words; one atomic per wave and word with a matched row
      const unsigned long long b = __ballot(live && matched);
      const int64_t row0         = i - lane;
      if (lane == 0 && b != 0ull) {
        const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
        if (flags & CJ_INVERT) {
          if (lo) atomicAnd(&po.left_bits[row0 >> 5], ~lo);
          if (hi) atomicAnd(&po.left_bits[(row0 >> 5) + 1], ~hi);
        } else {
          if (lo) atomicOr(&po.left_bits[row0 >> 5], lo);
          if (hi) atomicOr(&po.left_bits[(row0 >> 5) + 1], hi);
        }
      }
    }
    __syncthreads();  // the tile's LDS image is free
  }
  if (mode == CJ_COUNT) {
    const unsigned long long w = wave_reduce(tally, SumOp());
    if (lane == 0 && w != 0ull) atomicAdd(po.total, w);
  }
}

// FULL: the tail (INT32_MIN, r) of the unmatched right rows follows the pairs of the left-join part
__global__ void k_fill_i32(int32_t* __restrict__ out, int64_t n, int32_t v)
{
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) out[j] = v;
}
// LEFT / FULL: a left row without a match in any segment gets one place (in segment 0) and is remembered in lone[]
__global__ void k_outer_fix(int32_t* __restrict__ counts, int64_t n_left, int n_seg, uint8_t* __restrict__ lone, unsigned long long* __restrict__ total)
{
  unsigned long long added = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_left; i += (int64_t)gridDim.x * blockDim.x) {
    bool any = false;
    for (int s = 0; s < n_seg && !any; ++s) any = counts[i * n_seg + s] != 0;
    lone[i] = any ? 0 : 1;
    if (!any) {
      counts[i * n_seg] = 1;
      ++added;
    }
  }
  const unsigned long long w = wave_reduce(added, SumOp());
  if (lane_id() == 0 && w != 0ull) atomicAdd(total, w);
}
__global__ void k_full_sizes(int64_t* __restrict__ sizes, const int64_t* __restrict__ tail)
{
  sizes[1] = sizes[0];
  sizes[0] += *tail;
}
__global__ void k_copy_size(int64_t* __restrict__ sizes) { sizes[1] = sizes[0]; }
struct CountLoader {  // offsets wrap modulo 2^32 where the total does not fit: the write pass refuses such a total
  const uint32_t* c;
  __device__ __forceinline__ uint32_t operator()(int64_t i) const { return c[i]; }
};

// ---------------------------------------------------------------- host
static std::atomic<int> g_r{CJ_R}, g_tl{0}, g_tr{CJ_TR};

struct PairPlan {
  PairArgs a;
  bool heavy;
};

// 0, GX_EINVAL, GX_EDTYPE: the program of a BOOL8 predicate over the columns of two tables, its column sources staged per side
static int pair_plan(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits, int n_lits,
                     int64_t n_left, int64_t n_right, PairPlan* p)
{
  if (n_left < 0 || n_left > EX_MAX_ROWS || n_right < 0 || n_right > EX_MAX_ROWS) return GX_EINVAL;
  if (n_cols < 0 || n_cols > EX_MAX_COLS || n_lits < 0 || n_lits > EX_MAX_LITS) return GX_EINVAL;
  if ((n_cols > 0 && !cols) || (n_lits > 0 && !lits)) return GX_EINVAL;
  int32_t col_dtypes[EX_MAX_COLS], lit_dtypes[EX_MAX_LITS];
  for (int i = 0; i < n_cols; ++i) {
    col_dtypes[i] = cols[i].dtype;
    if (cols[i].begin_bit < 0 || cols[i].table < 0 || cols[i].table > 1) return GX_EINVAL;
  }
  for (int i = 0; i < n_lits; ++i) lit_dtypes[i] = lits[i].dtype;
  PairArgs& a = p->a;
  int dtype   = 0;
  if (int rc = plan(nodes, n_nodes, col_dtypes, n_cols, lit_dtypes, n_lits, a.ins, &a.n_instr, &a.n_slots, &dtype); rc != 0) return rc;
  if (dtype != GX_BOOL8) return GX_EDTYPE;
  int staged[EX_MAX_COLS];
  for (int i = 0; i < n_cols; ++i) staged[i] = -1;
  a.n_l = a.n_r = 0;
  for (int ip = 0; ip < a.n_instr; ++ip) {
    gx_expr_instr& in = a.ins[ip];
    if (in.kind == GX_EXPR_SPILL || in.kind == GX_EXPR_APPLY_UNARY) continue;
    if (in.src_kind == GX_EXPR_SRC_COLUMN) {
      const gx_expr_column& c = cols[in.src_index];
      const int64_t rows      = c.table ? n_right : n_left;
      if (rows > 0 && !c.data) return GX_EINVAL;  // only what the program reads needs a pointer
      if (staged[in.src_index] < 0) {
        staged[in.src_index] = c.table ? a.n_r : a.n_l;
        if (c.table) a.rcols[a.n_r++] = c; else a.lcols[a.n_l++] = c;
      }
      in.src_kind  = c.table ? CJ_SRC_RIGHT : GX_EXPR_SRC_COLUMN;
      in.src_index = (uint8_t)staged[in.src_index];
    } else if (in.src_kind == GX_EXPR_SRC_LITERAL) {
      if (!lits[in.src_index].value) return GX_EINVAL;
    }
  }
  for (int i = 0; i < n_lits; ++i) a.lits[i] = lits[i];
  a.n_lits = n_lits;
  p->heavy = program_is_heavy(a.ins, a.n_instr);
  return 0;
}

// The shape of a launch, host arithmetic on the row counts alone.  A workgroup walks one left tile against one segment of the right
// table, so that a join of two short tables still fills the device (2^14 x 2^14 rows are 64 tiles of 256 rows: measured at 64 G
// pairs/s with one segment, 676 G with 64, both at R = 4): the widest left tile that still gives CJ_MIN_WGS workgroups, and as many
// segments (whole chunks) as bring the grid to CJ_FILL_WGS.
constexpr int64_t CJ_MIN_WGS = 512, CJ_FILL_WGS = 4096;
struct PairShape {
  int tl, tr, n_seg;
  int64_t seg_rows;
};
static PairShape pair_shape(int64_t n_left, int64_t n_right)
{
  PairShape sh;
  sh.tr                = g_tr.load(std::memory_order_relaxed);
  const int64_t chunks = n_right > 0 ? div_up(n_right, (int64_t)sh.tr) : 1;
  sh.tl                = g_tl.load(std::memory_order_relaxed);
  if (sh.tl == 0) {
    sh.tl = CJ_TL;
    while (sh.tl > GX_WAVE && div_up(n_left, (int64_t)sh.tl) * chunks < CJ_MIN_WGS) sh.tl /= 2;
  }
  const int64_t tiles = n_left > 0 ? div_up(n_left, (int64_t)sh.tl) : 1;
  int64_t want        = div_up(CJ_FILL_WGS, tiles);
  if (want > chunks) want = chunks;
  const int64_t per = div_up(chunks, want);  // chunks of a segment
  sh.seg_rows       = per * sh.tr;
  sh.n_seg          = (int)div_up(chunks, per);
  return sh;
}
// at least n_left * n_seg whatever the knobs say, and monotone in both row counts: n_seg <= CJ_FILL_WGS / tiles + 1 with
// tiles >= n_left / CJ_TL, and n_seg <= the chunks of the narrowest chunk
static size_t count_cells_bound(int64_t n_left, int64_t n_right)
{
  const int64_t by_fill = n_left + CJ_FILL_WGS * CJ_TL, by_chunks = n_left * (n_right > 0 ? div_up(n_right, (int64_t)GX_WAVE) : 1);
  return (size_t)(by_fill < by_chunks ? by_fill : by_chunks);
}

template <int R, bool HEAVY>
static int pairs_launch_as(const PairPlan& p, int64_t n_left, int64_t n_right, int mode, int flags, const PairOut& po, hipStream_t s)
{
  Device dev;
  GX_HIP_TRY(device(&dev));
  const PairShape sh = pair_shape(n_left, n_right);
  const dim3 grid(capped_grid(n_left, sh.tl, CJ_GRID_CAP), (unsigned)sh.n_seg), block(sh.tl);
  const size_t lds = (size_t)pair_lds(sh.tl, sh.tr, p.a.n_l, p.a.n_r, p.a.n_slots, R).total;
  GX_HIP_TRY(launch_lds(dev, k_pairs<R, HEAVY>, grid, block, lds, s, p.a, PairSource{n_left, n_right, sh.seg_rows, sh.n_seg}, mode, flags, sh.tr, po));
  GX_LAUNCH_CHECK();
  return 0;
}
template <typename... A>
static int pairs_launch(const PairPlan& p, A... args)
{
  switch (g_r.load(std::memory_order_relaxed)) {
    case 2: return p.heavy ? pairs_launch_as<2, true>(p, args...) : pairs_launch_as<2, false>(p, args...);
    case 8: return p.heavy ? pairs_launch_as<8, true>(p, args...) : pairs_launch_as<8, false>(p, args...);
    default: return p.heavy ? pairs_launch_as<4, true>(p, args...) : pairs_launch_as<4, false>(p, args...);
  }
}

// the scratch of one join: what the count pass leaves for the write pass
struct PairScratch {
  int32_t* offsets;    // INNER / LEFT / FULL: the counts per (left row, segment), scanned in place
  uint32_t* partials;
  uint8_t* lone;       // LEFT / FULL: the left rows without a match
  uint32_t* bits;      // FULL: the unmatched right rows; SEMI / ANTI: the selected left rows
  void* select;        // the selection plan over `bits`
  int64_t* tail;       // FULL: the number of unmatched right rows
  size_t select_bytes;
  Carver c;
  PairScratch(void* tmp, int kind, int64_t n_left, int64_t n_right) : c(tmp)
  {
    const bool pairs   = kind <= GX_CJ_FULL;
    const int64_t nsel = kind == GX_CJ_FULL ? n_right : (pairs ? 0 : n_left);
    const size_t cells = pairs ? count_cells_bound(n_left, n_right) : 0;
    offsets            = c.take<int32_t>(cells);
    partials           = c.take<uint32_t>(pairs ? scan::partials_count((int64_t)cells) : 0);
    lone               = c.take<uint8_t>(pairs ? (size_t)n_left : 0);
    bits               = c.take<uint32_t>((size_t)div_up(nsel, 32) + 2);
    select_bytes       = gx_compact_plan_bytes(nsel);
    select             = c.take<char>(select_bytes);
    tail               = c.take<int64_t>(1);
  }
};

static bool kind_ok(int kind) { return kind >= GX_CJ_INNER && kind <= GX_CJ_ANTI; }

}  // namespace gx

extern "C" {

void gx_conditional_join_tile(int* left_rows, int* right_rows)
{
  if (left_rows) *left_rows = gx::CJ_TL;
  if (right_rows) *right_rows = gx::g_tr.load(std::memory_order_relaxed);
}
int gx_conditional_join_grid_cap(void) { return gx::CJ_GRID_CAP; }
int gx_conditional_join_pairs_per_run(void) { return gx::g_r.load(std::memory_order_relaxed); }

int gx_conditional_join_set_shape(int pairs_per_run, int left_rows, int right_rows)
{
  const int r = pairs_per_run == 0 ? gx::CJ_R : pairs_per_run, tr = right_rows == 0 ? gx::CJ_TR : right_rows;
  if ((r != 2 && r != 4 && r != 8) || (left_rows != 0 && left_rows != 64 && left_rows != 128 && left_rows != 256) || (tr != 64 && tr != 128 && tr != 256))
    return GX_EINVAL;
  gx::g_r.store(r, std::memory_order_relaxed);
  gx::g_tl.store(left_rows, std::memory_order_relaxed);
  gx::g_tr.store(tr, std::memory_order_relaxed);
  return 0;
}

int gx_conditional_join_count(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits,
                              int n_lits, int64_t n_left, int64_t n_right, int kind, int64_t* sizes_dev, void* tmp, size_t* tmp_bytes,
                              gx_stream_t stream)
{
  if (!gx::kind_ok(kind) || !tmp_bytes) return GX_EINVAL;
  gx::PairPlan p;
  if (int rc = gx::pair_plan(nodes, n_nodes, cols, n_cols, lits, n_lits, n_left, n_right, &p); rc != 0) return rc;
  gx::PairScratch sc(tmp, kind, n_left, n_right);
  if (int rc; !sc.c.ready(tmp_bytes, &rc)) return rc;
  if (!sizes_dev) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  GX_HIP_TRY(hipMemsetAsync(sizes_dev, 0, 2 * sizeof(int64_t), s));
  if (kind <= GX_CJ_FULL) {
    const int flags = kind == GX_CJ_INNER ? 0 : (kind == GX_CJ_LEFT ? gx::CJ_LEFT_OUTER : gx::CJ_LEFT_OUTER | gx::CJ_FULL);
    if (kind == GX_CJ_FULL) GX_HIP_TRY(hipMemsetAsync(sc.bits, 0xFF, ((size_t)gx::div_up(n_right, 32) + 2) * sizeof(uint32_t), s));
    if (n_left > 0) {
      const int64_t cells = n_left * gx::pair_shape(n_left, n_right).n_seg;
      gx::PairOut po{};
      po.counts          = sc.offsets;
      po.total           = reinterpret_cast<unsigned long long*>(sizes_dev);
      po.right_unmatched = sc.bits;
      if (int rc = gx::pairs_launch(p, n_left, n_right, (int)gx::CJ_COUNT, flags, po, s); rc != 0) return rc;
      if (kind != GX_CJ_INNER)
        hipLaunchKernelGGL(gx::k_outer_fix, dim3(gx::capped_grid(n_left, 256, 1024)), dim3(256), 0, s, sc.offsets, n_left,
                           gx::pair_shape(n_left, n_right).n_seg, sc.lone, po.total);
      if (int rc = gx::scan::device_scan<uint32_t, uint32_t>(gx::CountLoader{reinterpret_cast<const uint32_t*>(sc.offsets)}, cells, 0u, gx::SumOp(), false,
                                                            reinterpret_cast<uint32_t*>(sc.offsets), sc.partials, s);
          rc != 0)
        return rc;
    }
    if (kind == GX_CJ_FULL) {
      const uint32_t* vp = sc.bits;
      size_t bytes       = sc.select_bytes;
      if (int rc = gx_select_valid_count(1, &vp, nullptr, n_right, 1, sc.tail, sc.select, &bytes, stream); rc != 0) return rc;
      hipLaunchKernelGGL(gx::k_full_sizes, dim3(1), dim3(1), 0, s, sizes_dev, sc.tail);
    } else {
      hipLaunchKernelGGL(gx::k_copy_size, dim3(1), dim3(1), 0, s, sizes_dev);
    }
    GX_LAUNCH_CHECK();
    return 0;
  }
  GX_HIP_TRY(hipMemsetAsync(sc.bits, kind == GX_CJ_ANTI ? 0xFF : 0, ((size_t)gx::div_up(n_left, 32) + 2) * sizeof(uint32_t), s));
  if (n_left > 0) {
    gx::PairOut po{};
    po.left_bits = sc.bits;
    if (int rc = gx::pairs_launch(p, n_left, n_right, (int)gx::CJ_MARK, kind == GX_CJ_ANTI ? (int)gx::CJ_INVERT : 0, po, s); rc != 0) return rc;
  }
  const uint32_t* vp = sc.bits;
  size_t bytes       = sc.select_bytes;
  if (int rc = gx_select_valid_count(1, &vp, nullptr, n_left, 1, sizes_dev, sc.select, &bytes, stream); rc != 0) return rc;
  hipLaunchKernelGGL(gx::k_copy_size, dim3(1), dim3(1), 0, s, sizes_dev);
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_conditional_join_write(const gx_expr_node* nodes, int n_nodes, const gx_expr_column* cols, int n_cols, const gx_expr_literal* lits,
                              int n_lits, int64_t n_left, int64_t n_right, int kind, int64_t total, int64_t left_total, const void* tmp,
                              int32_t* out_left, int32_t* out_right, gx_stream_t stream)
{
  if (!gx::kind_ok(kind)) return GX_EINVAL;
  gx::PairPlan p;
  if (int rc = gx::pair_plan(nodes, n_nodes, cols, n_cols, lits, n_lits, n_left, n_right, &p); rc != 0) return rc;
  if (total < 0 || left_total < 0 || left_total > total) return GX_EINVAL;
  if (total > gx::EX_MAX_ROWS) return GX_EOVERFLOW;
  if (total == 0) return 0;
  if (!tmp || !out_left || (kind <= GX_CJ_FULL && !out_right)) return GX_EINVAL;
  gx::PairScratch sc(const_cast<void*>(tmp), kind, n_left, n_right);
  hipStream_t s = (hipStream_t)stream;
  if (kind > GX_CJ_FULL) return gx_compact_indices(n_left, sc.select, out_left, stream);
  if (left_total > 0) {
    const int flags = kind == GX_CJ_INNER ? 0 : gx::CJ_LEFT_OUTER;
    gx::PairOut po{};
    po.offsets = sc.offsets;
    po.lone    = sc.lone;
    po.out_l   = out_left;
    po.out_r   = out_right;
    if (int rc = gx::pairs_launch(p, n_left, n_right, (int)gx::CJ_WRITE, flags, po, s); rc != 0) return rc;
  }
  if (kind == GX_CJ_FULL && total > left_total) {
    const int64_t tail = total - left_total;
    hipLaunchKernelGGL(gx::k_fill_i32, dim3(gx::capped_grid(tail, 1024, 1024)), dim3(256), 0, s, out_left + left_total, tail, (int32_t)INT32_MIN);
    GX_LAUNCH_CHECK();
    return gx_compact_indices(n_right, sc.select, out_right + left_total, stream);
  }
  return 0;
}

}  // extern "C"
