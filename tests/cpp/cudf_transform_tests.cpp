// cudf::compute_column through the C++ surface (include/cudf/transform.hpp, include/cudf/ast/expressions.hpp).  Small literal
// vectors, expected values written out by hand; operands are sliced views made by cudf::slice where a case says so.  The minimal
// harness of cudf_binaryop_tests.cpp.
//   cudf_transform_tests --host   what is decided before the first device call: the throws, the empty results, ast::tree;
//                                 runs without a GPU (tests/test_expression_host.py)
//   cudf_transform_tests          the whole list; needs a GPU (tests/test_gpu_expression.py)
#include <cudf/ast/expressions.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/transform.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

using namespace cudf;
static int g_failed = 0, g_run = 0;
#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      std::printf("    CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      throw std::runtime_error("check failed");                                       \
    }                                                                                 \
  } while (0)

template <typename T>
std::unique_ptr<column> make_col(std::vector<T> const& v, std::vector<int> const& valid = {}, type_id id = type_to_id<T>())
{
  auto const n = static_cast<size_type>(v.size());
  rmm::device_buffer data{v.data(), v.size() * sizeof(T), get_default_stream()};
  rmm::device_buffer mask{};
  size_type nulls = 0;
  if (!valid.empty()) {
    std::vector<bitmask_type> w(bitmask_allocation_size_bytes(n) / 4, 0u);
    for (size_type i = 0; i < n; ++i) {
      if (valid[i]) w[i / 32] |= 1u << (i % 32); else ++nulls;
    }
    mask = rmm::device_buffer{w.data(), w.size() * 4, get_default_stream()};
  }
  get_default_stream().synchronize();
  return std::make_unique<column>(data_type{id}, n, std::move(data), std::move(mask), nulls);
}
template <typename T>
std::vector<T> to_host(column_view const& c)
{
  std::vector<T> h(c.size());
  if (c.size()) (void)hipMemcpy(h.data(), c.data<T>(), h.size() * sizeof(T), hipMemcpyDeviceToHost);
  return h;
}
std::vector<int> valid_host(column_view const& c)
{
  std::vector<int> v(c.size(), 1);
  if (!c.null_mask()) return v;
  std::vector<bitmask_type> w(num_bitmask_words(c.size() + c.offset()));
  if (!w.empty()) (void)hipMemcpy(w.data(), c.null_mask(), w.size() * 4, hipMemcpyDeviceToHost);
  for (size_type i = 0; i < c.size(); ++i) v[i] = (w[(i + c.offset()) / 32] >> ((i + c.offset()) % 32)) & 1;
  return v;
}
template <typename Exc, typename F>
bool throws(F&& f)
{
  try {
    f();
  } catch (Exc const&) {
    return true;
  } catch (...) {
    return false;
  }
  return false;
}
void run(char const* name, std::function<void()> f)
{
  ++g_run;
  try {
    f();
    std::printf("[ OK ] %s\n", name);
  } catch (std::exception const& e) {
    ++g_failed;
    std::printf("[FAIL] %s: %s\n", name, e.what());
  }
}

using I8  = std::vector<int8_t>;
using U8  = std::vector<uint8_t>;
using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
using OP  = ast::ast_operator;
static data_type dt(type_id id) { return data_type{id}; }

// a * b + c over columns 0, 1, 2, built inside a function: the tree owns the nodes the root refers to
static ast::tree make_fma_tree()
{
  ast::tree t;
  auto const& a   = t.push(ast::column_reference{0});
  auto const& b   = t.push(ast::column_reference{1});
  auto const& c   = t.emplace<ast::column_reference>(2);
  auto const& mul = t.emplace<ast::operation>(OP::MUL, a, b);
  t.emplace<ast::operation>(OP::ADD, mul, c);
  return t;
}

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view b5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view f5{dt(type_id::FLOAT64), 5, fake, nullptr, 0};
  column_view e32{dt(type_id::INT32), 0, nullptr, nullptr, 0};
  column_view e8{dt(type_id::INT8), 0, nullptr, nullptr, 0};
  table_view const t5{std::vector<column_view>{a5, b5, f5}};
  table_view const t0{std::vector<column_view>{e32, e32, e8}};
  ast::column_reference c0{0}, c1{1}, c2{2};
  run("compute_column: operands of different types throw cudf::data_type_error", [&] {
    ast::operation add{OP::ADD, c0, c2};
    CHECK(throws<data_type_error>([&] { (void)compute_column(t5, add); }));
    ast::operation cast{OP::CAST_TO_FLOAT64, c0};
    ast::operation ok{OP::ADD, cast, c2};
    CHECK(throws<data_type_error>([&] { (void)compute_column(t5, ast::operation{OP::LESS, ok, c0}); }));
  });
  run("compute_column: operators that do not take the type, or are not built, throw cudf::data_type_error", [&] {
    for (auto op : {OP::SIN, OP::COS, OP::TAN, OP::ARCSIN, OP::ARCCOS, OP::ARCTAN, OP::SINH, OP::COSH, OP::TANH, OP::ARCSINH, OP::ARCCOSH,
                    OP::ARCTANH, OP::EXP, OP::LOG, OP::CBRT}) {
      ast::operation e{op, c2};
      CHECK(throws<data_type_error>([&] { (void)compute_column(t5, e); }));
    }
    ast::operation bits{OP::BITWISE_AND, c2, c2};
    CHECK(throws<data_type_error>([&] { (void)compute_column(t5, bits); }));
    ast::operation root{OP::SQRT, c0};
    CHECK(throws<data_type_error>([&] { (void)compute_column(t5, root); }));
  });
  run("compute_column: a column index outside the table throws std::out_of_range", [&] {
    ast::column_reference c3{3}, neg{-1};
    ast::operation e{OP::ADD, c0, c3};
    CHECK(throws<std::out_of_range>([&] { (void)compute_column(t5, e); }));
    CHECK(throws<std::out_of_range>([&] { (void)compute_column(t5, neg); }));
  });
  run("compute_column: table_reference::RIGHT throws std::invalid_argument", [&] {
    ast::column_reference r{0, ast::table_reference::RIGHT};
    CHECK(throws<std::invalid_argument>([&] { (void)compute_column(t5, r); }));
  });
  run("compute_column: an expression beyond the limits throws std::invalid_argument", [&] {
    ast::tree t;
    ast::expression const* top = &t.push(ast::column_reference{0});
    for (int i = 0; i < 40; ++i) top = &t.emplace<ast::operation>(OP::IDENTITY, *top);
    CHECK(throws<std::invalid_argument>([&] { (void)compute_column(t5, *top); }));
    // five levels of (x + x) over a non-leaf need five spill slots
    ast::tree s;
    ast::expression const* lvl = &s.emplace<ast::operation>(OP::ABS, s.push(ast::column_reference{0}));
    for (int i = 0; i < 5; ++i) lvl = &s.emplace<ast::operation>(OP::ADD, *lvl, *lvl);
    CHECK(throws<std::invalid_argument>([&] { (void)compute_column(t5, *lvl); }));
  });
  run("ast::operation: the operator's arity is checked at construction", [&] {
    CHECK(throws<std::invalid_argument>([&] { ast::operation e{OP::ADD, c0}; }));
    CHECK(throws<std::invalid_argument>([&] { ast::operation e{OP::ABS, c0, c1}; }));
  });
  run("compute_column: no rows give an empty column of the result type, without a mask", [&] {
    auto r = compute_column(t0, ast::operation{OP::LESS, c0, c1});
    CHECK(r->size() == 0 && r->type().id() == type_id::BOOL8 && !r->nullable());
    ast::operation abs8{OP::ABS, c2};
    CHECK(compute_column(t0, abs8)->type().id() == type_id::INT32);
    ast::operation div{OP::FLOOR_DIV, c0, c1};
    CHECK(compute_column(t0, div)->type().id() == type_id::FLOAT64);
    CHECK(compute_column(t0, c2)->type().id() == type_id::INT8);
  });
  run("ast::tree: owns its nodes, keeps their addresses, and the enumerators have the reference's values", [&] {
    auto t = make_fma_tree();
    CHECK(t.size() == 5 && t.back().kind() == ast::expression_kind::OPERATION && t.front().kind() == ast::expression_kind::COLUMN_REFERENCE);
    auto const* root = &t.back();
    ast::tree moved  = std::move(t);
    CHECK(&moved.back() == root && &moved[4] == root && &moved.at(4) == root);
    auto const& op = static_cast<ast::operation const&>(moved.back());
    CHECK(op.get_operator() == OP::ADD && &op.lhs() == &moved[3] && &op.rhs() == &moved[2]);
    static_assert(static_cast<int>(OP::ADD) == 0 && static_cast<int>(OP::NULL_LOGICAL_OR) == 22 && static_cast<int>(OP::IDENTITY) == 23 &&
                  static_cast<int>(OP::CAST_TO_FLOAT64) == 49);
    // int32 * int32 + int32 over an empty table: typed through the moved tree
    table_view const e3{std::vector<column_view>{e32, e32, e32}};
    CHECK(compute_column(e3, moved.back())->type().id() == type_id::INT32);
  });
}

static void device_cases()
{
  run("a * b + c on FLOAT64: two roundings, no mask", [&] {
    auto a = make_col<double>({1.5, -2.0, 0.1, 3.0, 1e300}), b = make_col<double>({2.0, 4.0, 0.2, -1.0, 1e10}), c = make_col<double>({0.25, 1.0, 0.3, 0.5, 1.0});
    auto const t = make_fma_tree();
    auto r       = compute_column(table_view{std::vector<column_view>{*a, *b, *c}}, t.back());
    CHECK(r->type().id() == type_id::FLOAT64 && !r->nullable() && r->null_count() == 0);
    double const p = 0.1 * 0.2;
    CHECK((to_host<double>(*r) == F64{3.25, -7.0, p + 0.3, -2.5, std::numeric_limits<double>::infinity()}));
  });
  run("(a > b) & (c < 5) into BOOL8 with a literal and nulls", [&] {
    auto a = make_col<double>({1, 5, 3, 7, 2, 9}, {1, 1, 0, 1, 1, 1}), b = make_col<double>({0, 6, 1, 2, 2, 1});
    auto c = make_col<int64_t>({1, 2, 3, 9, 4, 4}, {1, 1, 1, 1, 1, 0});
    numeric_scalar<int64_t> five{5};
    ast::column_reference ra{0}, rb{1}, rc{2};
    ast::literal lit{five};
    ast::operation gt{OP::GREATER, ra, rb}, lt{OP::LESS, rc, lit}, both{OP::LOGICAL_AND, gt, lt};
    auto r = compute_column(table_view{std::vector<column_view>{*a, *b, *c}}, both);
    CHECK(r->type().id() == type_id::BOOL8 && r->null_count() == 2);
    auto const v = to_host<uint8_t>(*r);
    auto const k = valid_host(*r);
    CHECK((k == V{1, 1, 0, 1, 1, 0}) && v[0] == 1 && v[1] == 0 && v[3] == 0 && v[4] == 0);
  });
  run("sliced views from cudf::slice: values and bitmaps are read from the views' offsets", [&] {
    std::vector<int32_t> av(100), bv(100);
    V ak(100), bk(100);
    for (int i = 0; i < 100; ++i) {
      av[i] = i * 3 - 50;
      bv[i] = 7 - i;
      ak[i] = i % 3 != 0;
      bk[i] = i % 5 != 1;
    }
    auto a = make_col<int32_t>(av, ak), b = make_col<int32_t>(bv, bk);
    auto const sa = slice(*a, {33, 98})[0], sb = slice(*b, {1, 66})[0];
    ast::column_reference ra{0}, rb{1};
    ast::operation sub{OP::SUB, ra, rb};
    auto r       = compute_column(table_view{std::vector<column_view>{sa, sb}}, sub);
    auto const v = to_host<int32_t>(*r);
    auto const k = valid_host(*r);
    size_type nulls = 0;
    for (int i = 0; i < 65; ++i) {
      bool const ok = ak[33 + i] && bk[1 + i];
      CHECK(k[i] == ok);
      if (ok) CHECK(v[i] == av[33 + i] - bv[1 + i]); else ++nulls;
    }
    CHECK(r->size() == 65 && r->null_count() == nulls && nulls > 0);
  });
  run("nullable inputs without a null row give a result without a mask", [&] {
    auto a = make_col<int64_t>({1, 2, 3}, {1, 1, 1}), b = make_col<int64_t>({4, 5, 6});
    ast::column_reference ra{0}, rb{1};
    ast::operation mul{OP::MUL, ra, rb};
    auto r = compute_column(table_view{std::vector<column_view>{*a, *b}}, mul);
    CHECK(!r->nullable() && r->null_count() == 0 && (to_host<int64_t>(*r) == I64{4, 10, 18}));
  });
  run("an invalid literal makes every row null; IS_NULL of it is true everywhere", [&] {
    auto a = make_col<int32_t>({1, 2, 3, 4});
    numeric_scalar<int32_t> none{7, false};
    ast::column_reference ra{0};
    ast::literal lit{none};
    ast::operation add{OP::ADD, ra, lit}, isn{OP::IS_NULL, add};
    table_view const t{std::vector<column_view>{*a}};
    auto r = compute_column(t, add);
    CHECK(r->null_count() == 4 && r->nullable());
    auto q = compute_column(t, isn);
    CHECK(q->null_count() == 0 && (to_host<uint8_t>(*q) == U8{1, 1, 1, 1}));
  });
  run("IS_NULL(a + b) and NULL_EQUAL(a + b, c): null intermediates, valid results", [&] {
    auto a = make_col<int32_t>({1, 2, 3, 4}, {1, 0, 1, 1}), b = make_col<int32_t>({1, 1, 1, 1}, {1, 1, 0, 1}), c = make_col<int32_t>({2, 0, 0, 9}, {1, 0, 1, 1});
    ast::column_reference ra{0}, rb{1}, rc{2};
    ast::operation add{OP::ADD, ra, rb}, isn{OP::IS_NULL, add}, neq{OP::NULL_EQUAL, add, rc};
    table_view const t{std::vector<column_view>{*a, *b, *c}};
    auto r = compute_column(t, isn);
    CHECK(r->null_count() == 0 && (to_host<uint8_t>(*r) == U8{0, 1, 1, 0}));
    auto q = compute_column(t, neq);
    CHECK(q->null_count() == 0 && (to_host<uint8_t>(*q) == U8{1, 1, 0, 0}));
  });
  run("NULL_LOGICAL_OR / AND: a null intermediate becomes a valid result where the other side decides", [&] {
    auto a = make_col<int32_t>({5, 5, 5, 5}, {1, 0, 0, 1}), b = make_col<int32_t>({1, 1, 1, 9});
    auto c = make_col<uint8_t>({1, 1, 0, 0}, {}, type_id::BOOL8);
    ast::column_reference ra{0}, rb{1}, rc{2};
    ast::operation gt{OP::GREATER, ra, rb}, lor{OP::NULL_LOGICAL_OR, gt, rc}, land{OP::NULL_LOGICAL_AND, gt, rc};
    table_view const t{std::vector<column_view>{*a, *b, *c}};
    auto r = compute_column(t, lor);
    CHECK((valid_host(*r) == V{1, 1, 0, 1}) && r->null_count() == 1);
    auto const v = to_host<uint8_t>(*r);
    CHECK(v[0] == 1 && v[1] == 1 && v[3] == 0);
    auto q = compute_column(t, land);
    CHECK((valid_host(*q) == V{1, 0, 1, 1}) && q->null_count() == 1);
    auto const w = to_host<uint8_t>(*q);
    CHECK(w[0] == 1 && w[2] == 0 && w[3] == 0);
  });
  run("ABS and BIT_INVERT compute in the class: INT8 -128 -> 128, ~UINT8 is the int of C++", [&] {
    auto a = make_col<int8_t>({-128, -1, 0, 127}), u = make_col<uint8_t>({0, 1, 255, 128});
    ast::column_reference ra{0}, ru{1};
    ast::operation abs{OP::ABS, ra}, inv{OP::BIT_INVERT, ru};
    table_view const t{std::vector<column_view>{*a, *u}};
    auto r = compute_column(t, abs);
    CHECK(r->type().id() == type_id::INT32 && (to_host<int32_t>(*r) == I32{128, 1, 0, 127}));
    auto q = compute_column(t, inv);
    CHECK(q->type().id() == type_id::INT32 && (to_host<int32_t>(*q) == I32{~0, ~1, ~255, ~128}));
  });
  run("FLOOR_DIV is floor(double / double) into FLOAT64, TRUE_DIV the quotient", [&] {
    auto a = make_col<int32_t>({7, -7, 7, -7, 1}), b = make_col<int32_t>({2, 2, -2, -2, 3});
    ast::column_reference ra{0}, rb{1};
    ast::operation fd{OP::FLOOR_DIV, ra, rb}, td{OP::TRUE_DIV, ra, rb};
    table_view const t{std::vector<column_view>{*a, *b}};
    auto r = compute_column(t, fd);
    CHECK(r->type().id() == type_id::FLOAT64 && (to_host<double>(*r) == F64{3, -4, -4, 3, 0}));
    CHECK((to_host<double>(*compute_column(t, td)) == F64{3.5, -3.5, -3.5, 3.5, 1.0 / 3.0}));
  });
  run("(a + b) * (c + d): one spill, a null in the spilled side comes back", [&] {
    auto a = make_col<int64_t>({1, 2, 3}, {1, 0, 1}), b = make_col<int64_t>({10, 20, 30}), c = make_col<int64_t>({2, 2, 2}), d = make_col<int64_t>({1, 1, -2});
    ast::column_reference ra{0}, rb{1}, rc{2}, rd{3};
    ast::operation ab{OP::ADD, ra, rb}, cd{OP::ADD, rc, rd}, mul{OP::MUL, ab, cd};
    auto r = compute_column(table_view{std::vector<column_view>{*a, *b, *c, *d}}, mul);
    auto const v = to_host<int64_t>(*r);
    CHECK((valid_host(*r) == V{1, 0, 1}) && v[0] == 33 && v[2] == 0 && r->null_count() == 1);
  });
  run("one node under two parents, and the same column under both operands", [&] {
    auto a = make_col<double>({1.5, -2, 3}), b = make_col<double>({2, 2, 2});
    ast::column_reference ra{0}, rb{1};
    ast::operation s{OP::SUB, ra, rb}, sq{OP::MUL, s, s}, aa{OP::MUL, ra, ra}, sum{OP::ADD, sq, aa};
    auto r = compute_column(table_view{std::vector<column_view>{*a, *b}}, sum);
    CHECK((to_host<double>(*r) == F64{0.25 + 2.25, 16 + 4, 1 + 9}));
  });
  run("a right-deep chain: the accumulator on the right of SUB and DIV", [&] {
    auto a = make_col<double>({100, 50}), b = make_col<double>({8, 4}), c = make_col<double>({2, 1});
    ast::column_reference ra{0}, rb{1}, rc{2};
    ast::operation bc{OP::DIV, rb, rc}, abc{OP::SUB, ra, bc};
    numeric_scalar<double> one{1.0};
    ast::literal lit{one};
    ast::operation root{OP::SUB, lit, abc};
    auto r = compute_column(table_view{std::vector<column_view>{*a, *b, *c}}, root);
    CHECK((to_host<double>(*r) == F64{1 - (100 - 4), 1 - (50 - 4)}));
  });
  run("bare roots: a column reference over a sliced nullable view copies, a literal fills", [&] {
    std::vector<int16_t> av(70);
    V ak(70);
    for (int i = 0; i < 70; ++i) {
      av[i] = static_cast<int16_t>(i * 5 - 9);
      ak[i] = i % 4 != 2;
    }
    auto a        = make_col<int16_t>(av, ak);
    auto const sa = slice(*a, {3, 70})[0];
    ast::column_reference ra{0};
    table_view const t{std::vector<column_view>{sa}};
    auto r       = compute_column(t, ra);
    auto const v = to_host<int16_t>(*r);
    auto const k = valid_host(*r);
    for (int i = 0; i < 67; ++i) CHECK(k[i] == ak[3 + i] && (!k[i] || v[i] == av[3 + i]));
    CHECK(r->type().id() == type_id::INT16 && r->size() == 67);
    numeric_scalar<float> pi{3.25f};
    ast::literal lit{pi};
    auto q = compute_column(t, lit);
    CHECK(q->type().id() == type_id::FLOAT32 && q->size() == 67 && !q->nullable());
    for (auto x : to_host<float>(*q)) CHECK(x == 3.25f);
  });
  run("mixed widths: INT8 columns cast to INT64 beside an INT64 literal, BOOL8 out of 8-byte inputs", [&] {
    auto a = make_col<int8_t>({-128, 5, 127}), b = make_col<int8_t>({1, 1, 1});
    numeric_scalar<int64_t> big{int64_t{1} << 40};
    ast::column_reference ra{0}, rb{1};
    ast::literal lit{big};
    ast::operation ca{OP::CAST_TO_INT64, ra}, cb{OP::CAST_TO_INT64, rb}, sum{OP::ADD, ca, cb}, mul{OP::MUL, sum, lit}, neg{OP::LESS, mul, lit};
    table_view const t{std::vector<column_view>{*a, *b}};
    CHECK((to_host<int64_t>(*compute_column(t, mul)) == I64{-127 * (int64_t{1} << 40), 6 * (int64_t{1} << 40), 128 * (int64_t{1} << 40)}));
    CHECK((to_host<uint8_t>(*compute_column(t, neg)) == U8{1, 0, 0}));
  });
  run("ast::tree built in a function outlives it: 5000 rows through the owning tree", [&] {
    std::vector<int32_t> av(5000), bv(5000), cv(5000);
    for (int i = 0; i < 5000; ++i) {
      av[i] = i - 2500;
      bv[i] = 3 * i + 1;
      cv[i] = 7 - i;
    }
    auto a = make_col<int32_t>(av), b = make_col<int32_t>(bv), c = make_col<int32_t>(cv);
    auto const t = make_fma_tree();
    auto r       = compute_column(table_view{std::vector<column_view>{*a, *b, *c}}, t.back());
    auto const v = to_host<int32_t>(*r);
    for (int i = 0; i < 5000; ++i) CHECK(v[i] == av[i] * bv[i] + cv[i]);
  });
}

int main(int argc, char** argv)
{
  bool const host_only = argc > 1 && std::strcmp(argv[1], "--host") == 0;
  host_cases();
  if (!host_only) device_cases();
  std::printf("%d run, %d failed\n", g_run, g_failed);
  return g_failed ? 1 : 0;
}
