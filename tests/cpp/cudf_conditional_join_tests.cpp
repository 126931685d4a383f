// cudf::conditional_*_join through the C++ surface (include/cudf/join/conditional_join.hpp).  The literal vectors of the reference's
// cpp/tests/join/conditional_join_tests.cu that fit fixed-width types, expected pairs written out by hand in the order this library
// fixes (ascending (left, right); unmatched left rows in place; unmatched right rows last).  The minimal harness of
// cudf_transform_tests.cpp.
//   cudf_conditional_join_tests --host   what is decided before the first device call: every throw of the lowering;
//                                        runs without a GPU (tests/test_conditional_join_host.py)
//   cudf_conditional_join_tests          the whole list; needs a GPU (tests/test_gpu_conditional_join.py)
#include <cudf/ast/expressions.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/join/conditional_join.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/scalar/scalar.hpp>

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
std::vector<size_type> to_host(rmm::device_uvector<size_type> const& v)
{
  std::vector<size_type> h(v.size());
  if (v.size()) (void)hipMemcpy(h.data(), v.data(), h.size() * sizeof(size_type), hipMemcpyDeviceToHost);
  return h;
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

using I32   = std::vector<int32_t>;
using F64   = std::vector<double>;
using V     = std::vector<int>;
using Pairs = std::vector<std::pair<size_type, size_type>>;
using OP    = ast::ast_operator;
using TR    = ast::table_reference;
constexpr size_type NM = JoinNoMatch;
static data_type dt(type_id id) { return data_type{id}; }
static table_view tv(std::vector<column_view> const& cols) { return table_view{cols}; }

static Pairs pairs_of(join_result const& r)
{
  auto const l = to_host(*r.first), rr = to_host(*r.second);
  CHECK(l.size() == rr.size());
  Pairs p;
  for (std::size_t i = 0; i < l.size(); ++i) p.emplace_back(l[i], rr[i]);
  return p;
}

// all five kinds and the four sizes of one (left, right, predicate) against the inner pairs written out by hand
static void check_all_kinds(table_view const& left, table_view const& right, ast::expression const& pred, Pairs const& inner)
{
  auto const nl = left.num_rows(), nr = right.num_rows();
  std::vector<int> lhit(nl, 0), rhit(nr, 0);
  for (auto const& [l, r] : inner) lhit[l] = rhit[r] = 1;
  Pairs lj;
  std::vector<size_type> semi, anti;
  std::size_t at = 0;
  for (size_type i = 0; i < nl; ++i) {
    if (!lhit[i]) lj.emplace_back(i, NM);
    for (; at < inner.size() && inner[at].first == i; ++at) lj.push_back(inner[at]);
    (lhit[i] ? semi : anti).push_back(i);
  }
  Pairs fj = lj;
  for (size_type r = 0; r < nr; ++r)
    if (!rhit[r]) fj.emplace_back(NM, r);
  CHECK(pairs_of(conditional_inner_join(left, right, pred)) == inner);
  CHECK(pairs_of(conditional_left_join(left, right, pred)) == lj);
  CHECK(pairs_of(conditional_full_join(left, right, pred)) == fj);
  CHECK(to_host(*conditional_left_semi_join(left, right, pred)) == semi);
  CHECK(to_host(*conditional_left_anti_join(left, right, pred)) == anti);
  CHECK(conditional_inner_join_size(left, right, pred) == inner.size());
  CHECK(conditional_left_join_size(left, right, pred) == lj.size());
  CHECK(conditional_left_semi_join_size(left, right, pred) == semi.size());
  CHECK(conditional_left_anti_join_size(left, right, pred) == anti.size());
}

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view f5{dt(type_id::FLOAT64), 5, fake, nullptr, 0};
  table_view const l{std::vector<column_view>{a5, f5}};
  table_view const r{std::vector<column_view>{a5}};
  ast::column_reference l0{0}, l1{1}, r0{0, TR::RIGHT}, r1{1, TR::RIGHT}, l2{2}, out0{0, TR::OUTPUT};

  run("host: a predicate that is not BOOL8 -> data_type_error, every entry point", [&] {
    ast::operation add{OP::ADD, l0, r0};
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_inner_join(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_left_join(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_full_join(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_left_semi_join(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_left_anti_join(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_inner_join_size(l, r, add); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_left_anti_join_size(l, r, add); }));
  });
  run("host: operands of different types -> data_type_error", [&] {
    ast::operation lt{OP::LESS, l1, r0};  // FLOAT64 < INT32
    CHECK(throws<cudf::data_type_error>([&] { (void)conditional_inner_join(l, r, lt); }));
  });
  run("host: a column index out of range of ITS table -> out_of_range", [&] {
    ast::operation bad_r{OP::LESS, l0, r1};  // the right table has one column, the left one two
    ast::operation bad_l{OP::LESS, l2, r0};
    CHECK(throws<std::out_of_range>([&] { (void)conditional_inner_join(l, r, bad_r); }));
    CHECK(throws<std::out_of_range>([&] { (void)conditional_left_semi_join_size(l, r, bad_l); }));
  });
  run("host: table_reference::OUTPUT -> invalid_argument", [&] {
    ast::operation eq{OP::EQUAL, out0, r0};
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_inner_join(l, r, eq); }));
  });
  run("host: more than 16 columns over both tables -> invalid_argument", [&] {
    std::vector<column_view> nine(9, a5);
    table_view const l9{nine}, r9{nine};
    ast::tree t;
    ast::expression const* acc = nullptr;
    for (int side = 0; side < 2; ++side) {
      for (size_type c = 0; c < 9; ++c) {  // 18 distinct (table, column) pairs
        auto const& ref = t.emplace<ast::column_reference>(c, side ? TR::RIGHT : TR::LEFT);
        acc             = acc ? static_cast<ast::expression const*>(&t.emplace<ast::operation>(OP::ADD, *acc, ref)) : &ref;
      }
    }
    auto const& root = t.emplace<ast::operation>(OP::EQUAL, *acc, t.at(0));
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_inner_join(l9, r9, root); }));
  });
}

static void device_cases()
{
  ast::column_reference l0{0}, l1{1}, r0{0, TR::RIGHT}, r1{1, TR::RIGHT};
  ast::operation eq00{OP::EQUAL, l0, r0};

  run("one column, one row, all equal (TestOneColumnOneRowAllEqual)", [&] {
    auto a = make_col(I32{0}), b = make_col(I32{0});
    check_all_kinds(tv({a->view()}), tv({b->view()}), eq00, Pairs{{0, 0}});
  });
  run("one column, two rows, all equal (TestOneColumnTwoRowAllEqual)", [&] {
    auto a = make_col(I32{0, 1}), b = make_col(I32{0, 0});
    check_all_kinds(tv({a->view()}), tv({b->view()}), eq00, Pairs{{0, 0}, {0, 1}});
  });
  run("two columns, three rows, some equal (TestTwoColumnThreeRowSomeEqual)", [&] {
    auto a0 = make_col(I32{0, 1, 2}), a1 = make_col(I32{10, 20, 30}), b0 = make_col(I32{0, 1, 3}), b1 = make_col(I32{30, 40, 50});
    check_all_kinds(tv({a0->view(), a1->view()}), tv({b0->view(), b1->view()}), eq00, Pairs{{0, 0}, {1, 1}});
  });
  run("NOT of a left column: a predicate that reads one side (TestNotComparison)", [&] {
    auto a = make_col(I32{0, 1, 2}), b = make_col(I32{3, 4, 5});
    ast::operation nt{OP::NOT, l0};
    check_all_kinds(tv({a->view()}), tv({b->view()}), nt, Pairs{{0, 0}, {0, 1}, {0, 2}});
  });
  run("greater: one side larger on several rows (TestGreaterComparison)", [&] {
    auto a = make_col(I32{0, 1, 2}), b = make_col(I32{1, 0, 0});
    ast::operation gt{OP::GREATER, l0, r0};
    check_all_kinds(tv({a->view()}), tv({b->view()}), gt, Pairs{{1, 1}, {1, 2}, {2, 0}, {2, 1}, {2, 2}});
  });
  run("a condition over two columns of each side (TestComplexConditionMultipleColumns)", [&] {
    auto a0 = make_col(I32{0, 0, 0, 1}), a1 = make_col(I32{10, 20, 30, 40});
    auto b0 = make_col(I32{0, 1, 2, 3}), b1 = make_col(I32{30, 40, 50, 60});
    ast::operation gt{OP::GREATER, r1, l1};
    ast::operation both{OP::LOGICAL_AND, eq00, gt};  // l0 == r0 && r1 > l1: rows 0 and 1 against right row 0 (30 > 10, 30 > 20)
    check_all_kinds(tv({a0->view(), a1->view()}), tv({b0->view(), b1->view()}), both, Pairs{{0, 0}, {1, 0}});
  });
  run("doubles with a literal: l.x / r.y > 0.5, the HEAVY program", [&] {
    auto a = make_col(F64{1.0, 3.0, -2.0}), b = make_col(F64{4.0, 2.0});
    numeric_scalar<double> half{0.5};
    ast::literal lit{half};
    ast::operation div{OP::TRUE_DIV, l0, r0};
    ast::operation gt{OP::GREATER, div, lit};
    check_all_kinds(tv({a->view()}), tv({b->view()}), gt, Pairs{{1, 0}, {1, 1}});
  });
  run("nullable inputs on both sides: a null result is no match; NULL_EQUAL pairs null with null", [&] {
    auto a = make_col(I32{0, 1, 2, 1}, V{1, 0, 1, 1}), b = make_col(I32{1, 2, 7}, V{1, 1, 0});
    check_all_kinds(tv({a->view()}), tv({b->view()}), eq00, Pairs{{2, 1}, {3, 0}});
    ast::operation neq{OP::NULL_EQUAL, l0, r0};
    check_all_kinds(tv({a->view()}), tv({b->view()}), neq, Pairs{{1, 2}, {2, 1}, {3, 0}});
  });
  run("sliced views on both sides (cudf::slice): data offset and begin bit", [&] {
    auto a = make_col(I32{9, 9, 0, 1, 2, 9}, V{1, 1, 1, 0, 1, 1}), b = make_col(I32{5, 2, 0, 1, 5}, V{1, 1, 0, 1, 1});
    auto const as = cudf::slice(a->view(), {2, 5}), bs = cudf::slice(b->view(), {1, 4});  // {0, null, 2} x {2, null, 1}
    ast::operation ge{OP::GREATER_EQUAL, l0, r0};
    check_all_kinds(tv({as[0]}), tv({bs[0]}), ge, Pairs{{2, 0}, {2, 2}});
  });
  run("output_size right and wrong", [&] {
    auto a = make_col(I32{0, 1, 2}), b = make_col(I32{1, 0, 0});
    ast::operation gt{OP::GREATER, l0, r0};
    table_view const l = tv({a->view()}), r = tv({b->view()});
    CHECK(pairs_of(conditional_inner_join(l, r, gt, 5)).size() == 5);
    CHECK(pairs_of(conditional_left_join(l, r, gt, 6)).size() == 6);
    CHECK(conditional_left_semi_join(l, r, gt, 2)->size() == 2);
    CHECK(conditional_left_anti_join(l, r, gt, 1)->size() == 1);
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_inner_join(l, r, gt, 4); }));
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_left_join(l, r, gt, 5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_left_semi_join(l, r, gt, 3); }));
    CHECK(throws<std::invalid_argument>([&] { (void)conditional_left_anti_join(l, r, gt, 0); }));
  });
  run("an empty left side and an empty right side", [&] {
    auto a = make_col(I32{0, 1, 2}), e = make_col(I32{});
    table_view const t3 = tv({a->view()}), t0 = tv({e->view()});
    check_all_kinds(t0, t3, eq00, Pairs{});
    check_all_kinds(t3, t0, eq00, Pairs{});
    check_all_kinds(t0, t0, eq00, Pairs{});
    CHECK(pairs_of(conditional_full_join(t0, t3, eq00)) == (Pairs{{NM, 0}, {NM, 1}, {NM, 2}}));
    CHECK(pairs_of(conditional_left_join(t3, t0, eq00)) == (Pairs{{0, NM}, {1, NM}, {2, NM}}));
  });
  run("more rows than one tile and one chunk: l.a < r.b against a host loop", [&] {
    size_type const nl = 777, nr = 1031;
    I32 a(nl), b(nr);
    for (size_type i = 0; i < nl; ++i) a[i] = (i * 37) % 1000;
    for (size_type j = 0; j < nr; ++j) b[j] = (j * 91) % 1013;
    Pairs want;
    for (size_type i = 0; i < nl; ++i)
      for (size_type j = 0; j < nr; ++j)
        if (a[i] + 990 < b[j]) want.emplace_back(i, j);
    auto ca = make_col(a), cb = make_col(b);
    numeric_scalar<int32_t> k{990};
    ast::literal lit{k};
    ast::operation sum{OP::ADD, l0, lit};
    ast::operation lt{OP::LESS, sum, r0};
    check_all_kinds(tv({ca->view()}), tv({cb->view()}), lt, want);
  });
  run("more than 2^31 - 1 pairs: the size is exact, the join throws overflow_error", [&] {
    size_type const n = 46341;
    auto a = make_col(I32(n, 1)), b = make_col(I32(n, 1));
    table_view const l = tv({a->view()}), r = tv({b->view()});
    CHECK(conditional_inner_join_size(l, r, eq00) == std::size_t{2147488281u});
    CHECK(throws<std::overflow_error>([&] { (void)conditional_inner_join(l, r, eq00); }));
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
