// cudf::merge and cudf::lower_bound / upper_bound through the C++ surface (include/cudf/merge.hpp, include/cudf/search.hpp).  Small
// literal vectors, expected values written out by hand.  The minimal harness of cudf_distinct_tests.cpp.
//   cudf_merge_tests --host   argument checks only: everything decided before the first device call, runs without a GPU
//   cudf_merge_tests          the whole list; needs a GPU (tests/test_gpu_merge_search.py)
#include <cudf/column/column_factories.hpp>
#include <cudf/merge.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/search.hpp>

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
  if (!c.nullable()) return v;
  std::vector<bitmask_type> w(num_bitmask_words(c.size() + c.offset()));
  (void)hipMemcpy(w.data(), c.null_mask(), w.size() * 4, hipMemcpyDeviceToHost);
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
template <typename T>
std::vector<T> col_of(table const& t, size_type k)
{
  return to_host<T>(t.get_column(k).view());
}

using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
auto const ASC = order::ASCENDING, DESC = order::DESCENDING;
auto const BEFORE = null_order::BEFORE, AFTER = null_order::AFTER;

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  column_view a{data_type{type_id::INT32}, 5, fake, nullptr, 0};
  column_view f{data_type{type_id::FLOAT64}, 5, fake, nullptr, 0};
  column_view a3{data_type{type_id::INT32}, 3, fake, nullptr, 0};
  column_view f3{data_type{type_id::FLOAT64}, 3, fake, nullptr, 0};
  table_view t{{a, f}}, u{{a3, f3}}, swapped{{f3, a3}}, narrow{{a3}};
  run("merge: empty key_cols, more keys than columns, order vectors of the wrong size throw cudf::logic_error", [&] {
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {}, {}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0, 1, 0}, {ASC, ASC, ASC}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0}, {}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0}, {ASC, ASC}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0, 1}, {ASC}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0, 1}, {ASC, DESC}, {BEFORE}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u}, {0}, {ASC}, {BEFORE, AFTER}); }));
  });
  run("merge: tables whose column counts or types differ throw cudf::logic_error", [&] {
    CHECK(throws<logic_error>([&] { (void)merge({t, swapped}, {0}, {ASC}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, narrow}, {0}, {ASC}); }));
    CHECK(throws<logic_error>([&] { (void)merge({t, u, narrow}, {0}, {ASC}); }));
  });
  run("merge: a key index outside the table throws std::out_of_range (table_view::select)", [&] {
    CHECK(throws<std::out_of_range>([&] { (void)merge({t, u}, {2}, {ASC}); }));
    CHECK(throws<std::out_of_range>([&] { (void)merge({t, u}, {0, -1}, {ASC, ASC}); }));
    CHECK(throws<std::out_of_range>([&] { (void)merge({t}, {7}, {DESC}); }));
  });
  run("merge: a total row count beyond size_type throws std::overflow_error", [&] {
    column_view big{data_type{type_id::INT8}, std::numeric_limits<size_type>::max() - 1, fake, nullptr, 0};
    column_view two{data_type{type_id::INT8}, 2, fake, nullptr, 0};
    CHECK(throws<std::overflow_error>([&] { (void)merge({table_view{{big}}, table_view{{two}}}, {0}, {ASC}); }));
    CHECK(throws<std::overflow_error>([&] { (void)merge({table_view{{big}}, table_view{{big}}, table_view{{big}}}, {0}, {ASC}); }));
  });
  run("merge: no tables give an empty table, tables without rows an empty table of the same types", [&] {
    auto none = merge({}, {0}, {ASC});
    CHECK(none->num_columns() == 0 && none->num_rows() == 0);
    column_view e32{data_type{type_id::INT32}, 0, nullptr, nullptr, 0};
    column_view e64{data_type{type_id::FLOAT64}, 0, nullptr, nullptr, 0};
    table_view e{{e32, e64}};
    auto out = merge({e, e, e}, {1, 0}, {ASC, DESC});
    CHECK(out->num_columns() == 2 && out->num_rows() == 0);
    CHECK(out->get_column(0).type().id() == type_id::INT32 && out->get_column(1).type().id() == type_id::FLOAT64);
  });
  run("lower_bound / upper_bound: differing columns and order vectors of the wrong size throw cudf::logic_error", [&] {
    CHECK(throws<logic_error>([&] { (void)lower_bound(t, swapped, {ASC, ASC}, {}); }));
    CHECK(throws<logic_error>([&] { (void)upper_bound(t, narrow, {ASC, ASC}, {}); }));
    CHECK(throws<logic_error>([&] { (void)lower_bound(t, u, {ASC}, {}); }));
    CHECK(throws<logic_error>([&] { (void)upper_bound(t, u, {}, {}); }));
    CHECK(throws<logic_error>([&] { (void)lower_bound(t, u, {ASC, ASC}, {BEFORE}); }));
    CHECK(throws<logic_error>([&] { (void)upper_bound(t, u, {ASC, DESC}, {BEFORE, AFTER, AFTER}); }));
  });
  run("lower_bound / upper_bound: no needles give an empty INT32 column", [&] {
    column_view e32{data_type{type_id::INT32}, 0, nullptr, nullptr, 0};
    column_view e64{data_type{type_id::FLOAT64}, 0, nullptr, nullptr, 0};
    auto lo = lower_bound(t, table_view{{e32, e64}}, {ASC, ASC}, {});
    auto hi = upper_bound(t, table_view{{e32, e64}}, {DESC, ASC}, {AFTER, BEFORE});
    CHECK(lo->size() == 0 && lo->type().id() == type_id::INT32 && hi->size() == 0 && hi->type().id() == type_id::INT32);
  });
}

static void device_cases()
{
  constexpr double NaN = std::numeric_limits<double>::quiet_NaN();
  run("merge of two tables: stable on ties, the payload rides along", [&] {
    auto ak = make_col<int32_t>({1, 3, 3, 5, 9});
    auto ap = make_col<int64_t>({10, 11, 12, 13, 14});
    auto bk = make_col<int32_t>({0, 3, 4, 9, 9, 12});
    auto bp = make_col<int64_t>({20, 21, 22, 23, 24, 25});
    auto out = merge({table_view{{ak->view(), ap->view()}}, table_view{{bk->view(), bp->view()}}}, {0}, {ASC});
    CHECK((col_of<int32_t>(*out, 0) == I32{0, 1, 3, 3, 3, 4, 5, 9, 9, 9, 12}));
    CHECK((col_of<int64_t>(*out, 1) == I64{20, 10, 11, 12, 21, 22, 13, 14, 23, 24, 25}));
    CHECK(!out->get_column(0).nullable() && !out->get_column(1).nullable());
  });
  run("merge: one table is a copy; tables without rows are skipped", [&] {
    auto ak = make_col<int32_t>({4, 2, 1});
    auto e  = make_col<int32_t>({});
    auto one = merge({table_view{{ak->view()}}}, {0}, {DESC});
    CHECK((col_of<int32_t>(*one, 0) == I32{4, 2, 1}));
    auto bk  = make_col<int32_t>({3, 2});
    auto out = merge({table_view{{e->view()}}, table_view{{ak->view()}}, table_view{{e->view()}}, table_view{{bk->view()}}}, {0}, {DESC});
    CHECK((col_of<int32_t>(*out, 0) == I32{4, 3, 2, 2, 1}));
    auto alone = merge({table_view{{e->view()}}, table_view{{bk->view()}}, table_view{{e->view()}}}, {0}, {DESC});
    CHECK((col_of<int32_t>(*alone, 0) == I32{3, 2}));
  });
  run("merge of three tables: ties come out by table index", [&] {
    auto k0 = make_col<int16_t>({1, 2, 2});
    auto p0 = make_col<int32_t>({0, 1, 2});
    auto k1 = make_col<int16_t>({2, 2, 3});
    auto p1 = make_col<int32_t>({100, 101, 102});
    auto k2 = make_col<int16_t>({0, 2});
    auto p2 = make_col<int32_t>({200, 201});
    auto out = merge({table_view{{p0->view(), k0->view()}}, table_view{{p1->view(), k1->view()}}, table_view{{p2->view(), k2->view()}}}, {1}, {ASC});
    CHECK((col_of<int16_t>(*out, 1) == std::vector<int16_t>{0, 1, 2, 2, 2, 2, 2, 3}));
    CHECK((col_of<int32_t>(*out, 0) == I32{200, 0, 1, 2, 100, 101, 201, 102}));
  });
  run("merge on two keys, mixed directions, float key with NaN and -0.0", [&] {
    // order: k0 DESCENDING, then k1 ASCENDING (NaN greatest, -0.0 == +0.0)
    auto a0 = make_col<int8_t>({2, 2, 1, 1});
    auto a1 = make_col<double>({-0.0, NaN, 1.0, NaN});
    auto ar = make_col<int32_t>({0, 1, 2, 3});
    auto b0 = make_col<int8_t>({2, 2, 1});
    auto b1 = make_col<double>({0.0, 5.0, -NaN});
    auto br = make_col<int32_t>({10, 11, 12});
    auto out = merge({table_view{{a0->view(), a1->view(), ar->view()}}, table_view{{b0->view(), b1->view(), br->view()}}}, {0, 1}, {DESC, ASC});
    CHECK((col_of<int32_t>(*out, 2) == I32{0, 10, 11, 1, 2, 3, 12}));
  });
  run("merge with nullable keys: null_precedence per key, a null's bytes decide nothing", [&] {
    // ascending, nulls BEFORE:  A = null null 1 4     B = null 1 2
    auto ak = make_col<int32_t>({77, -5, 1, 4}, {0, 0, 1, 1});
    auto ar = make_col<int32_t>({0, 1, 2, 3});
    auto bk = make_col<int32_t>({1234, 1, 2}, {0, 1, 1});
    auto br = make_col<int32_t>({10, 11, 12});
    auto out = merge({table_view{{ak->view(), ar->view()}}, table_view{{bk->view(), br->view()}}}, {0}, {ASC}, {BEFORE});
    CHECK((col_of<int32_t>(*out, 1) == I32{0, 1, 10, 2, 11, 12, 3}));
    CHECK(out->get_column(0).null_count() == 3 && (valid_host(out->get_column(0).view()) == std::vector<int>{0, 0, 0, 1, 1, 1, 1}));
    // ascending, nulls AFTER:   A = 1 4 null     B = 2 null null
    auto ck = make_col<int32_t>({1, 4, 9}, {1, 1, 0});
    auto cr = make_col<int32_t>({0, 1, 2});
    auto dk = make_col<int32_t>({2, 0, 0}, {1, 0, 0});
    auto dr = make_col<int32_t>({10, 11, 12});
    auto after = merge({table_view{{ck->view(), cr->view()}}, table_view{{dk->view(), dr->view()}}}, {0}, {ASC}, {AFTER});
    CHECK((col_of<int32_t>(*after, 1) == I32{0, 10, 1, 2, 11, 12}));
  });
  run("merge: a null mask on a payload column only; a payload without nulls in the output comes back without a mask", [&] {
    auto ak = make_col<int64_t>({1, 2, 3});
    auto ap = make_col<int16_t>({7, 8, 9}, {1, 0, 1});
    auto bk = make_col<int64_t>({2, 2});
    auto bp = make_col<int16_t>({20, 21});
    auto out = merge({table_view{{ak->view(), ap->view()}}, table_view{{bk->view(), bp->view()}}}, {0}, {ASC});
    CHECK((col_of<int64_t>(*out, 0) == I64{1, 2, 2, 2, 3}));
    CHECK((valid_host(out->get_column(1).view()) == std::vector<int>{1, 0, 1, 1, 1}) && out->get_column(1).null_count() == 1);
    auto got = col_of<int16_t>(*out, 1);
    CHECK(got[0] == 7 && got[2] == 20 && got[3] == 21 && got[4] == 9);
    CHECK(!out->get_column(0).nullable());
  });
  run("merge of sliced views: nonzero offset on data and bitmap", [&] {
    //                  index: 0  1 | 2  3     4  5 | 6        the view is rows 2 .. 5: null 3 5 5
    auto ak = make_col<int32_t>({9, 9, 1234, 3, 5, 5, 0}, {1, 1, 0, 1, 1, 1, 0});
    auto ar = make_col<int8_t>({0, 1, 2, 3, 4, 5, 6});
    column_view sa{ak->type(), 4, ak->view().head<void>(), ak->view().null_mask(), 1, 2};
    column_view sr{ar->type(), 4, ar->view().head<void>(), nullptr, 0, 2};
    //                  index: 0 | 1  2  3         the view is rows 1 .. 3: null 4 5
    auto bk = make_col<int32_t>({8, 4321, 4, 5}, {1, 0, 1, 1});
    auto br = make_col<int8_t>({10, 11, 12, 13});
    column_view sb{bk->type(), 3, bk->view().head<void>(), bk->view().null_mask(), 1, 1};
    column_view sq{br->type(), 3, br->view().head<void>(), nullptr, 0, 1};
    auto out = merge({table_view{{sa, sr}}, table_view{{sb, sq}}}, {0}, {ASC}, {BEFORE});
    CHECK((col_of<int8_t>(*out, 1) == std::vector<int8_t>{2, 11, 3, 12, 4, 5, 13}));
    CHECK((valid_host(out->get_column(0).view()) == std::vector<int>{0, 0, 1, 1, 1, 1, 1}) && out->get_column(0).null_count() == 2);
  });
  run("lower_bound / upper_bound: duplicates, needles outside the range, NaN and null needles, both directions", [&] {
    auto hay = make_col<double>({10., 20., 20., 20., 30., NaN, NaN});
    auto nee = make_col<double>({5., 10., 20., 25., 30., 1e300, -NaN, 20.});
    auto lo  = lower_bound(table_view{{hay->view()}}, table_view{{nee->view()}}, {ASC}, {BEFORE});
    auto hi  = upper_bound(table_view{{hay->view()}}, table_view{{nee->view()}}, {ASC}, {BEFORE});
    CHECK((to_host<int32_t>(lo->view()) == I32{0, 0, 1, 4, 4, 5, 5, 1}));
    CHECK((to_host<int32_t>(hi->view()) == I32{0, 1, 4, 4, 5, 5, 7, 4}));
    CHECK(!lo->nullable() && lo->type().id() == type_id::INT32);
    // descending with nulls AFTER: the order is  50 40 40 10 null null   (a descending column puts "after" nulls ... first iff
    // null_before != descending: AFTER and DESCENDING -> first).  Written out: nulls first.
    auto hd = make_col<int32_t>({0, 0, 50, 40, 40, 10}, {0, 0, 1, 1, 1, 1});
    auto nd = make_col<int32_t>({60, 40, 5, 123}, {1, 1, 1, 0});
    auto lod = lower_bound(table_view{{hd->view()}}, table_view{{nd->view()}}, {DESC}, {AFTER});
    auto hid = upper_bound(table_view{{hd->view()}}, table_view{{nd->view()}}, {DESC}, {AFTER});
    CHECK((to_host<int32_t>(lod->view()) == I32{2, 3, 6, 0}));
    CHECK((to_host<int32_t>(hid->view()) == I32{2, 5, 6, 2}));
  });
  run("lower_bound / upper_bound on two columns and an empty haystack", [&] {
    auto h0 = make_col<int8_t>({1, 1, 2, 2, 2});
    auto h1 = make_col<uint16_t>({5, 7, 1, 1, 9});
    auto n0 = make_col<int8_t>({1, 2, 2, 3, 0});
    auto n1 = make_col<uint16_t>({6, 1, 10, 0, 99});
    table_view h{{h0->view(), h1->view()}}, x{{n0->view(), n1->view()}};
    CHECK((to_host<int32_t>(lower_bound(h, x, {ASC, ASC}, {})->view()) == I32{1, 2, 5, 5, 0}));
    CHECK((to_host<int32_t>(upper_bound(h, x, {ASC, ASC}, {})->view()) == I32{1, 4, 5, 5, 0}));
    auto e0 = make_col<int8_t>({});
    auto e1 = make_col<uint16_t>({});
    CHECK((to_host<int32_t>(upper_bound(table_view{{e0->view(), e1->view()}}, x, {ASC, ASC}, {})->view()) == I32{0, 0, 0, 0, 0}));
  });
}

int main(int argc, char** argv)
{
  setvbuf(stdout, nullptr, _IONBF, 0);
  bool const host_only = argc > 1 && std::string{argv[1]} == "--host";
  host_cases();
  if (!host_only) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
      std::printf("no GPU\n");
      return 77;
    }
    device_cases();
  }
  std::printf("%d run, %d failed\n", g_run, g_failed);
  return g_failed ? 1 : 0;
}
