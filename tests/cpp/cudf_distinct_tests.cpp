// Deduplication through the C++ surface: cudf::unique / distinct / stable_distinct / distinct_indices / unique_count / distinct_count
// (include/cudf/stream_compaction.hpp).  Small literal vectors, expected values written out by hand (the reference's suites pin the
// same contract: unique_tests.cpp, distinct_tests.cpp, stable_distinct_tests.cpp, unique_count_tests.cpp, distinct_count_tests.cpp).
// The minimal harness of cudf_compaction_tests.cpp.
//   cudf_distinct_tests --host   argument checks only: everything decided before the first device call, runs without a GPU
//   cudf_distinct_tests          the whole list; needs a GPU (tests/test_gpu_distinct.py)
#include <cudf/column/column_factories.hpp>
#include <cudf/stream_compaction.hpp>

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
template <typename T>
bool same_bits(std::vector<T> const& a, std::vector<T> const& b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
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

using K = duplicate_keep_option;
using I32 = std::vector<int32_t>;

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake      = reinterpret_cast<void const*>(0x10000);
  auto const* fake_mask = reinterpret_cast<bitmask_type const*>(0x20000);
  column_view a{data_type{type_id::INT32}, 5, fake, fake_mask, 1};
  column_view f{data_type{type_id::FLOAT64}, 5, fake, nullptr, 0};
  table_view t{{a, f}};
  run("a key index out of range throws std::out_of_range (table_view::select)", [&] {
    CHECK(throws<std::out_of_range>([&] { (void)unique(t, {2}, K::KEEP_FIRST); }));
    CHECK(throws<std::out_of_range>([&] { (void)unique(t, {0, -1}, K::KEEP_NONE); }));
    CHECK(throws<std::out_of_range>([&] { (void)distinct(t, {1, 7}); }));
    CHECK(throws<std::out_of_range>([&] { (void)stable_distinct(t, {5}, K::KEEP_LAST); }));
  });
  run("more than 32 key columns throw std::invalid_argument", [&] {
    std::vector<size_type> keys33(33, 0), keys32(32, 1);
    CHECK(throws<std::invalid_argument>([&] { (void)unique(t, keys33, K::KEEP_FIRST); }));
    CHECK(throws<std::invalid_argument>([&] { (void)distinct(t, keys33); }));
    CHECK(throws<std::invalid_argument>([&] { (void)stable_distinct(t, keys33); }));
    std::vector<column_view> wide(33, f);
    CHECK(throws<std::invalid_argument>([&] { (void)distinct_indices(table_view{wide}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)distinct_count(table_view{wide}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)unique_count(table_view{wide}); }));
  });
  run("no rows: a copy of the input, whatever the keys; counts are 0", [&] {
    column_view e32{data_type{type_id::INT32}, 0, nullptr, nullptr, 0};
    column_view e64{data_type{type_id::FLOAT64}, 0, nullptr, nullptr, 0};
    table_view e{{e32, e64}};
    for (auto keep : {K::KEEP_ANY, K::KEEP_FIRST, K::KEEP_LAST, K::KEEP_NONE}) {
      auto u = unique(e, {0, 1}, keep);
      auto d = distinct(e, {1}, keep);
      auto s = stable_distinct(e, {}, keep);
      for (auto const* o : {u.get(), d.get(), s.get()}) {
        CHECK(o->num_columns() == 2 && o->num_rows() == 0);
        CHECK(o->get_column(0).type().id() == type_id::INT32 && o->get_column(1).type().id() == type_id::FLOAT64);
      }
    }
    CHECK(throws<std::out_of_range>([&] { (void)distinct(e, {2}); }));
    auto idx = distinct_indices(e);
    CHECK(idx->size() == 0 && idx->type().id() == type_id::INT32);
    CHECK(distinct_count(e) == 0 && unique_count(e) == 0);
    CHECK(distinct_count(e32, null_policy::INCLUDE, nan_policy::NAN_IS_VALID) == 0);
    CHECK(unique_count(e64, null_policy::EXCLUDE, nan_policy::NAN_IS_NULL) == 0);
    CHECK(distinct_count(table_view{}) == 0 && unique_count(table_view{}) == 0);
  });
}

template <typename T>
std::vector<T> col_of(table const& t, size_type k)
{
  return to_host<T>(t.get_column(k).view());
}

static void device_cases()
{
  constexpr double NaN = std::numeric_limits<double>::quiet_NaN();
  // keys                 row: 0  1  2  3  4  5  6  7       classes 1: {0, 1, 6}  2: {2}  3: {3, 4, 5}  4: {7}
  std::vector<int64_t> const k{1, 1, 2, 3, 3, 3, 1, 4};
  I32 const row{0, 1, 2, 3, 4, 5, 6, 7};
  // one float key:        row: 0    1    2     3     4     5     6    7
  std::vector<double> const d{1.0, NaN, -NaN, 99.0, 98.0, -0.0, 0.0, 1.0};
  std::vector<int> const dv{1, 1, 1, 0, 0, 1, 1, 1};  // rows 3 and 4 are null (their bytes differ and must not matter)

  run("unique: every keep option on runs of consecutive rows", [&] {
    auto ck = make_col(k);
    auto cr = make_col(row);
    table_view t{{ck->view(), cr->view()}};
    CHECK((col_of<int32_t>(*unique(t, {0}, K::KEEP_FIRST), 1) == I32{0, 2, 3, 6, 7}));
    CHECK((col_of<int32_t>(*unique(t, {0}, K::KEEP_ANY), 1) == I32{0, 2, 3, 6, 7}));
    CHECK((col_of<int32_t>(*unique(t, {0}, K::KEEP_LAST), 1) == I32{1, 2, 5, 6, 7}));
    CHECK((col_of<int32_t>(*unique(t, {0}, K::KEEP_NONE), 1) == I32{2, 6, 7}));
    CHECK((col_of<int64_t>(*unique(t, {0}, K::KEEP_LAST), 0) == std::vector<int64_t>{1, 2, 3, 1, 4}));
    CHECK(unique(t, {}, K::KEEP_FIRST)->num_rows() == 8);  // no keys: a copy
    CHECK(unique(t, {0, 1}, K::KEEP_NONE)->num_rows() == 8);  // the row number is a key: nothing repeats
  });
  run("distinct / stable_distinct: every keep option over the whole table, input order", [&] {
    auto ck = make_col(k);
    auto cr = make_col(row);
    table_view t{{ck->view(), cr->view()}};
    for (auto* fn : {&distinct, &stable_distinct}) {
      auto call = [&](K keep) { return (*fn)(t, {0}, keep, null_equality::EQUAL, nan_equality::ALL_EQUAL, get_default_stream(),
                                             get_current_device_resource_ref()); };
      CHECK((col_of<int32_t>(*call(K::KEEP_FIRST), 1) == I32{0, 2, 3, 7}));
      CHECK((col_of<int32_t>(*call(K::KEEP_LAST), 1) == I32{2, 5, 6, 7}));
      CHECK((col_of<int32_t>(*call(K::KEEP_NONE), 1) == I32{2, 7}));
      auto any = call(K::KEEP_ANY);
      CHECK((col_of<int64_t>(*any, 0) == std::vector<int64_t>{1, 2, 3, 4}));  // one row per class; in this table input order = key order
      auto r = col_of<int32_t>(*any, 1);
      CHECK(r.size() == 4 && (r[0] == 0 || r[0] == 1) && r[1] == 2 && (r[2] == 3 || r[2] == 4 || r[2] == 5) && r[3] == 7);
    }
    CHECK(distinct(t, {})->num_rows() == 8);
    CHECK(distinct(t, {1, 0}, K::KEEP_NONE)->num_rows() == 8);
  });
  run("nulls_equal / nans_equal UNEQUAL: such rows equal nothing and are always kept; -0.0 == +0.0", [&] {
    auto cd = make_col(d, dv);
    auto cr = make_col(row);
    table_view t{{cd->view(), cr->view()}};
    auto rows = [&](K keep, null_equality ne, nan_equality na) { return col_of<int32_t>(*distinct(t, {0}, keep, ne, na), 1); };
    auto const EQ = null_equality::EQUAL, NE = null_equality::UNEQUAL;
    auto const AE = nan_equality::ALL_EQUAL, AU = nan_equality::UNEQUAL;
    CHECK((rows(K::KEEP_FIRST, EQ, AE) == I32{0, 1, 3, 5}));
    CHECK((rows(K::KEEP_LAST, EQ, AE) == I32{2, 4, 6, 7}));
    CHECK((rows(K::KEEP_NONE, EQ, AE) == I32{}));
    CHECK((rows(K::KEEP_FIRST, NE, AE) == I32{0, 1, 3, 4, 5}));
    CHECK((rows(K::KEEP_FIRST, EQ, AU) == I32{0, 1, 2, 3, 5}));
    CHECK((rows(K::KEEP_LAST, NE, AU) == I32{1, 2, 3, 4, 6, 7}));
    CHECK((rows(K::KEEP_NONE, NE, AU) == I32{1, 2, 3, 4}));
    CHECK((rows(K::KEEP_ANY, NE, AU).size() == 6));
    auto out = distinct(t, {0}, K::KEEP_FIRST);
    CHECK(out->get_column(0).null_count() == 1 && (valid_host(out->get_column(0).view()) == std::vector<int>{1, 1, 0, 1}));
    auto urows = [&](K keep, null_equality ne) { return col_of<int32_t>(*unique(t, {0}, keep, ne), 1); };
    CHECK((urows(K::KEEP_FIRST, EQ) == I32{0, 1, 3, 5, 7}));  // NaNs always compare equal in unique
    CHECK((urows(K::KEEP_FIRST, NE) == I32{0, 1, 3, 4, 5, 7}));
    CHECK((urows(K::KEEP_LAST, EQ) == I32{0, 2, 4, 6, 7}));
    CHECK((urows(K::KEEP_NONE, EQ) == I32{0, 7}));
    CHECK((urows(K::KEEP_NONE, NE) == I32{0, 3, 4, 7}));
  });
  run("keys from a sliced view: nonzero offset on data and bitmap", [&] {
    //                    index: 0  1  2 | 3  4  5  6     7     8  9 | 10 11      the view is rows 3 .. 9: 5 5 7 null null 7 5
    std::vector<int32_t> const a{9, 9, 9, 5, 5, 7, 1234, 4321, 7, 5, 9, 9};
    std::vector<int> const av{1, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1};
    std::vector<int16_t> const b{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    auto ca = make_col(a, av);
    auto cb = make_col(b);
    column_view sa{ca->type(), 7, ca->view().head<void>(), ca->view().null_mask(), 2, 3};
    column_view sb{cb->type(), 7, cb->view().head<void>(), nullptr, 0, 3};
    table_view t{{sa, sb}};
    using I16 = std::vector<int16_t>;
    CHECK((col_of<int16_t>(*distinct(t, {0}, K::KEEP_FIRST), 1) == I16{3, 5, 6}));
    CHECK((col_of<int16_t>(*distinct(t, {0}, K::KEEP_LAST), 1) == I16{7, 8, 9}));
    CHECK((col_of<int16_t>(*distinct(t, {0}, K::KEEP_NONE), 1) == I16{}));
    CHECK((col_of<int16_t>(*distinct(t, {0}, K::KEEP_FIRST, null_equality::UNEQUAL), 1) == I16{3, 5, 6, 7}));
    CHECK((col_of<int16_t>(*unique(t, {0}, K::KEEP_FIRST), 1) == I16{3, 5, 6, 8, 9}));
    CHECK((col_of<int16_t>(*unique(t, {0}, K::KEEP_LAST), 1) == I16{4, 5, 7, 8, 9}));
    CHECK((col_of<int16_t>(*unique(t, {0}, K::KEEP_NONE), 1) == I16{5, 8, 9}));
    auto out = distinct(t, {0}, K::KEEP_FIRST);
    CHECK((col_of<int32_t>(*out, 0)[0] == 5 && col_of<int32_t>(*out, 0)[1] == 7));
    CHECK((valid_host(out->get_column(0).view()) == std::vector<int>{1, 1, 0}) && out->get_column(0).null_count() == 1);
    CHECK((to_host<int32_t>(distinct_indices(table_view{{sa}}, K::KEEP_LAST)->view()) == I32{4, 5, 6}));
    CHECK(distinct_count(table_view{{sa}}) == 3 && unique_count(table_view{{sa}}) == 5);
    CHECK(distinct_count(sa, null_policy::EXCLUDE, nan_policy::NAN_IS_VALID) == 2);
    CHECK(unique_count(sa, null_policy::EXCLUDE, nan_policy::NAN_IS_VALID) == 4);
  });
  run("payload columns of every width, one of them nullable, from one plan; two key columns", [&] {
    std::vector<int8_t> const k0{1, 1, 1, 2, 2, 1, 2};
    std::vector<float> const k1{.5f, .5f, 1.5f, .5f, .5f, .5f, 1.5f};  // rows: (1,.5) (1,.5) (1,1.5) (2,.5) (2,.5) (1,.5) (2,1.5)
    std::vector<int8_t> const p8{10, 11, 12, 13, 14, 15, 16};
    std::vector<int16_t> const p16{100, 101, 102, 103, 104, 105, 106};
    std::vector<int32_t> const p32{1000, 1001, 1002, 1003, 1004, 1005, 1006};
    std::vector<double> const p64{.0, .1, .2, .3, .4, .5, .6};
    std::vector<int> const v64{1, 0, 1, 0, 1, 1, 1};
    auto c0 = make_col(k0);
    auto c1 = make_col(k1);
    auto c8 = make_col(p8);
    auto c16 = make_col(p16);
    auto c32 = make_col(p32);
    auto c64 = make_col(p64, v64);
    table_view t{{c8->view(), c0->view(), c16->view(), c1->view(), c32->view(), c64->view()}};
    auto out = distinct(t, {1, 3}, K::KEEP_LAST);  // classes {0, 1, 5} {2} {3, 4} {6} -> rows 2, 4, 5, 6
    CHECK(out->num_columns() == 6 && out->num_rows() == 4);
    CHECK((col_of<int8_t>(*out, 0) == std::vector<int8_t>{12, 14, 15, 16}));
    CHECK((col_of<int8_t>(*out, 1) == std::vector<int8_t>{1, 2, 1, 2}));
    CHECK((col_of<int16_t>(*out, 2) == std::vector<int16_t>{102, 104, 105, 106}));
    CHECK((col_of<float>(*out, 3) == std::vector<float>{1.5f, .5f, .5f, 1.5f}));
    CHECK((col_of<int32_t>(*out, 4) == I32{1002, 1004, 1005, 1006}));
    CHECK((col_of<double>(*out, 5) == std::vector<double>{.2, .4, .5, .6}));
    CHECK(!out->get_column(5).nullable() && out->get_column(5).null_count() == 0);  // every kept row is valid: no mask comes back
    auto first = distinct(t, {1, 3}, K::KEEP_FIRST);  // rows 0, 2, 3, 6
    CHECK((col_of<int32_t>(*first, 4) == I32{1000, 1002, 1003, 1006}));
    CHECK(first->get_column(5).null_count() == 1 && (valid_host(first->get_column(5).view()) == std::vector<int>{1, 1, 0, 1}));
    auto u = unique(t, {1, 3}, K::KEEP_FIRST);  // runs (0 1) (2) (3 4) (5) (6)
    CHECK((col_of<int16_t>(*u, 2) == std::vector<int16_t>{100, 102, 103, 105, 106}));
  });
  run("distinct_indices: the ascending row numbers distinct keeps", [&] {
    auto ck = make_col(k);
    auto cd = make_col(d, dv);
    CHECK((to_host<int32_t>(distinct_indices(table_view{{ck->view()}}, K::KEEP_FIRST)->view()) == I32{0, 2, 3, 7}));
    CHECK((to_host<int32_t>(distinct_indices(table_view{{ck->view()}}, K::KEEP_LAST)->view()) == I32{2, 5, 6, 7}));
    CHECK((to_host<int32_t>(distinct_indices(table_view{{ck->view()}}, K::KEEP_NONE)->view()) == I32{2, 7}));
    CHECK(distinct_indices(table_view{{ck->view()}})->size() == 4);
    auto both = distinct_indices(table_view{{ck->view(), cd->view()}}, K::KEEP_FIRST, null_equality::UNEQUAL, nan_equality::UNEQUAL);
    CHECK(both->size() == 8 && both->type().id() == type_id::INT32 && !both->nullable());
    // (k, d) rows: (1,1.0) (1,NaN) (2,NaN) (3,null) (3,null) (3,0) (1,0) (4,1.0): only rows 3 and 4 are equal
    CHECK((to_host<int32_t>(distinct_indices(table_view{{ck->view(), cd->view()}}, K::KEEP_LAST)->view()) == I32{0, 1, 2, 4, 5, 6, 7}));
  });
  run("counts: the table form and the column form under null_policy x nan_policy", [&] {
    auto ck = make_col(k);
    auto cd = make_col(d, dv);
    CHECK(distinct_count(table_view{{ck->view()}}) == 4 && unique_count(table_view{{ck->view()}}) == 5);
    CHECK(distinct_count(table_view{{cd->view()}}) == 4 && unique_count(table_view{{cd->view()}}) == 5);
    CHECK(distinct_count(table_view{{cd->view()}}, null_equality::UNEQUAL) == 5);
    CHECK(unique_count(table_view{{cd->view()}}, null_equality::UNEQUAL) == 6);
    CHECK(distinct_count(table_view{{ck->view(), cd->view()}}) == 7 && unique_count(table_view{{ck->view(), cd->view()}}) == 7);
    auto const INC = null_policy::INCLUDE, EXC = null_policy::EXCLUDE;
    auto const NV = nan_policy::NAN_IS_VALID, NN = nan_policy::NAN_IS_NULL;
    CHECK(distinct_count(cd->view(), INC, NV) == 4);  // 1.0, NaN, null, 0
    CHECK(distinct_count(cd->view(), INC, NN) == 3);  // 1.0, null = NaN, 0
    CHECK(distinct_count(cd->view(), EXC, NV) == 3);  // 1.0, NaN, 0
    CHECK(distinct_count(cd->view(), EXC, NN) == 2);  // 1.0, 0
    CHECK(unique_count(cd->view(), INC, NV) == 5);    // 1 | NaN NaN | null null | 0 0 | 1
    CHECK(unique_count(cd->view(), INC, NN) == 4);    // 1 | NaN NaN null null | 0 0 | 1
    CHECK(unique_count(cd->view(), EXC, NV) == 4);    // rows 0, 1, 5, 7
    CHECK(unique_count(cd->view(), EXC, NN) == 3);    // rows 0, 5, 7
    auto c1n1 = make_col<int32_t>({1, 77, 1}, {1, 0, 1});
    CHECK(unique_count(c1n1->view(), EXC, NV) == 2 && unique_count(c1n1->view(), INC, NV) == 3);
    CHECK(distinct_count(c1n1->view(), EXC, NV) == 1 && distinct_count(c1n1->view(), INC, NV) == 2);
    auto nulls = make_col<int64_t>({5, 6, 7}, {0, 0, 0});
    CHECK(distinct_count(nulls->view(), INC, NV) == 1 && distinct_count(nulls->view(), EXC, NV) == 0);
    CHECK(unique_count(nulls->view(), INC, NN) == 1 && unique_count(nulls->view(), EXC, NN) == 0);
    auto nans = make_col<float>({std::nanf(""), -std::nanf(""), std::nanf("")});
    CHECK(distinct_count(nans->view(), INC, NV) == 1 && distinct_count(nans->view(), EXC, NV) == 1);
    CHECK(distinct_count(nans->view(), INC, NN) == 1 && distinct_count(nans->view(), EXC, NN) == 0);
    CHECK(unique_count(nans->view(), EXC, NV) == 1 && unique_count(nans->view(), EXC, NN) == 0);
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
