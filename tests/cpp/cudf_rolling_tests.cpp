// cudf::rolling_window / grouped_rolling_window through the C++ surface (include/cudf/rolling.hpp).  Small literal vectors, expected
// values written out by hand.  The minimal harness of cudf_merge_tests.cpp.
//   cudf_rolling_tests --host   argument checks only: everything decided before the first device call, runs without a GPU
//   cudf_rolling_tests          the whole list; needs a GPU (tests/test_gpu_rolling.py)
#include <cudf/aggregation.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/rolling.hpp>

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

using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
auto sum_agg() { return make_sum_aggregation<rolling_aggregation>(); }
auto min_agg() { return make_min_aggregation<rolling_aggregation>(); }
auto max_agg() { return make_max_aggregation<rolling_aggregation>(); }
auto mean_agg() { return make_mean_aggregation<rolling_aggregation>(); }
auto count_valid_agg() { return make_count_aggregation<rolling_aggregation>(null_policy::EXCLUDE); }
auto count_all_agg() { return make_count_aggregation<rolling_aggregation>(null_policy::INCLUDE); }

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  auto const* fake_mask = reinterpret_cast<bitmask_type const*>(0x20000);
  column_view a{data_type{type_id::INT32}, 5, fake, nullptr, 0};
  column_view w5{data_type{type_id::INT32}, 5, fake, nullptr, 0};
  run("min_periods < 0 throws cudf::logic_error in all three overloads", [&] {
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, 2, 1, -1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w5, w5, -1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)grouped_rolling_window(table_view{{a}}, a, 2, 1, -1, *sum_agg()); }));
  });
  run("a key table whose row count differs from the input's throws cudf::logic_error", [&] {
    column_view k3{data_type{type_id::INT64}, 3, fake, nullptr, 0};
    CHECK(throws<logic_error>([&] { (void)grouped_rolling_window(table_view{{k3}}, a, 2, 1, 1, *sum_agg()); }));
  });
  run("window columns that are not non-nullable INT32 of input.size() rows throw cudf::logic_error", [&] {
    column_view w64{data_type{type_id::INT64}, 5, fake, nullptr, 0};
    column_view w4{data_type{type_id::INT32}, 4, fake, nullptr, 0};
    column_view wn{data_type{type_id::INT32}, 5, fake, fake_mask, 0};
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w64, w5, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w5, w64, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w4, w5, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w5, w4, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, wn, w5, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w5, wn, 1, *sum_agg()); }));
  });
  run("an aggregation kind other than the six throws cudf::logic_error", [&] {
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, 2, 1, 1, *make_product_aggregation<rolling_aggregation>()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, 2, 1, 1, *make_variance_aggregation<rolling_aggregation>()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(a, w5, w5, 1, *make_std_aggregation<rolling_aggregation>()); }));
    CHECK(throws<logic_error>([&] { (void)grouped_rolling_window(table_view{{a}}, a, 2, 1, 1, *make_argmax_aggregation<rolling_aggregation>()); }));
  });
  run("a non-numeric input type throws cudf::logic_error", [&] {
    column_view s{data_type{type_id::STRING}, 5, fake, nullptr, 0};
    column_view e{data_type{type_id::TIMESTAMP_DAYS}, 5, fake, nullptr, 0};
    CHECK(throws<logic_error>([&] { (void)rolling_window(s, 2, 1, 1, *sum_agg()); }));
    CHECK(throws<logic_error>([&] { (void)rolling_window(e, w5, w5, 1, *min_agg()); }));
    CHECK(throws<logic_error>([&] { (void)grouped_rolling_window(table_view{{a}}, s, 2, 1, 1, *max_agg()); }));
  });
  run("an input without rows gives an empty column of the result type", [&] {
    column_view e8{data_type{type_id::INT8}, 0, nullptr, nullptr, 0};
    column_view ef{data_type{type_id::FLOAT32}, 0, nullptr, nullptr, 0};
    column_view ew{data_type{type_id::INT32}, 0, nullptr, nullptr, 0};
    CHECK(rolling_window(e8, 2, 1, 1, *sum_agg())->type().id() == type_id::INT64);
    CHECK(rolling_window(ef, 2, 1, 1, *sum_agg())->type().id() == type_id::FLOAT32);
    CHECK(rolling_window(e8, ew, ew, 1, *mean_agg())->type().id() == type_id::FLOAT64);
    CHECK(grouped_rolling_window(table_view{{e8}}, e8, 2, 1, 1, *count_all_agg())->type().id() == type_id::INT32);
    CHECK(rolling_window(e8, 2, 1, 1, *min_agg())->size() == 0);
  });
}

static void device_cases()
{
  constexpr double NaN = std::numeric_limits<double>::quiet_NaN();
  run("fixed window (2, 1) SUM of INT32: INT64, the ends are cut, no mask when no row is null", [&] {
    auto c   = make_col<int32_t>({1, 2, 3, 4, 5});
    auto out = rolling_window(c->view(), 2, 1, 1, *sum_agg());
    CHECK(out->type().id() == type_id::INT64 && !out->nullable() && out->null_count() == 0);
    CHECK((to_host<int64_t>(out->view()) == I64{3, 6, 9, 12, 9}));
  });
  run("min_periods for values: counted in VALID values, and never below 1", [&] {
    //                              window (2, 0):  {1} {1,n} {n,3} {3,n} {n,n}
    auto c = make_col<int32_t>({1, 77, 3, 88, 99}, {1, 0, 1, 0, 0});
    auto s1 = rolling_window(c->view(), 2, 0, 1, *sum_agg());
    CHECK((valid_host(s1->view()) == V{1, 1, 1, 1, 0}) && s1->null_count() == 1);
    auto h1 = to_host<int64_t>(s1->view());
    CHECK(h1[0] == 1 && h1[1] == 1 && h1[2] == 3 && h1[3] == 3);
    auto s0 = rolling_window(c->view(), 2, 0, 0, *sum_agg());  // min_periods 0: a window without a valid value is still null
    CHECK((valid_host(s0->view()) == V{1, 1, 1, 1, 0}));
    auto s2 = rolling_window(c->view(), 2, 0, 2, *max_agg());
    CHECK(s2->null_count() == 5 && s2->type().id() == type_id::INT32);
    auto d  = make_col<int32_t>({1, 2, 3, 0, 5}, {1, 1, 1, 0, 1});
    auto m2 = rolling_window(d->view(), 2, 0, 2, *min_agg());
    CHECK((valid_host(m2->view()) == V{0, 1, 1, 0, 0}));
    auto hm = to_host<int32_t>(m2->view());
    CHECK(hm[1] == 1 && hm[2] == 2);
  });
  run("min_periods for counts: counted in ROWS of the cut window; an empty window is a valid 0 only at min_periods 0", [&] {
    auto c  = make_col<int16_t>({5, 6, 7, 8}, {1, 0, 0, 1});
    auto cv = rolling_window(c->view(), 2, 1, 3, *count_valid_agg());  // sizes 2 3 3 2
    CHECK(cv->type().id() == type_id::INT32 && (valid_host(cv->view()) == V{0, 1, 1, 0}));
    auto hv = to_host<int32_t>(cv->view());
    CHECK(hv[1] == 1 && hv[2] == 1);
    auto ca = rolling_window(c->view(), 2, 1, 0, *count_all_agg());
    CHECK(!ca->nullable() && (to_host<int32_t>(ca->view()) == I32{2, 3, 3, 2}));
    auto e0 = rolling_window(c->view(), 2, -3, 0, *count_all_agg());  // preceding + following < 0: every window is empty
    CHECK(!e0->nullable() && (to_host<int32_t>(e0->view()) == I32{0, 0, 0, 0}));
    auto e1 = rolling_window(c->view(), 2, -3, 1, *count_valid_agg());
    CHECK(e1->null_count() == 4);
    auto es = rolling_window(c->view(), 2, -3, 0, *sum_agg());
    CHECK(es->null_count() == 4);
  });
  run("negative preceding / following: windows that do not hold their row", [&] {
    auto c   = make_col<int64_t>({10, 20, 30, 40, 50});
    auto lag = rolling_window(c->view(), 3, -1, 1, *sum_agg());  // rows [i - 2, i - 1]
    CHECK((valid_host(lag->view()) == V{0, 1, 1, 1, 1}));
    auto h = to_host<int64_t>(lag->view());
    CHECK(h[1] == 10 && h[2] == 30 && h[3] == 50 && h[4] == 70);
    auto lead = rolling_window(c->view(), -1, 3, 1, *max_agg());  // rows [i + 2, i + 3]
    CHECK((valid_host(lead->view()) == V{1, 1, 1, 0, 0}));
    auto g = to_host<int64_t>(lead->view());
    CHECK(g[0] == 40 && g[1] == 50 && g[2] == 50);
  });
  run("result types per (dtype, op)", [&] {
    auto u8  = make_col<uint8_t>({200, 100, 50});
    auto u64 = make_col<uint64_t>({~0ull, 2, 3});
    auto f32 = make_col<float>({1.5f, 2.5f, -1.0f});
    auto b8  = make_col<uint8_t>({1, 0, 1}, {}, type_id::BOOL8);
    auto s = rolling_window(u8->view(), 3, 0, 1, *sum_agg());
    CHECK(s->type().id() == type_id::INT64 && (to_host<int64_t>(s->view()) == I64{200, 300, 350}));
    auto su = rolling_window(u64->view(), 2, 0, 1, *sum_agg());  // wraps mod 2^64
    CHECK(su->type().id() == type_id::UINT64 && (to_host<uint64_t>(su->view()) == std::vector<uint64_t>{~0ull, 1, 5}));
    auto sf = rolling_window(f32->view(), 2, 0, 1, *sum_agg());
    CHECK(sf->type().id() == type_id::FLOAT32 && (to_host<float>(sf->view()) == std::vector<float>{1.5f, 4.0f, 1.5f}));
    auto sb = rolling_window(b8->view(), 3, 0, 1, *sum_agg());
    CHECK(sb->type().id() == type_id::INT64 && (to_host<int64_t>(sb->view()) == I64{1, 1, 2}));
    auto mn = rolling_window(u8->view(), 2, 0, 1, *min_agg());
    CHECK(mn->type().id() == type_id::UINT8 && (to_host<uint8_t>(mn->view()) == std::vector<uint8_t>{200, 100, 50}));
    auto mx = rolling_window(f32->view(), 1, 1, 1, *max_agg());
    CHECK(mx->type().id() == type_id::FLOAT32 && (to_host<float>(mx->view()) == std::vector<float>{2.5f, 2.5f, -1.0f}));
    auto me = rolling_window(u8->view(), 2, 0, 1, *mean_agg());
    CHECK(me->type().id() == type_id::FLOAT64 && (to_host<double>(me->view()) == F64{200., 150., 75.}));
    auto mu = rolling_window(u64->view(), 1, 0, 1, *mean_agg());
    CHECK(to_host<double>(mu->view())[0] == 18446744073709551616.0);
    auto mf = rolling_window(f32->view(), 2, 0, 1, *mean_agg());
    CHECK(mf->type().id() == type_id::FLOAT64 && (to_host<double>(mf->view()) == F64{1.5, 2.0, 0.75}));
    CHECK(rolling_window(f32->view(), 2, 0, 1, *count_valid_agg())->type().id() == type_id::INT32);
    CHECK(rolling_window(b8->view(), 2, 0, 1, *max_agg())->type().id() == type_id::BOOL8);
  });
  run("floats: NaN is the greatest value, inf and NaN follow plain addition window by window", [&] {
    auto inf = std::numeric_limits<double>::infinity();
    auto c   = make_col<double>({1., NaN, 3., inf, -inf, 6., 7.});
    auto mx  = to_host<double>(rolling_window(c->view(), 2, 0, 1, *max_agg())->view());
    CHECK(mx[0] == 1. && std::isnan(mx[1]) && std::isnan(mx[2]) && mx[3] == inf && mx[4] == inf && mx[5] == 6. && mx[6] == 7.);
    auto mn = to_host<double>(rolling_window(c->view(), 2, 0, 1, *min_agg())->view());
    CHECK(mn[0] == 1. && mn[1] == 1. && mn[2] == 3. && mn[3] == 3. && mn[4] == -inf && mn[5] == -inf && mn[6] == 6.);
    auto s = to_host<double>(rolling_window(c->view(), 2, 0, 1, *sum_agg())->view());
    CHECK(s[0] == 1. && std::isnan(s[1]) && std::isnan(s[2]) && s[3] == inf && std::isnan(s[4]) && s[5] == -inf && s[6] == 13.);
  });
  run("sliced views: nonzero offset on data and bitmap", [&] {
    //                 index: 0  1 | 2     3  4  5 | 6      the view is rows 2 .. 5: null 3 5 7
    auto c = make_col<int32_t>({9, 9, 1234, 3, 5, 7, 100}, {1, 1, 0, 1, 1, 1, 1});
    column_view sl{c->type(), 4, c->view().head<void>(), c->view().null_mask(), 1, 2};
    auto out = rolling_window(sl, 2, 1, 1, *sum_agg());
    CHECK(!out->nullable() && (to_host<int64_t>(out->view()) == I64{3, 8, 15, 12}));
    auto mn = rolling_window(sl, 1, 0, 1, *min_agg());
    CHECK((valid_host(mn->view()) == V{0, 1, 1, 1}) && mn->null_count() == 1);
    auto wp = make_col<int32_t>({0, 0, 1, 2, 1, 4, 0});
    auto wf = make_col<int32_t>({0, 0, 0, 0, 2, 0, 0});
    column_view sp{wp->type(), 4, wp->view().head<void>(), nullptr, 0, 2}, sf{wf->type(), 4, wf->view().head<void>(), nullptr, 0, 2};
    auto pr = rolling_window(sl, sp, sf, 1, *sum_agg());  // windows {null} {null,3} {5,7} {null..7}
    CHECK((valid_host(pr->view()) == V{0, 1, 1, 1}));
    auto hp = to_host<int64_t>(pr->view());
    CHECK(hp[1] == 3 && hp[2] == 12 && hp[3] == 15);
  });
  run("one window per row", [&] {
    auto c = make_col<int64_t>({1, 2, 4, 8, 16});
    auto p = make_col<int32_t>({1, 2, 1, 5, -1});
    auto f = make_col<int32_t>({0, 0, 2, 0, 9});
    auto out = rolling_window(c->view(), p->view(), f->view(), 1, *sum_agg());
    CHECK((valid_host(out->view()) == V{1, 1, 1, 1, 0}));
    auto h = to_host<int64_t>(out->view());
    CHECK(h[0] == 1 && h[1] == 3 && h[2] == 28 && h[3] == 15);
  });
  run("grouped: windows stop at the group; two key columns of mixed types with nulls; no key columns = ungrouped", [&] {
    // groups:                    (1, a) (1, a) (1, a) | (1, null) (1, null) | (2, null) | (2, b) (2, b)
    auto k0 = make_col<int8_t>({1, 1, 1, 1, 1, 2, 2, 2});
    auto k1 = make_col<double>({.5, .5, .5, 7., 8., 9., 2., 2.}, {1, 1, 1, 0, 0, 0, 1, 1});
    auto c  = make_col<int32_t>({1, 2, 3, 10, 20, 100, 1000, 2000});
    auto out = grouped_rolling_window(table_view{{k0->view(), k1->view()}}, c->view(), 2, 1, 1, *sum_agg());
    CHECK((to_host<int64_t>(out->view()) == I64{3, 6, 5, 30, 30, 100, 3000, 3000}));
    auto cnt = grouped_rolling_window(table_view{{k0->view(), k1->view()}}, c->view(), 2, 1, 3, *count_all_agg());
    CHECK((valid_host(cnt->view()) == V{0, 1, 0, 0, 0, 0, 0, 0}));
    auto one = grouped_rolling_window(table_view{{k0->view()}}, c->view(), 3, 0, 1, *max_agg());
    CHECK((to_host<int32_t>(one->view()) == I32{1, 2, 3, 10, 20, 100, 1000, 2000}));
    auto none = grouped_rolling_window(table_view{}, c->view(), 2, 1, 1, *sum_agg());
    CHECK((to_host<int64_t>(none->view()) == I64{3, 6, 15, 33, 130, 1120, 3100, 3000}));
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
