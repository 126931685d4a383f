// Row filtering through the C++ surface: cudf::apply_boolean_mask / drop_nulls / drop_nans (include/cudf/stream_compaction.hpp).
// Expected values are computed on the host from the same vectors (the reference's suites check the same contract:
// apply_boolean_mask_tests.cpp, drop_nulls_tests.cpp, drop_nans_tests.cpp).  The minimal harness of cudf_api_tests.cpp.
//   cudf_compaction_tests --host   argument checks only: everything decided before the first device call, runs without a GPU
//   cudf_compaction_tests          the whole list; needs a GPU (tests/test_gpu_compaction.py)
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
std::unique_ptr<column> make_bool(std::vector<uint8_t> const& v, std::vector<int> const& valid = {})
{
  return make_col<uint8_t>(v, valid, type_id::BOOL8);
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

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake      = reinterpret_cast<void const*>(0x10000);
  auto const* fake_mask = reinterpret_cast<bitmask_type const*>(0x20000);
  run("apply_boolean_mask argument checks (apply_boolean_mask: Column size mismatch / Mask must be Boolean type)", [&] {
    column_view a{data_type{type_id::INT32}, 5, fake, nullptr, 0};
    column_view m_short{data_type{type_id::BOOL8}, 4, fake, nullptr, 0};
    column_view m_int{data_type{type_id::INT8}, 5, fake, nullptr, 0};
    CHECK(throws<cudf::logic_error>([&] { (void)apply_boolean_mask(table_view{{a}}, m_short); }));
    CHECK(throws<cudf::logic_error>([&] { (void)apply_boolean_mask(table_view{{a}}, m_int); }));
  });
  run("drop_nulls / drop_nans argument checks (table_view::select; drop_nans: Key column is not of floating-point type)", [&] {
    column_view a{data_type{type_id::INT32}, 5, fake, fake_mask, 1};
    column_view f{data_type{type_id::FLOAT64}, 5, fake, nullptr, 0};
    table_view t{{a, f}};
    CHECK(throws<std::out_of_range>([&] { (void)drop_nulls(t, {2}); }));
    CHECK(throws<std::out_of_range>([&] { (void)drop_nulls(t, {0, -1}, 1); }));
    CHECK(throws<std::out_of_range>([&] { (void)drop_nans(t, {1, 7}); }));
    CHECK(throws<cudf::logic_error>([&] { (void)drop_nans(t, {0}); }));
    CHECK(throws<cudf::logic_error>([&] { (void)drop_nans(t, {1, 0}, 1); }));
    CHECK(throws<std::invalid_argument>([&] { (void)drop_nulls(t, {0}, -1); }));
    CHECK(throws<std::invalid_argument>([&] { (void)drop_nans(t, {1}, -1); }));
  });
}

template <typename T>
std::vector<T> filter(std::vector<T> const& v, std::vector<int> const& keep)
{
  std::vector<T> o;
  for (std::size_t i = 0; i < v.size(); ++i)
    if (keep[i]) o.push_back(v[i]);
  return o;
}

static void device_cases()
{
  constexpr double NaN = std::numeric_limits<double>::quiet_NaN();
  constexpr double Inf = std::numeric_limits<double>::infinity();

  run("apply_boolean_mask: mixed widths from one plan, nullable column, bytes other than 0 / 1", [] {
    std::vector<int64_t> a{10, -20, 30, -40, 50, -60, 70, -80, 90, -100};
    std::vector<int16_t> b{1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
    std::vector<double> c{0.5, -0.0, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5};
    std::vector<int> cv{1, 1, 0, 1, 1, 1, 0, 1, 1, 1};
    std::vector<uint8_t> m{1, 0, 7, 0, 0, 255, 1, 0, 1, 2};
    std::vector<int> keep{1, 0, 1, 0, 0, 1, 1, 0, 1, 1};
    auto ca = make_col(a);
    auto cb = make_col(b);
    auto cc = make_col(c, cv);
    auto cm = make_bool(m);
    auto out = apply_boolean_mask(table_view{{ca->view(), cb->view(), cc->view()}}, cm->view());
    CHECK(out->num_columns() == 3 && out->num_rows() == 6);
    CHECK(same_bits(to_host<int64_t>(out->get_column(0).view()), filter(a, keep)));
    CHECK(same_bits(to_host<int16_t>(out->get_column(1).view()), filter(b, keep)));
    CHECK(same_bits(to_host<double>(out->get_column(2).view()), filter(c, keep)));
    CHECK(!out->get_column(0).nullable() && !out->get_column(1).nullable());
    CHECK(out->get_column(2).null_count() == 2);
    CHECK(valid_host(out->get_column(2).view()) == filter(cv, keep));
    CHECK(out->get_column(2).type().id() == type_id::FLOAT64 && out->get_column(1).type().id() == type_id::INT16);
  });
  run("apply_boolean_mask: a null mask element drops its row; a column whose nulls are all dropped loses its mask", [] {
    std::vector<int32_t> a{1, 2, 3, 4, 5, 6};
    std::vector<int> av{1, 0, 1, 1, 0, 1};
    std::vector<uint8_t> m{1, 1, 1, 0, 1, 1};
    std::vector<int> mv{1, 0, 1, 1, 0, 0};
    auto ca = make_col(a, av);
    auto cm = make_bool(m, mv);
    auto out = apply_boolean_mask(table_view{{ca->view()}}, cm->view());
    CHECK((to_host<int32_t>(out->get_column(0).view()) == std::vector<int32_t>{1, 3}));
    CHECK(out->get_column(0).null_count() == 0 && !out->get_column(0).nullable());
  });
  run("apply_boolean_mask: sliced views with a non-zero offset (data, validity and mask)", [] {
    std::size_t const N = 300, off = 37;
    std::vector<int64_t> a(N);
    std::vector<int> av(N), mv(N);
    std::vector<uint8_t> m(N);
    for (std::size_t i = 0; i < N; ++i) {
      a[i]  = static_cast<int64_t>(i * i) - 1000;
      av[i] = (i % 5) != 0;
      m[i]  = (i * 7 % 3) != 0;
      mv[i] = (i % 11) != 3;
    }
    auto ca = make_col(a, av);
    auto cm = make_bool(m, mv);
    auto const n = static_cast<size_type>(N - off - 13);
    size_type a_nulls = 0, m_nulls = 0;
    for (std::size_t i = off; i < off + static_cast<std::size_t>(n); ++i) {
      a_nulls += !av[i];
      m_nulls += !mv[i];
    }
    column_view sa{ca->type(), n, ca->view().head<void>(), ca->view().null_mask(), a_nulls, static_cast<size_type>(off)};
    column_view sm{cm->type(), n, cm->view().head<void>(), cm->view().null_mask(), m_nulls, static_cast<size_type>(off)};
    std::vector<int64_t> ea;
    std::vector<int> ev;
    for (std::size_t i = off; i < off + static_cast<std::size_t>(n); ++i)
      if (m[i] && mv[i]) {
        ea.push_back(a[i]);
        ev.push_back(av[i]);
      }
    auto out = apply_boolean_mask(table_view{{sa}}, sm);
    CHECK(!ea.empty() && ea.size() < static_cast<std::size_t>(n));
    CHECK(same_bits(to_host<int64_t>(out->get_column(0).view()), ea));
    CHECK(valid_host(out->get_column(0).view()) == ev);
    size_type nulls = 0;
    for (auto v : ev) nulls += !v;
    CHECK(out->get_column(0).null_count() == nulls);
  });
  run("apply_boolean_mask: empty tables, empty mask, nothing kept, everything kept", [] {
    auto e  = make_col<int32_t>({});
    auto em = make_bool({});
    auto o0 = apply_boolean_mask(table_view{{e->view()}}, em->view());
    CHECK(o0->num_columns() == 1 && o0->num_rows() == 0 && o0->get_column(0).type().id() == type_id::INT32);
    auto o1 = apply_boolean_mask(table_view{}, em->view());
    CHECK(o1->num_columns() == 0 && o1->num_rows() == 0);
    auto a    = make_col<float>({1.f, 2.f, 3.f});
    auto none = make_bool({0, 0, 0});
    auto all  = make_bool({1, 1, 1});
    auto o2   = apply_boolean_mask(table_view{{a->view()}}, none->view());
    CHECK(o2->num_rows() == 0 && o2->get_column(0).type().id() == type_id::FLOAT32);
    auto o3 = apply_boolean_mask(table_view{{a->view()}}, all->view());
    CHECK((to_host<float>(o3->get_column(0).view()) == std::vector<float>{1.f, 2.f, 3.f}));
    CHECK(throws<cudf::logic_error>([&] { (void)apply_boolean_mask(table_view{{a->view()}}, make_bool({1, 0})->view()); }));
    CHECK(throws<cudf::logic_error>([&] { (void)apply_boolean_mask(table_view{{a->view()}}, make_col<int8_t>({1, 0, 1})->view()); }));
  });
  run("drop_nulls: thresholds 0 .. len(keys) + 1 over two key columns, keys without nulls return the input", [] {
    std::vector<int32_t> a{1, 2, 3, 4, 5, 6, 7, 8};
    std::vector<int> av{1, 0, 1, 0, 1, 1, 0, 1};
    std::vector<double> b{.1, .2, .3, .4, .5, .6, .7, .8};
    std::vector<int> bv{1, 1, 0, 0, 1, 1, 1, 0};
    std::vector<int64_t> c{11, 12, 13, 14, 15, 16, 17, 18};
    auto ca = make_col(a, av);
    auto cb = make_col(b, bv);
    auto cc = make_col(c);
    table_view t{{ca->view(), cb->view(), cc->view()}};
    for (size_type thr = 0; thr <= 3; ++thr) {
      std::vector<int> keep(a.size());
      for (std::size_t i = 0; i < a.size(); ++i) keep[i] = (av[i] + bv[i]) >= thr;
      auto out = drop_nulls(t, {0, 1}, thr);
      CHECK(same_bits(to_host<int64_t>(out->get_column(2).view()), filter(c, keep)));
      CHECK(same_bits(to_host<int32_t>(out->get_column(0).view()), filter(a, keep)));
      if (out->num_rows()) CHECK(valid_host(out->get_column(0).view()) == filter(av, keep));
      if (out->num_rows()) CHECK(valid_host(out->get_column(1).view()) == filter(bv, keep));
    }
    auto d = drop_nulls(t, {0, 1});  // threshold = 2
    CHECK((to_host<int64_t>(d->get_column(2).view()) == std::vector<int64_t>{11, 15, 16}));
    CHECK(d->get_column(0).null_count() == 0 && !d->get_column(0).nullable());
    auto same = drop_nulls(t, {2}, 5);  // the key holds no null: a copy, whatever the threshold
    CHECK(same->num_rows() == 8 && same->get_column(0).null_count() == 3);
    auto nokeys = drop_nulls(t, {});
    CHECK(nokeys->num_rows() == 8);
    CHECK(throws<std::out_of_range>([&] { (void)drop_nulls(t, {3}); }));
  });
  run("drop_nans: f32 and f64 keys, +-Inf kept, a null element is not a NaN", [&] {
    std::vector<double> a{1.0, NaN, Inf, -Inf, -NaN, 5.0, NaN, -0.0};
    std::vector<int> av{1, 1, 1, 1, 1, 1, 0, 1};  // row 6: a null whose bytes are a NaN
    std::vector<float> b{1.f, 2.f, std::nanf(""), 4.f, std::nanf(""), 6.f, 7.f, 8.f};
    std::vector<int32_t> c{0, 1, 2, 3, 4, 5, 6, 7};
    auto ca = make_col(a, av);
    auto cb = make_col(b);
    auto cc = make_col(c);
    table_view t{{ca->view(), cb->view(), cc->view()}};
    auto o = drop_nans(t, {0});
    CHECK((to_host<int32_t>(o->get_column(2).view()) == std::vector<int32_t>{0, 2, 3, 5, 6, 7}));
    CHECK(o->get_column(0).null_count() == 1);
    auto o2 = drop_nans(t, {0, 1});
    CHECK((to_host<int32_t>(o2->get_column(2).view()) == std::vector<int32_t>{0, 3, 5, 6, 7}));
    auto o3 = drop_nans(t, {0, 1}, 1);
    CHECK((to_host<int32_t>(o3->get_column(2).view()) == std::vector<int32_t>{0, 1, 2, 3, 5, 6, 7}));
    auto o4 = drop_nans(t, {0, 1}, 3);
    CHECK(o4->num_rows() == 0 && o4->num_columns() == 3 && o4->get_column(1).type().id() == type_id::FLOAT32);
    CHECK(throws<cudf::logic_error>([&] { (void)drop_nans(t, {2}); }));
    CHECK(throws<std::out_of_range>([&] { (void)drop_nans(t, {5}); }));
    CHECK(drop_nans(t, {})->num_rows() == 8);
  });
  run("apply_boolean_mask: 100 003 rows of every width against the host, chunk edges included", [] {
    std::size_t const N = 100003;
    std::vector<int8_t> a(N);
    std::vector<int32_t> b(N);
    std::vector<int64_t> c(N);
    std::vector<uint8_t> m(N);
    std::vector<int> keep(N), cv(N);
    uint64_t s = 12345;
    for (std::size_t i = 0; i < N; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      a[i] = static_cast<int8_t>(s >> 56);
      b[i] = static_cast<int32_t>(s >> 20);
      c[i] = static_cast<int64_t>(s);
      m[i] = ((s >> 33) & 1) && (i / 5000) % 3 != 1;  // random halves with whole chunks dropped in between
      keep[i] = m[i];
      cv[i]   = ((s >> 40) % 7) != 0;
    }
    auto ca = make_col(a);
    auto cb = make_col(b);
    auto cc = make_col(c, cv);
    auto cm = make_bool(m);
    auto out = apply_boolean_mask(table_view{{ca->view(), cb->view(), cc->view()}}, cm->view());
    CHECK(same_bits(to_host<int8_t>(out->get_column(0).view()), filter(a, keep)));
    CHECK(same_bits(to_host<int32_t>(out->get_column(1).view()), filter(b, keep)));
    CHECK(same_bits(to_host<int64_t>(out->get_column(2).view()), filter(c, keep)));
    CHECK(valid_host(out->get_column(2).view()) == filter(cv, keep));
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
