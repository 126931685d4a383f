// cudf::quantile, cudf::quantiles (include/cudf/quantiles.hpp), the MEDIAN / QUANTILE reductions and groupby aggregations through
// the C++ surface.  Small literal vectors, expected values written out by hand (every LINEAR case below has an exact double result).
// The minimal harness of cudf_reshape_tests.cpp.
//   cudf_quantile_tests --host   what is decided before the first device call: the throws and the empty results; runs without
//                                a GPU (tests/test_quantile_host.py)
//   cudf_quantile_tests          the whole list; needs a GPU (tests/test_gpu_quantile.py)
#include <cudf/aggregation.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/groupby.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/quantiles.hpp>
#include <cudf/reduction.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/sorting.hpp>

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

using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
using F32 = std::vector<float>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
static data_type dt(type_id id) { return data_type{id}; }

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view bool5{dt(type_id::BOOL8), 5, fake, nullptr, 0};
  column_view s5{dt(type_id::STRING), 5, fake, nullptr, 0};
  column_view idx4{dt(type_id::INT32), 4, fake, nullptr, 0};
  column_view idx64{dt(type_id::INT64), 5, fake, nullptr, 0};
  column_view e64{dt(type_id::FLOAT64), 0, nullptr, nullptr, 0};
  run("quantile of BOOL8 or of a non-numeric column throws data_type_error", [&] {
    CHECK(throws<cudf::data_type_error>([&] { (void)quantile(bool5, {0.5}); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)quantile(s5, {0.5}); }));
  });
  run("quantile with ordered_indices of another size or type throws invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)quantile(a5, {0.5}, interpolation::LINEAR, idx4); }));
    CHECK(throws<std::invalid_argument>([&] { (void)quantile(a5, {0.5}, interpolation::LINEAR, idx64); }));
    CHECK(throws<std::invalid_argument>([&] { (void)quantile(a5, {std::nan("")}); }));
  });
  run("quantile with an empty q is an empty column of the result type", [&] {
    auto r = quantile(a5, {});
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT64);
    auto s = quantile(a5, {}, interpolation::LOWER, {}, false);
    CHECK(s->size() == 0 && s->type().id() == type_id::INT32);
  });
  run("quantiles with an arithmetic interpolation throws", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)quantiles(table_view{{a5}}, {0.5}, interpolation::LINEAR); }));
    CHECK(throws<std::invalid_argument>([&] { (void)quantiles(table_view{{a5}}, {0.5}, interpolation::MIDPOINT); }));
  });
  run("quantiles of a table without rows throws", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)quantiles(table_view{{e64}}, {0.5}); }));
  });
  run("reduce QUANTILE takes exactly one quantile; MEDIAN of BOOL8 throws", [&] {
    CHECK(throws<std::invalid_argument>(
      [&] { (void)reduce(a5, *make_quantile_aggregation<reduce_aggregation>({0.25, 0.75}), dt(type_id::FLOAT64)); }));
    CHECK(throws<std::invalid_argument>([&] { (void)reduce(a5, *make_quantile_aggregation<reduce_aggregation>({}), dt(type_id::FLOAT64)); }));
    CHECK(throws<cudf::data_type_error>([&] { (void)reduce(bool5, *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64)); }));
  });
  run("quantile aggregations compare, hash and clone by kind, quantiles and interpolation", [&] {
    auto a = make_quantile_aggregation<groupby_aggregation>({0.25, 0.75}, interpolation::LOWER);
    auto b = make_quantile_aggregation<groupby_aggregation>({0.25, 0.75}, interpolation::LOWER);
    auto c = make_quantile_aggregation<groupby_aggregation>({0.25, 0.5}, interpolation::LOWER);
    auto d = make_quantile_aggregation<groupby_aggregation>({0.25, 0.75}, interpolation::HIGHER);
    auto m = make_median_aggregation<groupby_aggregation>();
    auto q5 = make_quantile_aggregation<groupby_aggregation>({0.5});
    CHECK(a->kind == aggregation::QUANTILE && m->kind == aggregation::MEDIAN);
    CHECK(a->is_equal(*b) && a->do_hash() == b->do_hash());
    CHECK(!a->is_equal(*c) && !a->is_equal(*d) && !m->is_equal(*q5));
    auto cl = a->clone();
    CHECK(cl->is_equal(*a) && cl->kind == aggregation::QUANTILE);
    auto plain = make_median_aggregation();
    CHECK(plain->kind == aggregation::MEDIAN);
  });
}

static bool same(std::vector<double> const& a, std::vector<double> const& b)
{
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static void device_cases()
{
  run("quantile on sorted input: every interpolation", [] {
    auto c = make_col<double>({1.0, 2.0, 4.0, 8.0, 16.0});
    std::vector<double> q{0.0, 0.125, 0.5, 0.625, 1.0};  // pos = 0, 0.5, 2, 2.5, 4
    CHECK(same(to_host<double>(quantile(c->view(), q, interpolation::LINEAR)->view()), {1.0, 1.5, 4.0, 6.0, 16.0}));
    CHECK(same(to_host<double>(quantile(c->view(), q, interpolation::LOWER)->view()), {1.0, 1.0, 4.0, 4.0, 16.0}));
    CHECK(same(to_host<double>(quantile(c->view(), q, interpolation::HIGHER)->view()), {1.0, 2.0, 4.0, 8.0, 16.0}));
    CHECK(same(to_host<double>(quantile(c->view(), q, interpolation::MIDPOINT)->view()), {1.0, 1.5, 4.0, 6.0, 16.0}));
    CHECK(same(to_host<double>(quantile(c->view(), q, interpolation::NEAREST)->view()), {1.0, 1.0, 4.0, 4.0, 16.0}));  // ties to even
    CHECK(same(to_host<double>(quantile(c->view(), {-1.0, 7.0})->view()), {1.0, 16.0}));                                // clamped
  });
  run("quantile does not sort; ordered_indices gives the order", [] {
    auto c   = make_col<int32_t>({40, 10, 30, 20});
    auto idx = make_col<int32_t>({1, 3, 2, 0});
    CHECK(same(to_host<double>(quantile(c->view(), {0.5})->view()), {20.0}));                                          // (10 + 30) / 2 as stored
    CHECK(same(to_host<double>(quantile(c->view(), {0.5}, interpolation::LINEAR, idx->view())->view()), {25.0}));
    CHECK(same(to_host<double>(quantile(c->view(), {0.0, 1.0}, interpolation::LOWER, idx->view())->view()), {10.0, 40.0}));
  });
  run("quantile of a sliced view", [] {
    auto c = make_col<int64_t>({-99, -98, 1, 2, 3, 4, 5, 99}, {1, 0, 1, 1, 1, 1, 0, 1});
    auto s = slice(c->view(), {2, 6})[0];  // 1 2 3 4, all valid
    CHECK(same(to_host<double>(quantile(s, {0.5, 1.0})->view()), {2.5, 4.0}));
    auto t = slice(c->view(), {1, 7})[0];  // null 1 2 3 4 null
    auto r = quantile(t, {0.0, 0.5, 1.0}, interpolation::LOWER);
    CHECK(valid_host(r->view()) == V({0, 1, 0}) && r->null_count() == 2);
    CHECK(to_host<double>(r->view())[1] == 2.0);
  });
  run("quantile with nulls: a result is null when a row it reads is null", [] {
    auto c = make_col<double>({1.0, 2.0, 3.0, 4.0}, {1, 1, 0, 1});
    auto r = quantile(c->view(), {0.0, 0.5, 1.0 / 3.0, 1.0});  // rows 0; 1 and 2; 1; 3
    CHECK(valid_host(r->view()) == V({1, 0, 1, 1}) && r->null_count() == 1);
    auto h = to_host<double>(r->view());
    CHECK(h[0] == 1.0 && h[2] == 2.0 && h[3] == 4.0);
    auto lo = quantile(c->view(), {0.5}, interpolation::LOWER);
    CHECK(lo->null_count() == 0 && to_host<double>(lo->view())[0] == 2.0);
  });
  run("quantile with exact false keeps the type", [] {
    auto c = make_col<int32_t>({1, 2, 4, 9});
    auto r = quantile(c->view(), {0.5, 0.9}, interpolation::LINEAR, {}, false);  // 3.0 ; 0.3 * 4 + 0.7 * 9 = 7.5 -> 7
    CHECK(r->type().id() == type_id::INT32 && to_host<int32_t>(r->view()) == I32({3, 7}));
    auto f = make_col<float>({1.0f, 2.0f});
    auto g = quantile(f->view(), {0.5, 1.0}, interpolation::MIDPOINT, {}, false);
    CHECK(g->type().id() == type_id::FLOAT32 && to_host<float>(g->view()) == F32({1.5f, 2.0f}));
    auto hi = quantile(c->view(), {0.5}, interpolation::HIGHER, {}, false);
    CHECK(to_host<int32_t>(hi->view()) == I32({4}));
  });
  run("quantile of an empty column is q.size() nulls; more than 64 quantiles", [] {
    auto e = make_col<double>({});
    auto r = quantile(e->view(), {0.1, 0.9});
    CHECK(r->size() == 2 && r->null_count() == 2 && r->type().id() == type_id::FLOAT64);
    std::vector<double> v(101), q(101);
    for (int i = 0; i <= 100; ++i) {
      v[i] = i * 2.0;
      q[i] = i / 100.0;
    }
    auto c = make_col<double>(v);
    auto h = to_host<double>(quantile(c->view(), q, interpolation::NEAREST)->view());
    for (int i = 0; i <= 100; ++i) CHECK(h[i] == v[i]);
  });
  run("quantiles: rows at lower / higher / nearest", [] {
    auto a = make_col<int32_t>({3, 1, 2, 1, 3});
    auto b = make_col<double>({0.5, 9.0, 7.0, 8.0, 0.25});
    table_view t{{a->view(), b->view()}};  // sorted: (1,8) (1,9) (2,7) (3,.25) (3,.5)
    auto lo = quantiles(t, {0.0, 0.6, 1.0}, interpolation::LOWER);     // pos 0, 2.4, 4
    CHECK(to_host<int32_t>(lo->get_column(0).view()) == I32({1, 2, 3}) && to_host<double>(lo->get_column(1).view()) == F64({8.0, 7.0, 0.5}));
    auto hi = quantiles(t, {0.6}, interpolation::HIGHER);
    CHECK(to_host<int32_t>(hi->get_column(0).view()) == I32({3}) && to_host<double>(hi->get_column(1).view()) == F64({0.25}));
    auto ne = quantiles(t, {0.6, 0.125});                              // nearest of 2.4 -> 2; of 0.5 -> 0 (ties to even)
    CHECK(to_host<double>(ne->get_column(1).view()) == F64({7.0, 8.0}));
  });
  run("quantiles: pre-sorted input, descending order, nulls before", [] {
    auto a = make_col<int32_t>({5, 6, 7, 8});
    auto pre = quantiles(table_view{{a->view()}}, {0.0, 1.0}, interpolation::LOWER, sorted::YES);
    CHECK(to_host<int32_t>(pre->get_column(0).view()) == I32({5, 8}));
    auto un = make_col<int32_t>({7, 5, 8, 6});
    auto asis = quantiles(table_view{{un->view()}}, {0.0, 1.0}, interpolation::LOWER, sorted::YES);  // taken as it stands
    CHECK(to_host<int32_t>(asis->get_column(0).view()) == I32({7, 6}));
    auto desc = quantiles(table_view{{un->view()}}, {0.0, 1.0}, interpolation::LOWER, sorted::NO, {order::DESCENDING});
    CHECK(to_host<int32_t>(desc->get_column(0).view()) == I32({8, 5}));
    auto n = make_col<int32_t>({7, 5, 8, 6}, {1, 0, 1, 1});
    auto nb = quantiles(table_view{{n->view()}}, {0.0, 1.0}, interpolation::LOWER, sorted::NO, {order::ASCENDING}, {null_order::BEFORE});
    CHECK(valid_host(nb->get_column(0).view()) == V({0, 1}) && to_host<int32_t>(nb->get_column(0).view())[1] == 8);
    auto na = quantiles(table_view{{n->view()}}, {0.0, 1.0}, interpolation::LOWER, sorted::NO, {order::ASCENDING}, {null_order::AFTER});
    CHECK(valid_host(na->get_column(0).view()) == V({1, 0}) && to_host<int32_t>(na->get_column(0).view())[0] == 6);
  });
  run("reduce MEDIAN and QUANTILE on an unsorted column", [] {
    auto c = make_col<int32_t>({9, 1, 4, 2, 16});  // sorted 1 2 4 9 16
    auto m = reduce(c->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(m->is_valid() && static_cast<numeric_scalar<double>&>(*m).value() == 4.0);
    auto q = reduce(c->view(), *make_quantile_aggregation<reduce_aggregation>({0.125}), dt(type_id::FLOAT64));  // pos 0.5
    CHECK(q->is_valid() && static_cast<numeric_scalar<double>&>(*q).value() == 1.5);
    auto hi = reduce(c->view(), *make_quantile_aggregation<reduce_aggregation>({0.625}, interpolation::HIGHER), dt(type_id::FLOAT64));
    CHECK(static_cast<numeric_scalar<double>&>(*hi).value() == 9.0);
    std::vector<double> big(5000);
    for (int i = 0; i < 5000; ++i) big[i] = static_cast<double>((i * 7919) % 5000);  // a permutation of 0 .. 4999
    auto b = make_col<double>(big);
    auto bm = reduce(b->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(static_cast<numeric_scalar<double>&>(*bm).value() == 2499.5);
  });
  run("reduce MEDIAN with nulls, with no valid row, with output_type INT32", [] {
    auto c = make_col<double>({100.0, 1.0, -5.0, 3.0, 2.0}, {0, 1, 0, 1, 1});  // valid 1 3 2
    auto m = reduce(c->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(m->is_valid() && static_cast<numeric_scalar<double>&>(*m).value() == 2.0);
    auto s = slice(c->view(), {1, 4})[0];  // 1 null 3
    auto sm = reduce(s, *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(sm->is_valid() && static_cast<numeric_scalar<double>&>(*sm).value() == 2.0);
    auto none = make_col<double>({1.0, 2.0}, {0, 0});
    auto nm   = reduce(none->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(!nm->is_valid());
    auto e  = make_col<int32_t>({});
    auto em = reduce(e->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64));
    CHECK(!em->is_valid());
    auto i  = make_col<int32_t>({7, 1, 4, 2});  // median 3.0
    auto im = reduce(i->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::INT32));
    CHECK(im->type().id() == type_id::INT32 && im->is_valid() && static_cast<numeric_scalar<int32_t>&>(*im).value() == 3);
    auto with_init = numeric_scalar<int32_t>(1);
    CHECK(throws<std::invalid_argument>([&] {
      (void)reduce(i->view(), *make_median_aggregation<reduce_aggregation>(), dt(type_id::FLOAT64), std::cref(static_cast<scalar const&>(with_init)));
    }));
  });
  run("groupby MEDIAN and QUANTILE {0.25, 0.75} with null keys and values, group-major", [] {
    //            key:   2    1    2   null  1    3    2    1    3    2
    auto keys = make_col<int32_t>({2, 1, 2, 0, 1, 3, 2, 1, 3, 2}, {1, 1, 1, 0, 1, 1, 1, 1, 1, 1});
    auto vals = make_col<double>({8.0, 5.0, 0.0, 77.0, 1.0, 9.0, 4.0, 3.0, 9.0, 16.0}, {1, 1, 1, 1, 1, 0, 1, 0, 0, 1});
    // group 1: valid {5, 1} -> sorted 1 5;  group 2: {8, 0, 4, 16} -> 0 4 8 16;  group 3: no valid value
    groupby::groupby gb{table_view{{keys->view()}}};
    std::vector<groupby::aggregation_request> reqs(1);
    reqs[0].values = vals->view();
    reqs[0].aggregations.emplace_back(make_median_aggregation<groupby_aggregation>());
    reqs[0].aggregations.emplace_back(make_quantile_aggregation<groupby_aggregation>({0.25, 0.75}));
    reqs[0].aggregations.emplace_back(make_quantile_aggregation<groupby_aggregation>({0.5}, interpolation::HIGHER));
    auto [k, res] = gb.aggregate(reqs);
    CHECK(k->num_rows() == 3 && to_host<int32_t>(k->get_column(0).view()) == I32({1, 2, 3}));
    auto const& med = *res[0].results[0];
    CHECK(med.type().id() == type_id::FLOAT64 && med.size() == 3 && valid_host(med.view()) == V({1, 1, 0}) && med.null_count() == 1);
    auto mh = to_host<double>(med.view());
    CHECK(mh[0] == 3.0 && mh[1] == 6.0);
    auto const& qu = *res[0].results[1];
    CHECK(qu.size() == 6 && valid_host(qu.view()) == V({1, 1, 1, 1, 0, 0}) && qu.null_count() == 2);
    auto qh = to_host<double>(qu.view());
    CHECK(qh[0] == 2.0 && qh[1] == 4.0 && qh[2] == 3.0 && qh[3] == 10.0);  // group 1: 1 + .25 * 4, 1 + .75 * 4; group 2: pos .75, 2.25
    auto hh = to_host<double>(res[0].results[2]->view());
    CHECK(hh[0] == 5.0 && hh[1] == 8.0);
    // null keys kept (sort path with null_policy::INCLUDE): the null key's group is last, its one value 77
    groupby::groupby gbn{table_view{{keys->view()}}, null_policy::INCLUDE};
    std::vector<groupby::aggregation_request> r2(1);
    r2[0].values = vals->view();
    r2[0].aggregations.emplace_back(make_median_aggregation<groupby_aggregation>());
    auto [k2, res2] = gbn.aggregate(r2);
    CHECK(k2->num_rows() == 4);
    auto m2 = to_host<double>(res2[0].results[0]->view());
    CHECK(valid_host(res2[0].results[0]->view()) == V({1, 1, 0, 1}) && m2[3] == 77.0 && m2[0] == 3.0);
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
