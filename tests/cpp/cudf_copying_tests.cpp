// cudf::concatenate / concatenate_masks, scatter, copy_if_else, slice and split through the C++ surface (include/cudf/copying.hpp,
// include/cudf/concatenate.hpp).  Small literal vectors, expected values written out by hand; the inputs are sliced views made by
// cudf::slice wherever a function takes views.  The minimal harness of cudf_merge_tests.cpp.
//   cudf_copying_tests --host   what is decided before the first device call: the throws, the size_type overflow, slice index
//                               validation, empty results; runs without a GPU
//   cudf_copying_tests          the whole list; needs a GPU (tests/test_gpu_copying.py)
#include <cudf/column/column_factories.hpp>
#include <cudf/concatenate.hpp>
#include <cudf/copying.hpp>
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
template <typename T>
std::vector<T> to_host(column_view const& c)
{
  std::vector<T> h(c.size());
  if (c.size()) (void)hipMemcpy(h.data(), c.data<T>(), h.size() * sizeof(T), hipMemcpyDeviceToHost);
  return h;
}
std::vector<int> bits_host(bitmask_type const* mask, size_type offset, size_type n)
{
  std::vector<int> v(n, 1);
  if (!mask) return v;
  std::vector<bitmask_type> w(num_bitmask_words(n + offset));
  if (!w.empty()) (void)hipMemcpy(w.data(), mask, w.size() * 4, hipMemcpyDeviceToHost);
  for (size_type i = 0; i < n; ++i) v[i] = (w[(i + offset) / 32] >> ((i + offset) % 32)) & 1;
  return v;
}
std::vector<int> valid_host(column_view const& c) { return bits_host(c.null_mask(), c.offset(), c.size()); }
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
using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
using CV  = std::vector<column_view>;

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake      = reinterpret_cast<void const*>(0x10000);
  auto const* fake_mask = reinterpret_cast<bitmask_type const*>(0x20000);
  column_view a{data_type{type_id::INT32}, 5, fake, nullptr, 0};
  column_view b64{data_type{type_id::INT64}, 5, fake, nullptr, 0};
  column_view map3{data_type{type_id::INT32}, 3, fake, nullptr, 0};
  column_view bool5{data_type{type_id::BOOL8}, 5, fake, nullptr, 0};
  run("concatenate: an empty span throws", [&] {
    CV none;
    std::vector<table_view> no_tables;
    CHECK(throws<std::invalid_argument>([&] { (void)concatenate(host_span<column_view const>{none}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)concatenate(host_span<table_view const>{no_tables}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)concatenate_masks(host_span<column_view const>{none}); }));
  });
  run("concatenate: differing types throw cudf::data_type_error, differing column counts cudf::logic_error", [&] {
    CV mixed{a, b64};
    CHECK(throws<data_type_error>([&] { (void)concatenate(host_span<column_view const>{mixed}); }));
    std::vector<table_view> tabs{table_view{{a, a}}, table_view{{a}}};
    CHECK(throws<logic_error>([&] { (void)concatenate(host_span<table_view const>{tabs}); }));
    std::vector<table_view> tabs2{table_view{{a, a}}, table_view{{a, b64}}};
    CHECK(throws<data_type_error>([&] { (void)concatenate(host_span<table_view const>{tabs2}); }));
  });
  run("concatenate: more rows than size_type holds throw std::overflow_error before any device call", [&] {
    column_view big{data_type{type_id::INT8}, (1 << 30) + 5, fake, nullptr, 0};
    CV two{big, big};
    CHECK(throws<std::overflow_error>([&] { (void)concatenate(host_span<column_view const>{two}); }));
    CHECK(throws<std::overflow_error>([&] { (void)concatenate_masks(host_span<column_view const>{two}); }));
    std::vector<table_view> tabs{table_view{{big}}, table_view{{big}}};
    CHECK(throws<std::overflow_error>([&] { (void)concatenate(host_span<table_view const>{tabs}); }));
  });
  run("concatenate: inputs without rows give an empty column of the type, no mask without a nullable view", [&] {
    column_view e{data_type{type_id::FLOAT64}, 0, nullptr, nullptr, 0};
    CV three{e, e, e};
    auto r = concatenate(host_span<column_view const>{three});
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT64 && !r->nullable());
    std::vector<table_view> tabs{table_view{{e, e}}, table_view{{e, e}}};
    auto t = concatenate(host_span<table_view const>{tabs});
    CHECK(t->num_columns() == 2 && t->num_rows() == 0);
    CV plain{a, a};
    CHECK(concatenate_masks(host_span<column_view const>{plain}).size() == 0);
  });
  run("scatter: column count, type, map size, map type and a nullable map throw", [&] {
    CHECK(throws<logic_error>([&] { (void)scatter(table_view{{a, a}}, map3, table_view{{a}}); }));
    CHECK(throws<data_type_error>([&] { (void)scatter(table_view{{a}}, map3, table_view{{b64}}); }));
    column_view map9{data_type{type_id::INT32}, 9, fake, nullptr, 0};
    CHECK(throws<logic_error>([&] { (void)scatter(table_view{{a}}, map9, table_view{{a}}); }));
    column_view map64{data_type{type_id::INT64}, 3, fake, nullptr, 0};
    CHECK(throws<data_type_error>([&] { (void)scatter(table_view{{a}}, map64, table_view{{a}}); }));
    column_view mapn{data_type{type_id::INT32}, 3, fake, fake_mask, 1};
    CHECK(throws<std::invalid_argument>([&] { (void)scatter(table_view{{a}}, mapn, table_view{{a}}); }));
  });
  run("copy_if_else: a mask that is not BOOL8, differing types and sizes throw", [&] {
    column_view a4{data_type{type_id::INT32}, 4, fake, nullptr, 0};
    column_view bool4{data_type{type_id::BOOL8}, 4, fake, nullptr, 0};
    CHECK(throws<data_type_error>([&] { (void)copy_if_else(a, a, a); }));
    CHECK(throws<data_type_error>([&] { (void)copy_if_else(a, b64, bool5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)copy_if_else(a, a4, bool5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)copy_if_else(a, a, bool4); }));
  });
  run("copy_if_else: an empty mask gives an empty column", [&] {
    column_view e{data_type{type_id::INT32}, 0, nullptr, nullptr, 0};
    column_view be{data_type{type_id::BOOL8}, 0, nullptr, nullptr, 0};
    auto r = copy_if_else(e, e, be);
    CHECK(r->size() == 0 && r->type().id() == type_id::INT32);
  });
  run("slice / split: an odd number of indices, begin > end and indices out of range throw", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)slice(a, {1, 2, 3}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)slice(a, {3, 2}); }));
    CHECK(throws<std::out_of_range>([&] { (void)slice(a, {-1, 2}); }));
    CHECK(throws<std::out_of_range>([&] { (void)slice(a, {1, 6}); }));
    CHECK(throws<std::out_of_range>([&] { (void)slice(table_view{{a, b64}}, {0, 6}); }));
    CHECK(throws<std::out_of_range>([&] { (void)split(a, {6}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)split(a, {3, 2}); }));
    CHECK(throws<std::out_of_range>([&] { (void)split(table_view{{a}}, {-1}); }));
  });
  run("slice / split of a column without nulls: views that share the buffer, offsets added", [&] {
    column_view off{data_type{type_id::INT32}, 5, fake, nullptr, 0, 7};
    auto s = slice(off, {1, 4, 0, 0, 5, 5});
    CHECK(s.size() == 3 && s[0].size() == 3 && s[0].offset() == 8 && s[0].head<void>() == fake && s[0].null_count() == 0);
    CHECK(s[1].size() == 0 && s[2].size() == 0 && s[2].offset() == 12);
    auto p = split(off, {2, 2, 5});
    CHECK(p.size() == 4 && p[0].size() == 2 && p[1].size() == 0 && p[2].size() == 3 && p[3].size() == 0 && p[2].offset() == 9);
    auto none = split(off, {});
    CHECK(none.size() == 1 && none[0].size() == 5 && none[0].offset() == 7);
    auto tp = split(table_view{{a, b64}}, {2});
    CHECK(tp.size() == 2 && tp[0].num_rows() == 2 && tp[1].num_rows() == 3 && tp[1].column(1).offset() == 2);
  });
}

static void device_cases()
{
  auto const base = make_col<int32_t>({10, 11, 12, 13, 14, 15, 16, 17, 18, 19}, {1, 0, 1, 1, 0, 1, 1, 1, 0, 1});
  run("slice of a nullable column: null counts per piece from the device", [&] {
    auto s = slice(base->view(), {0, 3, 3, 9, 9, 10, 4, 5});
    CHECK(s[0].null_count() == 1 && s[1].null_count() == 2 && s[2].null_count() == 0 && s[3].null_count() == 1);
    CHECK((to_host<int32_t>(s[1]) == I32{13, 14, 15, 16, 17, 18}));
    CHECK((valid_host(s[1]) == V{1, 0, 1, 1, 1, 0}));
  });
  run("split followed by concatenate is the identity (values, validity, null count)", [&] {
    auto parts = split(base->view(), {1, 1, 4, 9});
    auto r     = concatenate(host_span<column_view const>{parts});
    CHECK(r->type().id() == type_id::INT32 && r->size() == 10 && r->null_count() == 3);
    CHECK((to_host<int32_t>(r->view()) == to_host<int32_t>(base->view())));
    CHECK((valid_host(r->view()) == valid_host(base->view())));
  });
  run("concatenate of sliced views in another order, one without nulls: mask only where an input has nulls", [&] {
    auto other = make_col<int32_t>({-1, -2, -3});
    auto s     = slice(base->view(), {5, 8, 1, 3});
    CV in{s[0], other->view(), s[1]};
    auto r = concatenate(host_span<column_view const>{in});
    CHECK((to_host<int32_t>(r->view()) == I32{15, 16, 17, -1, -2, -3, 11, 12}));
    CHECK((valid_host(r->view()) == V{1, 1, 1, 1, 1, 1, 0, 1}) && r->null_count() == 1);
    CV clean{s[0], other->view()};
    auto c = concatenate(host_span<column_view const>{clean});
    CHECK(!c->nullable() && c->null_count() == 0 && (to_host<int32_t>(c->view()) == I32{15, 16, 17, -1, -2, -3}));
  });
  run("concatenate of one input is a copy", [&] {
    auto s = slice(base->view(), {2, 7});
    auto r = concatenate(host_span<column_view const>{s});
    CHECK(r->view().head<void>() != base->view().head<void>() && r->size() == 5 && r->null_count() == 1);
    CHECK((to_host<int32_t>(r->view()) == I32{12, 13, 14, 15, 16}) && (valid_host(r->view()) == V{1, 1, 0, 1, 1}));
  });
  run("concatenate of tables: column by column, mixed widths", [&] {
    auto k  = make_col<int8_t>({1, 2, 3, 4, 5, 6, 7, 8, 9, 10});
    auto d  = make_col<double>({.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5}, {1, 1, 1, 0, 1, 1, 1, 1, 1, 0});
    auto ts = slice(table_view{{k->view(), base->view(), d->view()}}, {7, 10, 0, 2});
    auto r  = concatenate(host_span<table_view const>{ts});
    CHECK(r->num_columns() == 3 && r->num_rows() == 5);
    CHECK((to_host<int8_t>(r->view().column(0)) == I8{8, 9, 10, 1, 2}) && !r->get_column(0).nullable());
    CHECK((to_host<int32_t>(r->view().column(1)) == I32{17, 18, 19, 10, 11}) && (valid_host(r->view().column(1)) == V{1, 0, 1, 1, 0}));
    CHECK((valid_host(r->view().column(2)) == V{1, 1, 0, 1, 1}) && r->get_column(2).null_count() == 1);
    CHECK((to_host<double>(r->view().column(2))[3] == .5));
  });
  run("concatenate_masks: the bits of every view in order, set bits for views without a mask", [&] {
    auto other = make_col<int64_t>({1, 2});
    auto s     = slice(base->view(), {3, 6});
    CV in{other->view(), s[0], base->view()};
    auto m = concatenate_masks(host_span<column_view const>{in});
    CHECK(m.size() >= 4);
    CHECK((bits_host(static_cast<bitmask_type const*>(m.data()), 0, 15) == V{1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1}));
  });
  run("scatter of a sliced source into a sliced target: a copy with the rows written, negative indices wrap", [&] {
    auto src = slice(base->view(), {0, 3})[0];  // 10, null, 12
    auto tgt = slice(base->view(), {4, 10})[0];  // null 15 16 17 null 19
    auto map = make_col<int32_t>({5, 0, -4});
    auto r   = scatter(table_view{{src}}, map->view(), table_view{{tgt}});
    CHECK(r->num_columns() == 1 && r->num_rows() == 6);
    auto const v = to_host<int32_t>(r->view().column(0));
    CHECK(v[5] == 10 && v[2] == 12 && v[1] == 15 && v[3] == 17);
    CHECK((valid_host(r->view().column(0)) == V{0, 1, 1, 1, 0, 1}) && r->get_column(0).null_count() == 2);
    CHECK((to_host<int32_t>(base->view()) == I32{10, 11, 12, 13, 14, 15, 16, 17, 18, 19}));  // the target is not written
  });
  run("scatter: no mask when neither side has nulls; a mask that ends without nulls is dropped", [&] {
    auto src  = make_col<int64_t>({7, 8});
    auto tgt  = make_col<int64_t>({0, 1, 2, 3});
    auto map  = make_col<int32_t>({3, 1});
    auto r    = scatter(table_view{{src->view()}}, map->view(), table_view{{tgt->view()}});
    CHECK(!r->get_column(0).nullable() && (to_host<int64_t>(r->view().column(0)) == I64{0, 8, 2, 7}));
    auto tn = make_col<int64_t>({0, 1, 2, 3}, {1, 0, 1, 0});
    auto r2 = scatter(table_view{{src->view()}}, map->view(), table_view{{tn->view()}});
    CHECK(!r2->get_column(0).nullable() && r2->get_column(0).null_count() == 0);
    auto sn = make_col<int64_t>({7, 8}, {0, 1});
    auto r3 = scatter(table_view{{sn->view()}}, map->view(), table_view{{tgt->view()}});
    CHECK(r3->get_column(0).null_count() == 1 && (valid_host(r3->view().column(0)) == V{1, 1, 1, 0}));
  });
  run("scatter of scalars: a valid and an invalid scalar, two columns", [&] {
    numeric_scalar<int32_t> s1{42, true};
    numeric_scalar<double> s2{2.5, false};
    auto c1  = make_col<int32_t>({0, 1, 2, 3, 4});
    auto c2  = make_col<double>({0., 1., 2., 3., 4.});
    auto map = make_col<int32_t>({4, -5});
    std::vector<std::reference_wrapper<scalar const>> src{s1, s2};
    auto r = scatter(src, map->view(), table_view{{c1->view(), c2->view()}});
    CHECK((to_host<int32_t>(r->view().column(0)) == I32{42, 1, 2, 3, 42}) && !r->get_column(0).nullable());
    CHECK((valid_host(r->view().column(1)) == V{0, 1, 1, 1, 0}) && r->get_column(1).null_count() == 2);
    std::vector<std::reference_wrapper<scalar const>> one{s1};
    CHECK(throws<logic_error>([&] { (void)scatter(one, map->view(), table_view{{c1->view(), c2->view()}}); }));
    std::vector<std::reference_wrapper<scalar const>> swapped{s2, s1};
    CHECK(throws<data_type_error>([&] { (void)scatter(swapped, map->view(), table_view{{c1->view(), c2->view()}}); }));
  });
  run("copy_if_else of two sliced columns under a sliced nullable mask: a null mask element takes rhs", [&] {
    auto m   = make_col<int8_t>({1, 1, 0, 1, 0, 1, 1, 0}, {1, 1, 1, 0, 1, 1, 1, 1}, type_id::BOOL8);
    auto lhs = slice(base->view(), {0, 6})[0];   // 10 n 12 13 n 15
    auto rhs = slice(base->view(), {4, 10})[0];  // n 15 16 17 n 19
    auto mk  = slice(m->view(), {1, 7})[0];      // 1 0 null 0 1 1
    auto r   = copy_if_else(lhs, rhs, mk);
    CHECK(r->type().id() == type_id::INT32 && r->size() == 6);
    auto const v = to_host<int32_t>(r->view());
    CHECK(v[1] == 15 && v[2] == 16 && v[3] == 17 && v[5] == 15);
    CHECK((valid_host(r->view()) == V{1, 1, 1, 1, 0, 1}) && r->null_count() == 1);
  });
  run("copy_if_else with scalars: the three scalar overloads, result size from the mask, masks only where needed", [&] {
    auto m = make_col<int8_t>({1, 0, 1, 0}, {}, type_id::BOOL8);
    auto c = make_col<int64_t>({1, 2, 3, 4});
    numeric_scalar<int64_t> s{-9, true}, bad{0, false};
    auto r1 = copy_if_else(s, c->view(), m->view());
    CHECK((to_host<int64_t>(r1->view()) == I64{-9, 2, -9, 4}) && !r1->nullable());
    auto r2 = copy_if_else(c->view(), bad, m->view());
    CHECK((valid_host(r2->view()) == V{1, 0, 1, 0}) && r2->null_count() == 2 && to_host<int64_t>(r2->view())[2] == 3);
    auto r3 = copy_if_else(s, bad, m->view());
    CHECK(r3->size() == 4 && (valid_host(r3->view()) == V{1, 0, 1, 0}) && to_host<int64_t>(r3->view())[0] == -9);
    numeric_scalar<int32_t> other{1, true};
    CHECK(throws<data_type_error>([&] { (void)copy_if_else(other, c->view(), m->view()); }));
  });
  run("copy_if_else keeps bits: NaN payloads and -0.0", [&] {
    uint64_t const nan_bits = 0x7ff8000000abcdefull, negzero = 0x8000000000000000ull;
    double nanv, nz;
    std::memcpy(&nanv, &nan_bits, 8);
    std::memcpy(&nz, &negzero, 8);
    auto l = make_col<double>({nanv, 1.0});
    auto r = make_col<double>({2.0, nz});
    auto m = make_col<int8_t>({1, 0}, {}, type_id::BOOL8);
    auto o = to_host<double>(copy_if_else(l->view(), r->view(), m->view())->view());
    CHECK(std::memcmp(&o[0], &nan_bits, 8) == 0 && std::memcmp(&o[1], &negzero, 8) == 0);
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
