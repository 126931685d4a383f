// cudf::replace_nulls, replace_nans, find_and_replace_all, clamp and normalize_nans_and_zeros through the C++ surface
// (include/cudf/replace.hpp).  Small literal vectors, expected values written out by hand; operands are sliced views made by
// cudf::slice where a case says so.  The minimal harness of cudf_binaryop_tests.cpp.
//   cudf_replace_tests --host   what is decided before the first device call: the throws and the empty results; runs without a
//                               GPU (tests/test_replace_host.py)
//   cudf_replace_tests          the whole list; needs a GPU (tests/test_gpu_replace.py)
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/replace.hpp>
#include <cudf/scalar/scalar.hpp>

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
using U64 = std::vector<uint64_t>;
using F32 = std::vector<float>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
static data_type dt(type_id id) { return data_type{id}; }
static uint64_t bits_of(double d)
{
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}

// what is decided before any device call: "device pointers" that are never dereferenced (scalars live on the device, so the
// overloads that take one are device cases)
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  auto const* fmask = reinterpret_cast<bitmask_type const*>(0x20000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view a5n{dt(type_id::INT32), 5, fake, fmask, 2};
  column_view b4{dt(type_id::INT32), 4, fake, nullptr, 0};
  column_view l5{dt(type_id::INT64), 5, fake, nullptr, 0};
  column_view f5{dt(type_id::FLOAT64), 5, fake, nullptr, 0};
  column_view f4{dt(type_id::FLOAT64), 4, fake, nullptr, 0};
  column_view g5{dt(type_id::FLOAT32), 5, fake, nullptr, 0};
  column_view s5{dt(type_id::STRING), 5, fake, nullptr, 0};
  column_view e32{dt(type_id::INT32), 0, nullptr, nullptr, 0};
  column_view ef{dt(type_id::FLOAT32), 0, nullptr, nullptr, 0};
  run("type mismatches throw cudf::data_type_error", [&] {
    CHECK(throws<data_type_error>([&] { (void)replace_nulls(a5n, l5); }));
    CHECK(throws<data_type_error>([&] { (void)replace_nans(f5, g5); }));
    CHECK(throws<data_type_error>([&] { (void)find_and_replace_all(a5, l5, a5); }));
    CHECK(throws<data_type_error>([&] { (void)find_and_replace_all(a5, a5, l5); }));
    CHECK(throws<data_type_error>([&] { (void)replace_nulls(s5, s5); }));
    CHECK(throws<data_type_error>([&] { (void)replace_nulls(s5, replace_policy::PRECEDING); }));
  });
  run("size mismatches throw std::invalid_argument, and not cudf::data_type_error", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)replace_nulls(a5n, b4); }));
    CHECK(!throws<data_type_error>([&] { (void)replace_nulls(a5n, b4); }));
    CHECK(throws<std::invalid_argument>([&] { (void)replace_nans(f5, f4); }));
    CHECK(!throws<data_type_error>([&] { (void)replace_nans(f5, f4); }));
    CHECK(throws<std::invalid_argument>([&] { (void)find_and_replace_all(a5, a5, b4); }));
    CHECK(!throws<data_type_error>([&] { (void)find_and_replace_all(a5, a5, b4); }));
  });
  run("nulls in values_to_replace throw std::invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)find_and_replace_all(a5, a5n, a5); }));
    CHECK(!throws<data_type_error>([&] { (void)find_and_replace_all(a5, a5n, a5); }));
  });
  run("a non-float input to replace_nans / normalize_nans_and_zeros throws std::invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)replace_nans(a5, a5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)normalize_nans_and_zeros(a5); }));
    mutable_column_view m{dt(type_id::INT32), 5, const_cast<void*>(fake), nullptr, 0};
    CHECK(throws<std::invalid_argument>([&] { normalize_nans_and_zeros(m); }));
  });
  run("empty inputs give an empty column of the input's type", [&] {
    auto r = replace_nulls(e32, e32);
    CHECK(r->size() == 0 && r->type().id() == type_id::INT32 && !r->nullable());
    r = replace_nulls(e32, replace_policy::FOLLOWING);
    CHECK(r->size() == 0 && r->type().id() == type_id::INT32);
    r = replace_nans(ef, ef);
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT32);
    r = find_and_replace_all(e32, a5, a5);
    CHECK(r->size() == 0 && r->type().id() == type_id::INT32);
    r = normalize_nans_and_zeros(ef);
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT32);
    mutable_column_view m{dt(type_id::FLOAT32), 0, nullptr, nullptr, 0};
    normalize_nans_and_zeros(m);
  });
  run("replace_policy keeps the reference's values", [&] {
    CHECK(static_cast<int>(replace_policy::PRECEDING) == 0 && static_cast<int>(replace_policy::FOLLOWING) == 1);
  });
}

static void device_cases()
{
  run("replace_nulls(column): nulls take the replacement's row; null where both are; the count is the device's", [&] {
    auto a = make_col(I32{1, 2, 3, 4, 5, 6}, V{1, 0, 1, 0, 0, 1}), b = make_col(I32{10, 20, 30, 40, 50, 60}, V{1, 1, 0, 0, 1, 1});
    auto r = replace_nulls(a->view(), b->view());
    auto h = to_host<int32_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 0, 1, 1}) && r->null_count() == 1);
    CHECK(h[0] == 1 && h[1] == 20 && h[2] == 3 && h[4] == 50 && h[5] == 6);
    auto c = make_col(I32{10, 20, 30, 40, 50, 60});
    r      = replace_nulls(a->view(), c->view());
    CHECK(!r->nullable() && r->null_count() == 0 && to_host<int32_t>(r->view()) == (I32{1, 20, 3, 40, 50, 6}));
  });
  run("replace_nulls(scalar): a valid scalar fills, the result has no mask; an invalid scalar and an input without nulls copy", [&] {
    auto a = make_col(F64{1.0, 2.0, 3.0}, V{0, 1, 0});
    numeric_scalar<double> nine{9.0};
    auto r = replace_nulls(a->view(), nine);
    CHECK(to_host<double>(r->view()) == (F64{9.0, 2.0, 9.0}) && !r->nullable() && r->null_count() == 0);
    numeric_scalar<double> none{9.0, false};
    r = replace_nulls(a->view(), none);
    CHECK(r->null_count() == 2 && valid_host(r->view()) == (V{0, 1, 0}) && to_host<double>(r->view())[1] == 2.0);
    auto p = make_col(F64{1.0, 2.0, 3.0});
    r      = replace_nulls(p->view(), nine);
    CHECK(!r->nullable() && to_host<double>(r->view()) == (F64{1.0, 2.0, 3.0}));
    numeric_scalar<int32_t> wrong{1};
    CHECK(throws<data_type_error>([&] { (void)replace_nulls(a->view(), wrong); }));
  });
  run("replace_nulls(policy): PRECEDING and FOLLOWING; rows without a source stay null", [&] {
    auto a = make_col(I64{1, 2, 3, 4, 5, 6, 7}, V{0, 1, 0, 0, 1, 0, 0});
    auto r = replace_nulls(a->view(), replace_policy::PRECEDING);
    auto h = to_host<int64_t>(r->view());
    CHECK(valid_host(r->view()) == (V{0, 1, 1, 1, 1, 1, 1}) && r->null_count() == 1);
    CHECK(h[1] == 2 && h[2] == 2 && h[3] == 2 && h[4] == 5 && h[5] == 5 && h[6] == 5);
    r = replace_nulls(a->view(), replace_policy::FOLLOWING);
    h = to_host<int64_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 1, 1, 0, 0}) && r->null_count() == 2);
    CHECK(h[0] == 2 && h[1] == 2 && h[2] == 5 && h[3] == 5 && h[4] == 5);
    auto b = make_col(I64{1, 2, 3}, V{1, 0, 1});
    r      = replace_nulls(b->view(), replace_policy::PRECEDING);
    CHECK(!r->nullable() && r->null_count() == 0 && to_host<int64_t>(r->view()) == (I64{1, 1, 3}));
  });
  run("replace_nulls on views from cudf::slice at an unaligned begin bit: the fill does not see rows outside the view", [&] {
    std::vector<int32_t> av(200);
    V avalid(200);
    for (int i = 0; i < 200; ++i) {
      av[i] = i; avalid[i] = i % 7 == 0;
    }
    auto a  = make_col(av, avalid);
    auto s  = slice(a->view(), {33, 171});   // rows 33..170: the first valid row is 35, the last 168
    auto r  = replace_nulls(s[0], replace_policy::PRECEDING);
    auto h  = to_host<int32_t>(r->view());
    auto v  = valid_host(r->view());
    for (int i = 0; i < 138; ++i) {
      int const row = 33 + i;
      CHECK(v[i] == (row >= 35));
      if (row >= 35) CHECK(h[i] == row / 7 * 7);
    }
    CHECK(r->null_count() == 2 && r->size() == 138);
    r = replace_nulls(s[0], replace_policy::FOLLOWING);
    h = to_host<int32_t>(r->view());
    v = valid_host(r->view());
    for (int i = 0; i < 138; ++i) {
      int const row = 33 + i;
      CHECK(v[i] == (row <= 168));
      if (row <= 168) CHECK(h[i] == (row + 6) / 7 * 7);
    }
    CHECK(r->null_count() == 2);
    auto b  = make_col(std::vector<int32_t>(200, -1));
    auto bs = slice(b->view(), {1, 139});
    r       = replace_nulls(s[0], bs[0]);
    h       = to_host<int32_t>(r->view());
    CHECK(!r->nullable());
    for (int i = 0; i < 138; ++i) CHECK(h[i] == ((33 + i) % 7 == 0 ? 33 + i : -1));
  });
  run("replace_nans: a valid NaN takes the replacement's value and validity; a null row with NaN bits stays null", [&] {
    double const nan = std::nan("");
    auto a = make_col(F64{1.0, nan, -nan, nan, 5.0, -0.0}, V{1, 1, 1, 0, 0, 1});
    auto b = make_col(F64{10.0, 20.0, 30.0, 40.0, 50.0, 60.0}, V{1, 1, 0, 1, 1, 1});
    auto r = replace_nans(a->view(), b->view());
    auto h = to_host<double>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 0, 0, 0, 1}) && r->null_count() == 3);
    CHECK(h[0] == 1.0 && h[1] == 20.0 && bits_of(h[5]) == bits_of(-0.0));
    numeric_scalar<double> zero{0.0};
    r = replace_nans(a->view(), zero);
    h = to_host<double>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 0, 0, 1}) && r->null_count() == 2 && h[1] == 0.0 && h[2] == 0.0);
    auto p = make_col(F32{1.0f, std::nanf(""), 3.0f});
    numeric_scalar<float> seven{7.0f};
    r = replace_nans(p->view(), seven);
    CHECK(!r->nullable() && to_host<float>(r->view()) == (F32{1.0f, 7.0f, 3.0f}));
    numeric_scalar<float> none{7.0f, false};
    r = replace_nans(p->view(), none);   // a copy
    CHECK(!r->nullable() && std::isnan(to_host<float>(r->view())[1]));
  });
  run("find_and_replace_all: the first mapping wins, NaN matches nothing, -0.0 matches +0.0, nulls stay, a null replacement nulls", [&] {
    auto a = make_col(I32{1, 2, 3, 2, 5, 1}, V{1, 1, 1, 0, 1, 1});
    auto o = make_col(I32{2, 1, 2}), w = make_col(I32{20, 10, 99}, V{1, 0, 1});
    auto r = find_and_replace_all(a->view(), o->view(), w->view());
    auto h = to_host<int32_t>(r->view());
    CHECK(valid_host(r->view()) == (V{0, 1, 1, 0, 1, 0}) && r->null_count() == 3 && h[1] == 20 && h[2] == 3 && h[4] == 5);
    double const nan = std::nan("");
    auto f  = make_col(F64{nan, -0.0, 2.0});
    auto fo = make_col(F64{nan, 0.0}), fw = make_col(F64{7.0, 8.0});
    r       = find_and_replace_all(f->view(), fo->view(), fw->view());
    auto fh = to_host<double>(r->view());
    CHECK(!r->nullable() && std::isnan(fh[0]) && fh[1] == 8.0 && fh[2] == 2.0);
    auto e = make_col(I32{});
    r      = find_and_replace_all(a->view(), e->view(), e->view());   // an empty list: a copy
    CHECK(r->null_count() == 1 && valid_host(r->view()) == (V{1, 1, 1, 0, 1, 1}) && to_host<int32_t>(r->view())[4] == 5);
  });
  run("clamp: both bounds, one-sided bounds, distinct replacements, NaN passes, validity is the input's", [&] {
    auto a = make_col(I32{-5, 0, 5, 10, 15}, V{1, 1, 0, 1, 1});
    numeric_scalar<int32_t> lo{0}, hi{10}, lor{-1}, hir{11}, none{0, false};
    auto r = clamp(a->view(), lo, hi);
    auto h = to_host<int32_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 0, 1, 1}) && r->null_count() == 1 && h[0] == 0 && h[1] == 0 && h[3] == 10 && h[4] == 10);
    h = to_host<int32_t>(clamp(a->view(), lo, lor, hi, hir)->view());
    CHECK(h[0] == -1 && h[1] == 0 && h[3] == 10 && h[4] == 11);
    h = to_host<int32_t>(clamp(a->view(), none, hi)->view());
    CHECK(h[0] == -5 && h[4] == 10);
    h = to_host<int32_t>(clamp(a->view(), lo, none)->view());
    CHECK(h[0] == 0 && h[4] == 15);
    r = clamp(a->view(), none, none);   // a copy
    CHECK(r->null_count() == 1 && to_host<int32_t>(r->view())[0] == -5);
    CHECK(throws<std::invalid_argument>([&] { (void)clamp(a->view(), lo, none, hi, hir); }));
    CHECK(throws<std::invalid_argument>([&] { (void)clamp(a->view(), lo, lor, hi, none); }));
    numeric_scalar<int64_t> l64{0};
    CHECK(throws<data_type_error>([&] { (void)clamp(a->view(), l64, l64); }));
    auto f = make_col(F64{-1.0, std::nan(""), 2.0});
    numeric_scalar<double> flo{0.0}, fhi{1.0};
    auto fh = to_host<double>(clamp(f->view(), flo, fhi)->view());
    CHECK(fh[0] == 0.0 && std::isnan(fh[1]) && fh[2] == 1.0);
    auto u = make_col(U64{1ull, 0x8000000000000001ull, 0xFFFFFFFFFFFFFFFFull});
    numeric_scalar<uint64_t> ulo{2ull}, uhi{0x8000000000000002ull};
    CHECK(to_host<uint64_t>(clamp(u->view(), ulo, uhi)->view()) == (U64{2ull, 0x8000000000000001ull, 0x8000000000000002ull}));
  });
  run("normalize_nans_and_zeros: out of place keeps validity; in place on a sliced mutable view", [&] {
    double const nan = std::nan("");
    auto a = make_col(F64{-0.0, 0.0, -nan, nan, 1.5, -1.5}, V{1, 1, 1, 0, 1, 1});
    auto r = normalize_nans_and_zeros(a->view());
    auto h = to_host<double>(r->view());
    CHECK(r->null_count() == 1 && valid_host(r->view()) == (V{1, 1, 1, 0, 1, 1}));
    CHECK(bits_of(h[0]) == 0 && bits_of(h[1]) == 0 && bits_of(h[2]) == 0x7FF8000000000000ull && h[4] == 1.5 && h[5] == -1.5);
    auto b = make_col(F64{-0.0, -0.0, -nan, -0.0});
    auto m = b->mutable_view();
    mutable_column_view part{m.type(), 2, m.head<void>(), nullptr, 0, 1};
    normalize_nans_and_zeros(part);
    get_default_stream().synchronize();
    h = to_host<double>(b->view());
    CHECK(bits_of(h[0]) == bits_of(-0.0) && bits_of(h[1]) == 0 && bits_of(h[2]) == 0x7FF8000000000000ull && bits_of(h[3]) == bits_of(-0.0));
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
