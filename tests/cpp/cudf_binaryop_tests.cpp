// cudf::binary_operation, unary_operation, cast, is_null / is_valid, is_nan / is_not_nan through the C++ surface
// (include/cudf/binaryop.hpp, include/cudf/unary.hpp).  Small literal vectors, expected values written out by hand; operands are
// sliced views made by cudf::slice where a case says so.  The minimal harness of cudf_copying_tests.cpp.
//   cudf_binaryop_tests --host   what is decided before the first device call: the throws, the empty results, the support tables;
//                                runs without a GPU (tests/test_elementwise_host.py)
//   cudf_binaryop_tests          the whole list; needs a GPU (tests/test_gpu_elementwise.py)
#include <cudf/binaryop.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/unary.hpp>

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
using U32 = std::vector<uint32_t>;
using I64 = std::vector<int64_t>;
using F32 = std::vector<float>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
using BO  = binary_operator;
static data_type dt(type_id id) { return data_type{id}; }

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake = reinterpret_cast<void const*>(0x10000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view b4{dt(type_id::INT32), 4, fake, nullptr, 0};
  column_view f5{dt(type_id::FLOAT64), 5, fake, nullptr, 0};
  column_view e32{dt(type_id::INT32), 0, nullptr, nullptr, 0};
  column_view ef{dt(type_id::FLOAT32), 0, nullptr, nullptr, 0};
  run("binary_operation: a size mismatch throws cudf::logic_error \"Column sizes don't match\"", [&] {
    bool ok = false;
    try {
      (void)binary_operation(a5, b4, BO::ADD, dt(type_id::INT32));
    } catch (logic_error const& e) {
      ok = std::string{e.what()}.find("Column sizes don't match") != std::string::npos;
    }
    CHECK(ok);
  });
  run("binary_operation: operators that are not built throw cudf::logic_error", [&] {
    for (auto op : {BO::LOG_BASE, BO::ATAN2, BO::GENERIC_BINARY, BO::INVALID_BINARY})
      CHECK(throws<logic_error>([&] { (void)binary_operation(f5, f5, op, dt(type_id::FLOAT64)); }));
  });
  run("binary_operation: bitwise, shifts and INT_POW on a float operand, and a non-numeric type, throw cudf::data_type_error", [&] {
    for (auto op : {BO::BITWISE_AND, BO::BITWISE_OR, BO::BITWISE_XOR, BO::SHIFT_LEFT, BO::SHIFT_RIGHT, BO::SHIFT_RIGHT_UNSIGNED, BO::INT_POW}) {
      CHECK(throws<data_type_error>([&] { (void)binary_operation(a5, f5, op, dt(type_id::INT32)); }));
      CHECK(throws<data_type_error>([&] { (void)binary_operation(f5, a5, op, dt(type_id::INT32)); }));
      CHECK(!binops::is_supported_operation(dt(type_id::INT32), dt(type_id::FLOAT64), dt(type_id::INT32), op));
      CHECK(binops::is_supported_operation(dt(type_id::FLOAT64), dt(type_id::INT8), dt(type_id::UINT64), op));
    }
    CHECK(throws<data_type_error>([&] { (void)binary_operation(a5, a5, BO::ADD, dt(type_id::STRING)); }));
    column_view s5{dt(type_id::STRING), 5, fake, nullptr, 0};
    CHECK(throws<data_type_error>([&] { (void)binary_operation(s5, a5, BO::ADD, dt(type_id::INT32)); }));
    CHECK(throws<data_type_error>([&] { (void)cast(s5, dt(type_id::INT32)); }));
    CHECK(throws<data_type_error>([&] { (void)cast(a5, dt(type_id::STRING)); }));
    CHECK(is_supported_cast(dt(type_id::BOOL8), dt(type_id::FLOAT64)) && !is_supported_cast(dt(type_id::STRING), dt(type_id::INT8)));
  });
  run("unary_operation: operators that are not built throw cudf::logic_error, a wrong type cudf::data_type_error", [&] {
    for (auto op : {unary_operator::SIN, unary_operator::LOG, unary_operator::CBRT, unary_operator::BIT_COUNT})
      CHECK(throws<logic_error>([&] { (void)unary_operation(f5, op); }));
    for (auto op : {unary_operator::SQRT, unary_operator::CEIL, unary_operator::FLOOR, unary_operator::RINT})
      CHECK(throws<data_type_error>([&] { (void)unary_operation(a5, op); }));
    CHECK(throws<data_type_error>([&] { (void)unary_operation(f5, unary_operator::BIT_INVERT); }));
    CHECK(throws<data_type_error>([&] { (void)is_nan(a5); }));
    CHECK(throws<data_type_error>([&] { (void)is_not_nan(a5); }));
  });
  run("empty operands give an empty column of the output type", [&] {
    auto r = binary_operation(e32, ef, BO::ADD, dt(type_id::FLOAT64));
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT64 && !r->nullable());
    r = binary_operation(e32, e32, BO::LESS, dt(type_id::BOOL8));
    CHECK(r->size() == 0 && r->type().id() == type_id::BOOL8);
    r = cast(e32, dt(type_id::INT8));
    CHECK(r->size() == 0 && r->type().id() == type_id::INT8);
    r = unary_operation(ef, unary_operator::SQRT);
    CHECK(r->size() == 0 && r->type().id() == type_id::FLOAT32);
    r = unary_operation(e32, unary_operator::NOT);
    CHECK(r->size() == 0 && r->type().id() == type_id::BOOL8);
    CHECK(is_null(e32)->size() == 0 && is_valid(e32)->type().id() == type_id::BOOL8 && is_nan(ef)->size() == 0);
  });
  run("binary_operator and unary_operator keep the reference's integer values", [&] {
    CHECK(static_cast<int>(BO::ADD) == 0 && static_cast<int>(BO::PYMOD) == 8 && static_cast<int>(BO::INT_POW) == 10);
    CHECK(static_cast<int>(BO::SHIFT_RIGHT_UNSIGNED) == 15 && static_cast<int>(BO::EQUAL) == 21 && static_cast<int>(BO::NULL_EQUALS) == 27);
    CHECK(static_cast<int>(BO::GENERIC_BINARY) == 31 && static_cast<int>(BO::NULL_LOGICAL_OR) == 33 && static_cast<int>(BO::INVALID_BINARY) == 34);
    CHECK(static_cast<int>(unary_operator::SQRT) == 14 && static_cast<int>(unary_operator::ABS) == 18 && static_cast<int>(unary_operator::NEGATE) == 23);
  });
}

static void device_cases()
{
  run("column op column: int32 + int32, no mask on the output when neither side has one", [&] {
    auto a = make_col(I32{1, -2, 2147483647, 40, 5}), b = make_col(I32{10, 20, 1, -40, 0});
    auto r = binary_operation(a->view(), b->view(), BO::ADD, dt(type_id::INT32));
    CHECK(to_host<int32_t>(r->view()) == (I32{11, 18, std::numeric_limits<int32_t>::min(), 0, 5}));
    CHECK(!r->nullable() && r->null_count() == 0);
  });
  run("mixed types follow the usual arithmetic conversions: int32(-1) < uint32(1) is false, uint32 + uint32 wraps before widening", [&] {
    auto a = make_col(I32{-1, 0, 5}), b = make_col(U32{1, 1, 5});
    auto r = binary_operation(a->view(), b->view(), BO::LESS, dt(type_id::BOOL8));
    CHECK(to_host<uint8_t>(r->view()) == (U8{0, 1, 0}));
    auto c = make_col(U32{4294967295u, 7}), d = make_col(U32{2, 8});
    auto s = binary_operation(c->view(), d->view(), BO::ADD, dt(type_id::INT64));
    CHECK(to_host<int64_t>(s->view()) == (I64{1, 15}));
    auto e = make_col(I8{100, -100}), f = make_col(I8{100, -100});
    auto t = binary_operation(e->view(), f->view(), BO::ADD, dt(type_id::INT8));     // int32 200 -> int8
    CHECK(to_host<int8_t>(t->view()) == (I8{-56, 56}));
    auto u = binary_operation(e->view(), f->view(), BO::ADD, dt(type_id::FLOAT64));  // ... but 200.0 as a double
    CHECK(to_host<double>(u->view()) == (F64{200.0, -200.0}));
  });
  run("a mask on either side: the output bit is the AND, the null count is counted; a mask that nulls nothing is dropped", [&] {
    auto a = make_col(I64{1, 2, 3, 4, 5, 6}, V{1, 0, 1, 1, 0, 1}), b = make_col(I64{10, 20, 30, 40, 50, 60}, V{1, 1, 0, 1, 0, 1});
    auto r = binary_operation(a->view(), b->view(), BO::MUL, dt(type_id::INT64));
    CHECK(valid_host(r->view()) == (V{1, 0, 0, 1, 0, 1}) && r->null_count() == 3);
    auto h = to_host<int64_t>(r->view());
    CHECK(h[0] == 10 && h[3] == 160 && h[5] == 360);
    auto c = make_col(I64{1, 2, 3}, V{1, 1, 1});
    auto s = binary_operation(c->view(), c->view(), BO::SUB, dt(type_id::INT64));
    CHECK(s->null_count() == 0 && to_host<int64_t>(s->view()) == (I64{0, 0, 0}));
  });
  run("sliced views from cudf::slice on both operands at different offsets", [&] {
    std::vector<int32_t> av(100), bv(100);
    V avalid(100), bvalid(100);
    for (int i = 0; i < 100; ++i) {
      av[i] = i; bv[i] = 1000 * i; avalid[i] = i % 3 != 0; bvalid[i] = i % 5 != 0;
    }
    auto a = make_col(av, avalid), b = make_col(bv, bvalid);
    auto as = slice(a->view(), {1, 71}), bs = slice(b->view(), {30, 100});
    auto r  = binary_operation(as[0], bs[0], BO::ADD, dt(type_id::INT64));
    auto h  = to_host<int64_t>(r->view());
    auto v  = valid_host(r->view());
    size_type nulls = 0;
    for (int i = 0; i < 70; ++i) {
      int const want_valid = avalid[1 + i] && bvalid[30 + i];
      CHECK(v[i] == want_valid);
      if (want_valid) CHECK(h[i] == av[1 + i] + bv[30 + i]); else ++nulls;
    }
    CHECK(r->null_count() == nulls && r->size() == 70);
  });
  run("column op scalar and scalar op column; an invalid scalar makes every row null", [&] {
    auto a = make_col(F64{1.0, 2.0, 4.0});
    numeric_scalar<double> two{2.0};
    auto r = binary_operation(a->view(), two, BO::DIV, dt(type_id::FLOAT64));
    CHECK(to_host<double>(r->view()) == (F64{0.5, 1.0, 2.0}) && !r->nullable());
    auto s = binary_operation(two, a->view(), BO::DIV, dt(type_id::FLOAT64));
    CHECK(to_host<double>(s->view()) == (F64{2.0, 1.0, 0.5}));
    numeric_scalar<int32_t> none{7, false};
    auto t = binary_operation(a->view(), none, BO::ADD, dt(type_id::FLOAT64));
    CHECK(t->null_count() == 3 && valid_host(t->view()) == (V{0, 0, 0}));
    auto u = binary_operation(none, a->view(), BO::ADD, dt(type_id::FLOAT64));
    CHECK(u->null_count() == 3);
  });
  run("NULL_EQUALS / NULL_NOT_EQUALS never give a null; NULL_MAX / NULL_MIN take the valid side", [&] {
    auto a = make_col(I32{1, 2, 3, 4}, V{1, 0, 1, 0}), b = make_col(I32{1, 2, 9, 4}, V{1, 1, 0, 0});
    auto r = binary_operation(a->view(), b->view(), BO::NULL_EQUALS, dt(type_id::BOOL8));
    CHECK(to_host<uint8_t>(r->view()) == (U8{1, 0, 0, 1}) && r->null_count() == 0 && !r->nullable());
    r = binary_operation(a->view(), b->view(), BO::NULL_NOT_EQUALS, dt(type_id::BOOL8));
    CHECK(to_host<uint8_t>(r->view()) == (U8{0, 1, 1, 0}) && r->null_count() == 0);
    auto c = make_col(I32{5, 2, 3, 4}, V{1, 0, 1, 0});
    r      = binary_operation(c->view(), b->view(), BO::NULL_MAX, dt(type_id::INT32));
    auto h = to_host<int32_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 0}) && r->null_count() == 1 && h[0] == 5 && h[1] == 2 && h[2] == 3);
    r = binary_operation(c->view(), b->view(), BO::NULL_MIN, dt(type_id::INT32));
    h = to_host<int32_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 0}) && h[0] == 1 && h[1] == 2 && h[2] == 3);
  });
  run("NULL_LOGICAL_AND / OR: Kleene logic", [&] {
    //                       T&T   T&F   T&null F&null null&F null&T null&null
    auto a = make_col(U8{1, 1, 1, 0, 1, 1, 0}, V{1, 1, 1, 1, 0, 0, 0}, type_id::BOOL8);
    auto b = make_col(U8{1, 0, 1, 1, 0, 1, 0}, V{1, 1, 0, 0, 1, 1, 0}, type_id::BOOL8);
    auto r = binary_operation(a->view(), b->view(), BO::NULL_LOGICAL_AND, dt(type_id::BOOL8));
    auto h = to_host<uint8_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 0, 1, 1, 0, 0}) && r->null_count() == 3);
    CHECK(h[0] == 1 && h[1] == 0 && h[3] == 0 && h[4] == 0);
    r = binary_operation(a->view(), b->view(), BO::NULL_LOGICAL_OR, dt(type_id::BOOL8));
    h = to_host<uint8_t>(r->view());
    CHECK(valid_host(r->view()) == (V{1, 1, 1, 0, 0, 1, 0}) && r->null_count() == 3);
    CHECK(h[0] == 1 && h[1] == 1 && h[2] == 1 && h[5] == 1);
  });
  run("integer FLOOR_DIV, PYMOD, MOD over the four sign combinations; SHIFT_RIGHT_UNSIGNED on the operand's own width", [&] {
    auto a = make_col(I32{7, -7, 7, -7}), b = make_col(I32{2, 2, -2, -2});
    CHECK(to_host<int32_t>(binary_operation(a->view(), b->view(), BO::FLOOR_DIV, dt(type_id::INT32))->view()) == (I32{3, -4, -4, 3}));
    CHECK(to_host<int32_t>(binary_operation(a->view(), b->view(), BO::PYMOD, dt(type_id::INT32))->view()) == (I32{1, 1, -1, -1}));
    CHECK(to_host<int32_t>(binary_operation(a->view(), b->view(), BO::MOD, dt(type_id::INT32))->view()) == (I32{1, -1, 1, -1}));
    CHECK(to_host<int32_t>(binary_operation(a->view(), b->view(), BO::DIV, dt(type_id::INT32))->view()) == (I32{3, -3, -3, 3}));
    auto c = make_col(I8{-1, -128, 64}), d = make_col(I8{1, 7, 2});
    CHECK(to_host<int8_t>(binary_operation(c->view(), d->view(), BO::SHIFT_RIGHT_UNSIGNED, dt(type_id::INT8))->view()) == (I8{127, 1, 16}));
    CHECK(to_host<int8_t>(binary_operation(c->view(), d->view(), BO::SHIFT_RIGHT, dt(type_id::INT8))->view()) == (I8{-1, -1, 16}));
  });
  run("TRUE_DIV, POW and INT_POW", [&] {
    auto a = make_col(I32{1, 7, -3}), b = make_col(I32{2, 2, 2});
    CHECK(to_host<double>(binary_operation(a->view(), b->view(), BO::TRUE_DIV, dt(type_id::FLOAT64))->view()) == (F64{0.5, 3.5, -1.5}));
    CHECK(to_host<double>(binary_operation(a->view(), b->view(), BO::POW, dt(type_id::FLOAT64))->view()) == (F64{1.0, 49.0, 9.0}));
    auto e = make_col(I32{0, 10, -1});
    CHECK(to_host<int32_t>(binary_operation(a->view(), e->view(), BO::INT_POW, dt(type_id::INT32))->view()) == (I32{1, 282475249, 0}));
  });
  run("cast keeps the input's validity and null count, on a sliced view too", [&] {
    auto a = make_col(F64{1.9, -1.9, 300.0, 0.0, -0.0, 2.5}, V{1, 0, 1, 1, 0, 1});
    auto r = cast(a->view(), dt(type_id::INT32));
    CHECK(r->null_count() == 2 && valid_host(r->view()) == (V{1, 0, 1, 1, 0, 1}));
    auto h = to_host<int32_t>(r->view());
    CHECK(h[0] == 1 && h[2] == 300 && h[3] == 0 && h[5] == 2);
    auto s  = slice(a->view(), {1, 5});
    auto r2 = cast(s[0], dt(type_id::BOOL8));
    CHECK(r2->size() == 4 && r2->null_count() == 2 && valid_host(r2->view()) == (V{0, 1, 1, 0}));
    auto h2 = to_host<uint8_t>(r2->view());
    CHECK(h2[1] == 1 && h2[2] == 0);
    auto c = make_col(I32{-1, 256, 65537});
    CHECK(to_host<uint8_t>(cast(c->view(), dt(type_id::UINT8))->view()) == (U8{255, 0, 1}));
    CHECK(!cast(c->view(), dt(type_id::UINT8))->nullable());
  });
  run("unary_operation keeps the input's validity and null count", [&] {
    auto a = make_col(F64{4.0, 2.25, 0.5, 1.5, 2.5, -0.5}, V{1, 1, 0, 1, 1, 1});
    auto r = unary_operation(a->view(), unary_operator::SQRT);
    CHECK(r->null_count() == 1 && valid_host(r->view()) == (V{1, 1, 0, 1, 1, 1}));
    auto h = to_host<double>(r->view());
    CHECK(h[0] == 2.0 && h[1] == 1.5);
    h = to_host<double>(unary_operation(a->view(), unary_operator::RINT)->view());
    CHECK(h[0] == 4.0 && h[1] == 2.0 && h[3] == 2.0 && h[4] == 2.0 && h[5] == 0.0 && std::signbit(h[5]));
    auto b = make_col(I8{-128, -1, 0, 127});
    CHECK(to_host<int8_t>(unary_operation(b->view(), unary_operator::ABS)->view()) == (I8{-128, 1, 0, 127}));
    CHECK(to_host<int8_t>(unary_operation(b->view(), unary_operator::NEGATE)->view()) == (I8{-128, 1, 0, -127}));
    CHECK(to_host<int8_t>(unary_operation(b->view(), unary_operator::BIT_INVERT)->view()) == (I8{127, 0, -1, -128}));
    auto n = unary_operation(b->view(), unary_operator::NOT);
    CHECK(n->type().id() == type_id::BOOL8 && to_host<uint8_t>(n->view()) == (U8{0, 0, 1, 0}));
  });
  run("is_null / is_valid on a sliced nullable column; is_nan / is_not_nan", [&] {
    auto a = make_col(F64{1.0, std::nan(""), 3.0, std::nan("7"), 5.0, 6.0}, V{1, 1, 0, 1, 0, 1});
    auto s = slice(a->view(), {1, 6});
    auto n = is_null(s[0]);
    CHECK(n->type().id() == type_id::BOOL8 && !n->nullable() && to_host<uint8_t>(n->view()) == (U8{0, 1, 0, 1, 0}));
    CHECK(to_host<uint8_t>(is_valid(s[0])->view()) == (U8{1, 0, 1, 0, 1}));
    auto plain = make_col(I32{1, 2, 3});
    CHECK(to_host<uint8_t>(is_null(plain->view())->view()) == (U8{0, 0, 0}) && to_host<uint8_t>(is_valid(plain->view())->view()) == (U8{1, 1, 1}));
    auto q = is_nan(s[0]);
    CHECK(q->null_count() == 2 && valid_host(q->view()) == (V{1, 0, 1, 0, 1}));
    auto h = to_host<uint8_t>(q->view());
    CHECK(h[0] == 1 && h[2] == 1 && h[4] == 0);
    h = to_host<uint8_t>(is_not_nan(s[0])->view());
    CHECK(h[0] == 0 && h[2] == 0 && h[4] == 1);
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
