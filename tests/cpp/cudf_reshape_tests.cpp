// cudf::interleave_columns, tile, transpose (include/cudf/reshape.hpp, transpose.hpp) and cudf::fill, fill_in_place, repeat, sequence
// (include/cudf/filling.hpp) through the C++ surface.  Small literal vectors, expected values written out by hand or computed by
// a loop on the host; operands are sliced views made by cudf::slice where a case says so.  The minimal harness of
// cudf_replace_tests.cpp.
//   cudf_reshape_tests --host   what is decided before the first device call: the throws that need no scalar (a scalar lives on
//                               the device) and the empty results; runs without a GPU (tests/test_reshape_host.py)
//   cudf_reshape_tests          the whole list; needs a GPU (tests/test_gpu_reshape.py)
#include <cudf/column/column_factories.hpp>
#include <cudf/copying.hpp>
#include <cudf/filling.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/reshape.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/transpose.hpp>

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
static int count0(std::vector<int> const& v)
{
  int z = 0;
  for (int x : v) z += x == 0;
  return z;
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
using I16 = std::vector<int16_t>;
using I32 = std::vector<int32_t>;
using I64 = std::vector<int64_t>;
using F32 = std::vector<float>;
using F64 = std::vector<double>;
using V   = std::vector<int>;
static data_type dt(type_id id) { return data_type{id}; }

// what is decided before any device call: "device pointers" that are never dereferenced
static void host_cases()
{
  void const* fake  = reinterpret_cast<void const*>(0x10000);
  auto const* fmask = reinterpret_cast<bitmask_type const*>(0x20000);
  column_view a5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view b5{dt(type_id::INT32), 5, fake, nullptr, 0};
  column_view l5{dt(type_id::INT64), 5, fake, nullptr, 0};
  column_view s5{dt(type_id::STRING), 5, fake, nullptr, 0};
  column_view c5{dt(type_id::INT16), 5, fake, nullptr, 0};
  column_view c5n{dt(type_id::INT16), 5, fake, fmask, 2};
  column_view c4{dt(type_id::INT16), 4, fake, nullptr, 0};
  column_view f5{dt(type_id::FLOAT32), 5, fake, nullptr, 0};
  column_view bool5{dt(type_id::BOOL8), 5, fake, nullptr, 0};
  column_view e32{dt(type_id::INT32), 0, nullptr, nullptr, 0};
  column_view e64{dt(type_id::FLOAT64), 0, nullptr, nullptr, 0};
  column_view ec{dt(type_id::INT32), 0, nullptr, nullptr, 0};
  constexpr size_type big = std::numeric_limits<size_type>::max() / 2 + 1;  // 2^30
  column_view huge{dt(type_id::INT8), big, fake, nullptr, 0};
  run("mixed column types throw cudf::data_type_error", [&] {
    CHECK(throws<data_type_error>([&] { (void)interleave_columns(table_view{{a5, l5}}); }));
    CHECK(throws<data_type_error>([&] { (void)transpose(table_view{{a5, l5}}); }));
    CHECK(throws<data_type_error>([&] { (void)interleave_columns(table_view{{s5, s5}}); }));
    CHECK(throws<data_type_error>([&] { (void)tile(table_view{{s5}}, 2); }));
    CHECK(throws<data_type_error>([&] { (void)repeat(table_view{{s5}}, 2); }));
  });
  run("interleave_columns of a table without columns throws std::invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)interleave_columns(table_view{}); }));
    CHECK(!throws<data_type_error>([&] { (void)interleave_columns(table_view{}); }));
  });
  run("a negative count throws std::invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)tile(table_view{{a5}}, -1); }));
    CHECK(throws<std::invalid_argument>([&] { (void)repeat(table_view{{a5}}, -1); }));
  });
  run("a result beyond size_type throws std::overflow_error", [&] {
    CHECK(throws<std::overflow_error>([&] { (void)tile(table_view{{huge}}, 2); }));
    CHECK(throws<std::overflow_error>([&] { (void)repeat(table_view{{huge}}, 2); }));
    CHECK(throws<std::overflow_error>([&] { (void)interleave_columns(table_view{{huge, huge}}); }));
    CHECK(throws<std::overflow_error>([&] { (void)transpose(table_view{{huge, huge}}); }));
  });
  run("a count column that is not integral, has nulls or differs in length throws std::invalid_argument", [&] {
    CHECK(throws<std::invalid_argument>([&] { (void)repeat(table_view{{a5}}, f5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)repeat(table_view{{a5}}, bool5); }));
    CHECK(throws<std::invalid_argument>([&] { (void)repeat(table_view{{a5}}, c5n); }));
    CHECK(throws<std::invalid_argument>([&] { (void)repeat(table_view{{a5}}, c4); }));
    CHECK(!throws<data_type_error>([&] { (void)repeat(table_view{{a5}}, f5); }));
  });
  run("empty inputs give empty results of the input's types", [&] {
    auto r = interleave_columns(table_view{{e32, e32}});
    CHECK(r->size() == 0 && r->type().id() == type_id::INT32 && !r->nullable());
    auto t = tile(table_view{{e32, e64}}, 3);
    CHECK(t->num_columns() == 2 && t->num_rows() == 0 && t->get_column(1).type().id() == type_id::FLOAT64);
    t = tile(table_view{{a5, l5}}, 0);
    CHECK(t->num_columns() == 2 && t->num_rows() == 0 && t->get_column(1).type().id() == type_id::INT64);
    t = repeat(table_view{{a5}}, 0);
    CHECK(t->num_columns() == 1 && t->num_rows() == 0 && t->get_column(0).type().id() == type_id::INT32);
    t = repeat(table_view{{e32, e64}}, ec);
    CHECK(t->num_columns() == 2 && t->num_rows() == 0 && t->get_column(1).type().id() == type_id::FLOAT64);
    auto p = transpose(table_view{});
    CHECK(p.first->size() == 0 && p.second.num_columns() == 0);
    p = transpose(table_view{{e32, e32}});
    CHECK(p.first->size() == 0 && p.second.num_columns() == 0);
  });
}

static void device_cases()
{
  // 100 rows, nulls at multiples of 7 / of 5; the views used below start at row 33 (an unaligned begin bit)
  std::vector<int32_t> av(100), bv(100);
  V avalid(100), bvalid(100);
  for (int i = 0; i < 100; ++i) {
    av[i] = i; bv[i] = 1000 + i; avalid[i] = i % 7 != 0; bvalid[i] = i % 5 != 0;
  }
  auto a = make_col(av, avalid), b = make_col(bv, bvalid), c = make_col(bv);
  auto as = slice(a->view(), {33, 71})[0], bs = slice(b->view(), {33, 71})[0], cs = slice(c->view(), {33, 71})[0];   // 38 rows

  run("interleave_columns on sliced views: values, validity and the device's null count; no nulls, no bitmap", [&] {
    auto r = interleave_columns(table_view{{as, bs, cs}});
    auto h = to_host<int32_t>(r->view());
    auto v = valid_host(r->view());
    CHECK(r->size() == 114 && r->type().id() == type_id::INT32 && r->nullable());
    int nulls = 0;
    for (int i = 0; i < 38; ++i) {
      int const row = 33 + i;
      CHECK(v[3 * i] == (row % 7 != 0) && v[3 * i + 1] == (row % 5 != 0) && v[3 * i + 2] == 1);
      if (v[3 * i]) CHECK(h[3 * i] == row);
      if (v[3 * i + 1]) CHECK(h[3 * i + 1] == 1000 + row);
      CHECK(h[3 * i + 2] == 1000 + row);
      nulls += (row % 7 == 0) + (row % 5 == 0);
    }
    CHECK(r->null_count() == nulls);
    r = interleave_columns(table_view{{cs, cs}});
    CHECK(!r->nullable() && r->null_count() == 0 && r->size() == 76 && to_host<int32_t>(r->view())[75] == 1070);
    r = interleave_columns(table_view{{cs}});   // one column: a copy
    CHECK(r->size() == 38 && to_host<int32_t>(r->view())[0] == 1033 && to_host<int32_t>(r->view())[37] == 1070);
  });
  run("transpose on sliced views: shape, per-column null counts, and the transpose of the transpose is the input", [&] {
    auto p = transpose(table_view{{as, bs}});
    CHECK(p.first->size() == 76 && p.second.num_columns() == 38 && p.second.num_rows() == 2);
    for (int i = 0; i < 38; ++i) {
      int const row = 33 + i;
      auto const& col = p.second.column(i);
      CHECK(col.type().id() == type_id::INT32 && col.size() == 2);
      CHECK(col.null_count() == (row % 7 == 0) + (row % 5 == 0));
      CHECK(count0(valid_host(col)) == col.null_count());
      auto h = to_host<int32_t>(col);
      if (row % 7 != 0) CHECK(h[0] == row);
      if (row % 5 != 0) CHECK(h[1] == 1000 + row);
    }
    auto q = transpose(p.second);
    CHECK(q.second.num_columns() == 2 && q.second.num_rows() == 38);
    CHECK(valid_host(q.second.column(0)) == valid_host(as) && valid_host(q.second.column(1)) == valid_host(bs));
    CHECK(q.second.column(0).null_count() == as.null_count() && q.second.column(1).null_count() == bs.null_count());
    auto h0 = to_host<int32_t>(q.second.column(0)), h1 = to_host<int32_t>(q.second.column(1));
    auto v0 = valid_host(as), v1 = valid_host(bs);
    for (int i = 0; i < 38; ++i) {
      if (v0[i]) CHECK(h0[i] == 33 + i);
      if (v1[i]) CHECK(h1[i] == 1033 + i);
    }
    auto r = transpose(table_view{{cs, cs}});   // no nulls: no bitmap
    CHECK(!r.first->nullable() && r.second.column(5).null_count() == 0 && to_host<int32_t>(r.second.column(5)) == (I32{1038, 1038}));
  });
  run("tile on sliced views: the column count times, validity wraps, result types per column", [&] {
    auto d  = make_col(F64{0.5, 1.5, 2.5, 3.5, 4.5});
    auto ds = slice(d->view(), {1, 4})[0];
    auto as3 = slice(a->view(), {34, 37})[0];   // rows 34 35 36: 35 is null
    auto t  = tile(table_view{{as3, ds}}, 3);
    CHECK(t->num_columns() == 2 && t->num_rows() == 9);
    auto const& t0 = t->get_column(0);
    auto const& t1 = t->get_column(1);
    CHECK(t0.type().id() == type_id::INT32 && t1.type().id() == type_id::FLOAT64 && t0.null_count() == 3 && !t1.nullable());
    CHECK(valid_host(t0.view()) == (V{1, 0, 1, 1, 0, 1, 1, 0, 1}));
    auto h = to_host<int32_t>(t0.view());
    CHECK(h[0] == 34 && h[2] == 36 && h[3] == 34 && h[8] == 36);
    CHECK(to_host<double>(t1.view()) == (F64{1.5, 2.5, 3.5, 1.5, 2.5, 3.5, 1.5, 2.5, 3.5}));
    t = tile(table_view{{as}}, 1);
    CHECK(t->num_rows() == 38 && valid_host(t->get_column(0).view()) == valid_host(as) && t->get_column(0).null_count() == as.null_count());
  });
  run("repeat with a scalar count on sliced views", [&] {
    auto as3 = slice(a->view(), {34, 37})[0];
    auto t   = repeat(table_view{{as3, slice(c->view(), {34, 37})[0]}}, 2);
    CHECK(t->num_rows() == 6 && t->get_column(0).null_count() == 2 && !t->get_column(1).nullable());
    CHECK(valid_host(t->get_column(0).view()) == (V{1, 1, 0, 0, 1, 1}));
    CHECK(to_host<int32_t>(t->get_column(1).view()) == (I32{1034, 1034, 1035, 1035, 1036, 1036}));
    auto h = to_host<int32_t>(t->get_column(0).view());
    CHECK(h[0] == 34 && h[1] == 34 && h[4] == 36 && h[5] == 36);
  });
  run("repeat with a count column of each integral width, on sliced views; zero counts at both ends", [&] {
    auto as5 = slice(a->view(), {33, 38})[0];   // rows 33 34 35 36 37: 35 is null
    auto cs5 = slice(c->view(), {33, 38})[0];
    V const counts{0, 2, 3, 1, 0};
    I32 const want{1034, 1034, 1035, 1035, 1035, 1036};
    auto check = [&](column_view const& cnt) {
      auto t = repeat(table_view{{as5, cs5}}, cnt);
      CHECK(t->num_rows() == 6 && t->get_column(0).type().id() == type_id::INT32);
      CHECK(to_host<int32_t>(t->get_column(1).view()) == want && !t->get_column(1).nullable());
      CHECK(valid_host(t->get_column(0).view()) == (V{1, 1, 0, 0, 0, 1}) && t->get_column(0).null_count() == 3);
      auto h = to_host<int32_t>(t->get_column(0).view());
      CHECK(h[0] == 34 && h[1] == 34 && h[5] == 36);
    };
    check(make_col(I8{0, 2, 3, 1, 0})->view());
    {
      auto k = make_col(I8{9, 0, 2, 3, 1, 0, 9});
      check(slice(k->view(), {1, 6})[0]);   // the count column as a sliced view
    }
    check(make_col(I16{0, 2, 3, 1, 0})->view());
    check(make_col(I32{0, 2, 3, 1, 0})->view());
    check(make_col(I64{0, 2, 3, 1, 0})->view());
    check(make_col(std::vector<uint8_t>{0, 2, 3, 1, 0})->view());
    check(make_col(std::vector<uint16_t>{0, 2, 3, 1, 0})->view());
    check(make_col(std::vector<uint32_t>{0, 2, 3, 1, 0})->view());
    check(make_col(std::vector<uint64_t>{0, 2, 3, 1, 0})->view());
    auto t = repeat(table_view{{as5}}, make_col(I32{0, 0, 0, 0, 0})->view());
    CHECK(t->num_rows() == 0 && t->get_column(0).type().id() == type_id::INT32);
    auto big = make_col(I64{int64_t(1) << 30, int64_t(1) << 30, 0, 0, 0});   // a total of exactly 2^31
    CHECK(throws<std::overflow_error>([&] { (void)repeat(table_view{{as5}}, big->view()); }));
  });
  run("fill: a valid scalar validates the range, an invalid one nulls it; begin == end copies; on a sliced view", [&] {
    numeric_scalar<int32_t> seven{7}, none{7, false};
    auto r = fill(as, 1, 4, seven);   // rows 34..36 (35 was null)
    auto h = to_host<int32_t>(r->view());
    auto v = valid_host(r->view());
    CHECK(r->size() == 38 && h[0] == 33 && h[1] == 7 && h[2] == 7 && h[3] == 7 && h[4] == 37 && v[2] == 1);
    CHECK(r->null_count() == as.null_count() - 1 && count0(v) == r->null_count());
    r = fill(as, 1, 4, none);
    v = valid_host(r->view());
    CHECK(v[0] == 1 && v[1] == 0 && v[2] == 0 && v[3] == 0 && v[4] == 1 && r->null_count() == as.null_count() + 2);
    CHECK(to_host<int32_t>(r->view())[4] == 37);
    r = fill(cs, 0, 38, none);
    CHECK(r->null_count() == 38 && count0(valid_host(r->view())) == 38);
    r = fill(cs, 5, 5, seven);
    CHECK(!r->nullable() && to_host<int32_t>(r->view()) == to_host<int32_t>(cs));
    r = fill(cs, 37, 38, seven);
    CHECK(!r->nullable() && to_host<int32_t>(r->view())[37] == 7 && to_host<int32_t>(r->view())[36] == 1069);
    auto p = make_col(I32{1, 2, 3}, V{0, 0, 1});
    r      = fill(p->view(), 0, 2, seven);   // the last nulls go: no bitmap
    CHECK(!r->nullable() && r->null_count() == 0 && to_host<int32_t>(r->view()) == (I32{7, 7, 3}));
    numeric_scalar<int64_t> wrong{1};
    CHECK(throws<data_type_error>([&] { (void)fill(cs, 0, 1, wrong); }));
    CHECK(throws<std::out_of_range>([&] { (void)fill(cs, -1, 1, seven); }));
    CHECK(throws<std::out_of_range>([&] { (void)fill(cs, 0, 39, seven); }));
    CHECK(throws<std::out_of_range>([&] { (void)fill(cs, 3, 2, seven); }));
  });
  run("fill_in_place: on a sliced mutable view, values, bits and the null count; rows outside the view are kept", [&] {
    auto m  = make_col(I64{0, 1, 2, 3, 4, 5, 6, 7}, V{1, 0, 1, 0, 1, 0, 1, 0});
    auto mv = m->mutable_view();
    mutable_column_view part{mv.type(), 5, mv.head<void>(), mv.null_mask(), 2, 2};   // rows 2..6: nulls at 3 and 5
    numeric_scalar<int64_t> nine{9}, none{9, false};
    fill_in_place(part, 1, 3, nine);   // rows 3 and 4
    get_default_stream().synchronize();
    CHECK(part.null_count() == 1);
    CHECK(valid_host(m->view()) == (V{1, 0, 1, 1, 1, 0, 1, 0}));
    CHECK(to_host<int64_t>(m->view()) == (I64{0, 1, 2, 9, 9, 5, 6, 7}));
    fill_in_place(part, 3, 5, none);   // rows 5 and 6
    get_default_stream().synchronize();
    CHECK(part.null_count() == 2 && valid_host(m->view()) == (V{1, 0, 1, 1, 1, 0, 0, 0}));
    CHECK(to_host<int64_t>(m->view())[6] == 6);
    fill_in_place(part, 2, 2, nine);   // nothing
    auto plain = make_col(I64{1, 2, 3});
    auto pv    = plain->mutable_view();
    CHECK(throws<std::invalid_argument>([&] { fill_in_place(pv, 0, 1, none); }));
    CHECK(throws<std::out_of_range>([&] { fill_in_place(pv, 2, 4, nine); }));
    numeric_scalar<int32_t> wrong{1};
    CHECK(throws<data_type_error>([&] { fill_in_place(pv, 0, 1, wrong); }));
    fill_in_place(pv, 0, 3, nine);
    get_default_stream().synchronize();
    CHECK(to_host<int64_t>(plain->view()) == (I64{9, 9, 9}));
  });
  run("sequence: integers wrap, floats round twice, step defaults to 1; the throws", [&] {
    numeric_scalar<int8_t> i0{120}, i3{3};
    auto r = sequence(5, i0, i3);
    CHECK(r->type().id() == type_id::INT8 && !r->nullable());
    CHECK(to_host<int8_t>(r->view()) == (I8{120, 123, 126, static_cast<int8_t>(-127), static_cast<int8_t>(-124)}));
    numeric_scalar<int64_t> l0{10}, lm{-4};
    CHECK(to_host<int64_t>(sequence(4, l0, lm)->view()) == (I64{10, 6, 2, -2}));
    CHECK(to_host<int64_t>(sequence(3, l0)->view()) == (I64{10, 11, 12}));
    numeric_scalar<float> f0{1.0f / 3.0f}, fs{0.1f};
    auto hf = to_host<float>(sequence(64, f0, fs)->view());
    for (int i = 0; i < 64; ++i) {
      volatile float prod = static_cast<float>(i) * 0.1f;   // rounded to float before the sum
      volatile float want = (1.0f / 3.0f) + prod;
      float const w = want;
      CHECK(std::memcmp(&hf[i], &w, 4) == 0);
    }
    CHECK(sequence(0, l0, lm)->size() == 0 && sequence(0, l0)->type().id() == type_id::INT64);
    numeric_scalar<int32_t> w32{1};
    numeric_scalar<bool> b1{true};
    numeric_scalar<int64_t> invalid{1, false};
    CHECK(throws<data_type_error>([&] { (void)sequence(3, l0, w32); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(-1, l0, lm); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(-1, l0); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(3, invalid, lm); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(3, l0, invalid); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(3, invalid); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(3, b1, b1); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sequence(3, b1); }));
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
