// Host-only checks of the C++ drop-in surface: everything here is validated / computed BEFORE the first
// device call, so the binary runs without a GPU (tests/test_cpp_api.py::test_host_side_validation).
// The reference's tests pin the same behaviour: column_view_test.cpp / table_view tests (constructor checks,
// src/column/column_view.cpp:101-132), join_tests.cpp + hash_join.cu:49-58 (argument errors),
// groupby.cu:226-230 (size mismatch), sort_test.cpp MismatchInColumnOrderSize / MismatchInNullPrecedenceSize.
#include <cudf/aggregation.hpp>
#include <cudf/column/column_view.hpp>
#include <cudf/groupby.hpp>
#include <cudf/interop.hpp>
#include <cudf/join/distinct_hash_join.hpp>
#include <cudf/join/filtered_join.hpp>
#include <cudf/join/hash_join.hpp>
#include <cudf/sorting.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>

#include "../../cudf_amd/csrc/gx_dtype.hpp"     // plain C++: the dtype table behind every host-side dispatch (no HIP include)
#include "../../cudf_amd/csrc/gx_lds_book.hpp"  // plain C++: the bookkeeping behind gx::launch_lds (no HIP include)

#include <atomic>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
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

int main()
{
  // a "device pointer" that is never dereferenced on the host
  void const* fake = reinterpret_cast<void const*>(0x10000);
  auto const* fake_mask = reinterpret_cast<bitmask_type const*>(0x20000);

  run("types: sizes, traits, type_to_id (types.hpp:99-216, 278-341)", [] {
    CHECK(size_of(data_type{type_id::INT8}) == 1 && size_of(data_type{type_id::UINT16}) == 2);
    CHECK(size_of(data_type{type_id::FLOAT32}) == 4 && size_of(data_type{type_id::INT64}) == 8);
    CHECK(is_floating_point(data_type{type_id::FLOAT64}) && !is_floating_point(data_type{type_id::INT32}));
    CHECK(type_to_id<int32_t>() == type_id::INT32 && type_to_id<double>() == type_id::FLOAT64);
    CHECK(JoinNoMatch == std::numeric_limits<size_type>::min());
  });
  run("dtype table: every gx_dtype reaches the callable with its own row, anything else GX_EDTYPE and no call (csrc/gx_dtype.hpp)", [] {
    struct Row {
      int dtype;
      size_t value_size;
      bool is_signed, is_float;
      size_t word_size;
      int kind;  // 0 unsigned, 1 signed, 2 float
      bool is_bool;
    };
    const Row rows[] = {
      {GX_INT8, 1, true, false, 1, 1, false},    {GX_INT16, 2, true, false, 2, 1, false},   {GX_INT32, 4, true, false, 4, 1, false},
      {GX_INT64, 8, true, false, 8, 1, false},   {GX_UINT8, 1, false, false, 1, 0, false},  {GX_UINT16, 2, false, false, 2, 0, false},
      {GX_UINT32, 4, false, false, 4, 0, false}, {GX_UINT64, 8, false, false, 8, 0, false}, {GX_BOOL8, 1, false, false, 1, 0, true},
      {GX_FLOAT32, 4, true, true, 4, 2, false},  {GX_FLOAT64, 8, true, true, 8, 2, false},
    };
    CHECK(sizeof(rows) / sizeof(rows[0]) == 11);
    for (const Row& r : rows) {
      int calls    = 0;
      const int rc = gx::with_dtype(r.dtype, [&](auto t) {
        using D = decltype(t);
        using V = typename D::value_type;
        using W = typename D::word_type;
        ++calls;
        CHECK(sizeof(V) == r.value_size && std::is_signed<V>::value == r.is_signed && std::is_floating_point<V>::value == r.is_float);
        CHECK(sizeof(W) == r.word_size && std::is_unsigned<W>::value && std::is_integral<W>::value);
        CHECK((int)D::kind == r.kind && D::is_bool == r.is_bool);
        return 100 + r.dtype;
      });
      CHECK(calls == 1 && rc == 100 + r.dtype);  // the callable's own return code comes back
    }
    for (int bad : {0, -1, GX_BOOL8 + 1}) {
      int calls = 0;
      CHECK(gx::with_dtype(bad, [&](auto) { return ++calls; }) == GX_EDTYPE && calls == 0);
    }
  });
  run("launch layer: the dynamic-LDS limit is recorded per (kernel, device) (csrc/gx_lds_book.hpp)", [] {
    static gx::LdsBook book;  // (static: the table is too large for the stack)
    int ka = 0, kb = 0;       // two "kernels": only their addresses matter
    struct Call { const void* k; int bytes; };
    std::vector<Call> calls;
    int fail_with = 0;
    auto set = [&](const void* k, int bytes) {
      if (fail_with) return fail_with;
      calls.push_back({k, bytes});
      return 0;
    };
    CHECK(book.ensure(&ka, 0, 100, set) == 0 && calls.size() == 1 && calls[0].k == &ka && calls[0].bytes == 100);  // first request: one set
    CHECK(book.ensure(&ka, 0, 100, set) == 0 && book.ensure(&ka, 0, 40, set) == 0 && calls.size() == 1);           // same / smaller: none
    CHECK(book.ensure(&ka, 0, 0, set) == 0 && calls.size() == 1);
    CHECK(book.ensure(&ka, 0, 131072, set) == 0 && calls.size() == 2 && calls[1].k == &ka && calls[1].bytes == 131072);  // larger: one set, larger value
    CHECK(book.ensure(&ka, 0, 100, set) == 0 && calls.size() == 2);
    CHECK(book.ensure(&ka, 1, 100, set) == 0 && calls.size() == 3 && calls[2].k == &ka && calls[2].bytes == 100);  // another device: its own record
    CHECK(book.ensure(&ka, 1, 100, set) == 0 && calls.size() == 3);
    CHECK(book.ensure(&kb, 0, 64, set) == 0 && calls.size() == 4 && calls[3].k == &kb && calls[3].bytes == 64);    // the kernels are independent
    CHECK(book.ensure(&kb, 1, 64, set) == 0 && calls.size() == 5);
    CHECK(book.ensure(&ka, 0, 131072, set) == 0 && book.ensure(&ka, 1, 100, set) == 0 && calls.size() == 5);
    // a failing setter: its error comes back and the record stays, so the retry sets again
    fail_with = 719;
    CHECK(book.ensure(&kb, 0, 4096, set) == 719 && book.ensure(&kb, 0, 4096, set) == 719 && calls.size() == 5);
    CHECK(book.ensure(&kb, 0, 64, set) == 0);  // what was set before the failure still counts
    fail_with = 0;
    CHECK(book.ensure(&kb, 0, 4096, set) == 0 && calls.size() == 6 && calls[5].k == &kb && calls[5].bytes == 4096);
    CHECK(book.ensure(&kb, 0, 4096, set) == 0 && calls.size() == 6);
    // a device id the book has no room for is set on every launch (never skipped)
    CHECK(book.ensure(&kb, gx::LDS_BOOK_DEVICES, 8, set) == 0 && book.ensure(&kb, gx::LDS_BOOK_DEVICES, 8, set) == 0 && calls.size() == 8);
    CHECK(book.ensure(&kb, -1, 8, set) == 0 && calls.size() == 9);
    // 8 threads make the first launches of one (kernel, device): nobody "launches" before the limit covers its request
    // (sets may be repeated; they must never be missing and never lower the limit)
    for (int device = 0; device < 2; ++device) {
      int kc = 0;
      std::atomic<int> limit{0}, sets{0}, early{0}, lowered{0};
      auto set_mt = [&](const void*, int bytes) {
        if (bytes < limit.load()) ++lowered;
        std::this_thread::yield();  // widen the window between "set asked for" and "set done"
        limit.store(bytes);
        ++sets;
        return 0;
      };
      std::vector<std::thread> pool;
      for (int t = 0; t < 8; ++t)
        pool.emplace_back([&, t] {
          for (int i = 0; i < 2000; ++i) {
            const int bytes = 1024 * (1 + (i / 250)) + 16 * (t & 1);  // grows as the run goes on; two sizes in flight at a time
            if (book.ensure(&kc, device, bytes, set_mt) != 0 || limit.load() < bytes) ++early;
          }
        });
      for (auto& th : pool) th.join();
      CHECK(early == 0 && lowered == 0);
      CHECK(sets >= 8 && sets <= 16);  // 8 steps, each reached by the even or the odd size first
      CHECK(limit == 1024 * 8 + 16);
    }
  });
  run("column_view / table_view constructor checks (column_view.cpp:101-132, table_view.cpp)", [&] {
    column_view ok{data_type{type_id::INT32}, 5, fake, fake_mask, 2, 1};
    CHECK(ok.size() == 5 && ok.offset() == 1 && ok.null_count() == 2 && ok.nullable() && ok.has_nulls());
    CHECK(ok.data<int32_t>() == static_cast<int32_t const*>(fake) + 1);
    CHECK(throws<cudf::logic_error>([&] { column_view{data_type{type_id::INT32}, -1, fake, nullptr, 0}; }));
    CHECK(throws<cudf::logic_error>([&] { column_view{data_type{type_id::INT32}, 3, nullptr, nullptr, 0}; }));             // null data
    CHECK(throws<cudf::logic_error>([&] { column_view{data_type{type_id::INT32}, 3, fake, nullptr, 1}; }));     // nulls without a mask
    CHECK(throws<cudf::logic_error>([&] { column_view{data_type{type_id::INT32}, 3, fake, nullptr, 0, -1}; })); // negative offset
    column_view a{data_type{type_id::INT64}, 4, fake, nullptr, 0}, b{data_type{type_id::INT64}, 5, fake, nullptr, 0};
    CHECK(throws<cudf::logic_error>([&] { table_view{{a, b}}; }));                                              // column size mismatch
    table_view t{{a, a}};
    CHECK(t.num_columns() == 2 && t.num_rows() == 4);
    CHECK(t.select({1}).num_columns() == 1);
  });
  run("sort argument checks (sort_impl.cuh:45-52; sort_test.cpp Mismatch*)", [&] {
    column_view a{data_type{type_id::INT64}, 4, fake, nullptr, 0};
    table_view t{{a, a}};
    CHECK(throws<std::invalid_argument>([&] { (void)sorted_order(t, {order::ASCENDING}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sorted_order(t, {}, {null_order::BEFORE}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)sort(t, {order::ASCENDING, order::ASCENDING, order::ASCENDING}); }));
    column_view v{data_type{type_id::INT32}, 3, fake, nullptr, 0};
    CHECK(throws<std::invalid_argument>([&] { (void)sort_by_key(table_view{{v}}, t); }));                       // 3 value rows, 4 key rows
  });
  run("join argument checks (hash_join.cu:49-58, filtered_join.hpp:74-76, distinct_hash_join.hpp)", [&] {
    column_view a{data_type{type_id::INT64}, 0, nullptr, nullptr, 0};
    CHECK(throws<std::invalid_argument>([&] { hash_join hj{table_view{}, null_equality::EQUAL}; }));
    CHECK(throws<std::invalid_argument>([&] { hash_join hj{table_view{{a}}, nullable_join::NO, null_equality::EQUAL, 0.0}; }));
    CHECK(throws<std::invalid_argument>([&] { hash_join hj{table_view{{a}}, nullable_join::NO, null_equality::EQUAL, 1.5}; }));
    CHECK(throws<std::invalid_argument>([&] { distinct_hash_join dj{table_view{}}; }));
    CHECK(throws<std::invalid_argument>([&] { distinct_hash_join dj{table_view{{a}}, null_equality::EQUAL, -1.0}; }));
    CHECK(throws<std::invalid_argument>([&] { filtered_join fj{table_view{{a}}, null_equality::EQUAL, 0.0, get_default_stream()}; }));
  });
  run("groupby request checks (groupby.cu:226-230)", [&] {
    column_view keys{data_type{type_id::INT32}, 4, fake, nullptr, 0}, vals{data_type{type_id::FLOAT64}, 5, fake, nullptr, 0};
    groupby::groupby gb{table_view{{keys}}};
    std::vector<groupby::aggregation_request> reqs(1);
    reqs[0].values = vals;
    reqs[0].aggregations.emplace_back(make_sum_aggregation<groupby_aggregation>());
    CHECK(throws<std::invalid_argument>([&] { (void)gb.aggregate(reqs); }));
  });
  run("aggregation objects: kinds, ddof, equality, clone (aggregation.hpp)", [] {
    auto v1 = make_variance_aggregation<groupby_aggregation>();
    auto v2 = make_variance_aggregation<groupby_aggregation>(2);
    auto s1 = make_std_aggregation<groupby_aggregation>();
    CHECK(v1->kind == aggregation::VARIANCE && s1->kind == aggregation::STD);
    CHECK(!v1->is_equal(*v2) && !v1->is_equal(*s1) && v1->is_equal(*make_variance_aggregation<groupby_aggregation>(1)));
    auto c = v2->clone();
    CHECK(c->kind == aggregation::VARIANCE && c->is_equal(*v2) && c->do_hash() == v2->do_hash());
    CHECK(make_count_aggregation<groupby_aggregation>()->kind == aggregation::COUNT_VALID);
    CHECK(make_count_aggregation<groupby_aggregation>(null_policy::INCLUDE)->kind == aggregation::COUNT_ALL);
    CHECK(make_argmin_aggregation<groupby_aggregation>()->kind == aggregation::ARGMIN);
    CHECK(make_m2_aggregation<groupby_aggregation>()->kind == aggregation::M2);
  });
  run("Arrow schema export is host-only (interop.hpp:477-480)", [&] {
    column_view a{data_type{type_id::INT64}, 4, fake, nullptr, 0}, b{data_type{type_id::FLOAT32}, 4, fake, fake_mask, 1};
    std::vector<column_metadata> meta{{"k"}, {"v"}};
    auto s = to_arrow_schema(table_view{{a, b}}, meta);
    CHECK(std::string{s->format} == "+s" && s->n_children == 2 && s->release != nullptr);
    CHECK(std::string{s->children[0]->format} == "l" && std::string{s->children[0]->name} == "k" && s->children[0]->flags == 0);
    CHECK(std::string{s->children[1]->format} == "f" && (s->children[1]->flags & ARROW_FLAG_NULLABLE));
    CHECK(throws<std::invalid_argument>([&] { (void)to_arrow_schema(table_view{{a}}, meta); }));
    column_view bad{data_type{type_id::BOOL8}, 4, fake, nullptr, 0};
    CHECK(throws<cudf::data_type_error>([&] { (void)to_arrow_schema(table_view{{bad}}, std::vector<column_metadata>{{"x"}}); }));
    CHECK(throws<std::invalid_argument>([&] { (void)from_arrow_device(nullptr, nullptr); }));
  });
  std::printf("%d run, %d failed\n", g_run, g_failed);
  return g_failed ? 1 : 0;
}
