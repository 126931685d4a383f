// cudf::conditional_*_join over the C ABI (gx_conditional_join_count / _write; cudf_amd/csrc/gx_conditional_join.hip).
// reference: cpp/include/cudf/join/conditional_join.hpp, cpp/src/join/conditional_join.cu (a size pass, then a write pass that
// evaluates the predicate again).  The predicate is lowered by the tree walk compute_column uses (ast_lowering.hpp), with the table
// of every column reference in gx_expr_column::table; sliced views are read in place.  One host read per join: the two sizes of the
// count pass, which the allocation of the result needs.
#include "ast_lowering.hpp"
#include "common.hpp"

#include <cudf/join/conditional_join.hpp>

#include <limits>
#include <optional>
#include <stdexcept>
#include <string>

namespace cudf {
namespace {

constexpr std::size_t max_rows = static_cast<std::size_t>(std::numeric_limits<size_type>::max());

// one join: the lowered predicate, the scratch the count pass leaves for the write pass, the two sizes
struct conditional_join {
  detail::flat_expression f;
  int64_t n_left, n_right;
  int kind;
  rmm::cuda_stream_view stream;
  rmm::device_buffer tmp{};
  int64_t total{0}, left_total{0};

  conditional_join(table_view const& left, table_view const& right, ast::expression const& predicate, int kind_, rmm::cuda_stream_view s)
    : n_left{left.num_rows()}, n_right{right.num_rows()}, kind{kind_}, stream{s}
  {
    detail::flatten_expression(predicate, left, &right, stream, f);
    auto const type = detail::expression_result_type(f);
    CUDF_EXPECTS(type == GX_BOOL8, "The predicate of a conditional join must be a BOOL8 expression", cudf::data_type_error);
  }

  template <typename F>
  int call(F&& fn)
  {
    return fn(f.nodes.data(), static_cast<int>(f.nodes.size()), f.cols.data(), static_cast<int>(f.cols.size()), f.lits.data(),
              static_cast<int>(f.lits.size()), n_left, n_right, kind);
  }

  void count()
  {
    rmm::device_buffer sizes_dev{2 * sizeof(int64_t), stream};
    tmp = detail::run_with_scratch(
      [&](void* t, std::size_t* bytes) {
        return call([&](auto... head) {
          return gx_conditional_join_count(head..., static_cast<int64_t*>(sizes_dev.data()), t, bytes, detail::gxs(stream));
        });
      },
      "gx_conditional_join_count", stream);
    int64_t sizes[2] = {0, 0};
    CUDF_CUDA_TRY(hipMemcpyAsync(sizes, sizes_dev.data(), sizeof(sizes), hipMemcpyDeviceToHost, stream.value()));
    stream.synchronize();
    detail::throw_pending_sort_faults();  // a synchronisation point of this layer
    total      = sizes[0];
    left_total = sizes[1];
  }

  void check_size(std::optional<std::size_t> output_size) const
  {
    CUDF_EXPECTS(!output_size.has_value() || *output_size == static_cast<std::size_t>(total),
                 "output_size disagrees with the size of the join", std::invalid_argument);
    CUDF_EXPECTS(static_cast<std::size_t>(total) <= max_rows, "The conditional join has more than 2^31 - 1 rows", std::overflow_error);
  }

  void write(size_type* out_left, size_type* out_right)
  {
    detail::gx_check(call([&](auto... head) {
                       return gx_conditional_join_write(head..., total, left_total, tmp.data(), out_left, out_right, detail::gxs(stream));
                     }),
                     "gx_conditional_join_write");
  }
};

join_result pair_join(table_view const& left, table_view const& right, ast::expression const& predicate, int kind,
                      std::optional<std::size_t> output_size, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  conditional_join j{left, right, predicate, kind, stream};
  j.count();
  j.check_size(output_size);
  auto l = std::make_unique<rmm::device_uvector<size_type>>(static_cast<std::size_t>(j.total), stream, mr);
  auto r = std::make_unique<rmm::device_uvector<size_type>>(static_cast<std::size_t>(j.total), stream, mr);
  j.write(l->data(), r->data());
  return {std::move(l), std::move(r)};
}

std::unique_ptr<rmm::device_uvector<size_type>> row_join(table_view const& left, table_view const& right, ast::expression const& predicate,
                                                         int kind, std::optional<std::size_t> output_size, rmm::cuda_stream_view stream,
                                                         rmm::device_async_resource_ref mr)
{
  conditional_join j{left, right, predicate, kind, stream};
  j.count();
  j.check_size(output_size);
  auto l = std::make_unique<rmm::device_uvector<size_type>>(static_cast<std::size_t>(j.total), stream, mr);
  j.write(l->data(), nullptr);
  return l;
}

std::size_t join_size(table_view const& left, table_view const& right, ast::expression const& predicate, int kind, rmm::cuda_stream_view stream)
{
  conditional_join j{left, right, predicate, kind, stream};
  j.count();
  return static_cast<std::size_t>(j.total);
}

}  // namespace

join_result conditional_inner_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                   std::optional<std::size_t> output_size, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return pair_join(left, right, binary_predicate, GX_CJ_INNER, output_size, stream, mr);
}

join_result conditional_left_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                  std::optional<std::size_t> output_size, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return pair_join(left, right, binary_predicate, GX_CJ_LEFT, output_size, stream, mr);
}

join_result conditional_full_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                  rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return pair_join(left, right, binary_predicate, GX_CJ_FULL, std::nullopt, stream, mr);
}

std::unique_ptr<rmm::device_uvector<size_type>> conditional_left_semi_join(table_view const& left, table_view const& right,
                                                                           ast::expression const& binary_predicate,
                                                                           std::optional<std::size_t> output_size, rmm::cuda_stream_view stream,
                                                                           rmm::device_async_resource_ref mr)
{
  return row_join(left, right, binary_predicate, GX_CJ_SEMI, output_size, stream, mr);
}

std::unique_ptr<rmm::device_uvector<size_type>> conditional_left_anti_join(table_view const& left, table_view const& right,
                                                                           ast::expression const& binary_predicate,
                                                                           std::optional<std::size_t> output_size, rmm::cuda_stream_view stream,
                                                                           rmm::device_async_resource_ref mr)
{
  return row_join(left, right, binary_predicate, GX_CJ_ANTI, output_size, stream, mr);
}

std::size_t conditional_inner_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                        rmm::cuda_stream_view stream)
{
  return join_size(left, right, binary_predicate, GX_CJ_INNER, stream);
}
std::size_t conditional_left_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                       rmm::cuda_stream_view stream)
{
  return join_size(left, right, binary_predicate, GX_CJ_LEFT, stream);
}
std::size_t conditional_left_semi_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                            rmm::cuda_stream_view stream)
{
  return join_size(left, right, binary_predicate, GX_CJ_SEMI, stream);
}
std::size_t conditional_left_anti_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                            rmm::cuda_stream_view stream)
{
  return join_size(left, right, binary_predicate, GX_CJ_ANTI, stream);
}

}  // namespace cudf
