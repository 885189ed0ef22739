// dispatch.h — run-time values to compile-time template arguments, for every
// host function that launches a templated kernel.  Three visitors: the
// precision, the (dim, degree) pair, and a short list of ints (operator mode,
// geometry class, brick layers, flags).  Each calls a generic lambda with a
// tag and returns what the lambda returns.  Host only: no HIP here
// (tests/cpp/dispatch_check.cc compiles it alone).
#pragma once

#include "../../include/gls_op.h"

#include <stdexcept>
#include <string>
#include <type_traits>

namespace gls
{
// f(double{}) for GLS_F64, f(float{}) for GLS_F32; in f: using T = decltype(tag)
template <typename F>
auto
with_real(int prec, F &&f) -> decltype(f(double{}))
{
  if (prec == GLS_F64)
    return f(double{});
  if (prec == GLS_F32)
    return f(float{});
  throw std::runtime_error("precision must be GLS_F64 or GLS_F32, got " + std::to_string(prec));
}

// f(std::integral_constant<int, V>{}) for the V of the list that equals v;
// the list is the call site's: only the listed values are instantiated
template <int V, int... Rest, typename F>
auto
with_int(int v, const char *who, F &&f) -> decltype(f(std::integral_constant<int, V>{}))
{
  if (v == V)
    return f(std::integral_constant<int, V>{});
  if constexpr (sizeof...(Rest) > 0)
    return with_int<Rest...>(v, who, f);
  else
    throw std::runtime_error(std::string(who) + ": no kernel instantiation for value " +
                             std::to_string(v));
}

// the supported (dim, degree) pairs: the one list of them
template <int D, int K>
struct DimDegree
{};
template <typename... P>
struct DimDegreeList
{};
using SupportedDimDegrees = DimDegreeList<DimDegree<2, 1>, DimDegree<2, 2>, DimDegree<2, 3>,
                                          DimDegree<3, 1>, DimDegree<3, 2>, DimDegree<3, 3>>;

// f(integral_constant<int, D>{}, integral_constant<int, K>{}) for the
// supported pair (D, K) == (dim, k) of degree at most MAXK (pairs above MAXK
// are not instantiated: the multigrid transfers stop at Q2)
template <int MAXK, typename F, int D, int K, typename... Rest>
auto
with_dim_degree(int dim, int k, const char *who, F &&f, DimDegreeList<DimDegree<D, K>, Rest...>)
  -> decltype(f(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}))
{
  if constexpr (K <= MAXK)
    if (dim == D && k == K)
      return f(std::integral_constant<int, D>{}, std::integral_constant<int, K>{});
  if constexpr (sizeof...(Rest) > 0)
    return with_dim_degree<MAXK>(dim, k, who, f, DimDegreeList<Rest...>{});
  else
    throw std::runtime_error(std::string(who) + ": no kernel instantiation for (dim, degree) = (" +
                             std::to_string(dim) + ", " + std::to_string(k) + ")" +
                             (MAXK < 3 ? ", degree at most " + std::to_string(MAXK) : ""));
}

template <int MAXK = 3, typename F>
auto
with_dim_degree(int dim, int k, const char *who, F &&f)
  -> decltype(f(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}))
{
  return with_dim_degree<MAXK>(dim, k, who, f, SupportedDimDegrees{});
}
} // namespace gls
