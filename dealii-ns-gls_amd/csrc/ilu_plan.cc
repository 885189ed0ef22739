// ilu_plan.cc — ILU(k) on the host: pattern, values, level schedule and
// launch plan (ilu_plan.h has the rules and the tuning variables).
#include "ilu_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>

namespace gls
{
namespace
{
double
now_ms()
{
  using clk = std::chrono::steady_clock;
  return std::chrono::duration<double, std::milli>(clk::now().time_since_epoch()).count();
}

int
env_int(const char *name, int fallback)
{
  const char *s = std::getenv(name);
  if (!s || !*s)
    return fallback;
  char      *end = nullptr;
  const long v   = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < 0 || v > (1 << 30))
    throw std::runtime_error(std::string("ilu: ") + name + " is not a non-negative integer: " + s);
  return (int)v;
}

// level schedule of one factor: lower = rows ascending over the columns
// below the diagonal, upper = rows descending over the columns above it
void
schedule(const IluPlan &P, bool lower, IluTri &T)
{
  const int64_t n = P.n;
  T.level.assign((size_t)n, 0);
  int32_t n_levels = 0;
  for (int64_t s = 0; s < n; ++s)
    {
      const int64_t i  = lower ? s : n - 1 - s;
      const int64_t k0 = lower ? P.rp[(size_t)i] : P.diag[(size_t)i] + 1;
      const int64_t k1 = lower ? P.diag[(size_t)i] : P.rp[(size_t)i + 1];
      int32_t       l  = 0;
      for (int64_t k = k0; k < k1; ++k)
        l = std::max(l, T.level[(size_t)P.ci[(size_t)k]] + 1);
      T.level[(size_t)i] = l;
      n_levels           = std::max(n_levels, l + 1);
    }
  // positions: level by level, ascending row inside a level
  T.lev_ptr.assign((size_t)n_levels + 1, 0);
  for (int64_t i = 0; i < n; ++i)
    T.lev_ptr[(size_t)T.level[(size_t)i] + 1]++;
  T.max_level_rows = 0;
  for (int32_t l = 0; l < n_levels; ++l)
    {
      T.max_level_rows = std::max(T.max_level_rows, T.lev_ptr[(size_t)l + 1]);
      T.lev_ptr[(size_t)l + 1] += T.lev_ptr[(size_t)l];
    }
  T.order.resize((size_t)n);
  std::vector<int32_t> fill(T.lev_ptr.begin(), T.lev_ptr.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    T.order[(size_t)fill[(size_t)T.level[(size_t)i]]++] = (int32_t)i;
  T.rp.assign((size_t)n + 1, 0);
  T.ci.clear(), T.from.clear();
  for (int64_t p = 0; p < n; ++p)
    {
      const int64_t i  = T.order[(size_t)p];
      const int64_t k0 = lower ? P.rp[(size_t)i] : P.diag[(size_t)i] + 1;
      const int64_t k1 = lower ? P.diag[(size_t)i] : P.rp[(size_t)i + 1];
      for (int64_t k = k0; k < k1; ++k)
        {
          T.ci.push_back(P.ci[(size_t)k]);
          T.from.push_back(k);
        }
      T.rp[(size_t)p + 1] = (int32_t)T.ci.size();
    }
  T.v.assign(T.ci.size(), 0.0);
}

void
plan_launches(const std::vector<int32_t> &lev_ptr, int chain, int narrow,
              std::vector<IluLaunch> &launches)
{
  launches.clear();
  const int32_t n_levels = (int32_t)lev_ptr.size() - 1;
  for (int32_t l = 0; l < n_levels;)
    {
      IluLaunch q;
      q.lev0 = l, q.pos0 = lev_ptr[(size_t)l];
      const auto rows = [&](int32_t k) { return lev_ptr[(size_t)k + 1] - lev_ptr[(size_t)k]; };
      if (chain && rows(l) <= narrow)
        {
          q.chain = 1;
          while (l < n_levels && rows(l) <= narrow)
            ++l;
        }
      else
        ++l;
      q.lev1 = l, q.pos1 = lev_ptr[(size_t)l];
      launches.push_back(q);
    }
}
} // namespace

IluTuning
ilu_tuning_from_env()
{
  IluTuning t;
  t.chain  = env_int("GLS_ILU_CHAIN", 1) != 0;
  t.group  = env_int("GLS_ILU_GROUP", 0);
  t.narrow = env_int("GLS_ILU_NARROW", 0);
  t.factor_chain  = env_int("GLS_ILU_FACTOR_CHAIN", 1) != 0;
  t.factor_narrow = env_int("GLS_ILU_FACTOR_NARROW", 0);
  if (t.group != 0 && (t.group > 64 || (t.group & (t.group - 1)) != 0))
    throw std::runtime_error("ilu: GLS_ILU_GROUP must be a power of two in [1, 64]");
  return t;
}

IluPlan
ilu_make_plan(int64_t n, const int64_t *row_ptr, const int64_t *cols, const double *vals,
              const IluParams &prm, const IluTuning &tuning)
{
  if (!vals)
    throw std::runtime_error("ilu: empty matrix or null argument");
  IluPlan P = ilu_make_symbolic(n, row_ptr, cols, prm, tuning);
  ilu_refactor(P, vals);
  return P;
}

IluPlan
ilu_make_symbolic(int64_t n, const int64_t *row_ptr, const int64_t *cols, const IluParams &prm,
                  const IluTuning &tuning)
{
  if (n <= 0 || !row_ptr || !cols)
    throw std::runtime_error("ilu: empty matrix or null argument");
  if (n >= (int64_t)0x7fffffff)
    throw std::runtime_error("ilu: n does not fit the 32-bit device indices");
  if (prm.fill_level < 0 || !std::isfinite(prm.atol) || !std::isfinite(prm.rtol))
    throw std::runtime_error("ilu: invalid parameters (fill_level < 0 or non-finite atol / rtol)");
  if (tuning.group < 0 || tuning.group > 64 || (tuning.group & (tuning.group - 1)) != 0 ||
      tuning.narrow < 0 || tuning.factor_narrow < 0)
    throw std::runtime_error("ilu: invalid tuning (group: a power of two in [1, 64])");
  if (row_ptr[0] != 0)
    throw std::runtime_error("ilu: row_ptr[0] != 0");
  for (int64_t i = 0; i < n; ++i)
    {
      if (row_ptr[i + 1] < row_ptr[i])
        throw std::runtime_error("ilu: row_ptr decreases at row " + std::to_string(i));
      for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
        {
          if (cols[k] < 0 || cols[k] >= n)
            throw std::runtime_error("ilu: column index out of range in row " + std::to_string(i));
          if (k > row_ptr[i] && cols[k] <= cols[k - 1])
            throw std::runtime_error("ilu: columns of row " + std::to_string(i) +
                                     " are not sorted (ascending, no repeats)");
        }
    }
  const double t0 = now_ms();
  IluPlan      P;
  P.n      = n;
  P.nnz_a  = row_ptr[n];
  P.prm    = prm;
  P.tuning = tuning;
  // ---- symbolic: row by row; the finished rows' upper parts with their
  // levels are what a later row merges
  std::vector<int32_t> lev; // level of fill of each pattern entry
  P.rp.assign((size_t)n + 1, 0);
  P.diag.assign((size_t)n, 0);
  P.a_to_f.resize((size_t)P.nnz_a);
  const int             kmax = prm.fill_level;
  std::map<int32_t, int> row;
  for (int64_t i = 0; i < n; ++i)
    {
      row.clear();
      for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
        row.emplace((int32_t)cols[k], 0);
      row.emplace((int32_t)i, 0); // no-op when the diagonal is stored
      if (kmax > 0)
        // a pivot adds columns beyond itself only, so the walk meets them
        for (auto it = row.begin(); it != row.end() && it->first < i; ++it)
          {
            const int32_t p  = it->first;
            const int     li = it->second;
            for (int64_t k = P.diag[(size_t)p] + 1; k < P.rp[(size_t)p + 1]; ++k)
              {
                const int l = li + lev[(size_t)k] + 1;
                if (l > kmax)
                  continue;
                auto ins = row.emplace(P.ci[(size_t)k], l);
                if (!ins.second && ins.first->second > l)
                  ins.first->second = l;
              }
          }
      for (const auto &e : row)
        {
          if (e.first == i)
            P.diag[(size_t)i] = (int64_t)P.ci.size();
          P.ci.push_back(e.first);
          lev.push_back(e.second);
        }
      P.rp[(size_t)i + 1] = (int64_t)P.ci.size();
      if (P.rp[(size_t)i + 1] >= (int64_t)0x7fffffff)
        throw std::runtime_error("ilu: the factor's entries do not fit the 32-bit device indices");
      // where A's entries went (both sorted)
      int64_t f = P.rp[(size_t)i];
      for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k)
        {
          while (P.ci[(size_t)f] != cols[k])
            ++f;
          P.a_to_f[(size_t)k] = f;
        }
    }
  P.val.assign(P.ci.size(), 0.0);
  P.dinv.assign((size_t)n, 0.0);
  // ---- schedule and launches
  schedule(P, true, P.L);
  schedule(P, false, P.U);
  const double mean = (double)(P.L.ci.size() + P.U.ci.size()) / (2.0 * (double)n);
  int          g    = tuning.group;
  if (g == 0)
    for (g = 4; g < 64 && (double)g < mean; g *= 2)
      ;
  P.group  = g;
  P.narrow = tuning.narrow > 0 ? tuning.narrow : ILU_CHAIN_THREADS / g;
  plan_launches(P.L.lev_ptr, tuning.chain, P.narrow, P.L.launches);
  plan_launches(P.U.lev_ptr, tuning.chain, P.narrow, P.U.launches);
  // ---- the factorisation's launches over the schedule of L
  for (int64_t i = 0; i < n; ++i)
    P.max_row = std::max(P.max_row, P.rp[(size_t)i + 1] - P.rp[(size_t)i]);
  P.factor_group = tuning.group > 0 ? tuning.group : std::min(64, 2 * g);
  P.factor_rows  = (int)std::max<int64_t>(
    1, std::min<int64_t>(ILU_CHAIN_THREADS / P.factor_group, ILU_FACTOR_MAX_ROW / P.max_row));
  P.factor_narrow = tuning.factor_narrow > 0 ? tuning.factor_narrow : P.factor_rows;
  plan_launches(P.L.lev_ptr, tuning.factor_chain, P.factor_narrow, P.factor_launches);
  P.symbolic_ms = now_ms() - t0;
  return P;
}

void
ilu_refactor(IluPlan &P, const double *vals)
{
  if (!vals)
    throw std::runtime_error("ilu: null values");
  const double  t0 = now_ms();
  const int64_t n  = P.n;
  std::fill(P.val.begin(), P.val.end(), 0.0);
  for (int64_t k = 0; k < P.nnz_a; ++k)
    P.val[(size_t)P.a_to_f[(size_t)k]] = vals[k];
  // Ifpack's diagonal modification, on every row before the elimination
  for (int64_t i = 0; i < n; ++i)
    {
      double &d = P.val[(size_t)P.diag[(size_t)i]];
      d         = P.prm.rtol * d + (d < 0.0 ? -P.prm.atol : P.prm.atol);
    }
  std::vector<int64_t> where((size_t)n, -1); // column -> position in the current row
  double               min_pivot = HUGE_VAL;
  for (int64_t i = 0; i < n; ++i)
    {
      const int64_t r0 = P.rp[(size_t)i], r1 = P.rp[(size_t)i + 1], di = P.diag[(size_t)i];
      for (int64_t k = r0; k < r1; ++k)
        where[(size_t)P.ci[(size_t)k]] = k;
      for (int64_t k = r0; k < di; ++k)
        {
          const int64_t p = P.ci[(size_t)k];
          const double  l = P.val[(size_t)k] / P.val[(size_t)P.diag[(size_t)p]];
          P.val[(size_t)k] = l;
          for (int64_t q = P.diag[(size_t)p] + 1; q < P.rp[(size_t)p + 1]; ++q)
            {
              const int64_t w = where[(size_t)P.ci[(size_t)q]];
              if (w >= 0)
                P.val[(size_t)w] -= l * P.val[(size_t)q];
            }
        }
      for (int64_t k = r0; k < r1; ++k)
        where[(size_t)P.ci[(size_t)k]] = -1;
      const double piv = P.val[(size_t)di];
      if (piv == 0.0 || !std::isfinite(piv))
        throw std::runtime_error("ilu: zero or non-finite pivot in row " + std::to_string(i) +
                                 " (value " + std::to_string(piv) + ")");
      P.dinv[(size_t)i] = 1.0 / piv;
      min_pivot         = std::min(min_pivot, std::fabs(piv));
    }
  P.min_pivot = min_pivot;
  for (IluTri *T : {&P.L, &P.U})
    for (size_t k = 0; k < T->from.size(); ++k)
      T->v[k] = P.val[(size_t)T->from[k]];
  P.numeric_ms = now_ms() - t0;
}

void
ilu_refactor_scheduled(IluPlan &P, const double *vals)
{
  if (!vals)
    throw std::runtime_error("ilu: null values");
  const double  t0 = now_ms();
  const int64_t n  = P.n;
  // what k_ilu_load does
  std::fill(P.val.begin(), P.val.end(), 0.0);
  for (int64_t k = 0; k < P.nnz_a; ++k)
    P.val[(size_t)P.a_to_f[(size_t)k]] = vals[k];
  for (int64_t i = 0; i < n; ++i)
    {
      double &d = P.val[(size_t)P.diag[(size_t)i]];
      d         = P.prm.rtol * d + (d < 0.0 ? -P.prm.atol : P.prm.atol);
    }
  // what k_ilu_factor_level / k_ilu_factor_chain do, row by row
  std::vector<double>  sv((size_t)P.max_row);
  std::vector<int32_t> sc((size_t)P.max_row);
  for (const IluLaunch &lq : P.factor_launches)
    for (int32_t pos = lq.pos0; pos < lq.pos1; ++pos)
      {
        const int64_t i   = P.L.order[(size_t)pos];
        const int64_t r0  = P.rp[(size_t)i];
        const int32_t len = (int32_t)(P.rp[(size_t)i + 1] - r0);
        const int32_t nl  = (int32_t)(P.diag[(size_t)i] - r0);
        for (int32_t e = 0; e < len; ++e)
          sv[(size_t)e] = P.val[(size_t)(r0 + e)], sc[(size_t)e] = P.ci[(size_t)(r0 + e)];
        for (int32_t k = 0; k < nl; ++k)
          {
            const int64_t p = sc[(size_t)k];
            const double  l = sv[(size_t)k] / P.val[(size_t)P.diag[(size_t)p]];
            sv[(size_t)k]   = l;
            for (int64_t q = P.diag[(size_t)p] + 1; q < P.rp[(size_t)p + 1]; ++q)
              {
                const int32_t c  = P.ci[(size_t)q];
                int32_t       lo = k + 1, hi = len; // the first staged column >= c
                while (lo < hi)
                  {
                    const int32_t mid = lo + (hi - lo) / 2;
                    if (sc[(size_t)mid] < c)
                      lo = mid + 1;
                    else
                      hi = mid;
                  }
                if (lo < len && sc[(size_t)lo] == c)
                  sv[(size_t)lo] -= l * P.val[(size_t)q];
              }
          }
        for (int32_t e = 0; e < len; ++e)
          P.val[(size_t)(r0 + e)] = sv[(size_t)e];
      }
  // what k_ilu_store does
  for (IluTri *T : {&P.L, &P.U})
    for (size_t k = 0; k < T->from.size(); ++k)
      T->v[k] = P.val[(size_t)T->from[k]];
  double  min_pivot = HUGE_VAL;
  int64_t bad       = -1;
  for (int64_t i = 0; i < n; ++i)
    {
      const double piv  = P.val[(size_t)P.diag[(size_t)i]];
      P.dinv[(size_t)i] = 1.0 / piv;
      if (piv == 0.0 || !std::isfinite(piv))
        bad = bad < 0 ? i : bad;
      else
        min_pivot = std::min(min_pivot, std::fabs(piv));
    }
  P.numeric_ms = now_ms() - t0;
  if (bad >= 0)
    throw std::runtime_error("ilu: zero or non-finite pivot in row " + std::to_string(bad) +
                             " (value " +
                             std::to_string(P.val[(size_t)P.diag[(size_t)bad]]) + ")");
  P.min_pivot = min_pivot;
}

void
ilu_host_solve(const IluPlan &P, double *dst, const double *src)
{
  for (const IluLaunch &q : P.L.launches)
    for (int32_t p = q.pos0; p < q.pos1; ++p)
      {
        double s = 0;
        for (int32_t k = P.L.rp[(size_t)p]; k < P.L.rp[(size_t)p + 1]; ++k)
          s += P.L.v[(size_t)k] * dst[(size_t)P.L.ci[(size_t)k]];
        const int32_t r = P.L.order[(size_t)p];
        dst[(size_t)r]  = src[(size_t)r] - s;
      }
  for (const IluLaunch &q : P.U.launches)
    for (int32_t p = q.pos0; p < q.pos1; ++p)
      {
        double s = 0;
        for (int32_t k = P.U.rp[(size_t)p]; k < P.U.rp[(size_t)p + 1]; ++k)
          s += P.U.v[(size_t)k] * dst[(size_t)P.U.ci[(size_t)k]];
        const int32_t r = P.U.order[(size_t)p];
        dst[(size_t)r]  = (dst[(size_t)r] - s) * P.dinv[(size_t)r];
      }
}
} // namespace gls
