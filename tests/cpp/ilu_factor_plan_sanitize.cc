// ilu_factor_plan_sanitize.cc — the host side of the device ILU(k)
// factorisation (csrc/ilu_plan.cc, host only) as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_ilu_factor_plan.py
// compiles and runs it): ilu_make_symbolic, the factor launch plan (chains on
// and off, narrow thresholds, every group width) and ilu_refactor_scheduled,
// which must equal ilu_refactor bit for bit, on tridiagonal, Poisson and block
// matrices with fill levels 0 .. 2, a row without a stored diagonal, rows
// without L entries, refactorisation, and the bad-pivot paths.
#include "ilu_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                      \
  do                                                                     \
    {                                                                    \
      if (!(cond))                                                       \
        {                                                                \
          ++failures;                                                    \
          std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
        }                                                                \
    }                                                                    \
  while (0)

struct Csr
{
  int64_t              n = 0;
  std::vector<int64_t> rp, ci;
  std::vector<double>  v;
};

static Csr
tridiagonal(int64_t n, double d = 2.5, double lo = -1.0, double up = -0.7)
{
  Csr A;
  A.n = n;
  A.rp.push_back(0);
  for (int64_t i = 0; i < n; ++i)
    {
      if (i > 0)
        A.ci.push_back(i - 1), A.v.push_back(lo);
      A.ci.push_back(i), A.v.push_back(d);
      if (i + 1 < n)
        A.ci.push_back(i + 1), A.v.push_back(up);
      A.rp.push_back((int64_t)A.ci.size());
    }
  return A;
}

// m x m 5-point stencil with b x b dense blocks (b = 1: Poisson)
static Csr
poisson_block(int m, int b)
{
  Csr A;
  A.n = (int64_t)m * m * b;
  A.rp.push_back(0);
  for (int y = 0; y < m; ++y)
    for (int x = 0; x < m; ++x)
      for (int c = 0; c < b; ++c)
        {
          const int64_t node = (int64_t)y * m + x;
          const int     dx[5] = {0, -1, 0, 1, 0}, dy[5] = {-1, 0, 0, 0, 1};
          for (int k = 0; k < 5; ++k)
            {
              const int xx = x + dx[k], yy = y + dy[k];
              if (xx < 0 || xx >= m || yy < 0 || yy >= m)
                continue;
              const int64_t nb = (int64_t)yy * m + xx;
              for (int d = 0; d < b; ++d)
                {
                  A.ci.push_back(nb * b + d);
                  A.v.push_back(nb == node && d == c ? 4.0 * b + 1.0 :
                                                       -1.0 + 0.05 * (c - d) + 0.01 * (double)(k % 3));
                }
            }
          A.rp.push_back((int64_t)A.ci.size());
        }
  return A;
}

static bool
same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
  return a.size() == b.size() &&
         (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

// every row in exactly one launch, after every row of its L pattern
static void
check_factor_launches(const gls::IluPlan &P)
{
  const gls::IluTri   &T = P.L;
  const int64_t        n = P.n;
  std::vector<int>     seen((size_t)n, 0);
  std::vector<uint8_t> done((size_t)n, 0);
  int32_t              pos = 0, lev = 0;
  for (const gls::IluLaunch &q : P.factor_launches)
    {
      CHECK(q.pos0 == pos && q.lev0 == lev && q.pos1 > q.pos0 && q.lev1 > q.lev0);
      CHECK(P.tuning.factor_chain || !q.chain);
      CHECK(q.chain || q.lev1 == q.lev0 + 1);
      for (int32_t l = q.lev0; l < q.lev1; ++l)
        {
          const int32_t p0 = T.lev_ptr[(size_t)l], p1 = T.lev_ptr[(size_t)l + 1];
          CHECK(!q.chain || p1 - p0 <= P.factor_narrow);
          CHECK(q.chain || !P.tuning.factor_chain || p1 - p0 > P.factor_narrow);
          for (int32_t p = p0; p < p1; ++p)
            {
              const int32_t r = T.order[(size_t)p];
              seen[(size_t)r]++;
              for (int32_t k = T.rp[(size_t)p]; k < T.rp[(size_t)p + 1]; ++k)
                CHECK(done[(size_t)T.ci[(size_t)k]]);
            }
          for (int32_t p = p0; p < p1; ++p)
            done[(size_t)T.order[(size_t)p]] = 1;
        }
      pos = q.pos1, lev = q.lev1;
    }
  CHECK(pos == n && lev == (int32_t)T.lev_ptr.size() - 1);
  for (int s : seen)
    CHECK(s == 1);
  int64_t longest = 0;
  for (int64_t i = 0; i < n; ++i)
    longest = std::max(longest, P.rp[(size_t)i + 1] - P.rp[(size_t)i]);
  CHECK(P.max_row == longest);
  CHECK(P.factor_rows >= 1 && P.factor_rows * P.factor_group <= gls::ILU_CHAIN_THREADS);
  CHECK((int64_t)P.factor_rows * P.max_row * gls::ILU_FACTOR_ROW_BYTES <= gls::ILU_FACTOR_LDS_BYTES);
}

// the scheduled factorisation against the row-by-row one, bit for bit
static void
compare(const Csr &A, int k, double atol, double rtol, gls::IluTuning t = gls::IluTuning())
{
  gls::IluParams p;
  p.fill_level = k, p.atol = atol, p.rtol = rtol;
  const gls::IluPlan R = gls::ilu_make_plan(A.n, A.rp.data(), A.ci.data(), A.v.data(), p, t);
  gls::IluPlan       S = gls::ilu_make_symbolic(A.n, A.rp.data(), A.ci.data(), p, t);
  CHECK(S.rp == R.rp && S.ci == R.ci && S.diag == R.diag && S.a_to_f == R.a_to_f);
  CHECK(S.L.launches.size() == R.L.launches.size() && S.U.launches.size() == R.U.launches.size());
  check_factor_launches(S);
  gls::ilu_refactor_scheduled(S, A.v.data());
  CHECK(same_bits(S.val, R.val) && same_bits(S.dinv, R.dinv));
  CHECK(same_bits(S.L.v, R.L.v) && same_bits(S.U.v, R.U.v));
  CHECK(S.min_pivot == R.min_pivot);
  // new values on the same plan, in either order of the two routines
  std::vector<double> v2(A.v);
  for (size_t i = 0; i < v2.size(); ++i)
    v2[i] *= 1.0 + 0.3 * std::sin((double)i);
  gls::IluPlan R2 = R;
  gls::ilu_refactor(R2, v2.data());
  gls::ilu_refactor_scheduled(S, v2.data());
  CHECK(same_bits(S.val, R2.val) && same_bits(S.dinv, R2.dinv) && S.min_pivot == R2.min_pivot);
  gls::ilu_refactor_scheduled(R2, A.v.data());
  CHECK(same_bits(R2.val, R.val) && same_bits(R2.L.v, R.L.v) && same_bits(R2.U.v, R.U.v));
}

template <typename F>
static bool
throws(F f, const char *needle)
{
  try
    {
      f();
    }
  catch (const std::runtime_error &e)
    {
      return std::string(e.what()).find(needle) != std::string::npos;
    }
  return false;
}

int
main()
{
  // one chain of one-row levels; chains off: one launch per level
  {
    const Csr      A = tridiagonal(257);
    gls::IluParams p;
    gls::IluPlan   S = gls::ilu_make_symbolic(A.n, A.rp.data(), A.ci.data(), p, gls::IluTuning());
    CHECK(S.factor_launches.size() == 1 && S.factor_launches[0].chain && S.max_row == 3);
    compare(A, 0, 0.0, 1.0);
    gls::IluTuning t;
    t.factor_chain = 0;
    S = gls::ilu_make_symbolic(A.n, A.rp.data(), A.ci.data(), p, t);
    CHECK(S.factor_launches.size() == 257);
    CHECK(S.L.launches.size() == 1); // the solves' chains are another switch
    compare(A, 0, 0.0, 1.0, t);
  }
  // fill levels, blocks, every group width, narrow thresholds
  for (int k = 0; k < 3; ++k)
    compare(poisson_block(12, 1), k, 0.0, 1.0);
  compare(poisson_block(5, 1), 25, 0.0, 1.0); // full fill
  {
    const Csr A = poisson_block(12, 3);
    for (int g : {0, 1, 2, 4, 8, 16, 32, 64})
      for (int narrow : {0, 1, 3, 1000})
        for (int chain : {1, 0})
          {
            gls::IluTuning t;
            t.group = g, t.factor_narrow = narrow, t.factor_chain = chain;
            compare(A, 1, 1e-6, 1.1, t);
          }
    gls::IluTuning t;
    t.factor_narrow = 1;
    gls::IluParams p;
    p.fill_level = 1;
    const gls::IluPlan S = gls::ilu_make_symbolic(A.n, A.rp.data(), A.ci.data(), p, t);
    for (const gls::IluLaunch &q : S.factor_launches)
      CHECK(q.chain == (q.pos1 - q.pos0 == q.lev1 - q.lev0)); // one-row levels only
  }
  // rows without L entries (a diagonal matrix: one level)
  {
    Csr D;
    D.n = 5, D.rp = {0, 1, 2, 3, 4, 5}, D.ci = {0, 1, 2, 3, 4}, D.v = {2.0, -3.0, 0.5, 4.0, -1.5};
    compare(D, 0, 1e-12, 1.0);
    compare(D, 0, 0.25, 1.5);
  }
  // a row without a stored diagonal: a fill position A does not have
  {
    Csr           A = tridiagonal(9);
    const int64_t k = A.rp[4] + 1;
    A.ci.erase(A.ci.begin() + k), A.v.erase(A.v.begin() + k);
    for (int64_t i = 5; i <= 9; ++i)
      A.rp[(size_t)i]--;
    compare(A, 0, 1e-3, 1.0);
    compare(A, 2, 1e-3, 1.0);
  }
  // bad pivots: the smallest bad row, the one ilu_refactor names
  {
    const Csr      A = tridiagonal(9, 1.0, 1.0, 1.0); // u_11 = 1 - 1 * 1
    gls::IluParams p;
    gls::IluPlan   S = gls::ilu_make_symbolic(A.n, A.rp.data(), A.ci.data(), p, gls::IluTuning());
    CHECK(throws([&] { gls::ilu_refactor_scheduled(S, A.v.data()); }, "pivot in row 1"));
    CHECK(throws([&] { gls::ilu_refactor(S, A.v.data()); }, "pivot in row 1"));
    std::vector<double> zero(A.v.size(), 0.0);
    CHECK(throws([&] { gls::ilu_refactor_scheduled(S, zero.data()); }, "pivot in row 0"));
    std::vector<double> bad(tridiagonal(9).v);
    bad[(size_t)A.rp[5] + 1] = std::nan("");
    CHECK(throws([&] { gls::ilu_refactor_scheduled(S, bad.data()); }, "pivot in row 5"));
    const Csr G = tridiagonal(9);
    gls::ilu_refactor_scheduled(S, G.v.data()); // and a good factorisation afterwards
    gls::IluPlan R = gls::ilu_make_plan(G.n, G.rp.data(), G.ci.data(), G.v.data(), p, gls::IluTuning());
    CHECK(same_bits(S.val, R.val));
    CHECK(throws([&] { gls::ilu_refactor_scheduled(S, nullptr); }, "null"));
    gls::IluTuning t;
    t.factor_narrow = -1;
    CHECK(throws([&] { gls::ilu_make_symbolic(G.n, G.rp.data(), G.ci.data(), p, t); },
                 "invalid tuning"));
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
