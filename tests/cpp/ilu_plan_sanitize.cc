// ilu_plan_sanitize.cc — the ILU(k) host plan (csrc/ilu_plan.cc, host only)
// as a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_ilu_plan.py compiles and runs it): tridiagonal, 5-point
// Poisson and block matrices with fill levels 0 .. 2 and n, a row without a
// stored diagonal, chains on and off, every group width, refactorisation,
// and the error paths (zero pivot, unsorted columns, n = 0, bad indices).
// Each plan's schedule is checked (every row once, after its dependencies)
// and its solve against the exact answer where ILU is the exact LU.
#include "ilu_plan.h"

#include <cmath>
#include <cstdio>
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
tridiagonal(int64_t n)
{
  Csr A;
  A.n = n;
  A.rp.push_back(0);
  for (int64_t i = 0; i < n; ++i)
    {
      if (i > 0)
        A.ci.push_back(i - 1), A.v.push_back(-1.0 - 0.1 * (double)(i % 3));
      A.ci.push_back(i), A.v.push_back(2.5);
      if (i + 1 < n)
        A.ci.push_back(i + 1), A.v.push_back(-0.7);
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
                  A.v.push_back(nb == node && d == c ? 4.0 * b + 1.0 : -1.0 + 0.05 * (c - d));
                }
            }
          A.rp.push_back((int64_t)A.ci.size());
        }
  return A;
}

static std::vector<double>
multiply(const Csr &A, const std::vector<double> &x)
{
  std::vector<double> y((size_t)A.n, 0.0);
  for (int64_t i = 0; i < A.n; ++i)
    for (int64_t k = A.rp[(size_t)i]; k < A.rp[(size_t)i + 1]; ++k)
      y[(size_t)i] += A.v[(size_t)k] * x[(size_t)A.ci[(size_t)k]];
  return y;
}

static void
check_schedule(const gls::IluPlan &P, const gls::IluTri &T, bool chain_allowed)
{
  const int64_t        n = P.n;
  std::vector<int>     seen((size_t)n, 0);
  std::vector<uint8_t> done((size_t)n, 0);
  int32_t              pos = 0, lev = 0;
  for (const gls::IluLaunch &q : T.launches)
    {
      CHECK(q.pos0 == pos && q.lev0 == lev && q.pos1 > q.pos0 && q.lev1 > q.lev0);
      CHECK(chain_allowed || !q.chain);
      CHECK(q.chain || q.lev1 == q.lev0 + 1);
      for (int32_t l = q.lev0; l < q.lev1; ++l)
        {
          const int32_t p0 = T.lev_ptr[(size_t)l], p1 = T.lev_ptr[(size_t)l + 1];
          CHECK(!q.chain || p1 - p0 <= P.narrow);
          for (int32_t p = p0; p < p1; ++p)
            {
              const int32_t r = T.order[(size_t)p];
              CHECK(T.level[(size_t)r] == l);
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
}

static double
solve_error(const gls::IluPlan &P, const Csr &A)
{
  std::vector<double> x((size_t)A.n), got((size_t)A.n);
  for (int64_t i = 0; i < A.n; ++i)
    x[(size_t)i] = 1.0 + 0.01 * (double)(i % 17);
  const std::vector<double> b = multiply(A, x);
  gls::ilu_host_solve(P, got.data(), b.data());
  double e = 0;
  for (int64_t i = 0; i < A.n; ++i)
    e = std::fmax(e, std::fabs(got[(size_t)i] - x[(size_t)i]));
  return e;
}

static gls::IluPlan
plan(const Csr &A, int k, double atol, double rtol, gls::IluTuning t = gls::IluTuning())
{
  gls::IluParams p;
  p.fill_level = k, p.atol = atol, p.rtol = rtol;
  gls::IluPlan P = gls::ilu_make_plan(A.n, A.rp.data(), A.ci.data(), A.v.data(), p, t);
  check_schedule(P, P.L, t.chain != 0);
  check_schedule(P, P.U, t.chain != 0);
  return P;
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
  // ILU(0) of a tridiagonal matrix is its LU
  {
    const Csr    A = tridiagonal(37);
    gls::IluPlan P = plan(A, 0, 0.0, 1.0);
    CHECK((int)P.L.lev_ptr.size() - 1 == 37 && P.L.launches.size() == 1 && P.L.launches[0].chain);
    CHECK(solve_error(P, A) < 1e-13);
    gls::IluTuning t;
    t.chain = 0;
    P       = plan(A, 0, 0.0, 1.0, t);
    CHECK(P.L.launches.size() == 37 && P.U.launches.size() == 37);
    CHECK(solve_error(P, A) < 1e-13);
  }
  // fill level >= n is the LU; the fill and level counts of Poisson
  {
    const Csr A = poisson_block(5, 1);
    CHECK(solve_error(plan(A, 25, 0.0, 1.0), A) < 1e-13);
    for (int m : {6, 12})
      {
        const Csr B = poisson_block(m, 1);
        for (int k = 0; k < 3; ++k)
          {
            const gls::IluPlan P = plan(B, k, 0.0, 1.0);
            CHECK((int)P.L.lev_ptr.size() - 1 == (k + 2) * m - (k + 1));
            CHECK((int)P.U.lev_ptr.size() - 1 == (k + 2) * m - (k + 1));
            if (k == 1)
              CHECK((int64_t)P.ci.size() - B.rp.back() == 2 * (m - 1) * (m - 1));
          }
      }
  }
  // blocks, every group width, wide levels and chains mixed, refactor
  {
    const Csr A = poisson_block(12, 3);
    for (int g : {0, 1, 2, 4, 8, 16, 32, 64})
      for (int narrow : {0, 1, 3})
        {
          gls::IluTuning t;
          t.group = g, t.narrow = narrow;
          gls::IluPlan P = plan(A, 1, 1e-6, 1.0, t);
          CHECK(g == 0 || P.group == g);
          CHECK((P.group & (P.group - 1)) == 0 && P.group >= 1 && P.group <= 64);
          std::vector<double> v2(A.v);
          for (double &x : v2)
            x *= 1.5;
          const std::vector<double> before = P.val;
          gls::ilu_refactor(P, v2.data());
          check_schedule(P, P.L, true);
          Csr A2 = A;
          A2.v   = v2;
          const gls::IluPlan F = plan(A2, 1, 1e-6, 1.0, t);
          CHECK(F.val == P.val && F.dinv == P.dinv && F.L.v == P.L.v && F.U.v == P.U.v);
          CHECK(before != P.val);
        }
  }
  // a row without a stored diagonal gets one; atol gives it a pivot
  {
    Csr A = tridiagonal(9);
    // drop the diagonal of row 4 (entries: i-1, i, i+1)
    const int64_t k = A.rp[4] + 1;
    A.ci.erase(A.ci.begin() + k), A.v.erase(A.v.begin() + k);
    for (int64_t i = 5; i <= 9; ++i)
      A.rp[(size_t)i]--;
    const gls::IluPlan P = plan(A, 0, 0.0, 1.0);
    CHECK(P.ci[(size_t)P.diag[4]] == 4 && (int64_t)P.ci.size() == A.rp.back() + 1);
  }
  // error paths
  {
    Csr Z;
    Z.n = 2, Z.rp = {0, 1, 2}, Z.ci = {0, 1}, Z.v = {1.0, 0.0};
    CHECK(throws([&] { plan(Z, 0, 0.0, 1.0); }, "pivot in row 1"));
    Z.v = {1.0, std::nan("")};
    CHECK(throws([&] { plan(Z, 0, 0.0, 1.0); }, "pivot in row 1"));
    Csr U = tridiagonal(5);
    std::swap(U.ci[1], U.ci[2]);
    CHECK(throws([&] { plan(U, 0, 0.0, 1.0); }, "not sorted"));
    Csr E = tridiagonal(3);
    CHECK(throws([&] { gls::IluParams p; gls::ilu_make_plan(0, E.rp.data(), E.ci.data(),
                                                          E.v.data(), p, gls::IluTuning()); },
                 "empty"));
    Csr O = tridiagonal(3);
    O.ci.back() = 7;
    CHECK(throws([&] { plan(O, 0, 0.0, 1.0); }, "out of range"));
    CHECK(throws([&] { plan(tridiagonal(3), -1, 0.0, 1.0); }, "invalid parameters"));
    gls::IluTuning bad;
    bad.group = 3;
    CHECK(throws([&] { plan(tridiagonal(3), 0, 0.0, 1.0, bad); }, "invalid tuning"));
    gls::IluPlan P = plan(tridiagonal(4), 0, 0.0, 1.0);
    std::vector<double> zero((size_t)P.nnz_a, 0.0);
    CHECK(throws([&] { gls::ilu_refactor(P, zero.data()); }, "pivot in row 0"));
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
