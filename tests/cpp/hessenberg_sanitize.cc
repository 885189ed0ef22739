// hessenberg_sanitize.cc — csrc/hessenberg.h (the host least squares of the
// device GMRES solvers) as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_hessenberg.py builds and runs it).
//
// Random upper-Hessenberg matrices with m = 28 columns, fixed seeds, the
// sub-diagonal in [0.5, 1.5], the other entries in [-1, 1].  Checked here:
//   * the estimate push_column returns equals |g0 e_0 - H y| computed from
//     the untouched matrix, to 1e-12 g0 (jd = 1, jd = m and lengths between);
//   * pushing the columns one at a time (the CGS2 solvers) and reset +
//     pushing all jd columns after every step (the delayed CGS2 cycle, whose
//     step j + 1 corrects column j) give bitwise equal estimates and y;
//   * a zero sub-diagonal (lucky breakdown): the estimate is exactly 0 and
//     y solves the square system;
//   * a column whose two rotated entries are zero: the identity rotation,
//     no NaN.
// Each matrix and its y are printed as hex floats: the Python side checks
// the condition number and y against numpy.linalg.lstsq.
#include "hessenberg.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace
{
int failures = 0;

void
expect(bool ok, const char *what, int a = 0, int b = 0)
{
  if (!ok)
    {
      ++failures;
      std::printf("FAIL %s (%d, %d)\n", what, a, b);
    }
}

struct Rng
{
  uint64_t s;
  double
  uniform() // [0, 1)
  {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  }
};

constexpr int m = 28;

// column major, m + 1 rows
std::vector<double>
hessenberg(uint64_t seed)
{
  Rng                 rng{seed};
  std::vector<double> H((size_t)(m + 1) * m, 0.0);
  for (int c = 0; c < m; ++c)
    {
      for (int i = 0; i <= c; ++i)
        H[(size_t)c * (m + 1) + i] = 2.0 * rng.uniform() - 1.0;
      H[(size_t)c * (m + 1) + c + 1] = 0.5 + rng.uniform();
    }
  return H;
}

bool
same_bits(double a, double b)
{
  return std::memcmp(&a, &b, sizeof(double)) == 0;
}

// |g0 e_0 - H(0 .. jd, 0 .. jd-1) y|
double
residual(const std::vector<double> &H, int jd, double g0, const double *y)
{
  double r2 = 0;
  for (int i = 0; i <= jd; ++i)
    {
      double t = i == 0 ? g0 : 0.0;
      for (int c = 0; c < jd; ++c)
        t -= H[(size_t)c * (m + 1) + i] * y[c];
      r2 += t * t;
    }
  return std::sqrt(r2);
}

void
print_case(const char *name, uint64_t seed, const std::vector<double> &H, int jd, double g0,
           const double *y)
{
  std::printf("CASE %s-seed%llu-jd%d %d %a\nH", name, (unsigned long long)seed, jd, jd, g0);
  for (int i = 0; i <= jd; ++i)
    for (int c = 0; c < jd; ++c)
      std::printf(" %a", H[(size_t)c * (m + 1) + i]);
  std::printf("\nY");
  for (int c = 0; c < jd; ++c)
    std::printf(" %a", y[c]);
  std::printf("\n");
}

// the columns of H pushed one at a time up to jd_max, against reset + all
// columns after every step; the estimate against the direct residual at the
// lengths in `check`
void
run(const char *name, uint64_t seed, const std::vector<double> &H, double g0, int jd_max,
    const std::vector<int> &check)
{
  gls::HessenbergLsq inc(m), redo(m);
  std::vector<double> y(m), y2(m);
  inc.reset(g0);
  for (int j = 0; j < jd_max; ++j)
    {
      const double est = inc.push_column(j, &H[(size_t)j * (m + 1)]);
      const int    jd  = j + 1;
      redo.reset(g0);
      double est2 = 0;
      for (int c = 0; c < jd; ++c)
        est2 = redo.push_column(c, &H[(size_t)c * (m + 1)]);
      expect(same_bits(est, est2), "estimate: incremental vs re-factorised", (int)seed, jd);
      bool wanted = false;
      for (int k : check)
        wanted = wanted || k == jd;
      if (!wanted)
        continue;
      inc.solve(jd, y.data());
      redo.solve(jd, y2.data());
      for (int c = 0; c < jd; ++c)
        expect(same_bits(y[c], y2[c]), "y: incremental vs re-factorised", (int)seed, jd);
      const double r = residual(H, jd, g0, y.data());
      expect(std::fabs(est - r) <= 1e-12 * g0, "estimate vs direct residual", (int)seed, jd);
      print_case(name, seed, H, jd, g0, y.data());
    }
}
} // namespace

int
main()
{
  for (uint64_t seed = 1; seed <= 4; ++seed)
    {
      const std::vector<double> H  = hessenberg(seed);
      const double              g0 = 1.0 + (double)seed;
      run("random", seed, H, g0, m, {1, 2, 7, 19, m});
    }
  // lucky breakdown: column jd-1 with a zero sub-diagonal; the estimate is
  // exactly zero and y solves the square system
  for (int jd : {1, 5, m})
    {
      std::vector<double> H = hessenberg(10 + jd);
      H[(size_t)(jd - 1) * (m + 1) + jd] = 0.0;
      const double       g0 = 3.0;
      gls::HessenbergLsq q(m);
      std::vector<double> y(m);
      q.reset(g0);
      double est = -1;
      for (int c = 0; c < jd; ++c)
        est = q.push_column(c, &H[(size_t)c * (m + 1)]);
      expect(est == 0.0, "lucky breakdown: estimate exactly zero", jd);
      run("breakdown", 10 + jd, H, g0, jd, {jd});
    }
  // both rotated entries zero: the identity rotation (cs = 1, sn = 0), the
  // next column passes through it unchanged
  {
    gls::HessenbergLsq q(m);
    q.reset(2.0);
    const double zero[2] = {0.0, 0.0};
    const double est0    = q.push_column(0, zero);
    double       c = 0, s = 1;
    q.rotation(0, c, s);
    expect(est0 == 0.0 && c == 1.0 && s == 0.0, "zero column: identity rotation");
    const double col1[3] = {0.25, 3.0, 4.0};
    const double est1    = q.push_column(1, col1);
    q.rotation(1, c, s);
    expect(est1 == 0.0 && !std::isnan(c) && !std::isnan(s), "column after a zero column");
    expect(std::fabs(c - 0.6) < 1e-15 && std::fabs(s - 0.8) < 1e-15, "rotation of (3, 4)");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
