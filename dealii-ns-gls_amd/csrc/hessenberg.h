// hessenberg.h — the host side of a GMRES cycle, shared by the three device
// solvers (krylov.hip, coarse.hip's coarse GMRES, dist_mg.hip): the least-squares
// problem min |g0 e_0 - H y| over the upper-Hessenberg matrix the Arnoldi
// steps deliver column by column, by Givens rotations.  Plain C++17, no HIP
// (tests/cpp/hessenberg_sanitize.cc compiles it alone).
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace gls
{
class HessenbergLsq
{
public:
  explicit HessenbergLsq(int m)
    : m_(m)
    , H_((size_t)(m + 1) * m)
    , g_(m + 1)
    , cs_(m)
    , sn_(m)
  {}

  // a new cycle: g = beta e_0 (the columns are overwritten as they are pushed)
  void
  reset(double beta)
  {
    for (double &x : g_)
      x = 0.0;
    g_[0] = beta;
  }

  // column j of the Hessenberg matrix: col[0 .. j] and the sub-diagonal
  // col[j + 1].  Rotations 0 .. j-1 applied, rotation j formed (both entries
  // zero: the identity), g updated; returns the residual estimate |g[j + 1]|
  double
  push_column(int j, const double *col)
  {
    double *Hj = &H_[(size_t)j * (m_ + 1)];
    for (int i = 0; i <= j + 1; ++i)
      Hj[i] = col[i];
    for (int i = 0; i < j; ++i)
      {
        const double t = cs_[i] * Hj[i] + sn_[i] * Hj[i + 1];
        Hj[i + 1]      = -sn_[i] * Hj[i] + cs_[i] * Hj[i + 1];
        Hj[i]          = t;
      }
    const double rr = std::hypot(Hj[j], Hj[j + 1]);
    cs_[j]          = rr > 0 ? Hj[j] / rr : 1.0;
    sn_[j]          = rr > 0 ? Hj[j + 1] / rr : 0.0;
    Hj[j]           = rr;
    Hj[j + 1]       = 0;
    g_[j + 1]       = -sn_[j] * g_[j];
    g_[j]           = cs_[j] * g_[j];
    return std::fabs(g_[j + 1]);
  }

  // y = R^{-1} g over the first jd columns (upper triangular)
  void
  solve(int jd, double *y) const
  {
    for (int i = jd - 1; i >= 0; --i)
      {
        double t = g_[i];
        for (int c = i + 1; c < jd; ++c)
          t -= H_[(size_t)c * (m_ + 1) + i] * y[c];
        y[i] = t / H_[(size_t)i * (m_ + 1) + i];
      }
  }

  int
  m() const
  {
    return m_;
  }

  // rotation j as formed by push_column (tests)
  void
  rotation(int j, double &c, double &s) const
  {
    c = cs_[j];
    s = sn_[j];
  }

private:
  int                 m_;
  std::vector<double> H_, g_, cs_, sn_; // H column major, m + 1 rows
};
} // namespace gls
