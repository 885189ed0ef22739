// Point location of the solution probe (gls_op_set_probe_points): the host
// counterpart of Utilities::MPI::RemotePointEvaluation::reinit
// (simulation.cc:515-535).  Host only; see probe_locate.h.
#include "probe_locate.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace gls
{
void
gll_nodes(int k, double *x)
{
  x[0] = 0.0;
  x[k] = 1.0;
  if (k == 2)
    x[1] = 0.5;
  else if (k == 3)
    {
      const double r = std::sqrt(5.0) / 10.0;
      x[1]           = 0.5 - r;
      x[2]           = 0.5 + r;
    }
}

namespace
{
// 1D Lagrange basis on `nodes` at x: values v[i] and derivatives dv[i]
void
lagrange_all(int n, const double *nodes, double x, double *v, double *dv)
{
  for (int i = 0; i < n; ++i)
    {
      double val = 1, der = 0;
      for (int j = 0; j < n; ++j)
        if (j != i)
          {
            double prod = 1.0 / (nodes[i] - nodes[j]);
            for (int m = 0; m < n; ++m)
              if (m != i && m != j)
                prod *= (x - nodes[m]) / (nodes[i] - nodes[m]);
            der += prod;
            val *= (x - nodes[j]) / (nodes[i] - nodes[j]);
          }
      v[i]  = val;
      dv[i] = der;
    }
}

// Newton inversion of the cell's Q_k map at p, from the cell centre
bool
invert_map(int dim, int n, const double *nodes, const uint32_t *cn, const double *coords,
           const double *p, double tol, double *xi)
{
  const int nq = dim == 3 ? n * n * n : n * n;
  for (int e = 0; e < dim; ++e)
    xi[e] = 0.5;
  bool converged = false;
  for (int it = 0; it < 40; ++it)
    {
      double v[3][4], dv[3][4];
      for (int e = 0; e < dim; ++e)
        lagrange_all(n, nodes, xi[e], v[e], dv[e]);
      double x[3] = {0, 0, 0}, J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (int i = 0; i < nq; ++i)
        {
          const int     ia[3] = {i % n, (i / n) % n, dim == 3 ? i / (n * n) : 0};
          const double *X     = coords + (size_t)cn[i] * dim;
          double        ph = 1, g[3];
          for (int e = 0; e < dim; ++e)
            ph *= v[e][ia[e]];
          for (int e = 0; e < dim; ++e)
            {
              g[e] = dv[e][ia[e]];
              for (int e2 = 0; e2 < dim; ++e2)
                if (e2 != e)
                  g[e] *= v[e2][ia[e2]];
            }
          for (int d = 0; d < dim; ++d)
            {
              x[d] += X[d] * ph;
              for (int e = 0; e < dim; ++e)
                J[d][e] += X[d] * g[e];
            }
        }
      double r[3] = {0, 0, 0}, dxi[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d)
        r[d] = p[d] - x[d];
      if (dim == 2)
        {
          const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
          if (!(std::fabs(det) > 0))
            return false;
          dxi[0] = (J[1][1] * r[0] - J[0][1] * r[1]) / det;
          dxi[1] = (-J[1][0] * r[0] + J[0][0] * r[1]) / det;
        }
      else
        {
          const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1],
                       c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                       c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
          const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
          if (!(std::fabs(det) > 0))
            return false;
          dxi[0] = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] +
                    (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) /
                   det;
          dxi[1] = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] +
                    (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) /
                   det;
          dxi[2] = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] +
                    (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) /
                   det;
        }
      double step = 0;
      for (int e = 0; e < dim; ++e)
        {
          xi[e] += dxi[e];
          step = std::max(step, std::fabs(dxi[e]));
          // far outside the unit cell the map need not be invertible
          if (!(xi[e] > -2.0 && xi[e] < 3.0))
            return false;
        }
      if (step < 1e-13)
        {
          converged = true;
          break;
        }
    }
  if (!converged)
    return false;
  for (int e = 0; e < dim; ++e)
    {
      if (xi[e] < -tol || xi[e] > 1.0 + tol)
        return false;
      xi[e] = std::min(1.0, std::max(0.0, xi[e]));
    }
  return true;
}
} // namespace

void
locate_points(int dim, int degree, int64_t n_cells, const uint32_t *cell_nodes, int64_t n_nodes,
              const double *node_coords, int64_t n_points, const double *xyz, ProbePairs &out,
              double tol)
{
  if ((dim != 2 && dim != 3) || degree < 1 || degree > 3 || n_cells < 0 || n_nodes < 0 ||
      n_points < 0 || (n_cells > 0 && !cell_nodes) || (n_nodes > 0 && !node_coords) ||
      (n_points > 0 && !xyz))
    throw std::runtime_error("locate_points: bad arguments");
  const int n = degree + 1, nq = dim == 3 ? n * n * n : n * n;
  double    nodes[4];
  gll_nodes(degree, nodes);
  // node -> cells
  std::vector<int64_t> noff((size_t)n_nodes + 1, 0), ncell((size_t)n_cells * nq);
  for (int64_t i = 0; i < n_cells * nq; ++i)
    {
      if ((int64_t)cell_nodes[i] >= n_nodes)
        throw std::runtime_error("locate_points: node index out of range");
      ++noff[(size_t)cell_nodes[i] + 1];
    }
  for (int64_t v = 0; v < n_nodes; ++v)
    noff[(size_t)v + 1] += noff[(size_t)v];
  {
    std::vector<int64_t> fill(noff.begin(), noff.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)
      for (int i = 0; i < nq; ++i)
        ncell[(size_t)fill[cell_nodes[c * nq + i]]++] = c;
  }
  out.off.assign((size_t)n_points + 1, 0);
  out.cell.clear();
  out.xi.clear();
  std::vector<int64_t> cand;
  for (int64_t p = 0; p < n_points; ++p)
    {
      const double *x = xyz + (size_t)p * dim;
      // the closest node that belongs to a cell
      int64_t best = -1;
      double  bd   = 0;
      for (int64_t v = 0; v < n_nodes; ++v)
        {
          if (noff[(size_t)v + 1] == noff[(size_t)v])
            continue;
          double d2 = 0;
          for (int d = 0; d < dim; ++d)
            {
              const double t = node_coords[(size_t)v * dim + d] - x[d];
              d2 += t * t;
            }
          if (best < 0 || d2 < bd)
            {
              best = v;
              bd   = d2;
            }
        }
      if (best >= 0)
        {
          cand.assign(ncell.begin() + noff[(size_t)best], ncell.begin() + noff[(size_t)best + 1]);
          std::sort(cand.begin(), cand.end());
          cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
          for (const int64_t c : cand)
            {
              double xi[3] = {0, 0, 0};
              if (invert_map(dim, n, nodes, cell_nodes + (size_t)c * nq, node_coords, x, tol, xi))
                {
                  out.cell.push_back(c);
                  for (int e = 0; e < dim; ++e)
                    out.xi.push_back(xi[e]);
                }
            }
        }
      out.off[(size_t)p + 1] = (int64_t)out.cell.size();
    }
}
} // namespace gls
