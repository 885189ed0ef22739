// assemble_plan.cc — pattern, node pairs and node->cell incidence of the
// device assembly (assemble_plan.h).  Host only.
#include "assemble_plan.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace gls
{
AssemblePlan
assemble_make_plan(int dim, int degree, int64_t n_cells, int64_t n_nodes,
                   const uint32_t *cell_nodes, const uint8_t *cmask)
{
  if (dim != 2 && dim != 3)
    throw std::runtime_error("assemble plan: dim must be 2 or 3");
  if (degree < 1 || degree > 3)
    throw std::runtime_error("assemble plan: degree must be 1, 2 or 3");
  if (n_cells <= 0 || n_nodes <= 0)
    throw std::runtime_error("assemble plan: empty mesh");
  if (!cell_nodes || !cmask)
    throw std::runtime_error("assemble plan: null argument");
  AssemblePlan P;
  P.dim = dim, P.degree = degree, P.nc = dim + 1;
  P.nq = 1;
  for (int d = 0; d < dim; ++d)
    P.nq *= degree + 1;
  const int nq = P.nq, nc = P.nc;
  if (n_nodes > (INT64_C(0x7fffffff) / nc))
    throw std::runtime_error("assemble plan: " + std::to_string(n_nodes) + " nodes x " +
                             std::to_string(nc) +
                             " components do not fit the 32-bit column indices of the CSR");
  if (n_cells >= INT64_C(0x7fffffff) / nq)
    throw std::runtime_error("assemble plan: too many cells for the 32-bit incidence list");
  P.n_cells = n_cells, P.n_nodes = n_nodes, P.n_dofs = n_nodes * nc;
  const uint8_t all = (uint8_t)((1u << nc) - 1u);

  // incidence: count, prefix, fill in ascending cell order
  P.inc_ptr.assign((size_t)n_nodes + 1, 0);
  for (int64_t e = 0; e < n_cells * nq; ++e)
    {
      const uint32_t n = cell_nodes[e];
      if ((int64_t)n >= n_nodes)
        throw std::runtime_error("assemble plan: node " + std::to_string(n) + " of cell " +
                                 std::to_string(e / nq) + " out of range");
      ++P.inc_ptr[(size_t)n + 1];
    }
  for (int64_t n = 0; n < n_nodes; ++n)
    {
      P.max_cells_per_node = (int)std::max<int64_t>(P.max_cells_per_node, P.inc_ptr[(size_t)n + 1]);
      P.inc_ptr[(size_t)n + 1] += P.inc_ptr[(size_t)n];
    }
  P.inc_cell.resize((size_t)(n_cells * nq));
  P.inc_point.resize((size_t)(n_cells * nq));
  {
    std::vector<int64_t> fill(P.inc_ptr.begin(), P.inc_ptr.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)
      for (int q = 0; q < nq; ++q)
        {
          const uint32_t n = cell_nodes[(size_t)c * nq + q];
          const int64_t  k = fill[n]++;
          if (k > P.inc_ptr[n] && P.inc_cell[(size_t)k - 1] == (int32_t)c)
            throw std::runtime_error("assemble plan: cell " + std::to_string(c) +
                                     " names node " + std::to_string(n) + " twice");
          P.inc_cell[(size_t)k]  = (int32_t)c;
          P.inc_point[(size_t)k] = q;
        }
  }

  // node pairs: the nodes of a node's cells, sorted and uniqued
  P.pair_ptr.assign((size_t)n_nodes + 1, 0);
  std::vector<uint32_t> nb;
  for (int pass = 0; pass < 2; ++pass)
    {
      for (int64_t n = 0; n < n_nodes; ++n)
        {
          nb.clear();
          for (int64_t k = P.inc_ptr[(size_t)n]; k < P.inc_ptr[(size_t)n + 1]; ++k)
            {
              const uint32_t *cn = cell_nodes + (size_t)P.inc_cell[(size_t)k] * nq;
              nb.insert(nb.end(), cn, cn + nq);
            }
          std::sort(nb.begin(), nb.end());
          nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
          if (pass == 0)
            P.pair_ptr[(size_t)n + 1] = P.pair_ptr[(size_t)n] + (int64_t)nb.size();
          else
            {
              int64_t p   = P.pair_ptr[(size_t)n];
              int32_t off = 0;
              for (uint32_t m : nb)
                {
                  P.pair_row[(size_t)p]  = (int32_t)n;
                  P.pair_node[(size_t)p] = (int32_t)m;
                  P.pair_off[(size_t)p]  = off;
                  off += __builtin_popcount((unsigned)(~cmask[m] & all));
                  ++p;
                }
            }
        }
      if (pass == 0)
        {
          P.n_pairs = P.pair_ptr.back();
          P.pair_row.resize((size_t)P.n_pairs);
          P.pair_node.resize((size_t)P.n_pairs);
          P.pair_off.resize((size_t)P.n_pairs);
        }
    }

  // scalar pattern: a constrained row is its diagonal, the others hold the
  // unconstrained components of every neighbour node
  P.row_ptr.assign((size_t)P.n_dofs + 1, 0);
  for (int64_t n = 0; n < n_nodes; ++n)
    {
      int64_t len = 0;
      for (int64_t p = P.pair_ptr[(size_t)n]; p < P.pair_ptr[(size_t)n + 1]; ++p)
        len += __builtin_popcount((unsigned)(~cmask[P.pair_node[(size_t)p]] & all));
      for (int c = 0; c < nc; ++c)
        {
          const int64_t r           = n * nc + c;
          P.row_ptr[(size_t)r + 1] = P.row_ptr[(size_t)r] + (((cmask[n] >> c) & 1) ? 1 : len);
        }
    }
  P.nnz = P.row_ptr.back();
  P.cols.resize((size_t)P.nnz);
  for (int64_t n = 0; n < n_nodes; ++n)
    for (int c = 0; c < nc; ++c)
      {
        const int64_t r = n * nc + c;
        int64_t       k = P.row_ptr[(size_t)r];
        if ((cmask[n] >> c) & 1)
          {
            P.cols[(size_t)k] = (int32_t)r;
            continue;
          }
        for (int64_t p = P.pair_ptr[(size_t)n]; p < P.pair_ptr[(size_t)n + 1]; ++p)
          {
            const int64_t m = P.pair_node[(size_t)p];
            for (int cc = 0; cc < nc; ++cc)
              if (!((cmask[m] >> cc) & 1))
                P.cols[(size_t)k++] = (int32_t)(m * nc + cc);
          }
      }
  return P;
}
} // namespace gls
