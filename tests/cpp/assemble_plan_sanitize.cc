// assemble_plan_sanitize.cc — the host plan of the device assembly
// (csrc/assemble_plan.cc, host only) as a stand-alone program for
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_assemble_plan.py
// compiles and runs it): structured 2D and 3D meshes of degree 1 .. 3 with
// shuffled cells and mixed constraint masks, a single cell, every node
// constrained, and the error paths.  Each plan is checked the way the gather
// kernel uses it: walking the two incidence lists of every node pair (in
// chunks of cells) adds every unconstrained (cell, i, j) of a known element
// matrix exactly once onto the entry with the right column, and the result
// equals a direct scatter.
#include "assemble_plan.h"

#include <algorithm>
#include <cstdio>
#include <map>
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

struct Mesh
{
  int                   dim = 2, degree = 1, nq = 4;
  int64_t               n_cells = 0, n_nodes = 0;
  std::vector<uint32_t> cell_nodes;
  std::vector<uint8_t>  cmask;
};

// m^dim cells of degree k on a lattice of (m k + 1)^dim nodes; the cells in a
// scrambled order, constraint bits from a small pattern
static Mesh
lattice(int dim, int k, int m, unsigned seed)
{
  Mesh M;
  M.dim = dim, M.degree = k;
  const int     np = k + 1, L = m * k + 1;
  const int     mz = dim == 3 ? m : 1, npz = dim == 3 ? np : 1;
  M.nq      = np * np * npz;
  M.n_cells = (int64_t)m * m * mz;
  M.n_nodes = (int64_t)L * L * (dim == 3 ? L : 1);
  std::vector<int64_t> order((size_t)M.n_cells);
  for (int64_t c = 0; c < M.n_cells; ++c)
    order[(size_t)c] = c;
  unsigned s = seed;
  for (int64_t c = M.n_cells - 1; c > 0; --c)
    {
      s = s * 1664525u + 1013904223u;
      std::swap(order[(size_t)c], order[(size_t)((s >> 8) % (unsigned)(c + 1))]);
    }
  for (int64_t c : order)
    {
      const int cx = (int)(c % m), cy = (int)((c / m) % m), cz = (int)(c / ((int64_t)m * m));
      for (int z = 0; z < npz; ++z)
        for (int y = 0; y < np; ++y)
          for (int x = 0; x < np; ++x)
            M.cell_nodes.push_back(
              (uint32_t)(((int64_t)(cz * k + z) * L + (cy * k + y)) * L + (cx * k + x)));
    }
  M.cmask.resize((size_t)M.n_nodes);
  const uint8_t pat[7] = {0, 0, 1, 0, (uint8_t)((1u << dim) - 1u), 2, (uint8_t)((2u << dim) - 1u)};
  for (int64_t n = 0; n < M.n_nodes; ++n)
    M.cmask[(size_t)n] = seed ? pat[(size_t)((n * 5 + seed) % 7)] : 0;
  return M;
}

static double
emat(int64_t c, int i, int j)
{
  return 1.0 + (double)((c * 131 + i * 17 + j * 3) % 97);
}

static void
check_plan(const Mesh &M, int64_t chunk)
{
  const gls::AssemblePlan P = gls::assemble_make_plan(M.dim, M.degree, M.n_cells, M.n_nodes,
                                                      M.cell_nodes.data(), M.cmask.data());
  const int nc = M.dim + 1, nq = M.nq;
  const auto constrained = [&](int64_t dof) { return (M.cmask[(size_t)(dof / nc)] >> (dof % nc)) & 1; };
  CHECK(P.n_dofs == M.n_nodes * nc && (int64_t)P.row_ptr.size() == P.n_dofs + 1);
  CHECK((int64_t)P.inc_cell.size() == M.n_cells * nq && P.inc_ptr.back() == M.n_cells * nq);
  CHECK(P.row_ptr.back() == P.nnz && (int64_t)P.cols.size() == P.nnz);
  // the direct scatter into a map per row
  std::vector<std::map<int32_t, double>> ref((size_t)P.n_dofs);
  int64_t                                contributions = 0;
  for (int64_t r = 0; r < P.n_dofs; ++r)
    if (constrained(r))
      ref[(size_t)r][(int32_t)r] = 1.0;
  for (int64_t c = 0; c < M.n_cells; ++c)
    for (int i = 0; i < nq * nc; ++i)
      for (int j = 0; j < nq * nc; ++j)
        {
          const int64_t r   = (int64_t)M.cell_nodes[(size_t)c * nq + i / nc] * nc + i % nc;
          const int64_t col = (int64_t)M.cell_nodes[(size_t)c * nq + j / nc] * nc + j % nc;
          if (constrained(r) || constrained(col))
            continue;
          ref[(size_t)r][(int32_t)col] += emat(c, i, j);
          ++contributions;
        }
  // pattern: rows ascending, the columns of the scatter
  for (int64_t r = 0; r < P.n_dofs; ++r)
    {
      const int64_t b = P.row_ptr[(size_t)r], e = P.row_ptr[(size_t)r + 1];
      CHECK(e - b == (int64_t)ref[(size_t)r].size());
      int64_t k = b;
      for (const auto &kv : ref[(size_t)r])
        {
          if (k < e)
            CHECK(P.cols[(size_t)k] == kv.first);
          ++k;
        }
    }
  // incidence: ascending cells per node, the right local point
  for (int64_t n = 0; n < M.n_nodes; ++n)
    for (int64_t k = P.inc_ptr[(size_t)n]; k < P.inc_ptr[(size_t)n + 1]; ++k)
      {
        CHECK(k == P.inc_ptr[(size_t)n] || P.inc_cell[(size_t)k - 1] < P.inc_cell[(size_t)k]);
        CHECK(M.cell_nodes[(size_t)P.inc_cell[(size_t)k] * nq + P.inc_point[(size_t)k]] == n);
      }
  // the gather, chunk by chunk
  std::vector<double> vals((size_t)P.nnz, 0.0);
  std::vector<int>    writes((size_t)P.nnz, 0);
  for (int64_t r = 0; r < P.n_dofs; ++r)
    if (constrained(r))
      vals[(size_t)P.row_ptr[(size_t)r]] = 1.0;
  int64_t walked = 0;
  for (int64_t c0 = 0; c0 < M.n_cells; c0 += chunk)
    {
      const int64_t c1 = std::min(M.n_cells, c0 + chunk);
      std::fill(writes.begin(), writes.end(), 0);
      for (int64_t p = 0; p < P.n_pairs; ++p)
        {
          const int64_t n = P.pair_row[(size_t)p], m = P.pair_node[(size_t)p];
          CHECK(p >= P.pair_ptr[(size_t)n] && p < P.pair_ptr[(size_t)n + 1]);
          int64_t       ia = P.inc_ptr[(size_t)n], ib = P.inc_ptr[(size_t)m];
          const int64_t ea = P.inc_ptr[(size_t)n + 1], eb = P.inc_ptr[(size_t)m + 1];
          bool          any = false;
          while (ia < ea && ib < eb)
            {
              const int64_t ca = P.inc_cell[(size_t)ia], cb = P.inc_cell[(size_t)ib];
              if (ca < cb)
                ++ia;
              else if (cb < ca)
                ++ib;
              else
                {
                  if (ca >= c0 && ca < c1)
                    {
                      any = true;
                      for (int ci = 0; ci < nc; ++ci)
                        for (int cj = 0, rank = 0; cj < nc; ++cj)
                          {
                            if (constrained(m * nc + cj))
                              continue;
                            if (!constrained(n * nc + ci))
                              {
                                const int64_t at =
                                  P.row_ptr[(size_t)(n * nc + ci)] + P.pair_off[(size_t)p] + rank;
                                CHECK(at < P.row_ptr[(size_t)(n * nc + ci) + 1]);
                                if (at < P.nnz)
                                  {
                                    CHECK(P.cols[(size_t)at] == m * nc + cj);
                                    vals[(size_t)at] +=
                                      emat(ca, P.inc_point[(size_t)ia] * nc + ci,
                                           P.inc_point[(size_t)ib] * nc + cj);
                                    ++walked;
                                  }
                              }
                            ++rank;
                          }
                    }
                  ++ia, ++ib;
                }
            }
          if (any)
            for (int ci = 0; ci < nc; ++ci)
              for (int cj = 0, rank = 0; cj < nc; ++cj)
                if (!constrained(m * nc + cj))
                  {
                    if (!constrained(n * nc + ci))
                      ++writes[(size_t)(P.row_ptr[(size_t)(n * nc + ci)] + P.pair_off[(size_t)p] +
                                        rank)];
                    ++rank;
                  }
        }
      for (int w : writes)
        CHECK(w <= 1); // one writer per value and launch
    }
  CHECK(walked == contributions);
  for (int64_t r = 0; r < P.n_dofs; ++r)
    {
      int64_t k = P.row_ptr[(size_t)r];
      for (const auto &kv : ref[(size_t)r])
        CHECK(vals[(size_t)k++] == kv.second); // small integers: exact in any order
    }
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
  for (int k = 1; k <= 3; ++k)
    {
      check_plan(lattice(2, k, 5, 3 + k), 1 << 20);
      check_plan(lattice(2, k, 4, 0), 3);
    }
  check_plan(lattice(3, 1, 3, 9), 1 << 20);
  check_plan(lattice(3, 2, 3, 5), 7);
  check_plan(lattice(3, 3, 2, 2), 3);
  check_plan(lattice(2, 2, 1, 1), 1); // a single cell
  {
    Mesh M = lattice(2, 1, 3, 1);
    std::fill(M.cmask.begin(), M.cmask.end(), (uint8_t)7); // every row an identity row
    check_plan(M, 4);
  }
  // error paths
  {
    const Mesh M = lattice(2, 1, 2, 1);
    const auto make = [&](int dim, int k, int64_t nc, int64_t nn, const Mesh &X) {
      return [=, &X] {
        gls::assemble_make_plan(dim, k, nc, nn, X.cell_nodes.data(), X.cmask.data());
      };
    };
    CHECK(throws(make(2, 1, 0, M.n_nodes, M), "empty"));
    CHECK(throws(make(2, 1, M.n_cells, 0, M), "empty"));
    CHECK(throws(make(4, 1, M.n_cells, M.n_nodes, M), "dim"));
    CHECK(throws(make(2, 0, M.n_cells, M.n_nodes, M), "degree"));
    CHECK(throws(make(2, 1, M.n_cells, (INT64_C(1) << 31) / 3 + 1, M), "32-bit"));
    CHECK(throws(make(2, 1, M.n_cells, M.n_nodes - 1, M), "out of range"));
    Mesh D = M;
    D.cell_nodes[1] = D.cell_nodes[0];
    CHECK(throws(make(2, 1, D.n_cells, D.n_nodes, D), "twice"));
    CHECK(throws([&] { gls::assemble_make_plan(2, 1, 4, 9, nullptr, M.cmask.data()); }, "null"));
  }
  std::printf("%d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
