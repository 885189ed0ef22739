// coarse_nd_sanitize.cc — the nested-dissection planner (csrc/coarse_nd.cc,
// host only) as a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_coarse_nd_plan.py compiles and runs
// it): structured Q1 / Q2 grids in 2D and 3D, one cell, a leaf size above the
// cell count, two disconnected groups, a node in no cell, bad arguments.
// Each plan's ownership, boundary sets and maps are checked.
#include "coarse_nd.h"

#include <algorithm>
#include <cstdio>
#include <set>
#include <stdexcept>
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

// lexicographic Q_k grid of nx x ny x nz cells (nz = 0: 2D)
static std::vector<uint32_t>
grid(int k, int nx, int ny, int nz, int64_t &n_nodes, int &nq)
{
  const int dim = nz > 0 ? 3 : 2;
  const int Lx = k * nx + 1, Ly = k * ny + 1, Lz = dim == 3 ? k * nz + 1 : 1;
  n_nodes = (int64_t)Lx * Ly * Lz;
  nq      = dim == 3 ? (k + 1) * (k + 1) * (k + 1) : (k + 1) * (k + 1);
  std::vector<uint32_t> cn;
  for (int cz = 0; cz < (dim == 3 ? nz : 1); ++cz)
    for (int cy = 0; cy < ny; ++cy)
      for (int cx = 0; cx < nx; ++cx)
        for (int l = 0; l < (dim == 3 ? k + 1 : 1); ++l)
          for (int j = 0; j <= k; ++j)
            for (int i = 0; i <= k; ++i)
              cn.push_back((uint32_t)((cx * k + i) + Lx * ((cy * k + j) + Ly * (cz * k + l))));
  return cn;
}

static void
check_plan(const gls::NdPlan &p, const std::vector<uint32_t> &cn, int nq,
           const std::vector<int32_t> &w)
{
  const auto &T = p.nodes;
  std::vector<int32_t> owner((size_t)p.n_dofs, -1);
  for (size_t t = 0; t < T.size(); ++t)
    for (int32_t d : T[t].own)
      {
        CHECK(d >= 0 && d < p.n_dofs && owner[(size_t)d] == -1);
        owner[(size_t)d] = (int32_t)t;
      }
  for (int32_t o : owner)
    CHECK(o >= 0);
  std::vector<std::set<int32_t>> expect(T.size());
  for (int64_t c = 0; c < p.n_cells; ++c)
    {
      const int32_t leaf = p.cell_leaf[(size_t)c];
      CHECK(leaf >= 0 && T[(size_t)leaf].child[0] < 0);
      for (int q = 0; q < nq; ++q)
        {
          const uint32_t n = cn[(size_t)c * nq + q];
          for (int64_t d = p.dof0[n]; d < p.dof0[(size_t)n + 1]; ++d)
            {
              int32_t u = leaf;
              for (; u >= 0 && u != owner[(size_t)d]; u = T[(size_t)u].parent)
                expect[(size_t)u].insert((int32_t)d);
              CHECK(u >= 0); // the owner is on the leaf's path to the root
            }
        }
    }
  int64_t stored = 0;
  for (size_t t = 0; t < T.size(); ++t)
    {
      CHECK(std::vector<int32_t>(expect[t].begin(), expect[t].end()) == T[t].boundary);
      CHECK(T[t].map.size() == T[t].boundary.size());
      if (t > 0)
        {
          const auto &par = T[(size_t)T[t].parent];
          for (size_t k = 0; k < T[t].map.size(); ++k)
            {
              const size_t m = (size_t)T[t].map[k];
              CHECK(m < par.own.size() + par.boundary.size());
              if (m < par.own.size() + par.boundary.size())
                CHECK((m < par.own.size() ? par.own[m] : par.boundary[m - par.own.size()]) ==
                      T[t].boundary[k]);
            }
        }
      stored += (int64_t)T[t].own.size() * (int64_t)(T[t].own.size() + 2 * T[t].boundary.size());
    }
  CHECK(stored == p.stored);
  int64_t nf = 0;
  for (int32_t x : w)
    nf += x;
  CHECK(p.sum_own == nf && p.n_dofs == nf);
}

int
main()
{
  struct Case
  {
    int k, nx, ny, nz, leaf;
    bool condense;
  };
  const Case cases[] = {{1, 17, 13, 0, 6, false}, {2, 9, 5, 0, 4, true},  {1, 5, 4, 3, 7, false},
                        {2, 5, 4, 3, 5, true},    {2, 3, 3, 3, 1, false}, {1, 1, 1, 0, 3, false},
                        {2, 4, 4, 0, 16, true},   {2, 4, 4, 0, 100, true}};
  for (const Case &c : cases)
    {
      int64_t n_nodes;
      int     nq;
      const auto cn = grid(c.k, c.nx, c.ny, c.nz, n_nodes, nq);
      std::vector<int32_t> w((size_t)n_nodes);
      for (int64_t n = 0; n < n_nodes; ++n)
        w[(size_t)n] = (int32_t)(n % 4); // 0..3 dofs per node
      if (c.condense) // the cells' interior nodes take no part
        {
          const int k1 = c.k + 1;
          for (size_t e = 0; e < cn.size(); ++e)
            {
              const int q = (int)(e % (size_t)nq), i = q % k1, j = (q / k1) % k1,
                        l = c.nz > 0 ? q / (k1 * k1) : 1;
              if (i > 0 && i < c.k && j > 0 && j < c.k && l > 0 && l < c.k)
                w[cn[e]] = 0;
            }
        }
      const int64_t n_cells = (int64_t)cn.size() / nq;
      const auto    p = gls::nd_make_plan(cn.data(), n_cells, nq, n_nodes, w.data(), c.leaf);
      const auto    q = gls::nd_make_plan(cn.data(), n_cells, nq, n_nodes, w.data(), c.leaf);
      check_plan(p, cn, nq, w);
      CHECK(p.nodes.size() == q.nodes.size() && p.stored == q.stored);
      if (c.leaf >= n_cells)
        CHECK(p.nodes.size() == 1 && p.nodes[0].boundary.empty());
      std::printf("Q%d %dx%dx%d leaf %d: %zu tree nodes, depth %d, stored %lld of %lld\n", c.k,
                  c.nx, c.ny, c.nz, c.leaf, p.nodes.size(), p.depth, (long long)p.stored,
                  (long long)(p.n_dofs * p.n_dofs));
    }
  {
    // two disconnected strips and a participating node in no cell
    std::vector<uint32_t> cn;
    for (uint32_t c = 0; c < 9; ++c)
      for (uint32_t q : {2 * c, 2 * c + 2, 2 * c + 1, 2 * c + 3})
        cn.push_back(q);
    for (uint32_t c = 0; c < 14; ++c)
      for (uint32_t q : {2 * c, 2 * c + 2, 2 * c + 1, 2 * c + 3})
        cn.push_back(20 + q);
    std::vector<int32_t> w(51, 2);
    const auto p = gls::nd_make_plan(cn.data(), 23, 4, 51, w.data(), 3);
    check_plan(p, cn, 4, w);
    CHECK(p.nodes[0].own.size() == 2); // the orphan node's dofs: the root's
    CHECK(p.depth >= 3);
  }
  {
    const uint32_t cn[4] = {0, 1, 2, 9};
    const int32_t  w[4]  = {1, 1, 1, 1};
    int            thrown = 0;
    try
      {
        gls::nd_make_plan(cn, 1, 4, 4, w, 1);
      }
    catch (const std::runtime_error &)
      {
        ++thrown;
      }
    try
      {
        gls::nd_make_plan(cn, 1, 4, 10, w, 0);
      }
    catch (const std::runtime_error &)
      {
        ++thrown;
      }
    CHECK(thrown == 2);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
