// coarse_nd.cc — nested-dissection plan of the sparse direct coarse solver
// (coarse_nd.h): the elimination tree over the coarse cells, the own and
// boundary dof sets of its nodes and the extend-add maps.  Host only.
#include "coarse_nd.h"

#include <algorithm>
#include <stdexcept>

namespace gls
{
namespace
{
struct Builder
{
  const uint32_t *cn;
  int64_t         n_cells;
  int             nq;
  int             max_leaf;
  std::vector<int64_t> nc_off; // mesh node -> its cells (CSR, ascending)
  std::vector<int32_t> nc_ent;
  std::vector<int32_t> mark;   // [n_cells] stamp of the set being split
  int32_t              stamp = 0;
  NdPlan              *plan;

  // BFS over the cells marked `st` from `root`; cells in visiting order,
  // level_end[l]: one past the last cell of level l.  Visited cells are
  // re-marked st + 1.
  void
  bfs(int32_t root, int32_t st, std::vector<int32_t> &order, std::vector<int32_t> &level_end)
  {
    order.assign(1, root);
    level_end.clear();
    mark[(size_t)root] = st + 1;
    size_t head = 0;
    while (head < order.size())
      {
        const size_t end = order.size();
        for (; head < end; ++head)
          {
            const int32_t   c  = order[head];
            const uint32_t *nd = cn + (size_t)c * nq;
            for (int p = 0; p < nq; ++p)
              for (int64_t e = nc_off[nd[p]]; e < nc_off[(size_t)nd[p] + 1]; ++e)
                {
                  const int32_t o = nc_ent[(size_t)e];
                  if (mark[(size_t)o] == st)
                    {
                      mark[(size_t)o] = st + 1;
                      order.push_back(o);
                    }
                }
          }
        level_end.push_back((int32_t)end);
      }
  }

  void
  set_marks(const std::vector<int32_t> &cells, int32_t st)
  {
    for (int32_t c : cells)
      mark[(size_t)c] = st;
  }

  // the two halves of `cells` (ascending, more than one cell)
  void
  bisect(const std::vector<int32_t> &cells, std::vector<int32_t> &a, std::vector<int32_t> &b)
  {
    std::vector<int32_t> order, level_end;
    // connected components, in the order of their smallest cell
    stamp += 2;
    set_marks(cells, stamp);
    std::vector<std::vector<int32_t>> comps;
    for (int32_t c : cells)
      if (mark[(size_t)c] == stamp)
        {
          bfs(c, stamp, order, level_end);
          comps.push_back(order);
        }
    a.clear(), b.clear();
    if (comps.size() > 1)
      {
        // whole components into the first half until it holds half the cells
        // (the last component always goes to the second)
        size_t k = 0;
        for (; k + 1 < comps.size() && (k == 0 || 2 * a.size() < cells.size()); ++k)
          a.insert(a.end(), comps[k].begin(), comps[k].end());
        for (; k < comps.size(); ++k)
          b.insert(b.end(), comps[k].begin(), comps[k].end());
      }
    else
      {
        // pseudo-peripheral cell: restart the BFS from the smallest cell of
        // the last level while the number of levels grows
        int32_t root   = cells[0];
        size_t  height = 0;
        for (int it = 0; it < 8; ++it)
          {
            stamp += 2;
            set_marks(cells, stamp);
            bfs(root, stamp, order, level_end);
            if (it > 0 && level_end.size() <= height)
              break;
            height          = level_end.size();
            const size_t l0 = level_end.size() > 1 ? (size_t)level_end[level_end.size() - 2] : 0;
            root            = *std::min_element(order.begin() + (long)l0, order.end());
          }
        // the level boundary closest to the median, if it leaves a quarter
        // of the cells on either side; the median of the BFS order otherwise
        const size_t n = cells.size();
        size_t       cut = n / 2, best = n;
        for (size_t l = 0; l + 1 < level_end.size(); ++l)
          {
            const size_t e = (size_t)level_end[l];
            const size_t d = e > n / 2 ? e - n / 2 : n / 2 - e;
            if (4 * e >= n && 4 * (n - e) >= n && d < best)
              best = d, cut = e;
          }
        a.assign(order.begin(), order.begin() + (long)cut);
        b.assign(order.begin() + (long)cut, order.end());
      }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
  }

  void
  build(int32_t t, std::vector<int32_t> cells)
  {
    if ((int64_t)cells.size() <= (int64_t)max_leaf || cells.size() <= 1)
      {
        for (int32_t c : cells)
          plan->cell_leaf[(size_t)c] = t;
        plan->nodes[(size_t)t].cells = std::move(cells);
        return;
      }
    std::vector<int32_t> a, b;
    bisect(cells, a, b);
    cells.clear();
    cells.shrink_to_fit();
    const int32_t lvl = plan->nodes[(size_t)t].level;
    for (int k = 0; k < 2; ++k)
      {
        const int32_t ch = (int32_t)plan->nodes.size();
        plan->nodes.emplace_back();
        plan->nodes[(size_t)ch].parent   = t;
        plan->nodes[(size_t)ch].level    = lvl + 1;
        plan->nodes[(size_t)t].child[k] = ch;
      }
    const int32_t c0 = plan->nodes[(size_t)t].child[0], c1 = plan->nodes[(size_t)t].child[1];
    build(c0, std::move(a));
    build(c1, std::move(b));
  }
};
} // namespace

NdPlan
nd_make_plan(const uint32_t *cell_nodes, int64_t n_cells, int nodes_per_cell,
             int64_t n_mesh_nodes, const int32_t *node_dofs, int max_leaf_cells)
{
  if (!cell_nodes || !node_dofs || n_cells < 1 || nodes_per_cell < 1 || n_mesh_nodes < 1 ||
      max_leaf_cells < 1 || n_cells > INT32_MAX / 2)
    throw std::runtime_error("nested-dissection plan: invalid arguments");
  const int nq = nodes_per_cell;
  for (int64_t i = 0; i < n_cells * nq; ++i)
    if ((int64_t)cell_nodes[i] >= n_mesh_nodes)
      throw std::runtime_error("nested-dissection plan: cell node out of range");
  NdPlan plan;
  plan.n_cells        = n_cells;
  plan.n_mesh_nodes   = n_mesh_nodes;
  plan.max_leaf_cells = max_leaf_cells;
  plan.dof0.assign((size_t)n_mesh_nodes + 1, 0);
  for (int64_t n = 0; n < n_mesh_nodes; ++n)
    {
      if (node_dofs[n] < 0)
        throw std::runtime_error("nested-dissection plan: negative dof count");
      plan.dof0[(size_t)n + 1] = plan.dof0[(size_t)n] + node_dofs[n];
    }
  plan.n_dofs = plan.dof0[(size_t)n_mesh_nodes];
  if (plan.n_dofs > INT32_MAX / 2)
    throw std::runtime_error("nested-dissection plan: too many dofs");

  Builder bd;
  bd.cn       = cell_nodes;
  bd.n_cells  = n_cells;
  bd.nq       = nq;
  bd.max_leaf = max_leaf_cells;
  bd.plan     = &plan;
  bd.nc_off.assign((size_t)n_mesh_nodes + 1, 0);
  for (int64_t i = 0; i < n_cells * nq; ++i)
    ++bd.nc_off[(size_t)cell_nodes[i] + 1];
  for (int64_t n = 0; n < n_mesh_nodes; ++n)
    bd.nc_off[(size_t)n + 1] += bd.nc_off[(size_t)n];
  bd.nc_ent.resize((size_t)(n_cells * nq));
  {
    std::vector<int64_t> at(bd.nc_off.begin(), bd.nc_off.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)
      for (int p = 0; p < nq; ++p)
        bd.nc_ent[(size_t)at[cell_nodes[c * nq + p]]++] = (int32_t)c;
  }
  bd.mark.assign((size_t)n_cells, 0);
  plan.cell_leaf.assign((size_t)n_cells, -1);
  plan.nodes.emplace_back();
  {
    std::vector<int32_t> all((size_t)n_cells);
    for (int64_t c = 0; c < n_cells; ++c)
      all[(size_t)c] = (int32_t)c;
    bd.build(0, std::move(all));
  }
  std::vector<NdNode> &T = plan.nodes;

  // ownership: the lowest common ancestor of the leaves of a mesh node's
  // cells (a participating node in no cell: the root)
  std::vector<int32_t> owner((size_t)n_mesh_nodes, -1);
  for (int64_t n = 0; n < n_mesh_nodes; ++n)
    {
      if (node_dofs[n] == 0)
        continue;
      int32_t o = -1;
      for (int64_t e = bd.nc_off[(size_t)n]; e < bd.nc_off[(size_t)n + 1]; ++e)
        {
          int32_t l = plan.cell_leaf[(size_t)bd.nc_ent[(size_t)e]];
          if (o < 0)
            {
              o = l;
              continue;
            }
          while (o != l)
            if (T[(size_t)o].level >= T[(size_t)l].level)
              o = T[(size_t)o].parent;
            else
              l = T[(size_t)l].parent;
        }
      owner[(size_t)n] = o < 0 ? 0 : o;
      for (int64_t d = plan.dof0[(size_t)n]; d < plan.dof0[(size_t)n + 1]; ++d)
        T[(size_t)owner[(size_t)n]].own.push_back((int32_t)d); // ascending: n ascends
    }
  // boundary sets: a dof of a leaf's cell owned by ancestor o lies in B of
  // every tree node from the leaf up to o's child
  for (size_t t = 0; t < T.size(); ++t)
    for (int32_t c : T[t].cells)
      for (int p = 0; p < nq; ++p)
        {
          const int64_t n = cell_nodes[(size_t)c * nq + p];
          if (node_dofs[n] == 0)
            continue;
          for (int32_t u = (int32_t)t; u != owner[(size_t)n]; u = T[(size_t)u].parent)
            for (int64_t d = plan.dof0[(size_t)n]; d < plan.dof0[(size_t)n + 1]; ++d)
              T[(size_t)u].boundary.push_back((int32_t)d);
        }
  for (NdNode &nd : T)
    {
      std::sort(nd.boundary.begin(), nd.boundary.end());
      nd.boundary.erase(std::unique(nd.boundary.begin(), nd.boundary.end()), nd.boundary.end());
    }
  // extend-add maps
  for (size_t t = 1; t < T.size(); ++t)
    {
      const NdNode &p = T[(size_t)T[t].parent];
      T[t].map.resize(T[t].boundary.size());
      for (size_t k = 0; k < T[t].boundary.size(); ++k)
        {
          const int32_t d  = T[t].boundary[k];
          auto          it = std::lower_bound(p.own.begin(), p.own.end(), d);
          if (it != p.own.end() && *it == d)
            {
              T[t].map[k] = (int32_t)(it - p.own.begin());
              continue;
            }
          it = std::lower_bound(p.boundary.begin(), p.boundary.end(), d);
          if (it == p.boundary.end() || *it != d)
            throw std::runtime_error("nested-dissection plan: boundary dof missing in the parent");
          T[t].map[k] = (int32_t)(p.own.size() + (size_t)(it - p.boundary.begin()));
        }
    }
  for (size_t t = 0; t < T.size(); ++t)
    {
      const NdNode &nd = T[t];
      if ((size_t)nd.level >= plan.levels.size())
        plan.levels.resize((size_t)nd.level + 1);
      plan.levels[(size_t)nd.level].push_back((int32_t)t);
      const int64_t ni = (int64_t)nd.own.size(), nb = (int64_t)nd.boundary.size();
      plan.sum_own += ni;
      plan.stored += ni * ni + 2 * ni * nb;
      plan.max_own      = std::max(plan.max_own, (int32_t)ni);
      plan.max_boundary = std::max(plan.max_boundary, (int32_t)nb);
    }
  plan.depth = (int)plan.levels.size();
  return plan;
}
} // namespace gls
