// coarse_nd.h — the nested-dissection plan of the sparse direct coarse solver
// (host only, no HIP: a stand-alone program compiles coarse_nd.cc on its own).
#pragma once

#include <cstdint>
#include <vector>

namespace gls
{
// One node of the elimination tree over the cells.  The dofs are plan dofs:
// mesh node n's participating dofs are numbered dof0[n] .. dof0[n + 1) - 1.
struct NdNode
{
  int32_t parent = -1, child[2] = {-1, -1}, level = 0;
  std::vector<int32_t> own;      // I_t, ascending: dofs whose cells all lie in this subtree
                                 // and in no single child's
  std::vector<int32_t> boundary; // B_t, ascending: dofs of strict ancestors in a cell of
                                 // this subtree
  std::vector<int32_t> map;      // [|B_t|] position of boundary[k] in the parent's I ∪ B
                                 // (I first, then B)
  std::vector<int32_t> cells;    // a leaf's cells (caller order), ascending
};

struct NdPlan
{
  int64_t n_cells = 0, n_mesh_nodes = 0, n_dofs = 0;
  int     max_leaf_cells = 0;
  std::vector<NdNode>               nodes;  // node 0 is the root; a parent precedes its children
  std::vector<std::vector<int32_t>> levels; // tree nodes per level, level 0 = the root
  std::vector<int32_t>              cell_leaf; // [n_cells] the leaf of each cell
  std::vector<int64_t>              dof0;      // [n_mesh_nodes + 1]
  // statistics: stored = sum over tree nodes of |I|^2 + 2 |I| |B|
  int     depth = 0;
  int64_t sum_own = 0, stored = 0;
  int32_t max_own = 0, max_boundary = 0;
};

// Recursive bisection of the cell adjacency graph (two cells are adjacent
// when they share a mesh node): a BFS level structure from a pseudo-
// peripheral cell, split at the level boundary closest to the median (at the
// median cell of the BFS order where no level boundary leaves a quarter of
// the cells on either side); a disconnected cell set is split by components.
// Recursion stops at max_leaf_cells cells.  node_dofs[n]: the number of dofs
// of mesh node n that take part (0: none).  A dof belongs to the deepest tree
// node whose subtree holds every cell of its mesh node.  Deterministic:
// connectivity only, every iteration in index order.  Throws
// std::runtime_error on bad arguments.
NdPlan nd_make_plan(const uint32_t *cell_nodes, int64_t n_cells, int nodes_per_cell,
                    int64_t n_mesh_nodes, const int32_t *node_dofs, int max_leaf_cells);
} // namespace gls
