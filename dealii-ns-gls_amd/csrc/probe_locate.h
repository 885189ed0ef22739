// probe_locate.h — point location of the solution probe (host only, no HIP:
// a stand-alone program compiles probe_locate.cc on its own).
#pragma once

#include <cstdint>
#include <vector>

namespace gls
{
// (cell, reference point) pairs of a list of points, grouped by point:
// point p owns pairs [off[p], off[p + 1])
struct ProbePairs
{
  std::vector<int64_t> off;  // [n_points + 1]
  std::vector<int64_t> cell; // [n_pairs] caller cell
  std::vector<double>  xi;   // [n_pairs][dim] in [0, 1]^dim
};

// Support points of FE_Q(k) on [0, 1] (Gauss-Lobatto), k = 1..3
void gll_nodes(int k, double *x);

// Every cell whose Q_k mapping (node_coords at the cell's lexicographic
// nodes) contains the point: the cells around the mesh node closest to the
// point are tried, the map inverted by Newton, a reference point accepted
// within `tol` of the unit cell and clamped to it (the counterpart of
// RemotePointEvaluation's cell search, reference tolerance 1e-6).  A point
// in no cell owns no pair.  Throws std::runtime_error on bad arguments.
void locate_points(int dim, int degree, int64_t n_cells, const uint32_t *cell_nodes,
                   int64_t n_nodes, const double *node_coords, int64_t n_points,
                   const double *xyz, ProbePairs &out, double tol = 1e-6);
} // namespace gls
