// coarse_nd_solver.h — device side of the nested-dissection coarse solver
// (coarse_nd.hip) as the multigrid uses it.  Streams and the rocBLAS handle
// are passed as void * so that this header needs no HIP.
#pragma once

#include "coarse_nd.h"

namespace gls
{
struct NdSolver;

// the coarse cells' blocks on the participating dofs (element matrices, or
// element Schur complements with the cell interiors condensed), as the dense
// assembly scatters them
struct NdCellBlocks
{
  const void    *blocks;  // device: [internal cell][col j][row i], nloc x nloc each
  bool           f64;     // FP64 blocks (FP32 otherwise)
  int            nloc;
  const int32_t *cell_dof;    // host [internal cell][nloc]: plan dof, -1: takes no part
  const int64_t *cell_caller; // host [internal cell] -> caller cell (null: identity)
  const int32_t *d_color_cells; // device: internal cells sorted by colour
  const int64_t *color_begin;   // host [n_colors + 1]
  int            n_colors;
};

// uploads the plan's tables; the numeric setup is nd_solver_factor
NdSolver     *nd_solver_create(NdPlan plan);
void          nd_solver_destroy(NdSolver *);
const NdPlan &nd_solver_plan(const NdSolver *);
// fronts, factorisation bottom-up and the stored factors (FP32 or FP64).
// false: a pivot block was singular (nothing usable is kept).
bool nd_solver_factor(NdSolver *, void *rocblas_handle, const NdCellBlocks &cb, bool store_f32,
                      void *stream);
// sol[free[i]] = (A^-1 rhs)[i] for every plan dof i; rhs in plan dof order
void nd_solver_solve(NdSolver *, const double *rhs, void *sol, bool sol_f64,
                     const int32_t *d_free, void *stream);
void nd_solver_stats(const NdSolver *, int64_t *stored_entries, int64_t *stored_bytes,
                     double *ms_factor, double *ms_store);
} // namespace gls
