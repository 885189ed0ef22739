// coarse.h — the multigrid's coarse-level solvers that are built from the
// coarse matrix (coarse.hip): the dense direct solver with its static
// condensation, its nested-dissection form (coarse_nd.hip underneath), the
// ILU (host or device factorised), the AMG (plain or ILU-smoothed), and the
// coarse GMRES around any preconditioner.  One object owns their state, from
// "level-0 defect" to "level-0 solution"; the multigrid (mg.hip) keeps the
// relaxation and the identity coarse solves, which are its smoother and a
// copy, and hands the object the level-0 vectors it works on.
#pragma once

#include "../../include/gls_op.h"

#include <hip/hip_runtime.h>

#include <functional>
#include <memory>

namespace gls
{
// which coarse solver a multigrid runs: decided in one place (coarse_kind in
// coarse.hip) from the descriptor and gls_mg_set_coarse_ilu
enum class CoarseKind
{
  relaxation, // coarse_n_iterations > 0: sweeps of the level smoother (mg.hip)
  identity,   // coarse_n_iterations == 0: a copy (mg.hip)
  direct,     // coarse_n_iterations < 0: dense or nested-dissection solver
  ilu,        // gls_mg_set_coarse_ilu
  amg         // desc.coarse_amg
};

struct CoarseSolver
{
  // op0: the level-0 operator; prec: the level precision (GLS_F32 / GLS_F64)
  static std::unique_ptr<CoarseSolver> create(const glsMGDesc &desc, glsOp op0, int prec,
                                              bool partitioned);
  virtual ~CoarseSolver() = default;
  virtual CoarseKind kind() const = 0;

  // gls_mg_set_coarse_direct, gls_mg_set_coarse_ilu (+ _ilu_device) and
  // gls_mg_set_coarse_amg_ilu with their refusals
  virtual void set_direct(int method, int max_leaf_cells) = 0;
  virtual void set_ilu(const glsILUParams &prm)           = 0;
  virtual void set_ilu_device(bool on)                    = 0;
  virtual void set_amg_ilu(const glsAMGIluParams &prm)    = 0;

  // what gls_mg_setup refuses before it touches anything: a direct solver on
  // a coarse operator with node constraints
  virtual void check_operator() const = 0;
  // the numeric setup (nothing for relaxation / identity); sol and tmp: two
  // level-0 vectors, scratch of the "columns" reference assembly
  virtual void setup(void *sol, void *tmp, hipStream_t s) = 0;

  // sol = P^-1 def in the level precision (direct, ILU, AMG), and on FP64
  // vectors (ILU, AMG: as the coarse GMRES preconditions with them)
  virtual void apply(void *sol, const void *def, hipStream_t s)     = 0;
  virtual void apply(double *sol, const double *def, hipStream_t s) = 0;
  // coarse_iterate: FP64 GMRES on the level-0 operator from def into sol.
  // level_prec: "sol = P^-1 def in the level precision", whatever the kind
  // (the relaxation and the identity are the multigrid's)
  virtual void gmres(void *sol, void *def, const std::function<void()> &level_prec,
                     hipStream_t s) = 0;

  // the getters behind gls_mg_coarse_statistics, _ilu, _amg, _setup_times and
  // _direct_info
  virtual void   statistics(int *n_iterations, int *converged) const = 0;
  virtual glsILU ilu(double *setup_ms) const                         = 0;
  virtual glsAMG amg(double *setup_ms) const                         = 0;
  virtual void   setup_times(double *ms3, int *n_colors) const       = 0;
  virtual void   direct_info(glsCoarseDirectInfo *info) const        = 0;
};
} // namespace gls
