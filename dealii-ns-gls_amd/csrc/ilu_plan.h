// ilu_plan.h — host side of the ILU(k) preconditioner (host only, no HIP: a
// stand-alone program compiles ilu_plan.cc on its own): the symbolic and
// numeric factorisation, the level schedule of the two triangular solves and
// the launch plan over the levels that csrc/ilu.hip runs.
//
// The factorisation restates Ifpack's ILU as TrilinosWrappers::
// PreconditionILU drives it (preconditioner.cc:5-28, multigrid.cc:434-447;
// AdditionalData: ilu_fill, ilu_atol, ilu_rtol, no overlap):
//   * pattern: the level-of-fill rule.  Entries of A have level 0; an entry
//     (i, j) created through pivot p gets lev(i, p) + lev(p, j) + 1 (the
//     minimum over the pivots) and is kept if that is <= fill_level.  Rows in
//     the caller's order, no reordering; a row without a stored diagonal
//     gets one (value 0).
//   * values: row-wise (IKJ) elimination in FP64 on that pattern, after the
//     diagonal modification a_ii <- rtol a_ii + sign(a_ii) atol (sign(0) =
//     +1).  L has a unit diagonal and is kept strictly lower; U's pivots are
//     kept beside their reciprocals.  A zero or non-finite pivot throws with
//     the row in the message.
//   * schedule: level(i) = 1 + max level(j) over the row's off-diagonal
//     columns (0 without any), for L over j < i and for U over j > i.  The
//     rows of each factor are stored level by level (ascending row inside a
//     level), so a level is a contiguous range of positions.
//   * launches: a level with more than `narrow` rows is *wide*: one grid
//     launch over its rows.  A run of consecutive levels with at most
//     `narrow` rows each is a *chain*: one launch of one workgroup that walks
//     the levels with a workgroup barrier between them.
//
// Tuning, read from the environment when a plan is made (ilu_tuning_from_env):
//   GLS_ILU_CHAIN=0   every level is a launch of its own (the A/B of
//                     tools/ilu_apply.hip); default 1
//   GLS_ILU_GROUP=g   lanes per row, a power of two in [1, 64]; default: the
//                     smallest power of two >= the mean off-diagonal row
//                     length of L and U together, within [4, 64] (a row is
//                     then one pass of its group: the solve is latency bound,
//                     a second pass would double a level's time)
//   GLS_ILU_NARROW=r  most rows of a level that may join a chain; default one
//                     pass of the chain's workgroup, 1024 / group rows (a
//                     level of several passes on one CU loses to a grid
//                     launch: profiles/ilu/README.md)
//
// The numeric factorisation on the device (csrc/ilu_factor.hip) runs over the
// level schedule of L: row i of the IKJ elimination reads exactly the rows of
// its L pattern.  Its launch plan, IluPlan::factor_launches, has the form of
// the solves' plans with values of its own:
//   * lanes per row (factor_group): the row kernel stages the whole row (both
//     triangles, values and columns) in LDS and strides over the upper part
//     of one pivot row at a time, so the default is twice the solve's group
//     (at most 64: a group never spans waves); a forced GLS_ILU_GROUP is
//     taken as it is.
//   * rows at once in one workgroup (factor_rows): ILU_CHAIN_THREADS /
//     factor_group, and no more than fit ILU_FACTOR_LDS_BYTES with
//     max_row * 12 bytes each (FP64 value + int32 column per entry).  A
//     pattern whose longest row alone does not fit (max_row >
//     ILU_FACTOR_MAX_ROW) has no device factorisation.
//   GLS_ILU_FACTOR_CHAIN=0   every level of the factorisation is a launch of
//                            its own; default 1
//   GLS_ILU_FACTOR_NARROW=r  most rows of a level that may join a chain;
//                            default factor_rows, one pass of the chain's
//                            workgroup: a row is a serial walk over its L
//                            entries, each a dependent division and a pass
//                            over a pivot row, so a second pass doubles the
//                            level's time while a grid launch spreads the
//                            same rows over the other compute units
#pragma once

#include <cstdint>
#include <vector>

namespace gls
{
constexpr int ILU_CHAIN_THREADS = 1024; // the chain's single workgroup
constexpr int ILU_WIDE_THREADS  = 256;  // workgroups of a wide level's grid
constexpr int ILU_FACTOR_LDS_BYTES = 64 * 1024; // staged rows of one workgroup
constexpr int ILU_FACTOR_ROW_BYTES = 12;        // per entry: FP64 value, int32 column
constexpr int ILU_FACTOR_MAX_ROW   = ILU_FACTOR_LDS_BYTES / ILU_FACTOR_ROW_BYTES;

struct IluParams
{
  int    fill_level = 0;
  double atol = 0.0, rtol = 1.0;
};

struct IluTuning
{
  int chain  = 1;
  int group  = 0; // 0: from the factor
  int narrow = 0; // 0: from the group
  int factor_chain  = 1;
  int factor_narrow = 0; // 0: one pass of the factor chain's workgroup
};
IluTuning ilu_tuning_from_env();

struct IluLaunch
{
  int32_t pos0 = 0, pos1 = 0; // scheduled positions [pos0, pos1)
  int32_t lev0 = 0, lev1 = 0; // levels [lev0, lev1); a wide launch holds one
  int32_t chain = 0;          // 1: one workgroup walking the levels
};

// one triangular factor in scheduled order: position p holds row order[p];
// its off-diagonal entries are rp[p] .. rp[p + 1]) with the columns in the
// original numbering (the work vector is never permuted)
struct IluTri
{
  std::vector<int32_t>   rp, ci;
  std::vector<double>    v;
  std::vector<int64_t>   from;    // [nnz] position of the entry in IluPlan::val
  std::vector<int32_t>   order;   // [n] row at each position
  std::vector<int32_t>   level;   // [n] level of each row (original numbering)
  std::vector<int32_t>   lev_ptr; // [n_levels + 1] first position of each level
  std::vector<IluLaunch> launches;
  int32_t                max_level_rows = 0;
};

struct IluPlan
{
  int64_t   n = 0, nnz_a = 0;
  IluParams prm;
  IluTuning tuning;
  int       group = 0, narrow = 0; // as used
  // the factor's pattern, rows in the original order, columns ascending, the
  // diagonal always present: L strictly below it (unit diagonal implied), U
  // on and above it (the pivot itself)
  std::vector<int64_t> rp, diag; // [n + 1], [n] position of the diagonal
  std::vector<int32_t> ci;
  std::vector<double>  val;
  std::vector<int64_t> a_to_f;   // [nnz_a] position of each entry of A in the pattern
  std::vector<double>  dinv;     // [n] reciprocal pivots
  double               min_pivot = 0.0;
  IluTri               L, U;
  double               symbolic_ms = 0.0, numeric_ms = 0.0;
  // the device factorisation: launches over L.order / L.lev_ptr
  std::vector<IluLaunch> factor_launches;
  int     factor_group = 0, factor_rows = 0, factor_narrow = 0; // as used
  int64_t max_row = 0; // entries of the longest row of the pattern
};

// Symbolic factorisation, schedule and launch plans; the values are zero
// until a numeric factorisation.  Throws as ilu_make_plan does, but for the
// pivots.
IluPlan ilu_make_symbolic(int64_t n, const int64_t *row_ptr, const int64_t *cols,
                          const IluParams &prm, const IluTuning &tuning);

// ilu_make_symbolic, then ilu_refactor(vals).
// Throws std::runtime_error on bad arguments (n <= 0, unsorted or repeated
// columns, an index out of range, n or the factor's entries >= 2^31) and on
// a zero or non-finite pivot.
IluPlan ilu_make_plan(int64_t n, const int64_t *row_ptr, const int64_t *cols, const double *vals,
                      const IluParams &prm, const IluTuning &tuning);

// numeric factorisation with new values on the plan's pattern (vals in the
// order of the matrix the plan was made from); refreshes val, dinv, min_pivot
// and the scheduled copies L.v / U.v
void ilu_refactor(IluPlan &plan, const double *vals);

// The host emulation of the device factorisation: the scatter of vals onto
// the zeroed pattern and the diagonal modification, then the rows in the
// order of factor_launches, each staged (values and columns), eliminated
// against its L entries in ascending column order with the target of every
// update found by a binary search beyond the pivot in the staged columns, and
// written back; then the scheduled copies, the reciprocal pivots and the
// pivot check (the smallest bad row, which is the one ilu_refactor names: the
// rows before it do not depend on it).  Every entry sees the operations of
// ilu_refactor in the same order, so the two are bitwise equal.
void ilu_refactor_scheduled(IluPlan &plan, const double *vals);

// dst = U^-1 L^-1 src on the host, over the scheduled storage in launch order
// (what the device does, row by row)
void ilu_host_solve(const IluPlan &plan, double *dst, const double *src);
} // namespace gls
