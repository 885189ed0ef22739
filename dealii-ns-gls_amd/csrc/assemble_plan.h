// assemble_plan.h — host side of the device assembly of the system matrix
// (host only, no HIP: a stand-alone program compiles assemble_plan.cc on its
// own).  Built once per operator; csrc/assemble.hip uploads it and runs the
// gather and the matrix-based vmult over it.
//
//   * pattern: the scalar CSR of OperatorBase::get_system_matrix
//     (operator_ns.cc:1407-1430) as gls_op_system_matrix returns it: rows the
//     node-major dofs, every component pair of every node pair that shares a
//     cell, columns ascending per row; a constrained row holds only its unit
//     diagonal (the identity rows of vmult, operator_ns.cc:719-721) and
//     constrained columns are dropped from the other rows.  row_ptr is
//     64-bit, the columns are 32-bit (n_dofs >= 2^31 is refused).
//   * node pairs: the same pattern node by node.  Pair p couples row node
//     pair_row[p] with column node pair_node[p] (ascending per row node,
//     pair_ptr[n] .. pair_ptr[n + 1]).  Every unconstrained row of the row
//     node stores the columns of the column node at the same offset
//     pair_off[p] from its row start, one column per unconstrained component
//     in ascending order.
//   * incidence: per node its (cell, local point) pairs, ascending by cell
//     (inc_ptr[n] .. inc_ptr[n + 1]); n_cells * (k + 1)^dim entries.  The
//     cells two nodes share are the merge of their two lists, so no map from
//     (cell, i, j) to an entry (as large as the element matrices themselves)
//     is ever built.
//
// The cells are taken in the order given (the operator passes its internal
// order, the one its element matrices come in).
#pragma once

#include <cstdint>
#include <vector>

namespace gls
{
struct AssemblePlan
{
  int     dim = 0, degree = 0, nq = 0, nc = 0; // nq = (k + 1)^dim points, nc = dim + 1
  int64_t n_cells = 0, n_nodes = 0, n_dofs = 0, nnz = 0, n_pairs = 0;
  int     max_cells_per_node = 0;
  std::vector<int64_t> row_ptr;   // [n_dofs + 1]
  std::vector<int32_t> cols;      // [nnz]
  std::vector<int64_t> pair_ptr;  // [n_nodes + 1]
  std::vector<int32_t> pair_row;  // [n_pairs] row node
  std::vector<int32_t> pair_node; // [n_pairs] column node
  std::vector<int32_t> pair_off;  // [n_pairs] first column of the pair within a row
  std::vector<int64_t> inc_ptr;   // [n_nodes + 1]
  std::vector<int32_t> inc_cell;  // [n_cells * nq]
  std::vector<int32_t> inc_point; // [n_cells * nq] local point of the node in that cell
};

// Throws std::runtime_error on bad arguments: dim not 2 or 3, degree < 1, an
// empty mesh, n_dofs >= 2^31 (32-bit columns), n_cells >= 2^31, a node index
// out of range, a cell that names a node twice.
AssemblePlan assemble_make_plan(int dim, int degree, int64_t n_cells, int64_t n_nodes,
                                const uint32_t *cell_nodes, const uint8_t *cmask);
} // namespace gls
