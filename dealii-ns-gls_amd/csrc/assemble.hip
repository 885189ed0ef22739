// assemble.hip — the system matrix on the device (OperatorBase::
// get_system_matrix, operator_ns.cc:1407-1430) and the matrix-based operator
// mode (NavierStokesOperatorMatrixBased, operator_ns.cc:1525-1590, whose
// vmult is get_system_matrix().vmult()).
//
// The pattern, the node pairs and the node->cell incidence come from the host
// plan (assemble_plan.h), made at the first use and kept on the operator.
// The values are gathered from the element matrices op_element_matrices_device
// writes ([cell][col j][row i], chunks of internal cells): one work item per
// stored node pair merges the two nodes' incidence lists over the chunk's
// cells and adds the pair's (dim+1)^2 block of every common cell, in
// ascending cell order, onto the values it owns.  No atomics, one writer per
// value and launch, FP64 sums whatever the operator's precision; the running
// sum of a value continues across chunks, so the result does not depend on
// the chunk size.
#include "assemble_plan.h"
#include "op_internal.h"
#include "trace.h"

#include <algorithm>
#include <cstdlib>
#include <string>

namespace gls
{
struct SystemMatrix
{
  AssemblePlan plan; // host copy (the device arrays below mirror it)
  int64_t *d_row_ptr   = nullptr;
  int32_t *d_cols      = nullptr;
  double  *d_vals      = nullptr;
  int32_t *d_pair_row  = nullptr;
  int32_t *d_pair_node = nullptr;
  int32_t *d_pair_off  = nullptr;
  int64_t *d_inc_ptr   = nullptr;
  int32_t *d_inc_cell  = nullptr;
  int32_t *d_inc_point = nullptr;
  int      group       = 8; // lanes per row of k_csr_vmult
};
} // namespace gls

namespace
{
using gls::SystemMatrix;

// vals = 0 was done by a memset; the constrained rows' unit diagonals
__global__ void __launch_bounds__(256)
  k_csr_unit_diagonal(const int64_t *__restrict__ row_ptr, const uint8_t *__restrict__ cmask,
                      double *__restrict__ vals, int nc, int64_t n_dofs)
{
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_dofs)
    return;
  if ((cmask[r / nc] >> (int)(r % nc)) & 1)
    vals[row_ptr[r]] = 1.0;
}

// One work item per node pair p = (n, m).  E holds the element matrices of
// internal cells [c0, c1); the rows i of a column j are contiguous, so the NC
// row components of the pair are NC consecutive values and its column
// components sit at stride ndof.
template <typename T, int NC>
__global__ void __launch_bounds__(256)
  k_assemble_gather(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ pair_row,
                    const int32_t *__restrict__ pair_node, const int32_t *__restrict__ pair_off,
                    const int64_t *__restrict__ inc_ptr, const int32_t *__restrict__ inc_cell,
                    const int32_t *__restrict__ inc_point, const uint8_t *__restrict__ cmask,
                    const T *__restrict__ E, int64_t c0, int64_t c1, int ndof,
                    double *__restrict__ vals, int64_t n_pairs)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs)
    return;
  const int64_t  n = pair_row[p], m = pair_node[p];
  const unsigned all    = (1u << NC) - 1u;
  const unsigned free_n = ~(unsigned)cmask[n] & all, free_m = ~(unsigned)cmask[m] & all;
  if (!free_n || !free_m)
    return;
  int64_t       ia = inc_ptr[n], ib = inc_ptr[m];
  const int64_t ea = inc_ptr[n + 1], eb = inc_ptr[m + 1];
  while (ia < ea && inc_cell[ia] < c0)
    ++ia;
  while (ib < eb && inc_cell[ib] < c0)
    ++ib;
  double  acc[NC][NC]; // [column component][row component]
  int64_t at[NC] = {}; // row starts + the pair's offset
  bool    any = false;
  while (ia < ea && ib < eb)
    {
      const int64_t ca = inc_cell[ia], cb = inc_cell[ib];
      if (ca >= c1 || cb >= c1)
        break;
      if (ca < cb)
        ++ia;
      else if (cb < ca)
        ++ib;
      else
        {
          if (!any)
            {
              // continue the running sums of the earlier chunks
              any = true;
              const int64_t off = pair_off[p];
#pragma unroll
              for (int ci = 0; ci < NC; ++ci)
                at[ci] = row_ptr[n * NC + ci] + off;
#pragma unroll
              for (int cj = 0; cj < NC; ++cj)
                {
                  const int rank = __popc(free_m & ((1u << cj) - 1u));
#pragma unroll
                  for (int ci = 0; ci < NC; ++ci)
                    acc[cj][ci] = ((free_n >> ci) & 1u) && ((free_m >> cj) & 1u) ?
                                    vals[at[ci] + rank] :
                                    0.0;
                }
            }
          const T *Ec = E + (ca - c0) * (int64_t)ndof * ndof +
                        (int64_t)(inc_point[ib] * NC) * ndof + inc_point[ia] * NC;
#pragma unroll
          for (int cj = 0; cj < NC; ++cj)
#pragma unroll
            for (int ci = 0; ci < NC; ++ci)
              acc[cj][ci] += (double)Ec[(int64_t)cj * ndof + ci];
          ++ia, ++ib;
        }
    }
  if (!any)
    return;
#pragma unroll
  for (int cj = 0; cj < NC; ++cj)
    {
      const int rank = __popc(free_m & ((1u << cj) - 1u));
#pragma unroll
      for (int ci = 0; ci < NC; ++ci)
        if (((free_n >> ci) & 1u) && ((free_m >> cj) & 1u))
          vals[at[ci] + rank] = acc[cj][ci];
    }
}

// dst = A src: G lanes per row, FP64 products and sums, a fixed-order xor
// shuffle over the G lanes.  A constrained row is its unit diagonal: dst = src
// there exactly.
template <typename T, int G>
__global__ void __launch_bounds__(256)
  k_csr_vmult(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ cols,
              const double *__restrict__ vals, const T *__restrict__ src, T *__restrict__ dst,
              int64_t n)
{
  const int64_t r    = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int     lane = threadIdx.x & (G - 1);
  if (r >= n)
    return;
  const int64_t e = row_ptr[r + 1];
  double        s = 0.0;
  for (int64_t k = row_ptr[r] + lane; k < e; k += G)
    s += vals[k] * (double)src[cols[k]];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1)
    s += __shfl_xor(s, o);
  if (lane == 0)
    dst[r] = (T)s;
}

template <typename T>
void
upload(T **d, const std::vector<T> &h)
{
  HIP_THROW(hipMalloc((void **)d, std::max<size_t>(16, h.size() * sizeof(T))));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

void
free_device(SystemMatrix *M)
{
  void *bufs[] = {M->d_row_ptr,  M->d_cols,    M->d_vals,     M->d_pair_row, M->d_pair_node,
                  M->d_pair_off, M->d_inc_ptr, M->d_inc_cell, M->d_inc_point};
  for (void *b : bufs)
    if (b)
      (void)hipFree(b);
}

int64_t
ndof_of(const glsOp_ *op)
{
  return (int64_t)op->nq * (op->dim + 1);
}

// cells per chunk of element matrices: GLS_ASSEMBLE_CHUNK_CELLS, or 256 MB
int64_t
chunk_cells(const glsOp_ *op)
{
  const size_t per = (size_t)ndof_of(op) * ndof_of(op) * op->tsize();
  int64_t      c   = std::max<int64_t>(1, (int64_t)((256u << 20) / per));
  if (const char *e = std::getenv("GLS_ASSEMBLE_CHUNK_CELLS"))
    {
      char           *end = nullptr;
      const long long v   = std::strtoll(e, &end, 10);
      if (end == e || *end != '\0' || v < 1)
        throw std::runtime_error("GLS_ASSEMBLE_CHUNK_CELLS must be a positive integer");
      c = v;
    }
  return std::min<int64_t>(c, std::max<int64_t>(1, op->n_cells));
}

void
require_free_memory(size_t need, const char *what)
{
  size_t free_b = 0, total_b = 0;
  HIP_THROW(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    throw std::runtime_error(std::string("system matrix on the device: ") + what + " need " +
                             std::to_string(need >> 20) + " MB, " + std::to_string(free_b >> 20) +
                             " MB of device memory are free");
}

// the plan and its device copy (first use)
SystemMatrix *
make_system(glsOp_ *op)
{
  std::vector<uint32_t> cn;
  const uint32_t       *cell_nodes = op->h_cell_nodes.data();
  if (!op->cell_perm.empty())
    {
      // the element matrices come in the operator's internal cell order
      cn.resize(op->h_cell_nodes.size());
      for (int64_t c = 0; c < op->n_cells; ++c)
        std::copy_n(&op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * op->nq], op->nq,
                    &cn[(size_t)c * op->nq]);
      cell_nodes = cn.data();
    }
  auto *M = new SystemMatrix();
  try
    {
      M->plan = gls::assemble_make_plan(op->dim, op->degree, op->n_cells, op->n_nodes, cell_nodes,
                                        op->h_cmask.data());
      const gls::AssemblePlan &P = M->plan;
      const size_t need = (size_t)P.nnz * 12 + (size_t)(P.n_dofs + 1) * 8 +
                          (size_t)P.n_pairs * 12 + (size_t)(P.n_nodes + 1) * 8 +
                          (size_t)P.n_cells * P.nq * 8;
      require_free_memory(need, "the CSR and the assembly plan");
      upload(&M->d_row_ptr, P.row_ptr);
      upload(&M->d_cols, P.cols);
      HIP_THROW(hipMalloc((void **)&M->d_vals, std::max<size_t>(16, (size_t)P.nnz * 8)));
      upload(&M->d_pair_row, P.pair_row);
      upload(&M->d_pair_node, P.pair_node);
      upload(&M->d_pair_off, P.pair_off);
      upload(&M->d_inc_ptr, P.inc_ptr);
      upload(&M->d_inc_cell, P.inc_cell);
      upload(&M->d_inc_point, P.inc_point);
      // lanes per row as csrc/amg.hip chooses them: the smallest power of two
      // >= 8 covering half a mean row (27 entries in 2D Q1, up to 500 in 3D Q2)
      const double mean = (double)P.nnz / (double)P.n_dofs;
      M->group          = mean > 96 ? 64 : mean > 48 ? 32 : mean > 24 ? 16 : 8;
    }
  catch (...)
    {
      free_device(M);
      delete M;
      throw;
    }
  return M;
}

template <typename T>
void
launch_gather(const glsOp_ *op, const SystemMatrix *M, const void *E, int64_t c0, int64_t c1,
              hipStream_t s)
{
  const int64_t np = M->plan.n_pairs;
  const dim3    g((unsigned)((np + 255) / 256));
  gls::with_int<3, 4>(op->dim + 1, "system matrix", [&](auto nc) {
    hipLaunchKernelGGL((k_assemble_gather<T, decltype(nc)::value>), g, dim3(256), 0, s,
                       M->d_row_ptr, M->d_pair_row, M->d_pair_node, M->d_pair_off, M->d_inc_ptr,
                       M->d_inc_cell, M->d_inc_point, op->d_node_cmask, (const T *)E, c0, c1,
                       (int)ndof_of(op), M->d_vals, np);
  });
  HIP_THROW(hipGetLastError());
}

template <typename T>
void
launch_vmult(const SystemMatrix *M, void *dst, const void *src, hipStream_t s)
{
  const int64_t n = M->plan.n_dofs;
  gls::with_int<8, 16, 32, 64>(M->group, "matrix-based vmult", [&](auto grp) {
    constexpr int G = decltype(grp)::value;
    hipLaunchKernelGGL((k_csr_vmult<T, G>), dim3((unsigned)((n * G + 255) / 256)), dim3(256), 0,
                       s, M->d_row_ptr, M->d_cols, M->d_vals, (const T *)src, (T *)dst, n);
  });
  HIP_THROW(hipGetLastError());
}
} // namespace

namespace gls
{
void
system_matrix_release(glsOp_ *op)
{
  if (!op->sysmat)
    return;
  free_device(op->sysmat);
  delete op->sysmat;
  op->sysmat    = nullptr;
  op->sys_valid = false;
}

const SystemMatrix *
op_system_matrix_device(glsOp_ *op, hipStream_t s)
{
  if (op->sys_valid && op->sysmat)
    return op->sysmat;
  if (op->n_owned_nodes != op->n_nodes)
    throw std::runtime_error("system matrix on the device: single-domain operators only");
  if (!op->have_lin)
    throw std::runtime_error("system matrix before set_linearization_point");
  Section sec_("ns::initialize_system_matrix", s);
  if (!op->sysmat)
    op->sysmat = make_system(op);
  SystemMatrix       *M    = op->sysmat;
  const AssemblePlan &P    = M->plan;
  const int64_t       ndof = ndof_of(op), chunk = chunk_cells(op);
  const size_t        bytes = (size_t)chunk * ndof * ndof * op->tsize();
  require_free_memory(bytes, "the element matrices of one chunk");
  void *E = nullptr;
  HIP_THROW(hipMallocAsync(&E, std::max<size_t>(16, bytes), s));
  try
    {
      HIP_THROW(hipMemsetAsync(M->d_vals, 0, (size_t)P.nnz * 8, s));
      hipLaunchKernelGGL(k_csr_unit_diagonal, dim3((unsigned)((P.n_dofs + 255) / 256)), dim3(256),
                         0, s, M->d_row_ptr, op->d_node_cmask, M->d_vals, P.nc, P.n_dofs);
      HIP_THROW(hipGetLastError());
      for (int64_t b = 0; b < op->n_cells; b += chunk)
        {
          const int64_t e = std::min(op->n_cells, b + chunk);
          {
            Section sc("ns::initialize_system_matrix::element_matrices", s);
            op_element_matrices_device(op, E, b, e, s);
          }
          Section sc("ns::initialize_system_matrix::gather", s);
          with_real(op->prec, [&](auto t) { launch_gather<decltype(t)>(op, M, E, b, e, s); });
        }
      // node constraints: C^T A C on the same pattern
      nc_csr_device(op, M->d_row_ptr, M->d_cols, M->d_vals, s);
    }
  catch (...)
    {
      (void)hipFreeAsync(E, s);
      throw;
    }
  HIP_THROW(hipFreeAsync(E, s));
  op->sys_valid = true;
  return M;
}

void
op_csr_vmult_device(glsOp_ *op, void *dst, const void *src, hipStream_t s)
{
  const SystemMatrix *M = op_system_matrix_device(op, s);
  with_real(op->prec, [&](auto t) { launch_vmult<decltype(t)>(M, dst, src, s); });
}
} // namespace gls

extern "C" {

glsStatus
gls_op_set_matrix_based(glsOp op, int on)
{
  GLS_TRY
  if (!op)
    throw std::runtime_error("gls_op_set_matrix_based: null operator");
  if (on && op->n_owned_nodes != op->n_nodes)
    throw std::runtime_error("gls_op_set_matrix_based: single-domain operators only (a "
                             "partitioned operator stays matrix-free)");
  op->matrix_based = on != 0;
  GLS_CATCH
}

glsStatus
gls_op_invalidate_system(glsOp op)
{
  GLS_TRY
  if (!op)
    throw std::runtime_error("gls_op_invalidate_system: null operator");
  op->sys_valid = false;
  GLS_CATCH
}

glsStatus
gls_op_system_matrix_device(glsOp op, glsDeviceCSR *out, void *stream)
{
  GLS_TRY
  if (!op || !out)
    throw std::runtime_error("gls_op_system_matrix_device: null argument");
  gls::DeviceScope         dev(op->device);
  const gls::SystemMatrix *M = gls::op_system_matrix_device(op, (hipStream_t)stream);
  out->n       = M->plan.n_dofs;
  out->nnz     = M->plan.nnz;
  out->row_ptr = M->d_row_ptr;
  out->cols    = M->d_cols;
  out->vals    = M->d_vals;
  GLS_CATCH
}

glsStatus
gls_assemble_plan_host(int dim, int degree, int64_t n_cells, int64_t n_nodes,
                       const uint32_t *cell_nodes, const uint8_t *node_cmask,
                       glsAssemblePlanHost *out)
{
  GLS_TRY
  if (!out)
    throw std::runtime_error("gls_assemble_plan_host: null argument");
  const gls::AssemblePlan P =
    gls::assemble_make_plan(dim, degree, n_cells, n_nodes, cell_nodes, node_cmask);
  out->n_dofs = P.n_dofs, out->nnz = P.nnz, out->n_pairs = P.n_pairs;
  out->n_incidence        = (int64_t)P.inc_cell.size();
  out->max_cells_per_node = P.max_cells_per_node;
  const auto copy = [](auto *d, const auto &s) {
    if (d && !s.empty())
      std::copy(s.begin(), s.end(), d);
  };
  copy(out->row_ptr, P.row_ptr), copy(out->cols, P.cols);
  copy(out->pair_ptr, P.pair_ptr), copy(out->pair_node, P.pair_node);
  copy(out->pair_off, P.pair_off);
  copy(out->inc_ptr, P.inc_ptr), copy(out->inc_cell, P.inc_cell);
  copy(out->inc_point, P.inc_point);
  GLS_CATCH
}

} // extern "C"
