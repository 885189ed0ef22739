// node_constraints.hip — no-normal-flux (slip) constraints on curved
// boundaries.
//
// The reference turns every slip boundary id into
// VectorTools::compute_no_normal_flux_constraints (main.cc:285-287); on a
// curved surface such a constraint couples the velocity components of a
// node, u[node][comp] = sum_e coef[e] u[node][e], and is no entry of the
// Dirichlet mask.  The constraint matrix C (identity, with the row of every
// eliminated component replaced by coef) is block diagonal over the nodes,
// so the constrained operator C^T A C, identity on the eliminated rows, is
// the unchanged cell loop between two small kernels over the rows:
//
//   resolve    src[node][comp] <- sum_e coef[e] src[node][e]   (C x; the old
//              value kept, as the reference keeps its edge dofs,
//              operator_ns.cc:692-731)
//   transpose  r = dst[node][comp]; dst[node][e] += coef[e] r; dst[node][comp]
//              <- the kept source value (identity row, :719-721) or 0
//              (set_zero, :642, 678); the source restored
//
// The source vector is modified and restored in place on the call's stream:
// it must not be read on another stream during a vmult.  One lane per row, no
// atomics, a fixed summation order: results are bitwise repeatable.  Nothing
// on a launch path allocates, frees or synchronises.
#include "op_internal.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace gls
{
namespace
{
constexpr int NC_BLOCK = 256;

dim3
nc_grid(int64_t n)
{
  return dim3((unsigned)((n + NC_BLOCK - 1) / NC_BLOCK));
}

template <typename T, int dim>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_resolve(T *__restrict__ v, const int64_t *__restrict__ node,
               const int32_t *__restrict__ comp, const T *__restrict__ coef,
               T *__restrict__ save, int64_t n)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int64_t base = node[i] * (dim + 1);
  const int     c    = comp[i];
  T             acc  = T(0);
#pragma unroll
  for (int e = 0; e < dim; ++e)
    {
      const T k = coef[i * dim + e];
      if (e != c && k != T(0))
        acc += k * v[base + e];
    }
  if (save)
    save[i] = v[base + c];
  v[base + c] = acc;
}

template <typename T, int dim>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_transpose(T *__restrict__ dst, T *__restrict__ src, const int64_t *__restrict__ node,
                 const int32_t *__restrict__ comp, const T *__restrict__ coef,
                 const T *__restrict__ save, int64_t n, int zero)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int64_t base = node[i] * (dim + 1);
  const int     c    = comp[i];
  const T       r    = dst[base + c];
#pragma unroll
  for (int e = 0; e < dim; ++e)
    {
      const T k = coef[i * dim + e];
      if (e != c && k != T(0))
        dst[base + e] += k * r;
    }
  dst[base + c] = zero ? T(0) : save[i];
  if (src)
    src[base + c] = save[i];
}

template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_restore(T *__restrict__ v, const int64_t *__restrict__ node,
               const int32_t *__restrict__ comp, const T *__restrict__ save, int64_t n, int nc)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n)
    v[node[i] * nc + comp[i]] = save[i];
}

// AffineConstraints::distribute for the Dirichlet components: the value of
// gls_op_set_constraint_values, or zero
template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_dirichlet(T *__restrict__ v, const uint8_t *__restrict__ cmask,
                 const T *__restrict__ inhom, int64_t n_dofs, int nc)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_dofs)
    return;
  const int64_t nd = i / nc;
  const int     c  = (int)(i - nd * nc);
  if ((cmask[nd] >> c) & 1)
    v[i] = inhom ? inhom[i] : T(0);
}

// AffineConstraints::distribute for a periodic node map: one lane per slave
// entry, v[slave][c] <- v[master][c] (pairs: [n][2] slave node, master node;
// a master is no slave, so no lane reads what another writes)
template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_periodic_resolve(T *__restrict__ v, const int64_t *__restrict__ pairs, int64_t n_entries,
                     int nc)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_entries)
    return;
  const int64_t r = t / nc;
  const int     c = (int)(t - r * nc);
  v[pairs[2 * r] * nc + c] = v[pairs[2 * r + 1] * nc + c];
}

// the colour's unit vectors of component j: unit[node][j] <- value
template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_unit(T *__restrict__ unit, const int32_t *__restrict__ rows,
            const int64_t *__restrict__ node, int64_t n_rows, int nc, int j, T value)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_rows)
    return;
  unit[node[rows[t]] * nc + j] = value;
}

// after the unwrapped operator on the colour's unit vectors of component j:
// column comp of the node's velocity block (j == comp) or entry (comp, j) of
// its row comp; block [row][2][dim] = {column, row}.  Clears the unit vector.
template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_block(double *__restrict__ block, T *__restrict__ unit, const T *__restrict__ image,
             const int32_t *__restrict__ rows, const int64_t *__restrict__ node,
             const int32_t *__restrict__ comp, int64_t n_rows, int dim, int j)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_rows)
    return;
  const int64_t i    = rows[t];
  const int64_t base = node[i] * (dim + 1);
  const int     c    = comp[i];
  if (j == c)
    for (int e = 0; e < dim; ++e)
      block[(i * 2 + 0) * dim + e] = (double)image[base + e];
  else
    block[(i * 2 + 1) * dim + j] = (double)image[base + c];
  unit[base + j] = T(0);
}

// diagonal of C^T A C at a row's node, (P^T B P)_ee with P the identity whose
// row comp is coef: B_ee + coef_e (B_{e,comp} + B_{comp,e}) + coef_e^2
// B_{comp,comp}; B_ee is the assembled diagonal already in d64; 1 at comp
template <typename T>
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_diag(double *__restrict__ d64, const double *__restrict__ block,
            const int64_t *__restrict__ node, const int32_t *__restrict__ comp,
            const T *__restrict__ coef, int64_t n, int dim)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int64_t base = node[i] * (dim + 1);
  const int     c    = comp[i];
  const double *col  = block + (i * 2 + 0) * dim;
  const double *row  = block + (i * 2 + 1) * dim;
  const double  bcc  = col[c];
  for (int e = 0; e < dim; ++e)
    {
      const double k = (double)coef[i * dim + e];
      if (e != c && k != 0.0)
        d64[base + e] += k * (col[e] + row[e]) + k * k * bcc;
    }
  d64[base + c] = 1.0;
}

// C^T A C in the CSR of A, columns: one lane per matrix row of a node next to
// a listed node; every entry in an eliminated column c of node J is added,
// times coef[e], to the row's entry in column (J, e) and zeroed.  A lane owns
// its row.
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_csr_cols(const int64_t *__restrict__ rp, const int32_t *__restrict__ cols,
                double *__restrict__ vals, const int32_t *__restrict__ adj, int64_t n_adj,
                const int32_t *__restrict__ row_of, const int32_t *__restrict__ comp,
                const double *__restrict__ coef, int dim)
{
  const int     nc = dim + 1;
  const int64_t t  = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n_adj * nc)
    return;
  const int64_t r = (int64_t)adj[t / nc] * nc + t % nc;
  const int64_t b = rp[r], e_ = rp[r + 1];
  for (int64_t k = b; k < e_; ++k)
    {
      const int64_t col = cols[k];
      const int64_t J   = col / nc;
      const int     cc  = (int)(col - J * nc);
      const int32_t i   = row_of[J];
      if (i < 0 || cc != comp[i])
        continue;
      const double v = vals[k];
      vals[k]        = 0.0;
      for (int e = 0; e < dim; ++e)
        {
          const double ke = coef[(int64_t)i * dim + e];
          if (e == cc || ke == 0.0)
            continue;
          const int64_t target = J * nc + e;
          for (int64_t k2 = b; k2 < e_; ++k2)
            if (cols[k2] == target)
              {
                vals[k2] += ke * v;
                break;
              }
        }
    }
}

// rows: one lane per listed node; row (I, e) += coef[e] * row (I, c) (the
// rows of one node share their column pattern), then row (I, c) becomes the
// unit row.  A lane owns the rows of its node.
__global__ void __launch_bounds__(NC_BLOCK)
  k_nc_csr_rows(const int64_t *__restrict__ rp, const int32_t *__restrict__ cols,
                double *__restrict__ vals, const int64_t *__restrict__ node,
                const int32_t *__restrict__ comp, const double *__restrict__ coef, int64_t n,
                int dim)
{
  const int     nc = dim + 1;
  const int64_t i  = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int     c   = comp[i];
  const int64_t rc  = node[i] * nc + c;
  const int64_t bc  = rp[rc], len = rp[rc + 1] - bc;
  for (int e = 0; e < dim; ++e)
    {
      const double ke = coef[i * dim + e];
      if (e == c || ke == 0.0)
        continue;
      const int64_t be = rp[node[i] * nc + e];
      for (int64_t t = 0; t < len; ++t)
        vals[be + t] += ke * vals[bc + t];
    }
  for (int64_t t = 0; t < len; ++t)
    vals[bc + t] = cols[bc + t] == rc ? 1.0 : 0.0;
}

template <typename T>
void
diagonal_t(const glsOp_ *op, double *d64,
           void (*apply)(const glsOp_ *, void *, const void *, hipStream_t), hipStream_t s)
{
  const NodeConstraints &nc  = op->nc;
  const int              dim = op->dim;
  for (size_t k = 0; k + 1 < nc.colour_off.size(); ++k)
    {
      const int64_t  b = nc.colour_off[k], nr = nc.colour_off[k + 1] - b;
      const int32_t *rows = nc.d_rows + b;
      for (int j = 0; j < dim; ++j)
        {
          hipLaunchKernelGGL(k_nc_unit<T>, nc_grid(nr), dim3(NC_BLOCK), 0, s, (T *)nc.d_unit,
                             rows, nc.d_node, nr, dim + 1, j, T(1));
          HIP_THROW(hipGetLastError());
          apply(op, nc.d_image, nc.d_unit, s);
          hipLaunchKernelGGL(k_nc_block<T>, nc_grid(nr), dim3(NC_BLOCK), 0, s, nc.d_block,
                             (T *)nc.d_unit, (const T *)nc.d_image, rows, nc.d_node, nc.d_comp,
                             nr, dim, j);
          HIP_THROW(hipGetLastError());
        }
    }
  hipLaunchKernelGGL(k_nc_diag<T>, nc_grid(nc.n), dim3(NC_BLOCK), 0, s, d64, nc.d_block,
                     nc.d_node, nc.d_comp, (const T *)nc.d_coef, nc.n, dim);
  HIP_THROW(hipGetLastError());
}

template <typename T>
void
upload_vec(T **dptr, const std::vector<T> &h)
{
  HIP_THROW(hipMalloc((void **)dptr, std::max<size_t>(1, h.size()) * sizeof(T)));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

// rows by colour: no two nodes of a colour share a cell (greedy over the rows)
void
colour_rows(glsOp_ *op, std::vector<int32_t> &rows)
{
  NodeConstraints &nc = op->nc;
  const int        nq = op->nq;
  std::vector<int32_t> &row_of = nc.h_row_of;
  row_of.assign((size_t)op->n_nodes, -1);
  for (int64_t i = 0; i < nc.n; ++i)
    row_of[(size_t)nc.h_node[(size_t)i]] = (int32_t)i;
  std::vector<std::vector<int32_t>> nb((size_t)nc.n);
  std::vector<int32_t>              in_cell;
  std::vector<char>                 is_adj((size_t)op->n_nodes, 0);
  for (int64_t c = 0; c < op->n_cells; ++c)
    {
      in_cell.clear();
      for (int p = 0; p < nq; ++p)
        {
          const int64_t r = row_of[op->h_cell_nodes[(size_t)c * nq + p]];
          if (r >= 0)
            in_cell.push_back((int32_t)r);
        }
      if (!in_cell.empty())
        for (int p = 0; p < nq; ++p)
          is_adj[op->h_cell_nodes[(size_t)c * nq + p]] = 1;
      for (int32_t a : in_cell)
        for (int32_t b : in_cell)
          if (a != b)
            nb[(size_t)a].push_back(b);
    }
  nc.h_adj.clear();
  for (int64_t v = 0; v < op->n_nodes; ++v)
    if (is_adj[(size_t)v])
      nc.h_adj.push_back((int32_t)v);
  std::vector<int>  colour((size_t)nc.n, -1);
  std::vector<char> used;
  int               n_col = 0;
  for (int64_t i = 0; i < nc.n; ++i)
    {
      used.assign((size_t)n_col + 1, 0);
      for (int32_t b : nb[(size_t)i])
        if (colour[(size_t)b] >= 0)
          used[(size_t)colour[(size_t)b]] = 1;
      int k = 0;
      while (used[(size_t)k])
        ++k;
      colour[(size_t)i] = k;
      n_col             = std::max(n_col, k + 1);
    }
  rows.clear();
  nc.colour_off.assign(1, 0);
  for (int k = 0; k < n_col; ++k)
    {
      for (int64_t i = 0; i < nc.n; ++i)
        if (colour[(size_t)i] == k)
          rows.push_back((int32_t)i);
      nc.colour_off.push_back((int64_t)rows.size());
    }
}

void
free_dev(void *p)
{
  if (p)
    (void)hipFree(p);
}
} // namespace

void
nc_release(glsOp_ *op)
{
  NodeConstraints &nc = op->nc;
  free_dev(nc.d_node);
  free_dev(nc.d_comp);
  free_dev(nc.d_coef);
  free_dev(nc.d_save);
  free_dev(nc.d_rows);
  free_dev(nc.d_row_of);
  free_dev(nc.d_adj);
  free_dev(nc.d_cmask_all);
  free_dev(nc.d_coef64);
  free_dev(nc.d_unit);
  free_dev(nc.d_image);
  free_dev(nc.d_block);
  nc = NodeConstraints();
}

void
nc_resolve(const glsOp_ *op, void *v, bool save, hipStream_t s)
{
  if (op->nc.n == 0)
    return;
  const NodeConstraints &nc = op->nc;
  with_real(op->prec, [&](auto t) {
    using T = decltype(t);
    with_int<2, 3>(op->dim, "node constraints", [&](auto d) {
      hipLaunchKernelGGL((k_nc_resolve<T, decltype(d)::value>), nc_grid(nc.n), dim3(NC_BLOCK), 0,
                         s, (T *)v, nc.d_node, nc.d_comp, (const T *)nc.d_coef,
                         save ? (T *)nc.d_save : nullptr, nc.n);
    });
  });
  HIP_THROW(hipGetLastError());
}

void
nc_transpose(const glsOp_ *op, void *dst, void *restore_src, bool zero, hipStream_t s)
{
  if (op->nc.n == 0)
    return;
  const NodeConstraints &nc = op->nc;
  with_real(op->prec, [&](auto t) {
    using T = decltype(t);
    with_int<2, 3>(op->dim, "node constraints", [&](auto d) {
      hipLaunchKernelGGL((k_nc_transpose<T, decltype(d)::value>), nc_grid(nc.n), dim3(NC_BLOCK),
                         0, s, (T *)dst, (T *)restore_src, nc.d_node, nc.d_comp,
                         (const T *)nc.d_coef, (const T *)nc.d_save, nc.n, zero ? 1 : 0);
    });
  });
  HIP_THROW(hipGetLastError());
}

void
nc_restore(const glsOp_ *op, void *v, hipStream_t s)
{
  const NodeConstraints &nc = op->nc;
  if (nc.n == 0)
    return;
  with_real(op->prec, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_nc_restore<T>, nc_grid(nc.n), dim3(NC_BLOCK), 0, s, (T *)v, nc.d_node,
                       nc.d_comp, (const T *)nc.d_save, nc.n, op->dim + 1);
  });
  HIP_THROW(hipGetLastError());
}

void
nc_diagonal(const glsOp_ *op, double *d64,
            void (*apply)(const glsOp_ *, void *, const void *, hipStream_t), hipStream_t s)
{
  if (op->nc.n == 0)
    return;
  with_real(op->prec, [&](auto t) { diagonal_t<decltype(t)>(op, d64, apply, s); });
}

void
nc_csr_device(const glsOp_ *op, const int64_t *row_ptr, const int32_t *cols, double *vals,
              hipStream_t s)
{
  const NodeConstraints &nc = op->nc;
  if (nc.n == 0)
    return;
  const int64_t n_adj = (int64_t)nc.h_adj.size();
  hipLaunchKernelGGL(k_nc_csr_cols, nc_grid(n_adj * (op->dim + 1)), dim3(NC_BLOCK), 0, s, row_ptr,
                     cols, vals, nc.d_adj, n_adj, nc.d_row_of, nc.d_comp, nc.d_coef64, op->dim);
  HIP_THROW(hipGetLastError());
  hipLaunchKernelGGL(k_nc_csr_rows, nc_grid(nc.n), dim3(NC_BLOCK), 0, s, row_ptr, cols, vals,
                     nc.d_node, nc.d_comp, nc.d_coef64, nc.n, op->dim);
  HIP_THROW(hipGetLastError());
}

void
nc_csr_host(const glsOp_ *op, const int64_t *rp, const int64_t *cols, double *vals)
{
  const NodeConstraints &nc  = op->nc;
  const int              dim = op->dim, ncomp = dim + 1;
  for (int32_t adj : nc.h_adj)
    for (int cr = 0; cr < ncomp; ++cr)
      {
        const int64_t r = (int64_t)adj * ncomp + cr;
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k)
          {
            const int64_t J = cols[k] / ncomp;
            const int     cc = (int)(cols[k] % ncomp);
            const int32_t i  = nc.h_row_of[(size_t)J];
            if (i < 0 || cc != nc.h_comp[(size_t)i])
              continue;
            const double v = vals[k];
            vals[k]        = 0.0;
            for (int e = 0; e < dim; ++e)
              {
                const double ke = nc.h_coef[(size_t)i * dim + e];
                if (e == cc || ke == 0.0)
                  continue;
                const int64_t *it = std::lower_bound(cols + rp[r], cols + rp[r + 1], J * ncomp + e);
                vals[it - cols] += ke * v;
              }
          }
      }
  for (int64_t i = 0; i < nc.n; ++i)
    {
      const int     c   = nc.h_comp[(size_t)i];
      const int64_t rc  = nc.h_node[(size_t)i] * ncomp + c;
      const int64_t bc  = rp[rc], len = rp[rc + 1] - bc;
      for (int e = 0; e < dim; ++e)
        {
          const double ke = nc.h_coef[(size_t)i * dim + e];
          if (e == c || ke == 0.0)
            continue;
          const int64_t be = rp[nc.h_node[(size_t)i] * ncomp + e];
          for (int64_t t = 0; t < len; ++t)
            vals[be + t] += ke * vals[bc + t];
        }
      for (int64_t t = 0; t < len; ++t)
        vals[bc + t] = cols[bc + t] == rc ? 1.0 : 0.0;
    }
}

// a non-zero Dirichlet value on a node with a row: the row's coefficient on
// that component was dropped because the chain resolves to the homogeneous
// value, so such a value is not modelled
void
nc_check_values(const glsOp_ *op, const void *d_values, hipStream_t s)
{
  if (op->nc.n == 0 || !d_values)
    return;
  const int    nc = op->dim + 1;
  const size_t ts = op->tsize();
  std::vector<char> h((size_t)op->n_dofs * ts);
  HIP_THROW(hipMemcpyAsync(h.data(), d_values, h.size(), hipMemcpyDeviceToHost, s));
  HIP_THROW(hipStreamSynchronize(s));
  for (int64_t i = 0; i < op->nc.n; ++i)
    {
      const int64_t node = op->nc.h_node[(size_t)i];
      for (int e = 0; e < op->dim; ++e)
        if ((op->h_cmask[(size_t)node] >> e) & 1)
          {
            const size_t dof = (size_t)node * nc + e;
            const double v   = with_real(op->prec, [&](auto t) {
              return (double)((const decltype(t) *)h.data())[dof];
            });
            if (v != 0.0)
              throw std::runtime_error(
                "node constraints: a non-zero constraint value on component " +
                std::to_string(e) + " of node " + std::to_string(node) +
                ", which a node-constraint row references, is not supported");
          }
    }
}
} // namespace gls

extern "C" {

glsStatus
gls_op_set_node_constraints(glsOp op, int64_t n, const int64_t *nodes, const int32_t *comp,
                            const double *coef, void *stream)
{
  GLS_TRY
  using namespace gls;
  if (!op || n < 0 || (n > 0 && (!nodes || !comp || !coef)))
    throw std::runtime_error("gls_op_set_node_constraints: bad argument");
  if (n > 0 && op->n_owned_dofs != op->n_dofs)
    throw std::runtime_error("gls_op_set_node_constraints: node constraints on a partitioned "
                             "operator are not supported");
  const int dim = op->dim;
  for (int64_t i = 0; i < n; ++i)
    {
      const std::string at = " (row " + std::to_string(i) + ")";
      if (nodes[i] < 0 || nodes[i] >= op->n_nodes)
        throw std::runtime_error("gls_op_set_node_constraints: node out of range" + at);
      if (i > 0 && nodes[i] <= nodes[i - 1])
        throw std::runtime_error("gls_op_set_node_constraints: nodes must be ascending and "
                                 "unique (unsorted or repeated node" + at + ")");
      if (comp[i] < 0 || comp[i] >= dim)
        throw std::runtime_error("gls_op_set_node_constraints: comp must be a velocity "
                                 "component" + at);
      if (!op->h_master.empty() && op->h_master[(size_t)nodes[i]] != nodes[i])
        throw std::runtime_error("gls_op_set_node_constraints: node " +
                                 std::to_string(nodes[i]) + " is a slave of the periodic node "
                                 "map (its row belongs to its master)" + at);
      const unsigned mask = op->h_cmask[(size_t)nodes[i]];
      if ((mask >> comp[i]) & 1)
        throw std::runtime_error("gls_op_set_node_constraints: comp is in the node's Dirichlet "
                                 "mask" + at);
      for (int e = 0; e < dim; ++e)
        {
          const double k = coef[i * dim + e];
          if (!std::isfinite(k))
            throw std::runtime_error("gls_op_set_node_constraints: coefficient not finite" + at);
          if (e == comp[i] && k != 0.0)
            throw std::runtime_error("gls_op_set_node_constraints: coef[comp] must be zero" + at);
          if (((mask >> e) & 1) && k != 0.0)
            throw std::runtime_error("gls_op_set_node_constraints: non-zero coefficient on a "
                                     "Dirichlet component" + at);
        }
    }
  hipStream_t s = (hipStream_t)stream;
  DeviceScope scope(op->device);
  HIP_THROW(hipStreamSynchronize(s));
  nc_release(op);
  NodeConstraints &nc = op->nc;
  if (n > 0)
    {
      nc.h_node.assign(nodes, nodes + n);
      nc.h_comp.assign(comp, comp + n);
      nc.h_coef.assign(coef, coef + n * dim);
      nc.n = n;
      try
        {
          nc_check_values(op, op->d_inhom, s);
          upload_vec(&nc.d_node, nc.h_node);
          upload_vec(&nc.d_comp, nc.h_comp);
          const size_t ts = op->tsize();
          upload_real(op->prec, &nc.d_coef, nc.h_coef);
          HIP_THROW(hipMalloc(&nc.d_save, (size_t)n * ts));
          std::vector<int32_t> rows;
          colour_rows(op, rows);
          upload_vec(&nc.d_rows, rows);
          upload_vec(&nc.d_row_of, nc.h_row_of);
          upload_vec(&nc.d_adj, nc.h_adj);
          std::vector<uint8_t> all(op->h_cmask);
          for (int64_t i = 0; i < n; ++i)
            all[(size_t)nodes[i]] |= (uint8_t)(1u << comp[i]);
          upload_vec(&nc.d_cmask_all, all);
          upload_vec(&nc.d_coef64, nc.h_coef);
          HIP_THROW(hipMalloc(&nc.d_unit, (size_t)op->n_dofs * ts));
          HIP_THROW(hipMalloc(&nc.d_image, (size_t)op->n_dofs * ts));
          HIP_THROW(hipMalloc((void **)&nc.d_block, (size_t)n * 2 * dim * sizeof(double)));
          HIP_THROW(hipMemset(nc.d_unit, 0, (size_t)op->n_dofs * ts));
          HIP_THROW(hipMemset(nc.d_block, 0, (size_t)n * 2 * dim * sizeof(double)));
        }
      catch (...)
        {
          nc_release(op);
          throw;
        }
    }
  ++op->version;
  ++op->nc_version;
  op_invalidate_system(op);
  GLS_CATCH
}

glsStatus
gls_op_n_node_constraints(glsOp op, int64_t *n, int *n_colours)
{
  GLS_TRY
  if (!op || !n)
    throw std::runtime_error("gls_op_n_node_constraints: null argument");
  *n = op->nc.n;
  if (n_colours)
    *n_colours = op->nc.n ? (int)op->nc.colour_off.size() - 1 : 0;
  GLS_CATCH
}

glsStatus
gls_op_distribute(glsOp op, void *vec, int homogeneous, void *stream)
{
  GLS_TRY
  using namespace gls;
  if (!op || !vec)
    throw std::runtime_error("gls_op_distribute: null argument");
  hipStream_t s = (hipStream_t)stream;
  void       *v = vec;
  if (op->stage.active())
    {
      const void *x = op->stage.in_vec(vec, 0, s);
      v             = op->stage.out_vec(vec);
      HIP_THROW(hipMemcpyAsync(v, x, (size_t)op->n_dofs * op->tsize(), hipMemcpyDeviceToDevice,
                               s));
    }
  const void *inhom = homogeneous ? nullptr : op->d_inhom;
  if (op->n_dofs > 0)
    {
      with_real(op->prec, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_nc_dirichlet<T>, nc_grid(op->n_dofs), dim3(NC_BLOCK), 0, s, (T *)v,
                           op->d_node_cmask, (const T *)inhom, op->n_dofs, op->dim + 1);
      });
      HIP_THROW(hipGetLastError());
    }
  nc_resolve(op, v, false, s);
  // periodic node map: slave := master, after the masters took their values
  if (op->n_slaves > 0)
    {
      const int64_t n = op->n_slaves * (op->dim + 1);
      with_real(op->prec, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_periodic_resolve<T>, nc_grid(n), dim3(NC_BLOCK), 0, s, (T *)v,
                           op->d_slave_pairs, n, op->dim + 1);
      });
      HIP_THROW(hipGetLastError());
    }
  op->stage.finish_out(vec, s);
  op->stage.done(s);
  GLS_CATCH
}

} // extern "C"
