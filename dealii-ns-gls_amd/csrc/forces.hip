// forces.hip — drag / lift and pressure-drop evaluation on the device.
//
// SimulationCylinder::postprocess (simulation.cc:433-549) integrates
//   f = (-p I + 2 nu eps(u)) . n,  n = -(outward unit normal of the cell),
// over the cylinder's boundary faces with QGauss<dim-1>(3) (:451-497) and
// evaluates the pressure at two points through RemotePointEvaluation +
// point_values<1>(avg) (:512-541).  Both run once per time step.
//
// Surface force: one workgroup (one wavefront) per face.  The cell's nodal
// (u, p) -- read plain through d_nodes & NODE_MASK, as k_max_u -- and its
// node coordinates are staged in LDS as FP64; one lane per face Gauss point
// evaluates the reference gradients by the tensor product of the 1D Lagrange
// values / derivatives at the Gauss points and at the face end
// (xi_axis = side), forms J, J^{-1}, the normal and the area element in FP64
// and its point's force; the face's points are summed in point order into
// [n_faces][dim] (stage 1), one workgroup sums the faces in a fixed order
// (stage 2).  No atomics: the result is bitwise repeatable and does not
// depend on the operator's internal cell order.  Per-face device state is
// the cell, the face number and the cell's node coordinates only.
//
// Probe: (cell, xi) pairs found on the host (probe_locate.cc); one lane per
// point evaluates all dim+1 components at its pairs and averages.
#include "kernels.h"
#include "op_internal.h"
#include "probe_locate.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace gls
{
namespace
{
constexpr int FORCE_BLOCK = 64;
constexpr int MAX_Q1D     = 4;

// QGauss(n) on [0, 1] and the Gauss-Lobatto support points of FE_Q(k)
struct Rule1D
{
  int    n;
  double x[MAX_Q1D], w[MAX_Q1D];
  double gll[4];
  double rden[4][4]; // 1 / (gll[i] - gll[j])
};

Rule1D
make_rule(int n_q_1d, int degree)
{
  Rule1D r{};
  r.n = n_q_1d;
  double x[MAX_Q1D] = {0, 0, 0, 0}, w[MAX_Q1D] = {0, 0, 0, 0}; // on [-1, 1]
  switch (n_q_1d)
    {
      case 1:
        x[0] = 0, w[0] = 2;
        break;
      case 2:
        x[0] = -1.0 / std::sqrt(3.0), x[1] = -x[0], w[0] = w[1] = 1;
        break;
      case 3:
        x[0] = -std::sqrt(0.6), x[1] = 0, x[2] = -x[0];
        w[0] = w[2] = 5.0 / 9.0, w[1] = 8.0 / 9.0;
        break;
      default:
        {
          const double a = std::sqrt(3.0 / 7.0 - 2.0 / 7.0 * std::sqrt(1.2)),
                       b = std::sqrt(3.0 / 7.0 + 2.0 / 7.0 * std::sqrt(1.2));
          x[0] = -b, x[1] = -a, x[2] = a, x[3] = b;
          w[0] = w[3] = (18.0 - std::sqrt(30.0)) / 36.0;
          w[1] = w[2] = (18.0 + std::sqrt(30.0)) / 36.0;
        }
    }
  for (int i = 0; i < n_q_1d; ++i)
    {
      r.x[i] = 0.5 + 0.5 * x[i];
      r.w[i] = 0.5 * w[i];
    }
  gll_nodes(degree, r.gll);
  for (int i = 0; i <= degree; ++i)
    for (int j = 0; j <= degree; ++j)
      r.rden[i][j] = i == j ? 0.0 : 1.0 / (r.gll[i] - r.gll[j]);
  return r;
}

// 1D Lagrange basis on the n support points at x: values and derivatives
// (rden[i][j] = 1 / (x_i - x_j), formed on the host: no division here)
template <int n>
__device__ inline void
lagrange_1d(const Rule1D &r, double x, double *v, double *dv)
{
#pragma unroll
  for (int i = 0; i < n; ++i)
    {
      double val = 1, der = 0;
#pragma unroll
      for (int j = 0; j < n; ++j)
        if (j != i)
          {
            double prod = r.rden[i][j];
#pragma unroll
            for (int m = 0; m < n; ++m)
              if (m != i && m != j)
                prod *= (x - r.gll[m]) * r.rden[i][m];
            der += prod;
            val *= (x - r.gll[j]) * r.rden[i][j];
          }
      v[i]  = val;
      dv[i] = der;
    }
}

// inverse (inv[a][e] = d xi_a / d x_e) and determinant of J[d][a]
template <int dim>
__device__ inline double
invert(const double (&J)[3][3], double (&inv)[3][3])
{
  if (dim == 2)
    {
      const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0], r = 1.0 / det;
      inv[0][0] = J[1][1] * r, inv[0][1] = -J[0][1] * r;
      inv[1][0] = -J[1][0] * r, inv[1][1] = J[0][0] * r;
      return det;
    }
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1],
               c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
               c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, r = 1.0 / det;
  inv[0][0] = c00 * r;
  inv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r;
  inv[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r;
  inv[1][0] = c01 * r;
  inv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r;
  inv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r;
  inv[2][0] = c02 * r;
  inv[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r;
  inv[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r;
  return det;
}

// stage 1: out[f][d] = sum over the face's Gauss points (first tangential
// axis fastest) of ((-p I + 2 nu eps(u)) . (-n_outward))_d JxW
template <int dim, int k, typename T>
__global__ void __launch_bounds__(FORCE_BLOCK)
  k_face_force(const uint32_t *__restrict__ nodes, const T *__restrict__ vec,
               const int64_t *__restrict__ cell, const int32_t *__restrict__ face,
               const double *__restrict__ coords, Rule1D rule, double nu,
               double *__restrict__ out)
{
  constexpr int n = k + 1, nq = ipow(n, dim), nc = dim + 1;
  constexpr int MAX_NQF = MAX_Q1D * MAX_Q1D;
  __shared__ double sV[nq][nc];
  __shared__ double sX[nq][dim];
  __shared__ double sF[MAX_NQF][dim];
  const int64_t f = blockIdx.x, c = cell[f];
  const int     t = threadIdx.x, fn = face[f], ax = fn >> 1, side = fn & 1;
  const int     nqf = dim == 3 ? rule.n * rule.n : rule.n;
  for (int i = t; i < nq; i += FORCE_BLOCK)
    {
      const size_t node = nodes[c * nq + i] & NODE_MASK;
#pragma unroll
      for (int d = 0; d < nc; ++d)
        sV[i][d] = (double)vec[node * nc + d];
#pragma unroll
      for (int d = 0; d < dim; ++d)
        sX[i][d] = coords[((size_t)f * nq + i) * dim + d];
    }
  __syncthreads();
  if (t < nqf)
    {
      // reference point: xi_ax = side, the tangential axes at the Gauss points
      const int qt[2] = {t % rule.n, t / rule.n};
      double    v[dim][n], dv[dim][n], w = 1;
      int       nt = 0;
#pragma unroll
      for (int e = 0; e < dim; ++e)
        {
          double x = (double)side;
          if (e != ax)
            {
              x = rule.x[qt[nt]];
              w *= rule.w[qt[nt]];
              ++nt;
            }
          lagrange_1d<n>(rule, x, v[e], dv[e]);
        }
      double p = 0, GU[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}},
             J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
      for (int i = 0; i < nq; ++i)
        {
          const int ia[3] = {i % n, (i / n) % n, dim == 3 ? i / (n * n) : 0};
          double    ph = 1, g[dim];
#pragma unroll
          for (int e = 0; e < dim; ++e)
            ph *= v[e][ia[e]];
#pragma unroll
          for (int e = 0; e < dim; ++e)
            {
              g[e] = dv[e][ia[e]];
#pragma unroll
              for (int e2 = 0; e2 < dim; ++e2)
                if (e2 != e)
                  g[e] *= v[e2][ia[e2]];
            }
          p += ph * sV[i][dim];
#pragma unroll
          for (int d = 0; d < dim; ++d)
#pragma unroll
            for (int e = 0; e < dim; ++e)
              {
                GU[d][e] += sV[i][d] * g[e];
                J[d][e] += sX[i][d] * g[e];
              }
        }
      double       inv[3][3];
      const double det = invert<dim>(J, inv);
      // J^{-T} n_ref, n_ref = (2 side - 1) e_ax: length = area element /
      // |det J|, direction = outward normal
      double m[dim], mn = 0;
#pragma unroll
      for (int e = 0; e < dim; ++e)
        {
          double r = 0;
#pragma unroll
          for (int a = 0; a < dim; ++a)
            r += a == ax ? inv[a][e] : 0.0;
          m[e] = (2 * side - 1) * r;
          mn += m[e] * m[e];
        }
      mn               = sqrt(mn);
      const double jxw = fabs(det) * mn * w;
      // physical gradient G[d][e] = d u_d / d x_e
      double G[dim][dim];
#pragma unroll
      for (int d = 0; d < dim; ++d)
#pragma unroll
        for (int e = 0; e < dim; ++e)
          {
            double s = 0;
#pragma unroll
            for (int a = 0; a < dim; ++a)
              s += GU[d][a] * inv[a][e];
            G[d][e] = s;
          }
#pragma unroll
      for (int d = 0; d < dim; ++d)
        {
          double s = 0;
#pragma unroll
          for (int e = 0; e < dim; ++e)
            s += ((d == e ? -p : 0.0) + nu * (G[d][e] + G[e][d])) * (-m[e] / mn);
          sF[t][d] = s * jxw;
        }
    }
  __syncthreads();
  if (t < dim)
    {
      double s = 0;
      for (int q = 0; q < nqf; ++q)
        s += sF[q][t];
      out[f * dim + t] = s;
    }
}

// stage 2: total[d] = sum of out[f][d]: lane t adds faces t, t + 256, ... in
// order, then a fixed tree (total: host-mapped memory, read after the
// stream's synchronize without a copy)
__global__ void __launch_bounds__(256)
  k_force_sum(const double *__restrict__ out, int64_t n_faces, int dim, double *__restrict__ total)
{
  __shared__ double red[3][256];
  const int         t = threadIdx.x;
  for (int d = 0; d < dim; ++d)
    {
      double s = 0;
      for (int64_t f = t; f < n_faces; f += 256)
        s += out[f * dim + d];
      red[d][t] = s;
    }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1)
    {
      if (t < st)
        for (int d = 0; d < dim; ++d)
          red[d][t] += red[d][t + st];
      __syncthreads();
    }
  if (t < dim)
    total[t] = red[t][0];
}

// one lane per point: the dim+1 components at the point's (cell, xi) pairs,
// summed in pair order; averaged (avg) or left as the sum
template <int dim, int k, typename T>
__global__ void __launch_bounds__(FORCE_BLOCK)
  k_probe(const uint32_t *__restrict__ nodes, const T *__restrict__ vec,
          const int64_t *__restrict__ poff, const int64_t *__restrict__ pcell,
          const double *__restrict__ pxi, Rule1D rule, int64_t n_points, int avg,
          double *__restrict__ out)
{
  constexpr int n = k + 1, nq = ipow(n, dim), nc = dim + 1;
  const int64_t pt = (int64_t)blockIdx.x * FORCE_BLOCK + threadIdx.x;
  if (pt >= n_points)
    return;
  double val[nc];
#pragma unroll
  for (int d = 0; d < nc; ++d)
    val[d] = 0;
  const int64_t b = poff[pt], e_ = poff[pt + 1];
  for (int64_t j = b; j < e_; ++j)
    {
      const int64_t c = pcell[j];
      double        v[dim][n], dv[dim][n];
#pragma unroll
      for (int e = 0; e < dim; ++e)
        lagrange_1d<n>(rule, pxi[j * dim + e], v[e], dv[e]);
#pragma unroll
      for (int i = 0; i < nq; ++i)
        {
          const int ia[3] = {i % n, (i / n) % n, dim == 3 ? i / (n * n) : 0};
          double    ph = 1;
#pragma unroll
          for (int e = 0; e < dim; ++e)
            ph *= v[e][ia[e]];
          const size_t node = nodes[c * nq + i] & NODE_MASK;
#pragma unroll
          for (int d = 0; d < nc; ++d)
            val[d] += ph * (double)vec[node * nc + d];
        }
    }
  const double scale = (avg && e_ > b) ? 1.0 / (double)(e_ - b) : 1.0;
#pragma unroll
  for (int d = 0; d < nc; ++d)
    out[pt * nc + d] = val[d] * scale;
}

template <int dim, int k, typename T>
void
launch_force(const glsOp_ *op, const void *vec, hipStream_t s)
{
  const Forces &F = op->forces;
  hipLaunchKernelGGL((k_face_force<dim, k, T>), dim3((unsigned)F.n_faces), dim3(FORCE_BLOCK), 0,
                     s, op->d_nodes, (const T *)vec, F.d_cell, F.d_face, F.d_coords,
                     make_rule(F.n_q_1d, k), op->prm.nu, F.d_out);
}

template <int dim, int k, typename T>
void
launch_probe(const glsOp_ *op, const void *vec, bool avg, hipStream_t s)
{
  const Forces &F = op->forces;
  hipLaunchKernelGGL((k_probe<dim, k, T>),
                     dim3((unsigned)((F.n_points + FORCE_BLOCK - 1) / FORCE_BLOCK)),
                     dim3(FORCE_BLOCK), 0, s, op->d_nodes, (const T *)vec, F.d_poff, F.d_pcell,
                     F.d_pxi, make_rule(1, k), F.n_points, avg ? 1 : 0, F.d_pval);
}

// caller cell -> internal cell
std::vector<int64_t>
internal_cells(const glsOp_ *op)
{
  std::vector<int64_t> internal((size_t)op->n_cells);
  for (int64_t c = 0; c < op->n_cells; ++c)
    internal[(size_t)ext_cell(op, c)] = c;
  return internal;
}

template <typename V>
void
upload_new(V **d, const std::vector<V> &h)
{
  HIP_THROW(hipMalloc((void **)d, std::max<size_t>(1, h.size()) * sizeof(V)));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*d, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
}

void
release_faces(Forces &F)
{
  void *bufs[] = {F.d_cell, F.d_face, F.d_coords, F.d_out};
  for (void *p : bufs)
    if (p)
      (void)hipFree(p);
  if (F.h_total)
    (void)hipHostFree(F.h_total);
  F.d_cell = nullptr, F.d_face = nullptr, F.d_coords = nullptr, F.d_out = nullptr;
  F.h_total = F.d_total = nullptr;
  F.n_faces    = 0;
  F.have_faces = false;
}

void
release_points(Forces &F)
{
  void *bufs[] = {F.d_poff, F.d_pcell, F.d_pxi};
  for (void *p : bufs)
    if (p)
      (void)hipFree(p);
  if (F.h_pval)
    (void)hipHostFree(F.h_pval);
  F.d_poff = nullptr, F.d_pcell = nullptr, F.d_pxi = nullptr;
  F.h_pval = F.d_pval = nullptr;
  F.n_points = F.n_pairs = 0;
  F.h_count.clear();
  F.have_points = false;
}

void
check_geometry(const glsOp_ *op, const char *who)
{
  if (op->own_mapping)
    throw std::runtime_error(std::string(who) + ": not supported on an operator created with "
                                                "mapping_points");
}
} // namespace

void
forces_release(glsOp_ *op)
{
  release_faces(op->forces);
  release_points(op->forces);
}

// per-face forces into the operator's buffer ([n_faces][dim]) and their sum
// into its host-mapped total; vec: node-major device vector
void
forces_run(const glsOp_ *op, const void *vec, hipStream_t s)
{
  const Forces &F = op->forces;
  if (F.n_faces > 0)
    with_real(op->prec, [&](auto t) {
      with_dim_degree(op->dim, op->degree, "forces", [&](auto d, auto k) {
        launch_force<decltype(d)::value, decltype(k)::value, decltype(t)>(op, vec, s);
      });
    });
  hipLaunchKernelGGL(k_force_sum, dim3(1), dim3(256), 0, s, (const double *)F.d_out, F.n_faces,
                     op->dim, F.d_total);
  HIP_THROW(hipGetLastError());
}

// the probe values (avg) or their sums over the local cells into host
// values[n_points][dim + 1]; synchronises
void
probe_run(glsOp_ *op, const void *vec, bool avg, double *values, hipStream_t s)
{
  const Forces &F = op->forces;
  if (!F.have_points)
    throw std::runtime_error("gls_op_probe before gls_op_set_probe_points");
  if (F.n_points == 0)
    return;
  const void *x = op->stage.in_vec(vec, 0, s);
  with_real(op->prec, [&](auto t) {
    with_dim_degree(op->dim, op->degree, "probe", [&](auto d, auto k) {
      launch_probe<decltype(d)::value, decltype(k)::value, decltype(t)>(op, x, avg, s);
    });
  });
  HIP_THROW(hipGetLastError());
  // the kernel wrote host-mapped memory: complete after the synchronize
  HIP_THROW(hipStreamSynchronize(s));
  std::copy(F.h_pval, F.h_pval + (size_t)F.n_points * (op->dim + 1), values);
}

const std::vector<int64_t> &
probe_counts(const glsOp_ *op)
{
  return op->forces.h_count;
}
} // namespace gls

extern "C" {

glsStatus
gls_op_set_force_faces(glsOp op, int64_t n_faces, const int64_t *cells, const int32_t *face_no,
                       const double *node_coords, int n_q_1d)
{
  GLS_TRY
  if (!op || n_faces < 0 || (n_faces > 0 && (!cells || !face_no || !node_coords)))
    throw std::runtime_error("gls_op_set_force_faces: bad arguments");
  gls::check_geometry(op, "gls_op_set_force_faces");
  if (n_q_1d < 1 || n_q_1d > gls::MAX_Q1D)
    throw std::runtime_error("gls_op_set_force_faces: n_q_1d must be 1..4");
  const int dim = op->dim, nq = op->nq;
  for (int64_t f = 0; f < n_faces; ++f)
    if (cells[f] < 0 || cells[f] >= op->n_cells || face_no[f] < 0 || face_no[f] >= 2 * dim)
      throw std::runtime_error("gls_op_set_force_faces: bad cell or face number (face " +
                               std::to_string(f) + ")");
  gls::DeviceScope dev(op->device);
  gls::Forces     &F = op->forces;
  HIP_THROW(hipDeviceSynchronize()); // no launch on the old list may still run
  gls::release_faces(F);
  F.n_q_1d = n_q_1d;
  const std::vector<int64_t> internal = gls::internal_cells(op);
  std::vector<int64_t>       cell((size_t)n_faces);
  std::vector<int32_t>       face(face_no, face_no + n_faces);
  std::vector<double>        xc((size_t)n_faces * nq * dim);
  for (int64_t f = 0; f < n_faces; ++f)
    {
      cell[(size_t)f] = internal[(size_t)cells[f]];
      for (int i = 0; i < nq; ++i)
        {
          const size_t node = op->geo_nodes()[(size_t)cells[f] * nq + i];
          for (int d = 0; d < dim; ++d)
            xc[((size_t)f * nq + i) * dim + d] = node_coords[node * dim + d];
        }
    }
  gls::upload_new(&F.d_cell, cell);
  gls::upload_new(&F.d_face, face);
  gls::upload_new(&F.d_coords, xc);
  HIP_THROW(hipMalloc((void **)&F.d_out, (size_t)std::max<int64_t>(n_faces, 1) * dim * sizeof(double)));
  // the summed force lands in host-mapped memory (no copy back per step)
  HIP_THROW(hipHostMalloc((void **)&F.h_total, 3 * sizeof(double),
                          hipHostMallocMapped | hipHostMallocCoherent));
  HIP_THROW(hipHostGetDevicePointer((void **)&F.d_total, F.h_total, 0));
  F.n_faces    = n_faces;
  F.have_faces = true;
  GLS_CATCH
}

static void
surface_force(glsOp op, const void *vec, double *out, bool per_face, void *stream, const char *who)
{
  if (!op || !vec || !out)
    throw std::runtime_error(std::string(who) + ": null argument");
  const gls::Forces &F = op->forces;
  if (!F.have_faces)
    throw std::runtime_error(std::string(who) + " before gls_op_set_force_faces");
  if (!op->have_prm)
    throw std::runtime_error(std::string(who) + ": nu is not set (gls_op_set_parameters)");
  hipStream_t s = (hipStream_t)stream;
  const void *x = op->stage.in_vec(vec, 0, s);
  gls::forces_run(op, x, s);
  const size_t dim = (size_t)op->dim;
  if (per_face && F.n_faces > 0)
    HIP_THROW(hipMemcpyAsync(out, F.d_out, (size_t)F.n_faces * dim * sizeof(double),
                             hipMemcpyDeviceToHost, s));
  HIP_THROW(hipStreamSynchronize(s));
  if (!per_face)
    std::copy(F.h_total, F.h_total + dim, out);
}

glsStatus
gls_op_surface_force(glsOp op, const void *vec, double *force, void *stream)
{
  GLS_TRY
  surface_force(op, vec, force, false, stream, "gls_op_surface_force");
  GLS_CATCH
}

glsStatus
gls_op_surface_force_faces(glsOp op, const void *vec, double *per_face, void *stream)
{
  GLS_TRY
  surface_force(op, vec, per_face, true, stream, "gls_op_surface_force_faces");
  GLS_CATCH
}

glsStatus
gls_op_set_probe_points(glsOp op, int64_t n_points, const double *xyz, const double *node_coords,
                        int64_t *n_cells_found)
{
  GLS_TRY
  if (!op || n_points < 0 || (n_points > 0 && (!xyz || !node_coords)))
    throw std::runtime_error("gls_op_set_probe_points: bad arguments");
  gls::check_geometry(op, "gls_op_set_probe_points");
  gls::ProbePairs pairs;
  gls::locate_points(op->dim, op->degree, op->n_cells, op->geo_nodes().data(), op->n_nodes,
                     node_coords, n_points, xyz, pairs);
  gls::DeviceScope dev(op->device);
  gls::Forces     &F = op->forces;
  HIP_THROW(hipDeviceSynchronize()); // no launch on the old list may still run
  gls::release_points(F);
  const std::vector<int64_t> internal = gls::internal_cells(op);
  for (int64_t &c : pairs.cell)
    c = internal[(size_t)c];
  F.h_count.resize((size_t)n_points);
  for (int64_t p = 0; p < n_points; ++p)
    {
      F.h_count[(size_t)p] = pairs.off[(size_t)p + 1] - pairs.off[(size_t)p];
      if (n_cells_found)
        n_cells_found[p] = F.h_count[(size_t)p];
    }
  gls::upload_new(&F.d_poff, pairs.off);
  gls::upload_new(&F.d_pcell, pairs.cell);
  gls::upload_new(&F.d_pxi, pairs.xi);
  // the values land in host-mapped memory (no copy back per step)
  HIP_THROW(hipHostMalloc((void **)&F.h_pval,
                          std::max<size_t>(1, (size_t)n_points * (op->dim + 1)) * sizeof(double),
                          hipHostMallocMapped | hipHostMallocCoherent));
  HIP_THROW(hipHostGetDevicePointer((void **)&F.d_pval, F.h_pval, 0));
  F.n_points    = n_points;
  F.n_pairs     = (int64_t)pairs.cell.size();
  F.have_points = true;
  GLS_CATCH
}

glsStatus
gls_op_probe(glsOp op, const void *vec, double *values, void *stream)
{
  GLS_TRY
  if (!op || !vec || (!values && op->forces.n_points > 0))
    throw std::runtime_error("gls_op_probe: null argument");
  gls::probe_run(op, vec, true, values, (hipStream_t)stream);
  GLS_CATCH
}

} // extern "C"
