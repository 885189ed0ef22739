// coarse.hip — the multigrid's coarse-level solvers built from the coarse
// matrix, behind gls::CoarseSolver (coarse.h): the dense direct solver
// (free-block assembly, static condensation, LU, inverse, FP32 copy, GEMV),
// its nested-dissection form, the ILU and AMG coarse preconditioners and the
// coarse GMRES.  The substitute for the reference's Trilinos direct solver,
// ILU and AMG (multigrid.cc:372-530).
#include "coarse.h"
#include "common.h"
#include "kernels.h"
#include "op_internal.h"
#include "arnoldi.h"
#include "coarse_nd_solver.h"
#include "trace.h"

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace gls;

namespace
{
// a device allocation of the coarse solver.  Every buffer the solver keeps is
// one of these, so each is freed exactly once: by reset(), by the assignment
// that replaces it, or by the destructor
template <typename T>
struct DevBuf
{
  T *ptr = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)) {}
  DevBuf &
  operator=(DevBuf &&o) noexcept
  {
    std::swap(ptr, o.ptr);
    return *this;
  }
  ~DevBuf() { reset(); }
  void
  alloc(size_t count)
  {
    reset();
    HIP_THROW(hipMalloc((void **)&ptr, count * sizeof(T)));
  }
  void
  reset()
  {
    if (ptr)
      (void)hipFree(ptr);
    ptr = nullptr;
  }
  operator T *() const { return ptr; }
};

struct NdDelete
{
  void operator()(gls::NdSolver *nd) const { gls::nd_solver_destroy(nd); }
};

// a failed call of another part of the library (ILU, AMG, system matrix):
// its message under the coarse solver's prefix
void
check_status(glsStatus st, const char *prefix)
{
  if (st != 0)
    throw std::runtime_error(std::string(prefix) + gls_last_error());
}

// X = the unit lower triangle of the LU factors (column major n x n):
// strictly lower entries copied, 1 on the diagonal, 0 above
__global__ void
k_unit_lower(double *__restrict__ X, const double *__restrict__ LU, int64_t n)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n * n)
    return;
  const int64_t c = k / n, r = k - c * n;
  X[k]            = r > c ? LU[k] : (r == c ? 1.0 : 0.0);
}

// X[i][i] = 1 (column major n x n, X zeroed)
__global__ void
k_set_diag(double *X, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    X[(size_t)i * n + i] = 1.0;
}

template <typename T>
__global__ void
k_set_unit(T *x, int64_t j, int64_t n, int on)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && i == j)
    x[i] = on ? T(1) : T(0);
}

// y = M x for the dense coarse inverse (column major, n x n, FP64 or FP32
// storage, FP64 sums): the rows split over threads (coalesced column reads)
// and the columns over blockIdx.y chunks, partial sums reduced in a fixed
// order by k_gemv_sum; with ~64 chunks the launch has enough waves to stream
// the matrix at HBM rate (rocBLAS dgemv: 0.86 ms for the 2.2 GB inverse at
// n = 16,704)
constexpr int GEMV_CHUNKS = 64;
template <typename TM>
__global__ void __launch_bounds__(256)
  k_gemv_part(const TM *__restrict__ M, const double *__restrict__ x,
              double *__restrict__ part, int64_t n, int64_t ld)
{
  const int64_t i  = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t cw = (n + GEMV_CHUNKS - 1) / GEMV_CHUNKS;
  const int64_t j0 = blockIdx.y * cw, j1 = j0 + cw < n ? j0 + cw : n;
  if (i >= n)
    return;
  double  s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int64_t j  = j0;
  for (; j + 4 <= j1; j += 4)
    {
      s0 += (double)M[j * n + i] * x[j];
      s1 += (double)M[(j + 1) * n + i] * x[j + 1];
      s2 += (double)M[(j + 2) * n + i] * x[j + 2];
      s3 += (double)M[(j + 3) * n + i] * x[j + 3];
    }
  for (; j < j1; ++j)
    s0 += (double)M[j * n + i] * x[j];
  part[blockIdx.y * ld + i] = (s0 + s1) + (s2 + s3);
}

// The FP32-stored inverse, row major (row stride ld, a multiple of 4,
// padded columns zero): one wavefront per row streams the row as 16-byte
// loads (contiguous), x (FP32, the coarse defect's free entries: exact for
// FP32 levels) from L2, FP64 sums in a fixed order (lane partials, then a
// fixed shuffle tree), and writes y[free[row]] itself: no partial-sum pass.
typedef float gemv_f4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4
gemv_row_load(const float4 *p)
{
  if constexpr (NT)
    {
      const gemv_f4 t = __builtin_nontemporal_load(reinterpret_cast<const gemv_f4 *>(p));
      return make_float4(t.x, t.y, t.z, t.w);
    }
  else
    return *p;
}

template <typename T, bool NT>
__global__ void __launch_bounds__(256)
  k_gemv_rows_f32(const float4 *__restrict__ M, const float4 *__restrict__ x,
                  T *__restrict__ y, const int32_t *__restrict__ free, int64_t n, int64_t ld)
{
  const int64_t row  = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int     lane = threadIdx.x & 63;
  if (row >= n)
    return;
  const int64_t l4 = ld / 4;
  const float4 *mr = M + row * l4;
  double        a0 = 0, a1 = 0;
  int64_t       c  = lane;
  // four 16-byte row loads in flight per lane
  for (; c + 192 < l4; c += 256)
    {
      float4 m[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        m[u] = gemv_row_load<NT>(mr + c + 64 * u);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        xv[u] = x[c + 64 * u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        {
          a0 += (double)m[u].x * (double)xv[u].x + (double)m[u].y * (double)xv[u].y;
          a1 += (double)m[u].z * (double)xv[u].z + (double)m[u].w * (double)xv[u].w;
        }
    }
  for (; c < l4; c += 64)
    {
      const float4 m0 = gemv_row_load<NT>(mr + c), x0 = x[c];
      a0 += (double)m0.x * (double)x0.x + (double)m0.y * (double)x0.y;
      a1 += (double)m0.z * (double)x0.z + (double)m0.w * (double)x0.w;
    }
  double v = a0 + a1;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off);
  if (lane == 0)
    y[free[row]] = (T)v;
}

// coarse solve prologue for the row GEMV: sol = def on every dof (the
// constrained rows keep it), xf[i] = def[free[i]] in FP32 (padded to ld)
template <typename T>
__global__ void
k_coarse_prep(T *__restrict__ sol, const T *__restrict__ def, float *__restrict__ xf,
              const int32_t *__restrict__ free, int64_t n, int64_t nf, int64_t ld)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    sol[i] = def[i];
  if (i < ld)
    xf[i] = i < nf ? (float)def[free[i]] : 0.0f;
}

// y[free[i]] = sum of the chunk partials (leading dimension ld, fixed
// order), converted to the level precision
template <typename T>
__global__ void
k_gemv_sum(const double *__restrict__ part, T *__restrict__ y, const int32_t *__restrict__ free,
           int64_t n, int64_t ld)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  // eight independent partial loads per step, summed in a fixed order
  double s = 0;
  for (int c = 0; c < GEMV_CHUNKS; c += 8)
    {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = part[(c + u) * ld + i];
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
  y[free[i]] = (T)s;
}

// out[i] = in[free[i]] (FP64): the free rows of an assembled column, or the
// free entries of the coarse right-hand side
template <typename T>
__global__ void
k_gather_free(double *__restrict__ out, const T *__restrict__ in, const int32_t *__restrict__ free,
              int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = (double)in[free[i]];
}

// out = in^T rounded to FP32, row major with row stride ld >= n (padded
// columns zero): in is the n x n column-major inverse, so out's row i is
// in's row i (setup only; the strided reads do not matter)
__global__ void
k_narrow(float *__restrict__ out, const double *__restrict__ in, int64_t n, int64_t ld)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * ld)
    return;
  const int64_t i = e / ld, j = e - i * ld; // row i, column j
  out[e] = j < n ? (float)in[j * n + i] : 0.0f;
}

// Static condensation of the cells' interior dofs, one workgroup per cell:
// from the element matrix E (column major per cell: E[c][j][i] = entry
// (i, j)) with interior local dofs lint[ni] and boundary local dofs
// lbnd[nb] (free[b] = 0: a constrained boundary dof, its couplings dropped
// as the assembly drops them), C = E_II^-1 (Gauss-Jordan with partial
// pivoting, FP64), F = E_BI C, G = C E_IB, and the element Schur complement
// S = E_BB - F E_IB (column major [c][b2][b1]), assembled like E.
constexpr int COND_MAXI = 32;
// cells per leaf of the nested-dissection tree where the caller gives none
// (the fastest V-cycle of the leaf-size sweep at Re3900 r0)
constexpr int ND_DEFAULT_LEAF_CELLS = 50;
template <typename T>
__global__ void __launch_bounds__(256)
  k_condense(const T *__restrict__ E, int ndof, const int32_t *__restrict__ lint, int ni,
             const int32_t *__restrict__ lbnd, int nb, const int32_t *__restrict__ bfree,
             double *__restrict__ S, double *__restrict__ Cm, double *__restrict__ F,
             double *__restrict__ G, int32_t *__restrict__ bad)
{
  __shared__ double a[COND_MAXI][2 * COND_MAXI];
  __shared__ double f[128 * COND_MAXI / 4]; // F rows of this cell (nb <= 128, ni <= 8)
  const int64_t c   = blockIdx.x;
  const size_t  per = (size_t)ndof * ndof;
  const T      *Ec  = E + (size_t)c * per;
  auto          e   = [&](int row, int col) { return (double)Ec[(size_t)col * ndof + row]; };
  const int     t   = threadIdx.x;
  const int32_t *fr = bfree + (size_t)c * nb;
  // [E_II | I] in LDS, then Gauss-Jordan by one thread (ni <= COND_MAXI)
  for (int k = t; k < ni * 2 * ni; k += blockDim.x)
    {
      const int r = k / (2 * ni), q = k % (2 * ni);
      a[r][q] = q < ni ? e(lint[r], lint[q]) : (q - ni == r ? 1.0 : 0.0);
    }
  __syncthreads();
  if (t == 0)
    {
      // a pivot below 1e-12 of E_II's largest entry (or a non-finite one)
      // marks the cell: the host then assembles without condensation, where
      // getrf's info check covers a singular coarse matrix
      double scale = 0;
      for (int r = 0; r < ni; ++r)
        for (int q = 0; q < ni; ++q)
          scale = fmax(scale, fabs(a[r][q]));
      bool sing = !(scale > 0) || !isfinite(scale);
      for (int col = 0; col < ni && !sing; ++col)
        {
          int piv = col;
          for (int r = col + 1; r < ni; ++r)
            if (fabs(a[r][col]) > fabs(a[piv][col]))
              piv = r;
          if (!(fabs(a[piv][col]) > 1e-12 * scale))
            {
              sing = true;
              break;
            }
          if (piv != col)
            for (int q = 0; q < 2 * ni; ++q)
              {
                const double x = a[col][q];
                a[col][q]      = a[piv][q];
                a[piv][q]      = x;
              }
          const double d = 1.0 / a[col][col];
          for (int q = 0; q < 2 * ni; ++q)
            a[col][q] *= d;
          for (int r = 0; r < ni; ++r)
            if (r != col)
              {
                const double m = a[r][col];
                for (int q = 0; q < 2 * ni; ++q)
                  a[r][q] -= m * a[col][q];
              }
        }
      if (sing)
        bad[c] = 1;
    }
  __syncthreads();
  double *Cc = Cm + (size_t)c * ni * ni, *Fc = F + (size_t)c * nb * ni, *Gc = G + (size_t)c * ni * nb;
  for (int k = t; k < ni * ni; k += blockDim.x)
    Cc[k] = a[k / ni][ni + k % ni];
  // F[b][k] = sum_m E_BI(b, m) C(m, k); G[k][b] = sum_m C(k, m) E_IB(m, b)
  for (int k = t; k < nb * ni; k += blockDim.x)
    {
      const int b = k / ni, kk = k % ni;
      double    sf = 0, sg = 0;
      if (fr[b])
        for (int m = 0; m < ni; ++m)
          {
            sf += e(lbnd[b], lint[m]) * a[m][ni + kk];
            sg += a[kk][ni + m] * e(lint[m], lbnd[b]);
          }
      Fc[(size_t)b * ni + kk] = sf;
      f[b * ni + kk]          = sf;
      Gc[(size_t)kk * nb + b] = sg;
    }
  __syncthreads();
  // S[b2][b1] = E_BB(b1, b2) - sum_k F[b1][k] E_IB(k, b2)
  double *Sc = S + (size_t)c * nb * nb;
  for (int k = t; k < nb * nb; k += blockDim.x)
    {
      const int b2 = k / nb, b1 = k % nb;
      double    v  = e(lbnd[b1], lbnd[b2]);
      if (fr[b2])
        for (int m = 0; m < ni; ++m)
          v -= f[b1 * ni + m] * e(lint[m], lbnd[b2]);
      Sc[k] = v;
    }
}

// sum over the 64 lanes of a wavefront (butterfly, every lane gets it)
__device__ __forceinline__ double
cond_wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
  return v;
}

// the condensed right-hand side of GEMV column i: b_S[rin[i]] = def[rin[i]]
// - sum over its (cell, slot) pairs of F[c][slot] . b_I[c] (F = E_BI C
// already holds C, so the cell's interior right-hand side enters as is).
// Eight lanes per column, one (cell, slot) pair each (a vertex of a hex mesh
// usually has at most 8 cells; more loop), summed by a butterfly; sol = def
// on every dof (the constrained rows keep it); out padded to ld with zeros
template <typename T, typename O>
__global__ void __launch_bounds__(256)
  k_cond_rhs(T *__restrict__ sol, const T *__restrict__ def, O *__restrict__ out,
             const int32_t *__restrict__ rin, const int32_t *__restrict__ off,
             const int32_t *__restrict__ ent, const double *__restrict__ F,
             const int32_t *__restrict__ cint, int ni, int nb, int64_t n, int64_t nr,
             int64_t ld)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n)
    sol[g] = def[g];
  const int64_t i  = g >> 3;
  const int     l8 = (int)(g & 7);
  double        v  = 0;
  if (i < nr)
    for (int32_t e = off[i] + l8; e < off[i + 1]; e += 8)
      {
        const int32_t  cs = ent[e]; // cell * nb + slot
        const int64_t  c  = cs / nb;
        const double  *f  = F + (size_t)cs * ni;
        const int32_t *ic = cint + (size_t)c * ni;
        for (int m = 0; m < ni; ++m)
          v += f[m] * (double)def[ic[m]];
      }
#pragma unroll
  for (int o = 4; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
  if (l8 != 0 || i >= ld)
    return;
  out[i] = i < nr ? (O)((double)def[rin[i]] - v) : O(0);
}

// the interior dofs from the boundary solution: x_I = C b_I - G x_B, one
// wavefront per (cell, interior dof k): the lanes stride G's row (nb
// entries) and the first ni lanes add C's row times b_I
template <typename T>
__global__ void __launch_bounds__(256)
  k_cond_post(T *__restrict__ sol, const T *__restrict__ def, const double *__restrict__ Cm,
              const double *__restrict__ G, const int32_t *__restrict__ cint,
              const int32_t *__restrict__ cbnd, int ni, int nb, int64_t n_cells)
{
  const int64_t row  = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int     lane = threadIdx.x & 63;
  if (row >= n_cells * ni)
    return;
  const int64_t  c  = row / ni;
  const double  *gr = G + (size_t)row * nb;
  const int32_t *cb = cbnd + (size_t)c * nb;
  double         v  = 0;
  for (int b = lane; b < nb; b += 64)
    {
      const int32_t d = cb[b];
      if (d >= 0)
        v -= gr[b] * (double)sol[d];
    }
  if (lane < ni)
    v += Cm[(size_t)row * ni + lane] * (double)def[cint[(size_t)c * ni + lane]];
  v = cond_wave_sum(v);
  if (lane == 0)
    sol[cint[row]] = (T)v;
}

// A_ff[fj][fi] += E[c][j][i] over the cells of one colour (no two of them
// share a node, so no two threads of a launch touch the same entry): the
// element matrices scattered into the column-major free-dof block, the
// colours in a fixed order (deterministic sums)
template <typename T>
__global__ void
k_scatter_emat(double *__restrict__ A, int64_t nf, const T *__restrict__ E,
               const int32_t *__restrict__ cdof, const int32_t *__restrict__ cells,
               int64_t n_cells, int ndof)
{
  const int64_t per = (int64_t)ndof * ndof;
  const int64_t g   = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_cells * per)
    return;
  const int64_t ci = g / per;
  const int     r  = (int)(g - ci * per);
  const int     j = r / ndof, i = r - j * ndof;
  const int64_t c  = cells[ci];
  const int32_t fi = cdof[c * ndof + i], fj = cdof[c * ndof + j];
  if (fi < 0 || fj < 0)
    return;
  A[(size_t)fj * nf + fi] += (double)E[(size_t)c * per + r];
}

// GLS_COARSE_REFERENCE: a comma-separated list of reference forms of the
// dense coarse solver for tests -- "columns" (A_ff assembled column by
// column from unit-vector vmults instead of the element matrices), "getrs"
// / "getri" (the inverse by getrs with the identity / by getri instead of
// U^-1 L^-1), "nocond" (no static condensation)
bool
coarse_reference(const char *what)
{
  const char *e = getenv("GLS_COARSE_REFERENCE");
  if (!e)
    return false;
  const std::string list = std::string(",") + e + ",";
  return list.find(std::string(",") + what + ",") != std::string::npos;
}

// which form of the direct solver: nested dissection or the dense inverse,
// the cells' interior dofs condensed or not, the stored inverse FP32 or FP64
struct DirectForm
{
  bool nd = false, cond = false, f32 = false;
};

// the direct solver's device state, all of it (every form's): "start over"
// is the assignment of a fresh one
struct DirectState
{
  // dense LU (the substitute for the reference's Trilinos direct solver,
  // multigrid.cc:448-455, 477-481)
  DevBuf<double>      lu; // [nf][nf] column major: LU factors, then the inverse
  DevBuf<rocblas_int> ipiv, info;
  DevBuf<double>      rhs;  // [(2 + GEMV_CHUNKS) nf]: rhs | solution | partials
  DevBuf<int32_t>     free; // [nf] the free (unconstrained) coarse dofs
  // [nf] the GEMV's input gather: the free dof whose entry multiplies column
  // i of the stored inverse (free[p[i]] for the unpermuted U^-1 L^-1 of the
  // trtri path, A^-1 = U^-1 L^-1 P^T; free[i] otherwise)
  DevBuf<int32_t> free_in;
  int64_t         n_free = 0, ld_free = 0; // ld_free: nf rounded up to 4
  // static condensation of the cells' interior dofs (direct_setup): the dense
  // inverse covers the remaining free dofs only; per cell C = E_II^-1
  // [ni][ni], F = E_BI E_II^-1 [nb][ni], G = E_II^-1 E_IB [ni][nb]
  // (constrained boundary dofs: zero rows / columns), the interior / boundary
  // dofs' global indices (-1: constrained), and per GEMV column i the (cell,
  // boundary slot) pairs of its dof (CSR)
  DevBuf<double>  cC, cF, cG;
  DevBuf<int32_t> cint, cbnd, rg_off, rg_ent;
  DevBuf<float>   inv32; // [nf][ld_free] FP32 copy of the inverse
  // the nested-dissection form (coarse_nd.hip): it replaces the dense block,
  // its inverse and the GEMV between the condensed right-hand side and the
  // interior back-substitution
  std::unique_ptr<gls::NdSolver, NdDelete> nd;
};

// the kind of coarse solver, from the descriptor and gls_mg_set_coarse_ilu:
// the one place that reads them for it
CoarseKind
coarse_kind(const glsMGDesc &desc, bool ilu_set)
{
  if (ilu_set)
    return CoarseKind::ilu;
  if (desc.coarse_amg)
    return CoarseKind::amg;
  if (desc.coarse_n_iterations < 0)
    return CoarseKind::direct;
  return desc.coarse_n_iterations == 0 ? CoarseKind::identity : CoarseKind::relaxation;
}

struct CoarseImpl final : CoarseSolver
{
  glsMGDesc  desc{};
  glsOp      op          = nullptr;
  int        prec        = GLS_F32;
  bool       partitioned = false;
  bool       setup_done  = false;
  CoarseKind kind_       = CoarseKind::identity;

  // direct: the form asked for (gls_mg_set_coarse_direct), the live one, and
  // what a fallback took away for good (cond: a cell's E_II was numerically
  // singular; nd: a pivot block was singular, the dense solver took over)
  int         method = GLS_COARSE_DENSE, nd_leaf_cells = 0;
  DirectForm  form, lost;
  DirectState dir;
  int         cond_ni = 0, cond_nb = 0;
  std::vector<int32_t> cond_lint, cond_lbnd; // local interior / boundary dofs of a cell
  // last dense setup: assembly / getrf / inverse wall ms, cell colours
  double setup_ms[3] = {0, 0, 0};
  int    colors      = 0;
  double nd_plan_ms  = 0;
  // the one rocBLAS handle (direct solvers, coarse GMRES)
  rocblas_handle blas = nullptr;
  // coarse GMRES: FP64 Krylov workspace, two level-precision operand
  // buffers, statistics of the last solve
  DevBuf<double> cg_ws;
  DevBuf<char>   cg_lvl;
  double        *cg_host  = nullptr; // pinned: two Hessenberg columns (software pipeline)
  hipEvent_t     cg_ev[2] = {nullptr, nullptr};
  int            cg_iters = 0, cg_conv = 0;
  // "gmg coarse grid solver": "AMG": the smoothed-aggregation AMG on the
  // coarse level's system matrix (amg.hip), rebuilt by every setup
  // (PreconditionerGMG::initialize, multigrid.cc:372-433); its ILU form
  // (gls_mg_set_coarse_amg_ilu; smoother / coarsest ILU(k))
  glsAMG          amg_h        = nullptr;
  double          amg_setup_ms = 0;
  bool            amg_ilu      = false;
  glsAMGIluParams amg_ilu_prm{};
  // "gmg coarse grid solver": "ILU" (multigrid.cc:434-447): ILU(k) of the
  // coarse level's system matrix; created by the first setup, refactored on
  // the same pattern by the later ones
  bool         ilu_device = false; // gls_mg_set_coarse_ilu_device
  glsILUParams ilu_prm{};
  glsILU       ilu_h        = nullptr;
  double       ilu_setup_ms = 0;
  DevBuf<double> io64; // [2 n] FP64 in / out of an ILU / AMG solve of FP32 levels

  ~CoarseImpl() override
  {
    if (cg_host)
      (void)hipHostFree(cg_host);
    for (hipEvent_t ev : cg_ev)
      if (ev)
        (void)hipEventDestroy(ev);
    if (blas)
      rocblas_destroy_handle(blas);
    if (amg_h)
      gls_amg_destroy(amg_h);
    gls_ilu_destroy(ilu_h);
  }

  // the handle, created on first use, on stream s
  rocblas_handle
  blas_on(hipStream_t s)
  {
    if (!blas)
      check_blas(rocblas_create_handle(&blas), "rocblas_create_handle");
    check_blas(rocblas_set_stream(blas, s), "rocblas_set_stream");
    return blas;
  }

// A_ff from the element matrices of the coarse level operator (what the
// reference's coarse direct solver factorises: get_system_matrix ->
// MatrixFreeTools::compute_matrix, operator_ns.cc:1407-1430, assembled into
// the Trilinos matrix, multigrid.cc:448-455): one element-matrix launch over
// all coarse cells, then one scatter launch per cell colour (greedy colouring
// on the host, cells of a colour share no node), summed in FP64
// With `fronts` the cell blocks go to that function (the nested-dissection
// solver's fronts) instead of the dense block.
using CellBlockSink = std::function<void(gls::NdCellBlocks &)>;
template <typename T>
bool
assemble_free_block(const std::vector<int32_t> &freel, hipStream_t s,
                    const CellBlockSink &fronts = nullptr)
{
  bool ok = true; // false: a condensed cell's interior block is singular
  const int64_t n   = op->n_dofs, nf = (int64_t)freel.size(), nc_ = op->n_cells;
  const int     nc   = op->dim + 1, nq = op->nq, ndof = nq * nc;
  std::vector<int32_t> fidx((size_t)n, -1);
  for (int64_t j = 0; j < nf; ++j)
    fidx[(size_t)freel[(size_t)j]] = (int32_t)j;
  // internal cell c -> free index of each local dof (-1: constrained)
  std::vector<int32_t> cdof((size_t)nc_ * ndof);
  std::vector<std::vector<int32_t>> node_cells((size_t)op->n_nodes);
  for (int64_t c = 0; c < nc_; ++c)
    {
      const uint32_t *cn = &op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * nq];
      for (int p = 0; p < nq; ++p)
        {
          node_cells[cn[p]].push_back((int32_t)c);
          for (int k = 0; k < nc; ++k)
            cdof[(size_t)c * ndof + p * nc + k] = fidx[(size_t)cn[p] * nc + k];
        }
    }
  // greedy colouring: the smallest colour no node-sharing neighbour has
  std::vector<int> color((size_t)nc_, -1);
  int              n_colors = 0;
  std::vector<int> seen;
  for (int64_t c = 0; c < nc_; ++c)
    {
      seen.assign((size_t)n_colors + 1, 0);
      const uint32_t *cn = &op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * nq];
      for (int p = 0; p < nq; ++p)
        for (int32_t o : node_cells[cn[p]])
          if (color[(size_t)o] >= 0)
            seen[(size_t)color[(size_t)o]] = 1;
      int k = 0;
      while (seen[(size_t)k])
        ++k;
      color[(size_t)c] = k;
      n_colors         = std::max(n_colors, k + 1);
    }
  std::vector<int32_t> order;
  std::vector<int64_t> cbeg(1, 0);
  for (int k = 0; k < n_colors; ++k)
    {
      for (int64_t c = 0; c < nc_; ++c)
        if (color[(size_t)c] == k)
          order.push_back((int32_t)c);
      cbeg.push_back((int64_t)order.size());
    }
  const size_t eb = (size_t)nc_ * ndof * ndof * sizeof(T);
  void        *E = nullptr, *d_cdof = nullptr, *d_order = nullptr;
  HIP_THROW(hipMallocAsync(&E, eb, s));
  HIP_THROW(hipMallocAsync(&d_cdof, cdof.size() * sizeof(int32_t), s));
  HIP_THROW(hipMallocAsync(&d_order, order.size() * sizeof(int32_t), s));
  HIP_THROW(hipMemcpyAsync(d_cdof, cdof.data(), cdof.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
  HIP_THROW(hipMemcpyAsync(d_order, order.data(), order.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
  gls::op_element_matrices_device(op, E, 0, nc_, s);
  gls::NdCellBlocks cb{};
  cb.cell_caller   = op->cell_perm.empty() ? nullptr : op->cell_perm.data();
  cb.d_color_cells = (const int32_t *)d_order;
  cb.color_begin   = cbeg.data();
  cb.n_colors      = n_colors;
  if (!fronts)
    HIP_THROW(hipMemsetAsync(dir.lu, 0, (size_t)nf * nf * sizeof(double), s));
  if (!form.cond && fronts)
    {
      cb.blocks = E, cb.f64 = std::is_same<T, double>::value, cb.nloc = ndof;
      cb.cell_dof = cdof.data();
      fronts(cb);
    }
  else if (!form.cond)
    {
      const int64_t per = (int64_t)ndof * ndof;
      for (int k = 0; k < n_colors; ++k)
        {
          const int64_t cnt = cbeg[(size_t)k + 1] - cbeg[(size_t)k];
          hipLaunchKernelGGL(k_scatter_emat<T>, g1(cnt * per), dim3(256), 0, s, dir.lu, nf,
                             (const T *)E, (const int32_t *)d_cdof,
                             (const int32_t *)d_order + cbeg[(size_t)k], cnt, ndof);
        }
      HIP_THROW(hipGetLastError());
    }
  else
    {
      // element Schur complements over the boundary dofs (k_condense), then
      // assembled like the element matrices
      const int ni = cond_ni, nb = cond_nb;
      std::vector<int32_t> cdb((size_t)nc_ * nb), bfree((size_t)nc_ * nb), cint((size_t)nc_ * ni),
        cbnd((size_t)nc_ * nb);
      for (int64_t c = 0; c < nc_; ++c)
        {
          const uint32_t *cn = &op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * nq];
          for (int b = 0; b < nb; ++b)
            {
              const int     l = cond_lbnd[(size_t)b];
              const int32_t f = cdof[(size_t)c * ndof + l];
              cdb[(size_t)c * nb + b]   = f;
              bfree[(size_t)c * nb + b] = f >= 0 ? 1 : 0;
              cbnd[(size_t)c * nb + b]  = f >= 0 ? (int32_t)(cn[l / nc] * nc + l % nc) : -1;
            }
          for (int m = 0; m < ni; ++m)
            {
              const int l = cond_lint[(size_t)m];
              cint[(size_t)c * ni + m] = (int32_t)(cn[l / nc] * nc + l % nc);
            }
        }
      if (!dir.cC)
        {
          dir.cC.alloc((size_t)nc_ * ni * ni);
          dir.cF.alloc((size_t)nc_ * nb * ni);
          dir.cG.alloc((size_t)nc_ * ni * nb);
          dir.cint.alloc((size_t)nc_ * ni);
          dir.cbnd.alloc((size_t)nc_ * nb);
        }
      HIP_THROW(hipMemcpyAsync(dir.cint, cint.data(), cint.size() * 4, hipMemcpyHostToDevice, s));
      HIP_THROW(hipMemcpyAsync(dir.cbnd, cbnd.data(), cbnd.size() * 4, hipMemcpyHostToDevice, s));
      void *Sd = nullptr, *d_lint = nullptr, *d_lbnd = nullptr, *d_bfree = nullptr, *d_cdb = nullptr;
      HIP_THROW(hipMallocAsync(&Sd, (size_t)nc_ * nb * nb * 8, s));
      HIP_THROW(hipMallocAsync(&d_lint, (size_t)ni * 4, s));
      HIP_THROW(hipMallocAsync(&d_lbnd, (size_t)nb * 4, s));
      HIP_THROW(hipMallocAsync(&d_bfree, bfree.size() * 4, s));
      HIP_THROW(hipMallocAsync(&d_cdb, cdb.size() * 4, s));
      HIP_THROW(hipMemcpyAsync(d_lint, cond_lint.data(), (size_t)ni * 4, hipMemcpyHostToDevice, s));
      HIP_THROW(hipMemcpyAsync(d_lbnd, cond_lbnd.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
      HIP_THROW(hipMemcpyAsync(d_bfree, bfree.data(), bfree.size() * 4, hipMemcpyHostToDevice, s));
      HIP_THROW(hipMemcpyAsync(d_cdb, cdb.data(), cdb.size() * 4, hipMemcpyHostToDevice, s));
      int32_t *d_bad = nullptr;
      HIP_THROW(hipMallocAsync((void **)&d_bad, (size_t)nc_ * 4, s));
      HIP_THROW(hipMemsetAsync(d_bad, 0, (size_t)nc_ * 4, s));
      hipLaunchKernelGGL(k_condense<T>, dim3((unsigned)nc_), dim3(256), 0, s, (const T *)E, ndof,
                         (const int32_t *)d_lint, ni, (const int32_t *)d_lbnd, nb,
                         (const int32_t *)d_bfree, (double *)Sd, dir.cC, dir.cF, dir.cG,
                         d_bad);
      std::vector<int32_t> hbad((size_t)nc_);
      HIP_THROW(hipMemcpyAsync(hbad.data(), d_bad, (size_t)nc_ * 4, hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      HIP_THROW(hipFreeAsync(d_bad, s));
      for (int32_t b : hbad)
        ok = ok && b == 0;
      const int64_t per = (int64_t)nb * nb;
      if (fronts && ok)
        {
          cb.blocks = Sd, cb.f64 = true, cb.nloc = nb, cb.cell_dof = cdb.data();
          fronts(cb);
        }
      for (int k = 0; k < n_colors && !fronts; ++k)
        {
          const int64_t cnt = cbeg[(size_t)k + 1] - cbeg[(size_t)k];
          hipLaunchKernelGGL(k_scatter_emat<double>, g1(cnt * per), dim3(256), 0, s, dir.lu, nf,
                             (const double *)Sd, (const int32_t *)d_cdb,
                             (const int32_t *)d_order + cbeg[(size_t)k], cnt, nb);
        }
      HIP_THROW(hipGetLastError());
      for (void *q : {Sd, d_lint, d_lbnd, d_bfree, d_cdb})
        HIP_THROW(hipFreeAsync(q, s));
    }
  HIP_THROW(hipFreeAsync(E, s));
  HIP_THROW(hipFreeAsync(d_cdof, s));
  HIP_THROW(hipFreeAsync(d_order, s));
  colors = n_colors;
  // (the synchronised setup of the caller waits for these launches)
  return ok;
}

// Assemble the coarse level operator into FP64 and LU-factorise it.  Only
// the free (unconstrained) dofs take part: a constrained dof's row and
// column of A are both the unit vector (identity rows of vmult, homogeneous
// constraints read as 0), so A = diag(A_ff, I) in free / constrained order
// and the direct solve is x_c = b_c, x_f = A_ff^{-1} b_f — the same solution
// as the full matrix, on nf^2 instead of n^2 entries (Re3900 r0: 14,206 of
// 16,704 dofs free, 1.61 instead of 2.23 GB).
template <typename T>
void
direct_setup(void *sol, void *tmp, hipStream_t s)
{
  const int64_t n  = op->n_dofs;
  const int     nc = op->dim + 1;
  // the form is decided here (nd; cond and f32 below) from what was asked
  // for, the test references and what a fallback lost
  // (the nested-dissection solver checks the free device memory instead)
  const bool nd = method == GLS_COARSE_ND && !lost.nd && !coarse_reference("columns");
  if (nd && !op->h_master.empty())
    throw std::runtime_error("the \"nd\" coarse solver does not take a coarse level with a "
                             "periodic node map (node_master); use the dense direct solver");
  if (n > 40000 && !nd)
    throw std::runtime_error("dense LU coarse solver: coarse level too large");
  std::vector<int32_t> freel;
  freel.reserve((size_t)n);
  for (int64_t d = 0; d < n; ++d)
    if (!((op->h_cmask[(size_t)(d / nc)] >> (d % nc)) & 1))
      freel.push_back((int32_t)d);
  // static condensation of the cells' interior dofs (default with the
  // element-matrix assembly; GLS_COARSE_REFERENCE=nocond off): a node with every
  // lattice coordinate inside (0, k) belongs to one cell only, so its dofs
  // are eliminated cell by cell (Schur complement of the element matrix) and
  // the dense inverse covers the other free dofs (Re3900 r0: 12,606 of
  // 14,206, 0.70x the factorisation flops, 0.79x the GEMV's bytes); the
  // coarse solve adds the condensed right-hand side b_B - F b_I before the
  // GEMV and x_I = C b_I - G x_B after it (k_cond_rhs / k_cond_post)
  const bool columns = coarse_reference("columns");
  {
    const int   k  = op->degree, dim = op->dim, nq = op->nq;
    cond_lint.clear(), cond_lbnd.clear();
    for (int p = 0; p < nq; ++p)
      {
        const int  co[3] = {p % (k + 1), (p / (k + 1)) % (k + 1), dim == 3 ? p / ((k + 1) * (k + 1)) : 1};
        const bool in    = co[0] > 0 && co[0] < k && co[1] > 0 && co[1] < k && co[2] > 0 && co[2] < k;
        for (int q = 0; q < nc; ++q)
          (in ? cond_lint : cond_lbnd).push_back(p * nc + q);
      }
    const int ni = (int)cond_lint.size(), nb = (int)cond_lbnd.size();
    bool      cond = !columns && !coarse_reference("nocond") && !lost.cond && ni > 0 && ni <= COND_MAXI &&
                nb <= 128 && nb * ni <= 1024;
    std::vector<char> is_int((size_t)n, 0);
    for (int64_t c = 0; cond && c < op->n_cells; ++c)
      {
        const uint32_t *cn = &op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * nq];
        for (int m = 0; m < ni && cond; ++m)
          {
            const int     l = cond_lint[(size_t)m];
            const int64_t d = (int64_t)cn[l / nc] * nc + l % nc;
            // every interior dof free and in this cell alone
            if (((op->h_cmask[(size_t)cn[l / nc]] >> (l % nc)) & 1) || is_int[(size_t)d])
              cond = false;
            is_int[(size_t)d] = 1;
          }
      }
    form.cond = cond, cond_ni = ni, cond_nb = nb;
    if (cond)
      {
        std::vector<int32_t> rl;
        rl.reserve(freel.size());
        for (int32_t d : freel)
          if (!is_int[(size_t)d])
            rl.push_back(d);
        freel.swap(rl);
      }
  }
  const int64_t nf = (int64_t)freel.size();
  if (nf == 0)
    throw std::runtime_error("dense LU coarse solver: no free coarse dofs");
  blas_on(s);
  if (dir.free && dir.n_free != nf)
    throw std::runtime_error("dense LU coarse solver: constrained dofs changed");
  if (!dir.free)
    {
      dir.info.alloc(1);
      dir.ld_free = (nf + 3) / 4 * 4;
      dir.rhs.alloc((size_t)(2 + GEMV_CHUNKS) * dir.ld_free);
      dir.free.alloc((size_t)nf);
      dir.free_in.alloc((size_t)nf);
      dir.n_free = nf;
    }
  if (dir.n_free != nf)
    throw std::runtime_error("dense LU coarse solver: constrained dofs changed");
  HIP_THROW(hipMemcpyAsync(dir.free, freel.data(), (size_t)nf * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
  // a cell's interior block E_II is singular: start over without the
  // static condensation (the free-dof buffers are sized for nf, the
  // nested-dissection plan for the condensed dofs): the direct solver's
  // whole device state goes, the form with it
  auto restart_without_condensation = [&]() {
    HIP_THROW(hipStreamSynchronize(s));
    dir       = DirectState{};
    form      = DirectForm{};
    lost.cond = true;
    fprintf(stderr, "[glsamd] coarse solver: singular interior block in a coarse cell, "
                    "assembling without static condensation\n");
  };
  // per GEMV column i: the (cell, boundary slot) pairs of dof fin[i]
  // (k_cond_rhs)
  auto cond_tables = [&](const std::vector<int32_t> &fin) {
    const int     nb = cond_nb, nq = op->nq;
    std::vector<std::vector<int32_t>> at((size_t)n);
    for (int64_t c = 0; c < op->n_cells; ++c)
      {
        const uint32_t *cn = &op->h_cell_nodes[(size_t)gls::ext_cell(op, c) * nq];
        for (int b = 0; b < nb; ++b)
          {
            const int     l = cond_lbnd[(size_t)b];
            const int64_t d = (int64_t)cn[l / nc] * nc + l % nc;
            if (!((op->h_cmask[(size_t)cn[l / nc]] >> (l % nc)) & 1))
              at[(size_t)d].push_back((int32_t)(c * nb + b));
          }
      }
    std::vector<int32_t> off(1, 0), ent;
    for (int64_t i = 0; i < nf; ++i)
      {
        for (int32_t e : at[(size_t)fin[(size_t)i]])
          ent.push_back(e);
        off.push_back((int32_t)ent.size());
      }
    if (dir.rg_off) // the last setup's tables: no solve still reads them
      HIP_THROW(hipStreamSynchronize(s));
    dir.rg_off.alloc(off.size());
    dir.rg_ent.alloc(std::max<size_t>(1, ent.size()));
    HIP_THROW(hipMemcpy(dir.rg_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (!ent.empty())
      HIP_THROW(hipMemcpy(dir.rg_ent, ent.data(), ent.size() * 4, hipMemcpyHostToDevice));
  };
  const char *e32 = getenv("GLS_COARSE_INV_F32");
  form.f32 = !(e32 && e32[0] == '0') && prec == GLS_F32;
  if (nd)
    {
      // the nested-dissection solver (coarse_nd.hip): the plan once per
      // multigrid object (the mesh and the constraints do not change), the
      // fronts from the same cell blocks as the dense block
      const auto w0  = std::chrono::steady_clock::now();
      nd_plan_ms = 0;
      if (!dir.nd)
        {
          std::vector<int32_t> node_dofs((size_t)op->n_nodes, 0);
          for (int32_t d : freel)
            ++node_dofs[(size_t)(d / nc)];
          dir.nd.reset(gls::nd_solver_create(gls::nd_make_plan(
            op->h_cell_nodes.data(), op->n_cells, op->nq, op->n_nodes, node_dofs.data(),
            nd_leaf_cells > 0 ? nd_leaf_cells : ND_DEFAULT_LEAF_CELLS)));
          nd_plan_ms = std::chrono::duration<double, std::milli>(
                             std::chrono::steady_clock::now() - w0)
                             .count();
        }
      form.nd       = true;
      bool factored = false;
      if (!assemble_free_block<T>(freel, s, [&](gls::NdCellBlocks &cb) {
            factored = gls::nd_solver_factor(dir.nd.get(), blas, cb, form.f32, s);
          }))
        {
          restart_without_condensation();
          return direct_setup<T>(sol, tmp, s);
        }
      if (factored)
        {
          HIP_THROW(hipMemcpyAsync(dir.free_in, freel.data(), (size_t)nf * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
          if (form.cond)
            cond_tables(freel);
          HIP_THROW(hipStreamSynchronize(s));
          return;
        }
      // pivoting is confined to the pivot blocks: a singular one hands the
      // coarse level to the dense solver for good
      HIP_THROW(hipStreamSynchronize(s));
      dir.nd.reset();
      lost.nd = true;
      fprintf(stderr, "[glsamd] coarse solver: singular pivot block in the nested-dissection "
                      "factorisation, falling back to the dense solver\n");
      if (n > 40000)
        throw std::runtime_error("dense LU coarse solver: coarse level too large");
    }
  form.nd = false;
  // the FP64 factors are released after an FP32 setup (k_narrow below)
  if (!dir.lu)
    dir.lu.alloc((size_t)nf * nf);
  if (!dir.ipiv)
    dir.ipiv.alloc((size_t)nf);
  const auto  t0 = std::chrono::steady_clock::now();
  if (columns)
    {
      // reference path of the assembly test: A_ff column by column from
      // unit-vector vmults (nf vmults of the level operator)
      T *e = (T *)sol, *col = (T *)tmp;
      HIP_THROW(hipMemsetAsync(e, 0, n * sizeof(T), s));
      for (int64_t j = 0; j < nf; ++j)
        {
          const int64_t dj = freel[(size_t)j];
          hipLaunchKernelGGL(k_set_unit<T>, g1(n), dim3(256), 0, s, e, dj, n, 1);
          gls::op_vmult_device(op, col, e, s);
          hipLaunchKernelGGL(k_gather_free<T>, g1(nf), dim3(256), 0, s,
                             dir.lu + (size_t)j * nf, (const T *)col,
                             (const int32_t *)dir.free, nf);
          hipLaunchKernelGGL(k_set_unit<T>, g1(n), dim3(256), 0, s, e, dj, n, 0);
        }
      HIP_THROW(hipGetLastError());
    }
  else if (!assemble_free_block<T>(freel, s))
    {
      restart_without_condensation();
      return direct_setup<T>(sol, tmp, s);
    }
  HIP_THROW(hipStreamSynchronize(s));
  const auto t1 = std::chrono::steady_clock::now();
  check_blas(rocsolver_dgetrf(blas, (rocblas_int)nf, (rocblas_int)nf, dir.lu,
                              (rocblas_int)nf, dir.ipiv, dir.info),
             "rocsolver_dgetrf");
  rocblas_int info = 0;
  HIP_THROW(hipMemcpyAsync(&info, dir.info, sizeof(info), hipMemcpyDeviceToHost, s));
  HIP_THROW(hipStreamSynchronize(s));
  const auto t2 = std::chrono::steady_clock::now();
  if (info != 0)
    throw std::runtime_error("dense LU coarse solver: singular coarse matrix (info " +
                             std::to_string(info) + ")");
  // the inverse from the LU factors, once: every coarse solve is then one
  // GEMV streaming the nf x nf matrix at HBM rate (the two triangular solves
  // of getrs ran 33.7 ms per V-cycle at n = 16,704 on MI355X).  Default
  // Z = U^-1 L^-1 from the unit lower
  // factor inverted in place (rocsolver_dtrtri, n^3 / 3 flops) and one
  // triangular solve with U (rocblas_dtrsm, n^3): 4/3 n^3 instead of the
  // 2 n^3 of getrs with the identity, and A^-1 = Z P^T needs no column
  // permutation of the matrix: the GEMV gathers its input through free[p[i]]
  // (d_free_in).  Reference forms (GLS_COARSE_REFERENCE): "getrs", the
  // identity as right-hand side (rocsolver dgetrs); "getri", rocsolver_dgetri
  // in place.
  std::vector<int32_t> fin = freel; // the GEMV's input gather
  const std::string inv_mode = coarse_reference("getri") ? "getri" :
                               coarse_reference("getrs") ? "getrs" : "trtri";
  if (inv_mode == "getri")
    {
      check_blas(rocsolver_dgetri(blas, (rocblas_int)nf, dir.lu, (rocblas_int)nf,
                                  dir.ipiv, dir.info),
                 "rocsolver_dgetri");
      HIP_THROW(hipMemcpyAsync(&info, dir.info, sizeof(info), hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      if (info != 0)
        throw std::runtime_error("dense LU coarse solver: singular coarse matrix in getri "
                                 "(info " + std::to_string(info) + ")");
    }
  else
    {
      const bool trtri = inv_mode != "getrs";
      DevBuf<double> X; // the inverse; a throw below releases it
      X.alloc((size_t)nf * nf);
        {
          if (trtri)
            {
              hipLaunchKernelGGL(k_unit_lower, g1(nf * nf), dim3(256), 0, s, X,
                                 (const double *)dir.lu, nf);
              HIP_THROW(hipGetLastError());
              check_blas(rocsolver_dtrtri(blas, rocblas_fill_lower, rocblas_diagonal_unit,
                                          (rocblas_int)nf, X, (rocblas_int)nf, dir.info),
                         "rocsolver_dtrtri");
              const double one = 1.0;
              check_blas(rocblas_set_pointer_mode(blas, rocblas_pointer_mode_host),
                         "pointer mode");
              check_blas(rocblas_dtrsm(blas, rocblas_side_left, rocblas_fill_upper,
                                       rocblas_operation_none, rocblas_diagonal_non_unit,
                                       (rocblas_int)nf, (rocblas_int)nf, &one, dir.lu,
                                       (rocblas_int)nf, X, (rocblas_int)nf),
                         "rocblas_dtrsm");
              // P^T from the pivots (1-based row interchanges, in order)
              std::vector<rocblas_int> ip((size_t)nf);
              HIP_THROW(hipMemcpyAsync(ip.data(), dir.ipiv, (size_t)nf * sizeof(rocblas_int),
                                       hipMemcpyDeviceToHost, s));
              HIP_THROW(hipMemcpyAsync(&info, dir.info, sizeof(info), hipMemcpyDeviceToHost, s));
              HIP_THROW(hipStreamSynchronize(s));
              if (info != 0)
                throw std::runtime_error("dense LU coarse solver: singular unit factor (info " +
                                         std::to_string(info) + ")");
              std::vector<int32_t> p((size_t)nf);
              for (int64_t i = 0; i < nf; ++i)
                p[(size_t)i] = (int32_t)i;
              for (int64_t j = 0; j < nf; ++j)
                std::swap(p[(size_t)j], p[(size_t)ip[(size_t)j] - 1]);
              for (int64_t i = 0; i < nf; ++i)
                fin[(size_t)i] = freel[(size_t)p[(size_t)i]];
            }
          else
            {
              HIP_THROW(hipMemsetAsync(X, 0, (size_t)nf * nf * sizeof(double), s));
              hipLaunchKernelGGL(k_set_diag, g1(nf), dim3(256), 0, s, X, nf);
              HIP_THROW(hipGetLastError());
              check_blas(rocsolver_dgetrs(blas, rocblas_operation_none, (rocblas_int)nf,
                                          (rocblas_int)nf, dir.lu, (rocblas_int)nf, dir.ipiv,
                                          X, (rocblas_int)nf),
                         "rocsolver_dgetrs");
            }
          HIP_THROW(hipStreamSynchronize(s));
        }
      dir.lu = std::move(X); // (the factors go with X)
    }
  HIP_THROW(hipMemcpyAsync(dir.free_in, fin.data(), (size_t)nf * sizeof(int32_t),
                           hipMemcpyHostToDevice, s));
  if (form.cond)
    cond_tables(fin);
  const auto t3 = std::chrono::steady_clock::now();
  auto       ms = [](auto a, auto b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  setup_ms[0] = ms(t0, t1);
  setup_ms[1] = ms(t1, t2);
  setup_ms[2] = ms(t2, t3);
  // FP32 levels keep an FP32 copy of the inverse (FP64 sums): half the bytes
  // per coarse solve; the Re3900 r0..r2 V-cycle differs from the FP64-stored
  // inverse's by 2.1e-7 (relative l2), the FP32 level arithmetic's own
  // round-off.  GLS_COARSE_INV_F32=0 keeps the FP64 inverse.
  if (form.f32)
    {
      const int64_t ld = dir.ld_free;
      if (!dir.inv32)
        dir.inv32.alloc((size_t)nf * ld);
      hipLaunchKernelGGL(k_narrow, g1(nf * ld), dim3(256), 0, s, dir.inv32,
                         (const double *)dir.lu, nf, ld);
      HIP_THROW(hipGetLastError());
      // the FP32 solve reads inv32 only: release the nf x nf FP64 factors
      // (1.6 GB at Re3900 r0) and the pivots; a re-setup allocates them again
      HIP_THROW(hipStreamSynchronize(s));
      dir.lu.reset();
      dir.ipiv.reset();
    }
}

// the condensed coarse right-hand side into out (GEMV column order, padded
// to ld_free) and sol = def; then, after the GEMV, the interior dofs
template <typename T, typename O>
void
cond_rhs_t(void *sol, const void *def, O *out, hipStream_t s)
{
  const int64_t n = op->n_dofs;
  hipLaunchKernelGGL((k_cond_rhs<T, O>), g1(std::max(n, 8 * dir.ld_free)), dim3(256), 0, s,
                     (T *)sol, (const T *)def, out,
                     (const int32_t *)dir.free_in, (const int32_t *)dir.rg_off,
                     (const int32_t *)dir.rg_ent, (const double *)dir.cF,
                     (const int32_t *)dir.cint, cond_ni, cond_nb, n, dir.n_free,
                     dir.ld_free);
  HIP_THROW(hipGetLastError());
}

template <typename T>
void
cond_post_t(void *sol, const void *def, hipStream_t s)
{
  const int64_t nc_ = op->n_cells;
  hipLaunchKernelGGL(k_cond_post<T>, g1(64 * nc_ * cond_ni), dim3(256), 0, s,
                     (T *)sol, (const T *)def, (const double *)dir.cC,
                     (const double *)dir.cG, (const int32_t *)dir.cint,
                     (const int32_t *)dir.cbnd, cond_ni, cond_nb, nc_);
  HIP_THROW(hipGetLastError());
}

template <typename T>
void
direct_solve(void *sol, const void *def, hipStream_t s)
{
  const int64_t n = op->n_dofs, nf = dir.n_free, ld = dir.ld_free;
  // sol = def (constrained dofs: x_c = b_c, their rows of A are the identity)
  // and the condensed (or gathered) right-hand side: FP32 for the FP32-stored
  // dense inverse, FP64 otherwise
  float *xf = reinterpret_cast<float *>(dir.rhs.ptr);
  if (form.cond && form.f32 && !form.nd)
    cond_rhs_t<T, float>(sol, def, xf, s);
  else if (form.cond)
    cond_rhs_t<T, double>(sol, def, dir.rhs.ptr, s);
  else if (form.f32 && !form.nd)
    hipLaunchKernelGGL(k_coarse_prep<T>, g1(std::max(n, ld)), dim3(256), 0, s, (T *)sol,
                       (const T *)def, xf, (const int32_t *)dir.free_in, n, nf, ld);
  else
    {
      copy_words(sol, def, n * (int64_t)sizeof(T) / 4, s);
      hipLaunchKernelGGL(k_gather_free<T>, g1(nf), dim3(256), 0, s, dir.rhs, (const T *)def,
                         (const int32_t *)dir.free_in, nf);
    }
  HIP_THROW(hipGetLastError());
  if (form.nd) // the two sweeps over the elimination tree
    gls::nd_solver_solve(dir.nd.get(), dir.rhs, sol, std::is_same<T, double>::value, dir.free, s);
  else if (form.f32)
    // sol[free] = A_ff^{-1} def[free], one wave per row.  The inverse is read
    // once per solve and is larger than the MALL: non-temporal row loads (132
    // against 146 us with the default policy, round 3)
    hipLaunchKernelGGL((k_gemv_rows_f32<T, true>), dim3((unsigned)((nf + 3) / 4)), dim3(256), 0,
                       s, (const float4 *)dir.inv32.ptr, (const float4 *)xf, (T *)sol,
                       (const int32_t *)dir.free, nf, ld);
  else
    {
      double *part = dir.rhs + 2 * ld;
      hipLaunchKernelGGL(k_gemv_part<double>, dim3((unsigned)((nf + 255) / 256), GEMV_CHUNKS),
                         dim3(256), 0, s, (const double *)dir.lu, (const double *)dir.rhs, part,
                         nf, ld);
      hipLaunchKernelGGL(k_gemv_sum<T>, g1(nf), dim3(256), 0, s, (const double *)part, (T *)sol,
                         (const int32_t *)dir.free, nf, ld);
    }
  HIP_THROW(hipGetLastError());
  if (form.cond) // the cells' interior dofs
    cond_post_t<T>(sol, def, s);
}

// coarse_grid_iterate (multigrid.cc:491-530, MGCoarseGridIterativeSolver):
// SolverGMRES<VectorType<double>> with deal.II's defaults (left
// preconditioning, max_n_tmp_vectors 30 -> restart after 28) under
// ReductionControl(maxiter, 1e-20, reltol) on the coarse level operator,
// preconditioned by level_prec (the substitute for Trilinos AMG / ILU:
// relaxation sweeps or the dense LU).  FP64 Krylov vectors, the level
// operator and preconditioner in the level precision (the reference solves
// with the FP64 system matrix assembled from the MGNumber operator).  Every
// vector stays on the device.  The restart loop, the pipelined cycle (step
// j + 1 enqueued before the host waits for step j's Hessenberg column,
// pinned and double-buffered; a converged solve runs one discarded step) and
// the CGS2 step are the shared ones of arnoldi.h, as in the outer solver
// (krylov.hip); the lambdas below are their space.
template <typename T>
void
gmres_t(void *sol, void *def, const std::function<void()> &level_prec, hipStream_t s)
{
  const int64_t n  = op->n_dofs;
  const int     m  = 28;
  const int     HC = 2 * (m + 1) + 1; // both CGS passes' coefficients and |w|
  if (n > (int64_t)0x7fffffff)
    throw std::runtime_error("coarse GMRES: level too large for 32-bit rocBLAS sizes");
  rocblas_handle h = blas_on(s);
  check_blas(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host), "pointer mode");
  if (!cg_ws)
    {
      cg_ws.alloc((size_t)(m + 4) * n + HC + (size_t)CGS_PART);
      cg_lvl.alloc((size_t)2 * n * sizeof(T));
      HIP_THROW(hipHostMalloc((void **)&cg_host, (size_t)2 * HC * 8,
                              hipHostMallocMapped | hipHostMallocCoherent));
      for (hipEvent_t &e : cg_ev)
        HIP_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
  double *V = cg_ws, *w = V + (size_t)(m + 1) * n, *x = w + n, *b = x + n,
         *dh = b + n, *cpart = dh + HC;
  double *host_dev = nullptr; // cg_host as the device sees it (k_cgs_unit writes it)
  HIP_THROW(hipHostGetDevicePointer((void **)&host_dev, cg_host, 0));
  T *la = (T *)cg_lvl.ptr, *lb = la + n;
  auto cvt_in = [&](T *dst, const double *src) {
    hipLaunchKernelGGL((k_convert<double, T>), g1(n), dim3(256), 0, s, dst, src, n);
  };
  auto cvt_out = [&](double *dst, const T *src) {
    hipLaunchKernelGGL((k_convert<T, double>), g1(n), dim3(256), 0, s, dst, src, n);
  };
  // dst = P^{-1} src (through def -> sol); ILU and AMG: on the FP64 vectors
  // directly (the reference's Trilinos AMG on the FP64 matrix)
  auto precond = [&](double *dst, const double *src) {
    if (kind_ == CoarseKind::ilu || kind_ == CoarseKind::amg)
      {
        apply(dst, src, s);
        return;
      }
    cvt_in((T *)def, src);
    level_prec();
    cvt_out(dst, (const T *)sol);
  };
  // FP32 brick levels: the FP64 result written by the brick write-out and
  // the reduction themselves (RelaxStep.out64), no conversion pass
  const bool fused_out = std::is_same<T, float>::value && gls::deferred_reduce_ok(op);
  auto apply_A = [&](double *dst, const double *src) {
    cvt_in(la, src);
    if (fused_out)
      {
        gls::RelaxStep r;
        r.out64 = dst;
        gls::brick_launch(op, gls::op_vmult_mode(op), lb, la, 0, op->n_bricks,
                          gls::BRICK_RUN | gls::BRICK_REDUCE, s, &r);
      }
    else
      {
        gls::op_vmult_device(op, lb, la, s);
        cvt_out(dst, lb);
      }
  };
  auto nrm2 = [&](const double *v) {
    double r = 0;
    check_blas(rocblas_dnrm2(h, (rocblas_int)n, v, 1, &r), "rocblas_dnrm2");
    return r;
  };
  auto vc = [&](int j) { return V + (size_t)j * n; };
  // Arnoldi step j, enqueued only: v_{j+1} = P^{-1} A v_j orthogonalised
  // (CGS2) and normalised on the device, its Hessenberg column to pinned
  // host buffer j % 2 (event cg_ev[j % 2])
  auto arnoldi = [&](int j) {
    apply_A(w, vc(j));
    double *wv = vc(j + 1);
    precond(wv, w);
    cgs2_step(V, n, wv, wv, dh, cpart, cg_host + (j % 2) * HC, host_dev + (j % 2) * HC, HC, m,
              j, h, s, cg_ev[j % 2], false, false);
  };
  cvt_out(b, (const T *)def);
  HIP_THROW(hipMemsetAsync(x, 0, n * 8, s));
  // r0 = P^{-1} (b - A 0)
  precond(vc(0), b);
  const double res0 = nrm2(vc(0));
  const double tol  = std::max(desc.coarse_reltol * res0, 1e-20);
  double       col[m + 1];
  gls::GmresSpace sp{
    [&](double beta) {
      const double sc = 1.0 / beta;
      check_blas(rocblas_dscal(h, (rocblas_int)n, &sc, vc(0), 1), "rocblas_dscal");
    },
    arnoldi,
    [&](int j) {
      HIP_THROW(hipEventSynchronize(cg_ev[j % 2]));
      return cgs2_column(cg_host + (j % 2) * HC, m, j, col);
    },
    // x += V y (left preconditioning: the update is in the Krylov space)
    [&](int jd, const double *y) {
      HIP_THROW(hipMemcpyAsync(dh, y, jd * 8, hipMemcpyHostToDevice, s));
      const double one = 1.0;
      check_blas(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, jd, &one, V,
                               (rocblas_int)n, dh, 1, &one, x, 1),
                 "rocblas_dgemv");
      HIP_THROW(hipStreamSynchronize(s)); // y is a host buffer reused by the next cycle
    },
    // restart: r = P^{-1} (b - A x)
    [&] {
      apply_A(w, x);
      hipLaunchKernelGGL(k_residual<double>, g1(n), dim3(256), 0, s, w, (const double *)b, n);
      precond(vc(0), w);
      return nrm2(vc(0));
    }};
  const gls::GmresRun run = gls::gmres_restarted(sp, m, res0, tol, desc.coarse_maxiter);
  const int           it  = run.iterations;
  const double        res = run.residual;
  cg_iters = it;
  cg_conv  = run.converged;
  // deal.II's SolverGMRES inside MGCoarseGridIterativeSolver throws
  // SolverControl::NoConvergence when maxiter is reached (multigrid.cc:
  // 494-530): the V-cycle fails the same way instead of continuing with an
  // unconverged coarse correction
  if (!cg_conv)
    throw std::runtime_error("coarse GMRES: no convergence in " + std::to_string(it) +
                             " iterations (residual " + std::to_string(res) + ", tolerance " +
                             std::to_string(tol) + "; SolverControl::NoConvergence)");
  cvt_in((T *)sol, x);
  HIP_THROW(hipGetLastError());
}

  // y = P^-1 x by the ILU factor or one AMG V-cycle, on FP64 vectors
  void
  apply(double *y, const double *x, hipStream_t s) override
  {
    if (kind_ == CoarseKind::ilu)
      check_status(gls_ilu_vmult(ilu_h, y, x, s), "coarse ILU: ");
    else
      check_status(gls_amg_vmult(amg_h, y, x, s), "coarse AMG: ");
  }

  // the same in the level precision: FP32 levels converted through io64
  void
  apply(void *sol, const void *def, hipStream_t s) override
  {
    if (kind_ == CoarseKind::direct)
      {
        gls::with_real(prec, [&](auto t) { direct_solve<decltype(t)>(sol, def, s); });
        return;
      }
    const int64_t n = op->n_dofs;
    if (prec == GLS_F64)
      apply((double *)sol, (const double *)def, s);
    else
      {
        hipLaunchKernelGGL((k_convert<float, double>), g1(n), dim3(256), 0, s, io64.ptr,
                           (const float *)def, n);
        apply(io64 + n, (const double *)io64, s);
        hipLaunchKernelGGL((k_convert<double, float>), g1(n), dim3(256), 0, s, (float *)sol,
                           io64 + n, n);
      }
    HIP_THROW(hipGetLastError());
  }

  // the coarse level's system matrix (FP64, constrained rows / columns
  // identity) as host CSR
  struct HostCsr
  {
    std::vector<int64_t> rp, ci;
    std::vector<double>  va;
  };
  HostCsr
  system_matrix(const char *prefix) const
  {
    HostCsr m;
    int64_t nnz = 0;
    check_status(gls_op_system_matrix(op, &nnz, nullptr, nullptr, nullptr), prefix);
    m.rp.resize((size_t)op->n_dofs + 1), m.ci.resize((size_t)nnz), m.va.resize((size_t)nnz);
    check_status(gls_op_system_matrix(op, &nnz, m.rp.data(), m.ci.data(), m.va.data()), prefix);
    return m;
  }

  void
  setup(void *sol, void *tmp, hipStream_t s) override
  {
    using clock   = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) {
      return std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    };
    if (kind_ == CoarseKind::ilu)
      {
        // the pattern never changes, so every setup after the first refactors
        HIP_THROW(hipStreamSynchronize(s));
        gls::Section sc("gmg::initialize::ilu", s);
        const auto   t0 = clock::now();
        if (ilu_device)
          {
            // assembled and factorised on the device, on the setup stream
            glsDeviceCSR m{};
            check_status(gls_op_system_matrix_device(op, &m, s), "coarse ILU: ");
            check_status(ilu_h ? gls_ilu_refactor_device(ilu_h, m.vals, s) :
                                 gls_ilu_create_device(&m, &ilu_prm, s, &ilu_h),
                         "coarse ILU: ");
          }
        else
          {
            const HostCsr m = system_matrix("coarse ILU: ");
            check_status(ilu_h ? gls_ilu_refactor(ilu_h, m.va.data()) :
                                 gls_ilu_create(op->n_dofs, m.rp.data(), m.ci.data(), m.va.data(),
                                                &ilu_prm, &ilu_h),
                         "coarse ILU: ");
          }
        if (!io64)
          io64.alloc((size_t)2 * op->n_dofs);
        ilu_setup_ms = ms_since(t0);
      }
    else if (kind_ == CoarseKind::amg)
      {
        // the AMG hierarchy on the coarse level's system matrix
        HIP_THROW(hipStreamSynchronize(s));
        gls::Section  sc("gmg::initialize::amg", s);
        const auto    t0 = clock::now();
        const HostCsr m = system_matrix("coarse AMG: ");
        if (amg_h)
          gls_amg_destroy(amg_h), amg_h = nullptr;
        check_status(amg_ilu ? gls_amg_create_ilu(op->n_dofs, m.rp.data(), m.ci.data(),
                                                  m.va.data(), &desc.amg, &amg_ilu_prm, &amg_h) :
                               gls_amg_create(op->n_dofs, m.rp.data(), m.ci.data(), m.va.data(),
                                              &desc.amg, &amg_h),
                     "coarse AMG: ");
        if (!io64)
          io64.alloc((size_t)2 * op->n_dofs);
        amg_setup_ms = ms_since(t0);
      }
    else if (kind_ == CoarseKind::direct)
      {
        gls::Section sc("gmg::initialize::direct", s);
        gls::with_real(prec, [&](auto t) { direct_setup<decltype(t)>(sol, tmp, s); });
      }
    setup_done = true;
  }

  CoarseKind
  kind() const override
  {
    return kind_;
  }

  void
  set_direct(int m, int max_leaf_cells) override
  {
    if (m != GLS_COARSE_DENSE && m != GLS_COARSE_ND)
      throw std::runtime_error("gls_mg_set_coarse_direct: unknown method");
    if (max_leaf_cells < 0)
      throw std::runtime_error("gls_mg_set_coarse_direct: negative max_leaf_cells");
    if (kind_ != CoarseKind::direct)
      throw std::runtime_error("gls_mg_set_coarse_direct: the coarse solver is not the direct one "
                               "(coarse_n_iterations < 0)");
    if (partitioned)
      throw std::runtime_error("gls_mg_set_coarse_direct: partitioned levels");
    if (setup_done)
      throw std::runtime_error("gls_mg_set_coarse_direct: call it before gls_mg_setup");
    method        = m;
    nd_leaf_cells = max_leaf_cells;
  }

  void
  set_ilu(const glsILUParams &prm) override
  {
    if (prm.fill_level < 0 || !std::isfinite(prm.atol) || !std::isfinite(prm.rtol))
      throw std::runtime_error("gls_mg_set_coarse_ilu: invalid parameters");
    if (partitioned)
      throw std::runtime_error("gls_mg_set_coarse_ilu: the ILU coarse solver is single-domain");
    if (kind_ == CoarseKind::amg)
      throw std::runtime_error("gls_mg_set_coarse_ilu: the coarse solver is the AMG");
    if (method != GLS_COARSE_DENSE)
      throw std::runtime_error("gls_mg_set_coarse_ilu: a direct coarse solver was chosen");
    if (setup_done)
      throw std::runtime_error("gls_mg_set_coarse_ilu: call it before gls_mg_setup");
    kind_   = coarse_kind(desc, true);
    ilu_prm = prm;
  }

  void
  set_ilu_device(bool on) override
  {
    if (kind_ != CoarseKind::ilu)
      throw std::runtime_error("gls_mg_set_coarse_ilu_device: the coarse solver is not the ILU "
                               "(gls_mg_set_coarse_ilu first)");
    if (setup_done)
      throw std::runtime_error("gls_mg_set_coarse_ilu_device: call it before gls_mg_setup");
    ilu_device = on;
  }

  void
  set_amg_ilu(const glsAMGIluParams &prm) override
  {
    if (prm.fill_level < 0 || !std::isfinite(prm.atol) || !std::isfinite(prm.rtol))
      throw std::runtime_error("gls_mg_set_coarse_amg_ilu: invalid parameters");
    if (kind_ != CoarseKind::amg)
      throw std::runtime_error("gls_mg_set_coarse_amg_ilu: the coarse solver is not the AMG "
                               "(coarse_amg = 1)");
    if (partitioned)
      throw std::runtime_error("gls_mg_set_coarse_amg_ilu: the AMG coarse solver is single-domain");
    if (setup_done)
      throw std::runtime_error("gls_mg_set_coarse_amg_ilu: call it before gls_mg_setup");
    amg_ilu     = prm.smoother_ilu || prm.coarse_ilu;
    amg_ilu_prm = prm;
  }

  void
  check_operator() const override
  {
    // the direct coarse solvers assemble from element matrices themselves and
    // know the Dirichlet mask only (an ILU set over coarse_n_iterations < 0 is
    // refused in the same words)
    const bool direct_asked =
      kind_ == CoarseKind::direct || (kind_ == CoarseKind::ilu && desc.coarse_n_iterations < 0);
    if (direct_asked && op->nc.n)
      throw std::runtime_error(
        method == GLS_COARSE_ND ?
          "gls_mg_setup: the nested-dissection (\"nd\") direct coarse solver does not support a "
          "coarse operator with node constraints" :
          "gls_mg_setup: the dense Schur-complement direct coarse solver does not support a "
          "coarse operator with node constraints");
  }

  void
  gmres(void *sol, void *def, const std::function<void()> &level_prec, hipStream_t s) override
  {
    gls::with_real(prec, [&](auto t) { gmres_t<decltype(t)>(sol, def, level_prec, s); });
  }

  void
  statistics(int *n_iterations, int *converged) const override
  {
    *n_iterations = cg_iters;
    *converged    = cg_conv;
  }

  glsILU
  ilu(double *setup_ms) const override
  {
    if (setup_ms)
      *setup_ms = ilu_setup_ms;
    return ilu_h;
  }

  glsAMG
  amg(double *setup_ms) const override
  {
    if (setup_ms)
      *setup_ms = amg_setup_ms;
    return amg_h;
  }

  void
  setup_times(double *ms3, int *n_colors) const override
  {
    for (int i = 0; i < 3; ++i)
      ms3[i] = setup_ms[i];
    if (n_colors)
      *n_colors = colors;
  }

  void
  direct_info(glsCoarseDirectInfo *info) const override
  {
    if (kind_ != CoarseKind::direct)
      throw std::runtime_error("gls_mg_coarse_direct_info: the coarse solver is not the direct one");
    *info           = glsCoarseDirectInfo{};
    info->requested = method;
    info->max_leaf_cells = nd_leaf_cells > 0 ? nd_leaf_cells : ND_DEFAULT_LEAF_CELLS;
    info->n_free         = dir.n_free;
    if (form.nd)
      {
        const gls::NdPlan &pl = gls::nd_solver_plan(dir.nd.get());
        info->method         = GLS_COARSE_ND;
        info->tree_nodes     = (int)pl.nodes.size();
        info->depth          = pl.depth;
        info->max_own        = pl.max_own;
        info->max_boundary   = pl.max_boundary;
        info->plan_ms        = nd_plan_ms;
        gls::nd_solver_stats(dir.nd.get(), &info->stored_entries, &info->stored_bytes,
                             &info->factor_ms, &info->narrow_ms);
      }
    else
      {
        const bool f32   = form.f32;
        info->method     = GLS_COARSE_DENSE;
        info->tree_nodes = info->depth = dir.n_free > 0 ? 1 : 0;
        info->max_own    = (int)dir.n_free;
        info->stored_entries = dir.n_free * (f32 ? dir.ld_free : dir.n_free);
        info->stored_bytes   = info->stored_entries * (f32 ? 4 : 8);
        info->factor_ms      = setup_ms[0] + setup_ms[1] + setup_ms[2];
      }
  }
};
} // namespace

std::unique_ptr<CoarseSolver>
gls::CoarseSolver::create(const glsMGDesc &desc, glsOp op0, int prec, bool partitioned)
{
  auto c         = std::make_unique<CoarseImpl>();
  c->desc        = desc;
  c->op          = op0;
  c->prec        = prec;
  c->partitioned = partitioned;
  c->kind_       = coarse_kind(desc, false);
  return c;
}
