// arnoldi.h — what the three device GMRES solvers share beyond the kernels of
// cgs.h: the single-domain CGS2 Arnoldi orthonormalisation (krylov.hip and the
// coarse GMRES of coarse.hip), the pipelined cycle and the restart loop (those two
// and the partitioned solver of dist_mg.hip), over the host least squares of
// hessenberg.h.  A solver supplies a "space" (gls::GmresSpace of its own
// callables, which keep their stream synchronisations):
//   normalise(beta)      column 0 of the basis (the residual) times 1 / beta
//   enqueue_step(j)      Arnoldi step j enqueued only: preconditioner, operator,
//                        orthonormalisation into column j + 1, the Hessenberg
//                        record to pinned host buffer j % 2, event j % 2
//   record(j)            waits for event j % 2; column j of the Hessenberg
//                        matrix, j + 2 entries, the last one |w|
//   update(jd, y)        x += the cycle's correction with coefficients y
//   restart_residual()   the true residual into column 0, its norm returned
#pragma once

#include "cgs.h"
#include "common.h"
#include "hessenberg.h"

#include <rocblas/rocblas.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace
{
// t = b - t (t holds A x: the restart residual, the multigrid's residual step)
template <typename T>
__global__ void
k_residual(T *__restrict__ t, const T *__restrict__ b, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    t[i] = b[i] - t[i];
}

// dst = src converted (the FP64 outer vectors of FP32 multigrid levels)
template <typename Tin, typename Tout>
__global__ void
k_convert(Tout *__restrict__ dst, const Tin *__restrict__ src, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] = (Tout)src[i];
}

inline void
check_blas(rocblas_status st, const char *what)
{
  if (st != rocblas_status_success)
    throw std::runtime_error(std::string(what) + ": " + rocblas_status_to_string(st));
}

// v = w orthogonalised against the first j + 1 columns of V (n rows) twice
// (CGS2) and normalised, enqueued only; v may be w.  dh: h1 at [0, m + 1), h2
// at [m + 1, 2 (m + 1)), |w| at 2 (m + 1), n_rec doubles in all, the step's
// record: to rec (pinned, rec_dev as the device sees it), then event ev.  Up
// to 31 columns the second update is folded into the normalisation
// (k_cgs_unit: norm by Pythagoras, the record written by the kernel), at 32
// columns three fused passes, beyond that rocBLAS GEMVs (h in host pointer
// mode).  force_rocblas / force_three_pass: GLS_GMRES_ORTHO's reference forms.
inline void
cgs2_step(const double *V, int64_t n, double *w, double *v, double *dh, double *cpart, double *rec,
          double *rec_dev, int n_rec, int m, int j, rocblas_handle h, hipStream_t s, hipEvent_t ev,
          bool force_rocblas, bool force_three_pass)
{
  const int  J    = j + 1;
  double    *h2   = dh + (m + 1), *hn = dh + 2 * (m + 1);
  const bool fold = J < CGS_MAXJ && !force_rocblas && !force_three_pass;
  if (J <= CGS_MAXJ && !force_rocblas)
    {
      // dots; update + dots (fold: + |w|^2); then the normalising update, or
      // update + norm (three basis passes)
      hipLaunchKernelGGL(k_cgs_dots, dim3(CGS_BLOCKS), dim3(256), 0, s, V, J, (const double *)w,
                         cpart, n, n);
      hipLaunchKernelGGL(k_cgs_finish, dim3(J), dim3(256), 0, s, (const double *)cpart, dh, 0);
      hipLaunchKernelGGL(k_cgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, V, J, (const double *)dh,
                         w, cpart, n, n, n, fold ? 2 : 0);
      hipLaunchKernelGGL(k_cgs_finish, dim3(fold ? J + 1 : J), dim3(256), 0, s,
                         (const double *)cpart, h2, 0);
      if (fold)
        hipLaunchKernelGGL(k_cgs_unit, dim3(CGS_BLOCKS), dim3(256), 0, s, V, J, (const double *)h2,
                           (const double *)w, v, hn, n, n, (const double *)dh, rec_dev, n_rec,
                           2 * (m + 1));
      else
        {
          hipLaunchKernelGGL(k_cgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, V, J,
                             (const double *)h2, w, cpart, n, n, n, 1);
          hipLaunchKernelGGL(k_cgs_finish, dim3(1), dim3(256), 0, s, (const double *)cpart, hn, 1);
        }
      HIP_THROW(hipGetLastError());
    }
  else
    {
      const double one = 1.0, zero = 0.0, mone = -1.0;
      for (double *hp : {dh, h2})
        {
          check_blas(rocblas_dgemv(h, rocblas_operation_transpose, (rocblas_int)n, J, &one, V,
                                   (rocblas_int)n, w, 1, &zero, hp, 1),
                     "rocblas_dgemv");
          check_blas(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, J, &mone, V,
                                   (rocblas_int)n, hp, 1, &one, w, 1),
                     "rocblas_dgemv");
        }
      check_blas(rocblas_set_pointer_mode(h, rocblas_pointer_mode_device), "pointer mode");
      check_blas(rocblas_dnrm2(h, (rocblas_int)n, w, 1, hn), "rocblas_dnrm2");
      check_blas(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host), "pointer mode");
    }
  if (!fold)
    HIP_THROW(hipMemcpyAsync(rec, dh, n_rec * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_THROW(hipEventRecord(ev, s));
  if (!fold)
    hipLaunchKernelGGL(k_unit_col, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v,
                       (const double *)w, (const double *)hn, n);
  HIP_THROW(hipGetLastError());
}

// column j of the Hessenberg matrix from a CGS2 record: both passes'
// coefficients added, the norm below them
inline const double *
cgs2_column(const double *rec, int m, int j, double *col)
{
  for (int i = 0; i <= j; ++i)
    col[i] = rec[i] + rec[(m + 1) + i];
  col[j + 1] = rec[2 * (m + 1)];
  return col;
}
} // namespace

namespace gls
{
template <class N, class E, class R, class U, class Q>
struct GmresSpace
{
  N normalise;
  E enqueue_step;
  R record;
  U update;
  Q restart_residual;
};
template <class N, class E, class R, class U, class Q>
GmresSpace(N, E, R, U, Q) -> GmresSpace<N, E, R, U, Q>;

struct GmresRun
{
  int    iterations = 0, restarts = 0;
  double residual  = 0;
  bool   converged = false;
};

// One cycle of at most lsq.m() steps from the normalised residual in column
// 0 (norm beta), software-pipelined: step j + 1 is enqueued before the host
// waits for step j's column, so the device does not idle through the host
// round trip; when step j converges, the enqueued step j + 1 runs to
// completion and is discarded.  The residual estimate is checked every
// iteration; a lucky breakdown (|w| == 0) means it is exact.  Returns the
// number of columns, their coefficients in y.
template <class Space>
int
gmres_cycle(Space &sp, HessenbergLsq &lsq, double beta, double tol, int max_it, GmresRun &run,
            double *y)
{
  lsq.reset(beta);
  int jd = 0;
  sp.enqueue_step(0);
  for (int j = 0; j < lsq.m() && run.iterations < max_it; ++j)
    {
      if (j + 1 < lsq.m() && run.iterations + 1 < max_it)
        sp.enqueue_step(j + 1);
      const double *col = sp.record(j);
      run.residual      = lsq.push_column(j, col);
      ++run.iterations;
      ++jd;
      if (run.residual <= tol || col[j + 1] == 0)
        break;
    }
  lsq.solve(jd, y);
  return jd;
}

// restarted GMRES(m) from the residual in column 0 of the space's basis
// (norm res0); cycle(beta, run, y) runs one cycle as gmres_cycle does
template <class Space, class Cycle>
GmresRun
gmres_restarted(Space &sp, int m, double res0, double tol, int max_it, Cycle &&cycle)
{
  GmresRun run;
  run.residual = res0;
  std::vector<double> y((size_t)m);
  while (run.residual > tol && run.iterations < max_it)
    {
      sp.normalise(run.residual);
      const int jd = cycle(run.residual, run, y.data());
      sp.update(jd, y.data());
      if (run.residual <= tol || run.iterations >= max_it)
        break;
      ++run.restarts;
      run.residual = sp.restart_residual();
    }
  run.converged = run.residual <= tol;
  return run;
}

template <class Space>
GmresRun
gmres_restarted(Space &sp, int m, double res0, double tol, int max_it)
{
  HessenbergLsq lsq(m);
  return gmres_restarted(sp, m, res0, tol, max_it, [&](double beta, GmresRun &run, double *y) {
    return gmres_cycle(sp, lsq, beta, tol, max_it, run, y);
  });
}
} // namespace gls
