// krylov.hip — device-resident right-preconditioned restarted GMRES
// (SURVEY §8f rank 2): LinearSolverGMRES::solve, solver_l.cc:45-74, over
// deal.II SolverGMRES(max_n_tmp_vectors = 30, right_preconditioning = true).
//
// Every vector (the Krylov basis V, the preconditioned direction, the
// solution) stays in HBM; per iteration only the j+1 Hessenberg entries and a
// norm cross to the host (what deal.II's MPI_Allreduce of the dots returns on
// every rank), and the next Arnoldi step is already enqueued while the host
// waits for them (the device does not idle through the round trip).
// Orthogonalisation is classical Gram-Schmidt with one re-orthogonalisation
// (CGS2): passes over the contiguous basis per iteration instead of j+1
// dependent dot/axpy pairs — the same projector as deal.II's modified
// Gram-Schmidt in exact arithmetic, and the stable choice for a streaming
// device.  The restart loop, the pipelined cycle and the CGS2 step are the
// shared ones of arnoldi.h (gls::gmres_restarted, gls::gmres_cycle,
// cgs2_step), the host least squares hessenberg.h; this file holds what only
// the outer solver has: its workspace on the operator, the preconditioner
// kinds, the kept directions Z and the delayed CGS2 cycle (cycle_dcgs).
#include "../../include/gls_op.h"
#include "arnoldi.h"
#include "trace.h"
#include "op_internal.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace gls
{
// csrc/ilu.hip: gls_ilu_vmult on the factor's device without the scope
void    ilu_apply(glsILU_ *ilu, double *dst, const double *src, hipStream_t st);
int64_t ilu_size(const glsILU_ *ilu);
} // namespace gls

namespace
{
#define RB_THROW(expr)                                                                       \
  do                                                                                         \
    {                                                                                        \
      const rocblas_status s_ = (expr);                                                      \
      if (s_ != rocblas_status_success)                                                      \
        throw std::runtime_error(std::string(#expr) + ": " + rocblas_status_to_string(s_));   \
    }                                                                                        \
  while (0)

// one rocBLAS handle per host thread and device, created on first use
// (creating one per solve cost milliseconds in a Newton loop); bound to the
// caller's stream on every solve
struct HandleCache
{
  rocblas_handle h[64] = {};
  ~HandleCache()
  {
    for (rocblas_handle x : h)
      if (x)
        (void)rocblas_destroy_handle(x);
  }
};

rocblas_handle
blas_handle(int dev, hipStream_t s)
{
  static thread_local HandleCache cache;
  if (dev < 0 || dev >= 64)
    throw std::runtime_error("gls_gmres_solve: device ordinal out of range");
  rocblas_handle &h = cache.h[dev];
  if (!h)
    RB_THROW(rocblas_create_handle(&h));
  RB_THROW(rocblas_set_stream(h, s));
  RB_THROW(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
  return h;
}

void
check(glsStatus st, const char *what)
{
  if (st != 0)
    throw std::runtime_error(std::string(what) + ": " + gls_last_error());
}

void
check_arguments(glsOp op, int kind, void *prec, const glsGMRESDesc *desc, void *x, const void *b)
{
  if (!op || !desc || !x || !b)
    throw std::runtime_error("gls_gmres_solve: null argument");
  if (kind != GLS_PREC_MG && kind != GLS_PREC_ILU && kind != GLS_PREC_AMG)
    throw std::runtime_error("gls_gmres_solve_prec: unknown preconditioner kind");
  if (kind != GLS_PREC_MG && !prec)
    throw std::runtime_error("gls_gmres_solve_prec: null preconditioner");
  if (op->prec != GLS_F64)
    throw std::runtime_error("gls_gmres_solve: the outer operator must be FP64 "
                             "(LinearSolverGMRES works on VectorType<double>)");
  if (op->n_owned_dofs != op->n_dofs)
    throw std::runtime_error("gls_gmres_solve: single-domain operators only (a partitioned "
                             "solve needs all-reduced dots)");
  if (desc->max_n_tmp_vectors < 3)
    throw std::runtime_error("gls_gmres_solve: max_n_tmp_vectors must be >= 3");
  if (kind == GLS_PREC_MG && prec)
    gls::mg_check_outer((glsMG)prec, op); // FP64 outer vectors of op's size, set up
  // ILU / AMG of gls_op_system_matrix: its rows are the node-major dofs the
  // Krylov vectors hold on the device (the caller layout is staged at the
  // solve's ends), so the factor applies to them as they are
  if (kind == GLS_PREC_ILU && gls::ilu_size((glsILU)prec) != op->n_dofs)
    throw std::runtime_error("gls_gmres_solve_prec: the ILU is not of the operator's size");
  if (kind == GLS_PREC_AMG)
    {
      int     nl = 0;
      int64_t sizes[64];
      check(gls_amg_info((glsAMG)prec, &nl, nullptr, nullptr, nullptr), "gls_amg_info");
      if (nl < 1 || nl > 64)
        throw std::runtime_error("gls_gmres_solve_prec: AMG hierarchy out of range");
      check(gls_amg_info((glsAMG)prec, &nl, sizes, nullptr, nullptr), "gls_amg_info");
      if (sizes[0] != op->n_dofs)
        throw std::runtime_error("gls_gmres_solve_prec: the AMG is not of the operator's size");
    }
  if (op->n_dofs > (int64_t)0x7fffffff)
    throw std::runtime_error("gls_gmres_solve: vector too long for 32-bit rocBLAS sizes");
}

// One solve's Krylov workspace [V (m+1) n | w n | z n | dh HC | cpart | Z m n]
// and the two pinned step records (by step parity) as the host and the device
// (k_cgs_unit, k_dcgs_finish write them directly) see them
struct Workspace
{
  int64_t n;
  int     m, HC;
  bool    zkeep;
  double *V, *w, *z, *dh, *cpart, *Zd, *host, *host_dev;
};

// The workspace is kept on the operator and grown on demand (a hipMalloc /
// hipFree of the basis per solve synchronises the device and costs more than
// the solve's setup).  linear: the preconditioner is a linear operator
Workspace
workspace(glsOp op, int m, bool linear, hipStream_t s)
{
  const int64_t n = op->n_dofs;
  // dh: the two CGS passes' coefficients and |w| (HC values, one D2H copy),
  // or a DCGS2 step's record (DCGS_D values)
  const int HC = std::max(2 * (m + 1) + 1, DCGS_D);
  // the preconditioned directions z_j = M^{-1} v_j are kept (Z, m columns):
  // the cycle's update is then x += Z y, the same iterate as deal.II's
  // x += M^{-1} (V y) (SolverGMRES, right preconditioning: solver_l.cc:62)
  // without the V-cycle per restart -- but only for a LINEAR preconditioner.
  // A V-cycle whose coarse solve iterates to a tolerance (coarse_iterate,
  // the reference's default coarse_grid_iterate, multigrid.h:36) is not
  // linear, so x += Z y would leave deal.II's iterate; there, and when the m
  // extra columns would take more than a quarter of the free device memory,
  // the M^{-1} (V y) form runs.  GLS_GMRES_ZKEEP=0 / 1 forces it off / on
  // (1: tests pinning the deviation of the kept form).
  bool zkeep = linear;
  {
    const size_t zbytes = (size_t)m * n * sizeof(double);
    const bool   have_z = op->gmres_ws_bytes >= (size_t)(2 * m + 3) * n * sizeof(double);
    size_t       fr = 0, tot = 0;
    if (zkeep && !have_z && hipMemGetInfo(&fr, &tot) == hipSuccess && zbytes > fr / 4)
      zkeep = false;
    if (const char *e = getenv("GLS_GMRES_ZKEEP"))
      zkeep = e[0] != '0';
  }
  const size_t nz = zkeep ? (size_t)m * n : 0;
  // Z starts 256-byte aligned (the operator's 16-byte pack loads read it)
  const size_t z_off = ((size_t)(m + 3) * n + HC + (size_t)DCGS_PART + 31) / 32 * 32;
  const size_t ws    = (z_off + nz) * sizeof(double);
  if (op->gmres_ws_bytes < ws)
    {
      if (op->gmres_ws)
        {
          HIP_THROW(hipStreamSynchronize(s));
          HIP_THROW(hipFree(op->gmres_ws));
          op->gmres_ws = nullptr;
        }
      HIP_THROW(hipMalloc(&op->gmres_ws, ws));
      op->gmres_ws_bytes = ws;
    }
  if (op->gmres_host_count < (size_t)(2 * HC))
    {
      if (op->gmres_host)
        {
          HIP_THROW(hipStreamSynchronize(s));
          HIP_THROW(hipHostFree(op->gmres_host));
          op->gmres_host = nullptr;
        }
      HIP_THROW(hipHostMalloc((void **)&op->gmres_host, 2 * HC * sizeof(double),
                              hipHostMallocMapped | hipHostMallocCoherent));
      op->gmres_host_count = 2 * HC;
    }
  Workspace k{n, m, HC, zkeep};
  k.V     = (double *)op->gmres_ws;
  k.w     = k.V + (size_t)(m + 1) * n;
  k.z     = k.w + n;
  k.dh    = k.z + n;
  k.cpart = k.dh + HC;
  k.Zd    = k.V + z_off;
  k.host  = op->gmres_host;
  HIP_THROW(hipHostGetDevicePointer((void **)&k.host_dev, op->gmres_host, 0));
  return k;
}

// ---- delayed CGS2 (cgs.h).  Step j holds the TENTATIVE vector u_j
// (orthogonalised once) in column j of V: w_j = A M^{-1} u_j; one pass of
// dots s = Q^T u_j, z = Q^T w_j, u_j.u_j, u_j.w_j (Q: the final columns
// 0..j-1); one update pass q_j = (u_j - Q s) / alpha_j into column j and
// the next tentative u_{j+1} = (w_j - Q z - q_j h_jj) / alpha_j into column
// j+1, with |u_{j+1}|^2.  With the Arnoldi relation of the earlier columns
// (A M^{-1} Q_j = Q_{j+1} H_j, M linear), A M^{-1} q_j = ([z; h_jj] -
// H_j s_j) / alpha_j (the Q_{j+1} part) + u_{j+1}, and u_{j+1} = Q_{j+1}
// s_{j+1} + alpha_{j+1} q_{j+1}: column j of H is final once step j+1's
// s_{j+1}, alpha_{j+1} are known; until then the convergence estimate uses
// |u_{j+1}| for H_{j+1,j} and leaves out s_{j+1} (O(eps) terms).  The kept
// directions are M^{-1} u_j; with U = Q R (R_ij = s_j[i], R_jj = alpha_j),
// M^{-1} Q y = Z (R^{-1} y).
//
// One DCGS2 cycle from the tentative u_0 = r / beta in column 0, pipelined as
// gls::gmres_cycle: the update coefficients (R^{-1} y with kept directions,
// else y) into y; returns the number of columns.  apply(j): w = A M^{-1} u_j.
// wide: the wide passes (cgs.h: 8-wave blocks, 16-byte row pairs; an even
// row count), else the narrow ones.
template <class Apply>
int
cycle_dcgs(const Workspace &k, hipStream_t s, hipEvent_t *ev, bool wide, Apply &&apply,
           double beta, double tol, int max_it, gls::GmresRun &run, double *y)
{
  const int     m = k.m;
  const int64_t n = k.n;
  auto vcol       = [&](int j) { return k.V + (size_t)j * n; };
  auto dcgs_dots  = [&](int J, const double *u, const double *wv) {
    if (wide)
      hipLaunchKernelGGL(k_dcgs_dots_wide, dim3(CGS_BLOCKS), dim3(DCGS_WIDE), 0, s,
                         (const double *)k.V, J, u, wv, k.cpart, n, n);
    else
      hipLaunchKernelGGL(k_dcgs_dots, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)k.V, J, u,
                         wv, k.cpart, n, n);
  };
  // step j, enqueued only: its record to pinned host buffer j % 2
  auto arnoldi_d = [&](int j) {
    apply(j);
    double *dd = k.dh;
    dcgs_dots(j, (const double *)vcol(j), (const double *)k.w);
    hipLaunchKernelGGL(k_dcgs_finish, dim3(DCGS_W), dim3(256), 0, s, (const double *)k.cpart, dd, j,
                       -1, (double *)nullptr);
    if (wide)
      hipLaunchKernelGGL(k_dcgs_update_wide, dim3(CGS_BLOCKS), dim3(DCGS_WIDE), 0, s,
                         (const double *)k.V, j, dd, vcol(j), (const double *)k.w, vcol(j + 1),
                         k.cpart, n, n);
    else
      hipLaunchKernelGGL(k_dcgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)k.V, j,
                         dd, vcol(j), (const double *)k.w, vcol(j + 1), k.cpart, n, n);
    hipLaunchKernelGGL(k_dcgs_finish, dim3(1), dim3(256), 0, s, (const double *)k.cpart, dd, -1,
                       DCGS_W + 2, k.host_dev + (j % 2) * k.HC);
    HIP_THROW(hipGetLastError());
    HIP_THROW(hipEventRecord(ev[j % 2], s));
  };
  // raw (unrotated) Hessenberg, column major with m+1 rows, and R
  std::vector<double> Hr((size_t)(m + 1) * m, 0.0), Rm((size_t)m * m, 0.0);
  auto                HR = [&](int i, int c) -> double & { return Hr[(size_t)c * (m + 1) + i]; };
  auto                RR = [&](int i, int c) -> double & { return Rm[(size_t)c * m + i]; };
  // step j's record: column j-1 finished, column j estimated, R column j
  auto absorb = [&](int j, const double *rc) {
    const double *sj = rc, *zj = rc + CGS_MAXJ;
    const double  alpha = rc[DCGS_W], hjj = rc[DCGS_W + 1], nu = rc[DCGS_W + 2];
    if (j >= 1)
      {
        for (int i = 0; i < j; ++i)
          HR(i, j - 1) += sj[i];
        HR(j, j - 1) = alpha;
      }
    for (int i = 0; i <= j; ++i)
      {
        double t = i < j ? zj[i] : hjj;
        for (int c = 0; c < j; ++c)
          t -= HR(i, c) * sj[c];
        HR(i, j) = alpha > 0 ? t / alpha : 0.0;
      }
    HR(j + 1, j) = std::sqrt(nu > 0 ? nu : 0.0);
    for (int i = 0; i < j; ++i)
      RR(i, j) = sj[i];
    RR(j, j) = alpha;
  };
  // least squares min |g0 e_0 - H y| over the first jd columns, re-factorised
  // from the raw Hessenberg (step j + 1 corrects column j): the estimate
  gls::HessenbergLsq lsq(m);
  auto               estimate = [&](int jd, double g0) {
    double res = 0;
    lsq.reset(g0);
    for (int c = 0; c < jd; ++c)
      res = lsq.push_column(c, &HR(0, c));
    return res;
  };
  double g0    = beta;
  int    jd    = 0;
  bool   ahead = false; // step jd enqueued (its record finishes column jd-1)
  arnoldi_d(0);
  for (int j = 0; j < m && run.iterations < max_it; ++j)
    {
      ahead = j + 1 < m && run.iterations + 1 < max_it;
      if (ahead)
        arnoldi_d(j + 1);
      HIP_THROW(hipEventSynchronize(ev[j % 2]));
      const double *rc = k.host + (j % 2) * k.HC;
      absorb(j, rc);
      if (j == 0)
        g0 = beta * rc[DCGS_W]; // r = beta u_0 = beta alpha_0 q_0
      ++run.iterations;
      ++jd;
      run.residual = estimate(jd, g0);
      if (run.residual <= tol || HR(j + 1, j) == 0)
        break;
    }
  // column jd-1's re-orthogonalisation terms: the record of the step run
  // ahead, or the dots of u_jd alone
  if (ahead)
    {
      HIP_THROW(hipEventSynchronize(ev[jd % 2]));
      const double *rc = k.host + (jd % 2) * k.HC;
      for (int i = 0; i < jd; ++i)
        HR(i, jd - 1) += rc[i];
      HR(jd, jd - 1) = rc[DCGS_W];
    }
  else
    {
      dcgs_dots(jd, (const double *)vcol(jd), (const double *)nullptr);
      hipLaunchKernelGGL(k_dcgs_finish, dim3(DCGS_W), dim3(256), 0, s, (const double *)k.cpart,
                         k.dh, jd, -1, (double *)nullptr);
      HIP_THROW(hipGetLastError());
      std::vector<double> rc(DCGS_W);
      HIP_THROW(hipMemcpyAsync(rc.data(), k.dh, DCGS_W * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      double s2 = 0;
      for (int i = 0; i < jd; ++i)
        {
          HR(i, jd - 1) += rc[i];
          s2 += rc[i] * rc[i];
        }
      const double a2 = rc[2 * CGS_MAXJ] - s2;
      HR(jd, jd - 1)  = std::sqrt(a2 > 0 ? a2 : 0.0);
    }
  run.residual = estimate(jd, g0);
  lsq.solve(jd, y);
  if (k.zkeep) // t = R^{-1} y
    for (int i = jd - 1; i >= 0; --i)
      {
        double t = y[i];
        for (int c = i + 1; c < jd; ++c)
          t -= RR(i, c) * y[c];
        y[i] = t / RR(i, i);
      }
  return jd;
}

} // namespace

// the solver behind gls_gmres_solve (kind GLS_PREC_MG, prec a glsMG or null:
// identity) and gls_gmres_solve_prec
static glsStatus
gmres_solve(glsOp op, int kind, void *prec, const glsGMRESDesc *desc, void *x_, const void *b_,
            glsGMRESResult *result, void *stream)
{
  GLS_TRY
  gls::Section sec_("gmres::solve", (hipStream_t)stream);
  check_arguments(op, kind, prec, desc, x_, b_);
  const glsMG  mg  = kind == GLS_PREC_MG ? (glsMG)prec : nullptr;
  const glsILU ilu = kind == GLS_PREC_ILU ? (glsILU)prec : nullptr;
  const glsAMG amg = kind == GLS_PREC_AMG ? (glsAMG)prec : nullptr;
  // the operator's device for the whole solve (staging buffers included),
  // the caller's current device restored on return
  gls::DeviceScope dev(op->device);
  hipStream_t      s = (hipStream_t)stream;
  // caller layout (host memory / dof numbering): b staged in, x written to
  // a device buffer and copied / permuted back at the end
  const double  *b = (const double *)op->stage.in_vec(b_, 1, s);
  double        *x = (double *)op->stage.out_vec(x_);
  rocblas_handle h = blas_handle(op->device, s);
  const bool     linear = !mg || gls::mg_is_linear(mg);
  // deal.II SolverGMRES restarts after max_n_tmp_vectors - 2 iterations
  const Workspace k = workspace(op, desc->max_n_tmp_vectors - 2, linear, s);
  const int64_t   n = k.n;
  const int       m = k.m, HC = k.HC;
  auto vcol = [&](int j) { return k.V + (size_t)j * n; };
  auto zcol = [&](int j) { return k.zkeep ? k.Zd + (size_t)j * n : k.z; };
  auto precondition = [&](double *dst, const double *src) {
    if (mg)
      {
        gls::Section sc("gmg::vmult", s);
        gls::mg_vcycle_device(mg, dst, src, s);
      }
    else if (ilu)
      {
        gls::Section sc("ilu::vmult", s);
        gls::ilu_apply(ilu, dst, src, s);
      }
    else if (amg)
      {
        gls::Section sc("amg::vmult", s);
        check(gls_amg_vmult(amg, dst, src, s), "gls_amg_vmult");
      }
    else
      HIP_THROW(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  };
  auto vmult = [&](double *dst, const double *src) {
    gls::Section sc("ns::vmult", s);
    gls::op_vmult_device(op, dst, src, s);
  };
  auto nrm2 = [&](const double *v) {
    double r = 0;
    RB_THROW(rocblas_dnrm2(h, (rocblas_int)n, v, 1, &r));
    return r;
  };
  // solver_l.cc:52-53: tolerance = max(rel * |b|, abs); dst = 0 (:66)
  const double bnorm = nrm2(b);
  const double tol   = std::max(desc->relative_tolerance * bnorm, desc->absolute_tolerance);
  HIP_THROW(hipMemsetAsync(x, 0, n * sizeof(double), s));
  struct Events
  {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events()
    {
      for (hipEvent_t x : e)
        if (x)
          (void)hipEventDestroy(x);
    }
  } ev;
  for (hipEvent_t &e : ev.e)
    HIP_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // orthogonalisation: delayed CGS2 (one reduction, two basis passes per
  // step; cycle_dcgs) for a linear preconditioner within the fused lengths,
  // else CGS2 (arnoldi.h).  GLS_GMRES_ORTHO = cgs2 / cgs3 (the explicit second
  // update and norm) / rocblas selects a reference form, dcgs-narrow the
  // narrow DCGS2 passes (tests)
  const std::string ortho = getenv("GLS_GMRES_ORTHO") ? getenv("GLS_GMRES_ORTHO") : "";
  const bool dcgs = (ortho.empty() || ortho == "dcgs-narrow") && linear && m + 1 < CGS_MAXJ;
  const bool wide = n % 2 == 0 && ortho != "dcgs-narrow";
  // w = A M^{-1} v_j
  auto apply = [&](int j) {
    precondition(zcol(j), vcol(j));
    vmult(k.w, zcol(j));
  };
  std::vector<double> col((size_t)m + 1);
  gls::GmresSpace     sp{
    [&](double beta) {
      const double sc = 1.0 / beta;
      RB_THROW(rocblas_dscal(h, (rocblas_int)n, &sc, vcol(0), 1));
    },
    // CGS2 Arnoldi step j: h = V^T w, w -= V h, twice; v_{j+1} = w / |w|
    [&](int j) {
      apply(j);
      cgs2_step(k.V, n, k.w, vcol(j + 1), k.dh, k.cpart, k.host + (j % 2) * HC,
                k.host_dev + (j % 2) * HC, HC, m, j, h, s, ev.e[j % 2], ortho == "rocblas",
                ortho == "cgs3");
    },
    [&](int j) {
      HIP_THROW(hipEventSynchronize(ev.e[j % 2]));
      return cgs2_column(k.host + (j % 2) * HC, m, j, col.data());
    },
    // x += Z y with kept directions, else x += M^{-1} (V y)
    [&](int jd, const double *y) {
      HIP_THROW(hipMemcpyAsync(k.dh, y, jd * sizeof(double), hipMemcpyHostToDevice, s));
      const double one = 1.0, zero = 0.0;
      if (jd > 0 && k.zkeep)
        RB_THROW(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, jd, &one, k.Zd,
                               (rocblas_int)n, k.dh, 1, &one, x, 1));
      else if (jd > 0)
        {
          RB_THROW(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, jd, &one, k.V,
                                 (rocblas_int)n, k.dh, 1, &zero, k.w, 1));
          precondition(k.z, k.w);
          RB_THROW(rocblas_daxpy(h, (rocblas_int)n, &one, k.z, 1, x, 1));
        }
    },
    // restart: the true residual r = b - A x into column 0
    [&] {
      vmult(vcol(0), x);
      hipLaunchKernelGGL(k_residual<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                         vcol(0), b, n);
      HIP_THROW(hipGetLastError());
      return nrm2(vcol(0));
    }};
  // r (in column 0 of V) = b - A x, x = 0
  HIP_THROW(hipMemcpyAsync(vcol(0), b, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  const int           max_it = desc->max_iterations;
  auto dcgs_cycle = [&](double beta, gls::GmresRun &r, double *y) {
    return cycle_dcgs(k, s, ev.e, wide, apply, beta, tol, max_it, r, y);
  };
  const gls::GmresRun run = dcgs ? gls::gmres_restarted(sp, m, bnorm, tol, max_it, dcgs_cycle) :
                                   gls::gmres_restarted(sp, m, bnorm, tol, max_it);
  op->stage.finish_out(x_, s);
  HIP_THROW(hipStreamSynchronize(s));
  // a resident smoothing sweep that stalled poisoned a V-cycle with NaN:
  // reported here (the multigrid continues with one launch per step)
  if (mg)
    gls::mg_check_stall(mg, "gls_gmres_solve");
  if (result)
    {
      result->n_iterations     = run.iterations;
      result->n_restarts       = run.restarts;
      result->initial_residual = bnorm;
      result->final_residual   = run.residual;
      result->tolerance        = tol;
      result->converged        = run.converged ? 1 : 0;
    }
  if (!run.converged)
    throw std::runtime_error("gls_gmres_solve: no convergence in " +
                             std::to_string(run.iterations) + " iterations (residual " +
                             std::to_string(run.residual) + " > " + std::to_string(tol) + ")");
  GLS_CATCH
}

extern "C" glsStatus
gls_gmres_solve(glsOp op, glsMG mg, const glsGMRESDesc *desc, void *x_, const void *b_,
                glsGMRESResult *result, void *stream)
{
  return gmres_solve(op, GLS_PREC_MG, mg, desc, x_, b_, result, stream);
}

extern "C" glsStatus
gls_gmres_solve_prec(glsOp op, int kind, void *prec, const glsGMRESDesc *desc, void *x_,
                     const void *b_, glsGMRESResult *result, void *stream)
{
  return gmres_solve(op, kind, prec, desc, x_, b_, result, stream);
}
