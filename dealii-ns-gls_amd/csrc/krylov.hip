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
// device.  Up to 31 basis columns the passes are this file's fused kernels
// (cgs.h: dots; update + dots + norm; the second update folded into the
// normalisation), beyond that rocBLAS GEMVs; the operator apply and the
// V-cycle are this library's own kernels.
#include "../../include/gls_op.h"
#include "cgs.h"
#include "common.h"
#include "trace.h"
#include "op_internal.h"

#include <rocblas/rocblas.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

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

// r = b - r (r holds A x on entry)
__global__ void
k_residual(double *__restrict__ r, const double *__restrict__ b, int64_t n)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n)
    r[i] = b[i] - r[i];
}

dim3
grid1(int64_t n)
{
  return dim3((unsigned)((n + 255) / 256));
}

void
check(glsStatus st, const char *what)
{
  if (st != 0)
    throw std::runtime_error(std::string(what) + ": " + gls_last_error());
}

} // namespace

namespace gls
{
// csrc/ilu.hip: gls_ilu_vmult on the factor's device without the scope
void    ilu_apply(glsILU_ *ilu, double *dst, const double *src, hipStream_t st);
int64_t ilu_size(const glsILU_ *ilu);
} // namespace gls

// the solver behind gls_gmres_solve (kind GLS_PREC_MG, prec a glsMG or null:
// identity) and gls_gmres_solve_prec
static glsStatus
gmres_solve(glsOp op, int kind, void *prec, const glsGMRESDesc *desc, void *x_, const void *b_,
            glsGMRESResult *result, void *stream)
{
  GLS_TRY
  gls::Section sec_("gmres::solve", (hipStream_t)stream);
  if (!op || !desc || !x_ || !b_)
    throw std::runtime_error("gls_gmres_solve: null argument");
  if (kind != GLS_PREC_MG && kind != GLS_PREC_ILU && kind != GLS_PREC_AMG)
    throw std::runtime_error("gls_gmres_solve_prec: unknown preconditioner kind");
  if (kind != GLS_PREC_MG && !prec)
    throw std::runtime_error("gls_gmres_solve_prec: null preconditioner");
  const glsMG  mg  = kind == GLS_PREC_MG ? (glsMG)prec : nullptr;
  const glsILU ilu = kind == GLS_PREC_ILU ? (glsILU)prec : nullptr;
  const glsAMG amg = kind == GLS_PREC_AMG ? (glsAMG)prec : nullptr;
  if (op->prec != GLS_F64)
    throw std::runtime_error("gls_gmres_solve: the outer operator must be FP64 "
                             "(LinearSolverGMRES works on VectorType<double>)");
  if (op->n_owned_dofs != op->n_dofs)
    throw std::runtime_error("gls_gmres_solve: single-domain operators only (a partitioned "
                             "solve needs all-reduced dots)");
  if (desc->max_n_tmp_vectors < 3)
    throw std::runtime_error("gls_gmres_solve: max_n_tmp_vectors must be >= 3");
  if (mg)
    gls::mg_check_outer(mg, op); // FP64 outer vectors of op's size, set up
  // ILU / AMG of gls_op_system_matrix: its rows are the node-major dofs the
  // Krylov vectors hold on the device (the caller layout is staged at the
  // solve's ends), so the factor applies to them as they are
  if (ilu && gls::ilu_size(ilu) != op->n_dofs)
    throw std::runtime_error("gls_gmres_solve_prec: the ILU is not of the operator's size");
  if (amg)
    {
      int     nl = 0;
      int64_t sizes[64];
      check(gls_amg_info(amg, &nl, nullptr, nullptr, nullptr), "gls_amg_info");
      if (nl < 1 || nl > 64)
        throw std::runtime_error("gls_gmres_solve_prec: AMG hierarchy out of range");
      check(gls_amg_info(amg, &nl, sizes, nullptr, nullptr), "gls_amg_info");
      if (sizes[0] != op->n_dofs)
        throw std::runtime_error("gls_gmres_solve_prec: the AMG is not of the operator's size");
    }
  // the operator's device for the whole solve (staging buffers included),
  // the caller's current device restored on return
  gls::DeviceScope dev(op->device);
  hipStream_t    s = (hipStream_t)stream;
  const int64_t  n = op->n_dofs;
  // deal.II SolverGMRES restarts after max_n_tmp_vectors - 2 iterations
  const int      m = desc->max_n_tmp_vectors - 2;
  // caller layout (host memory / dof numbering): b staged in, x written to
  // a device buffer and copied / permuted back at the end
  const double  *b = (const double *)op->stage.in_vec(b_, 1, s);
  double        *x = (double *)op->stage.out_vec(x_);
  // the operator's device, its rocBLAS handle, and the Krylov workspace
  // [V (m+1) n | w n | z n | dh 2 (m+1)] kept on the operator and grown on
  // demand (a hipMalloc/hipFree of the basis per solve synchronises the
  // device and costs more than the solve's setup)
  rocblas_handle h  = blas_handle(op->device, s);
  // dh: the two CGS passes' coefficients and |w| (HC values, one D2H copy),
  // or a DCGS2 step's record (DCGS_D values)
  const int      HC = std::max(2 * (m + 1) + 1, DCGS_D);
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
  bool zkeep = !mg || gls::mg_is_linear(mg);
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
  struct View
  {
    double *p;
    double *
    d() const
    {
      return p;
    }
  };
  double    *wsd = (double *)op->gmres_ws;
  // the pinned Hessenberg buffers as the device sees them (k_cgs_unit writes
  // them directly)
  double *host_dev = nullptr;
  HIP_THROW(hipHostGetDevicePointer((void **)&host_dev, op->gmres_host, 0));
  const View V{wsd}, w{wsd + (size_t)(m + 1) * n}, z{wsd + (size_t)(m + 2) * n},
    dh{wsd + (size_t)(m + 3) * n}, cpart{wsd + (size_t)(m + 3) * n + HC};
  auto vcol = [&](int j) { return V.d() + (size_t)j * n; };
  // Z after the CGS partials (ws layout [V | w | z | dh | cpart | Z])
  double *Zd   = wsd + z_off;
  auto    zcol = [&](int j) { return zkeep ? Zd + (size_t)j * n : z.d(); };
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
  auto nrm2 = [&](const double *v) {
    double r = 0;
    RB_THROW(rocblas_dnrm2(h, (rocblas_int)n, v, 1, &r));
    return r;
  };
  if (n > (int64_t)0x7fffffff)
    throw std::runtime_error("gls_gmres_solve: vector too long for 32-bit rocBLAS sizes");

  // solver_l.cc:52-53: tolerance = max(rel * |b|, abs); dst = 0 (:66)
  const double bnorm = nrm2(b);
  const double tol   = std::max(desc->relative_tolerance * bnorm, desc->absolute_tolerance);
  HIP_THROW(hipMemsetAsync(x, 0, n * sizeof(double), s));

  std::vector<double> H((size_t)(m + 1) * m), g(m + 1), cs(m), sn(m), y(m);
  int    it    = 0;
  double res   = bnorm; // x = 0: r = b
  bool   conv  = res <= tol;
  int    n_rst = 0;
  // Arnoldi step j, enqueued only: w = A M^{-1} v_j, CGS2 (h = V^T w;
  // w -= V h; twice), |w| on the device, the Hessenberg column to pinned
  // host buffer j % 2 (event ev[j % 2]), v_{j+1} = w / |w|
  struct Events
  {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events()
    {
      for (hipEvent_t x : e)
        if (x)
          (void)hipEventDestroy(x);
    }
  } evs;
  hipEvent_t *ev = evs.e;
  for (int i = 0; i < 2; ++i)
    HIP_THROW(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
  // orthogonalisation: delayed CGS2 (one reduction, two basis passes per
  // step; below) for a linear preconditioner within the fused lengths, else
  // CGS2 (three fused passes, the second update folded into a Pythagorean
  // normalisation), rocBLAS GEMVs beyond 31 columns.  GLS_GMRES_ORTHO =
  // cgs2 / cgs3 (the explicit second update and norm) / rocblas selects a
  // reference form (tests)
  const std::string ortho        = getenv("GLS_GMRES_ORTHO") ? getenv("GLS_GMRES_ORTHO") : "";
  const bool        force_rocblas    = ortho == "rocblas";
  const bool        force_three_pass = ortho == "cgs3";
  const bool        dcgs = (ortho.empty() || ortho == "dcgs-narrow") &&
                    (!mg || gls::mg_is_linear(mg)) && m + 1 < CGS_MAXJ;
  auto              arnoldi       = [&](int j) {
    precondition(zcol(j), vcol(j));
    {
      gls::Section sc("ns::vmult", s);
      gls::op_vmult_device(op, w.d(), zcol(j), s);
    }
    double *hn        = dh.d() + 2 * (m + 1);
    bool    unit_done = false;
    if (j + 1 < CGS_MAXJ && !force_rocblas && !force_three_pass)
      {
        // fused CGS2: dots; update + dots + |w|^2; the second update folded
        // into the normalisation (k_cgs_unit, norm by Pythagoras)
        const int J = j + 1;
        hipLaunchKernelGGL(k_cgs_dots, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(), J,
                           (const double *)w.d(), cpart.d(), n, n);
        hipLaunchKernelGGL(k_cgs_finish, dim3(J), dim3(256), 0, s, (const double *)cpart.d(),
                           dh.d(), 0);
        hipLaunchKernelGGL(k_cgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(),
                           J, (const double *)dh.d(), w.d(), cpart.d(), n, n, n, 2);
        hipLaunchKernelGGL(k_cgs_finish, dim3(J + 1), dim3(256), 0, s, (const double *)cpart.d(),
                           dh.d() + (m + 1), 0);
        hipLaunchKernelGGL(k_cgs_unit, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(), J,
                           (const double *)(dh.d() + (m + 1)), (const double *)w.d(), vcol(j + 1),
                           hn, n, n, (const double *)dh.d(), host_dev + (j % 2) * HC, HC,
                           2 * (m + 1));
        HIP_THROW(hipGetLastError());
        unit_done = true;
      }
    else if (j + 1 <= CGS_MAXJ && !force_rocblas)
      {
        // fused CGS2: dots, update + dots, update + norm (three basis passes)
        const int J = j + 1;
        hipLaunchKernelGGL(k_cgs_dots, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(), J,
                           (const double *)w.d(), cpart.d(), n, n);
        hipLaunchKernelGGL(k_cgs_finish, dim3(J), dim3(256), 0, s, (const double *)cpart.d(),
                           dh.d(), 0);
        hipLaunchKernelGGL(k_cgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(),
                           J, (const double *)dh.d(), w.d(), cpart.d(), n, n, n, 0);
        hipLaunchKernelGGL(k_cgs_finish, dim3(J), dim3(256), 0, s, (const double *)cpart.d(),
                           dh.d() + (m + 1), 0);
        hipLaunchKernelGGL(k_cgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(),
                           J, (const double *)(dh.d() + (m + 1)), w.d(), cpart.d(), n, n, n, 1);
        hipLaunchKernelGGL(k_cgs_finish, dim3(1), dim3(256), 0, s, (const double *)cpart.d(), hn, 1);
        HIP_THROW(hipGetLastError());
      }
    else
      {
        const double one = 1.0, zero = 0.0, mone = -1.0;
        for (int pass = 0; pass < 2; ++pass)
          {
            double *hp = dh.d() + pass * (m + 1);
            RB_THROW(rocblas_dgemv(h, rocblas_operation_transpose, (rocblas_int)n, j + 1, &one,
                                   V.d(), (rocblas_int)n, w.d(), 1, &zero, hp, 1));
            RB_THROW(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, j + 1, &mone, V.d(),
                                   (rocblas_int)n, hp, 1, &one, w.d(), 1));
          }
        RB_THROW(rocblas_set_pointer_mode(h, rocblas_pointer_mode_device));
        RB_THROW(rocblas_dnrm2(h, (rocblas_int)n, w.d(), 1, hn));
        RB_THROW(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
      }
    if (!unit_done)
      HIP_THROW(hipMemcpyAsync(op->gmres_host + (j % 2) * HC, dh.d(), HC * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    HIP_THROW(hipEventRecord(ev[j % 2], s));
    if (!unit_done)
      hipLaunchKernelGGL(k_unit_col, grid1(n), dim3(256), 0, s, vcol(j + 1),
                         (const double *)w.d(), (const double *)hn, n);
    HIP_THROW(hipGetLastError());
  };
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
  // the wide DCGS2 passes (cgs.h: 8-wave blocks, 16-byte row pairs) for an
  // even row count; GLS_GMRES_ORTHO=dcgs-narrow keeps the round-5 passes
  const bool wide = n % 2 == 0 && ortho != "dcgs-narrow";
  auto dcgs_dots = [&](int J, const double *u, const double *wv) {
    if (wide)
      hipLaunchKernelGGL(k_dcgs_dots_wide, dim3(CGS_BLOCKS), dim3(DCGS_WIDE), 0, s,
                         (const double *)V.d(), J, u, wv, cpart.d(), n, n);
    else
      hipLaunchKernelGGL(k_dcgs_dots, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(), J,
                         u, wv, cpart.d(), n, n);
  };
  auto arnoldi_d = [&](int j) {
    precondition(zcol(j), vcol(j));
    {
      gls::Section sc("ns::vmult", s);
      gls::op_vmult_device(op, w.d(), zcol(j), s);
    }
    double *dd = dh.d();
    dcgs_dots(j, (const double *)vcol(j), (const double *)w.d());
    hipLaunchKernelGGL(k_dcgs_finish, dim3(DCGS_W), dim3(256), 0, s, (const double *)cpart.d(),
                       dd, j, -1, (double *)nullptr);
    if (wide)
      hipLaunchKernelGGL(k_dcgs_update_wide, dim3(CGS_BLOCKS), dim3(DCGS_WIDE), 0, s,
                         (const double *)V.d(), j, dd, vcol(j), (const double *)w.d(),
                         vcol(j + 1), cpart.d(), n, n);
    else
      hipLaunchKernelGGL(k_dcgs_update, dim3(CGS_BLOCKS), dim3(256), 0, s, (const double *)V.d(),
                         j, dd, vcol(j), (const double *)w.d(), vcol(j + 1), cpart.d(), n, n);
    hipLaunchKernelGGL(k_dcgs_finish, dim3(1), dim3(256), 0, s, (const double *)cpart.d(), dd, -1,
                       DCGS_W + 2, host_dev + (j % 2) * HC);
    HIP_THROW(hipGetLastError());
    HIP_THROW(hipEventRecord(ev[j % 2], s));
  };
  // raw (unrotated) Hessenberg, column major with m+1 rows, and R
  std::vector<double> Hr((size_t)(m + 1) * m), Rm((size_t)m * m);
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
        for (int k = 0; k < j; ++k)
          t -= HR(i, k) * sj[k];
        HR(i, j) = alpha > 0 ? t / alpha : 0.0;
      }
    HR(j + 1, j) = std::sqrt(nu > 0 ? nu : 0.0);
    for (int i = 0; i < j; ++i)
      RR(i, j) = sj[i];
    RR(j, j) = alpha;
  };
  // least squares min |g0 e_0 - H y| over the first jd columns (Givens QR of
  // a copy of the raw Hessenberg): the residual estimate, and y if asked
  std::vector<double> Hw((size_t)(m + 1) * m);
  auto lsq = [&](int jd, double g0, double *yout) {
    Hw = Hr;
    auto HW = [&](int i, int c) -> double & { return Hw[(size_t)c * (m + 1) + i]; };
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = g0;
    for (int j = 0; j < jd; ++j)
      {
        for (int i = 0; i < j; ++i)
          {
            const double t = cs[i] * HW(i, j) + sn[i] * HW(i + 1, j);
            HW(i + 1, j)   = -sn[i] * HW(i, j) + cs[i] * HW(i + 1, j);
            HW(i, j)       = t;
          }
        const double rr = std::hypot(HW(j, j), HW(j + 1, j));
        cs[j]           = rr > 0 ? HW(j, j) / rr : 1.0;
        sn[j]           = rr > 0 ? HW(j + 1, j) / rr : 0.0;
        HW(j, j)        = rr;
        HW(j + 1, j)    = 0;
        g[j + 1]        = -sn[j] * g[j];
        g[j]            = cs[j] * g[j];
      }
    if (yout)
      for (int i = jd - 1; i >= 0; --i)
        {
          double t = g[i];
          for (int c = i + 1; c < jd; ++c)
            t -= HW(i, c) * yout[c];
          yout[i] = t / HW(i, i);
        }
    return std::fabs(g[jd]);
  };
  // one DCGS2 cycle from the tentative u_0 = r / beta in column 0: the
  // update coefficients (R^{-1} y with kept directions, else y) into y;
  // returns the number of columns
  auto cycle_dcgs = [&](double beta) {
    std::fill(Hr.begin(), Hr.end(), 0.0);
    std::fill(Rm.begin(), Rm.end(), 0.0);
    double g0      = beta;
    int    jd      = 0;
    bool   ahead   = false; // step jd enqueued (its record finishes column jd-1)
    arnoldi_d(0);
    for (int j = 0; j < m && it < desc->max_iterations; ++j)
      {
        ahead = j + 1 < m && it + 1 < desc->max_iterations;
        if (ahead)
          arnoldi_d(j + 1);
        HIP_THROW(hipEventSynchronize(ev[j % 2]));
        const double *rc = op->gmres_host + (j % 2) * HC;
        absorb(j, rc);
        if (j == 0)
          g0 = beta * rc[DCGS_W]; // r = beta u_0 = beta alpha_0 q_0
        ++it;
        ++jd;
        res = lsq(jd, g0, nullptr);
        if (res <= tol || HR(j + 1, j) == 0)
          break;
      }
    // column jd-1's re-orthogonalisation terms: the record of the step run
    // ahead, or the dots of u_jd alone
    if (ahead)
      {
        HIP_THROW(hipEventSynchronize(ev[jd % 2]));
        const double *rc = op->gmres_host + (jd % 2) * HC;
        for (int i = 0; i < jd; ++i)
          HR(i, jd - 1) += rc[i];
        HR(jd, jd - 1) = rc[DCGS_W];
      }
    else
      {
        double *dd = dh.d();
        dcgs_dots(jd, (const double *)vcol(jd), (const double *)nullptr);
        hipLaunchKernelGGL(k_dcgs_finish, dim3(DCGS_W), dim3(256), 0, s,
                           (const double *)cpart.d(), dd, jd, -1, (double *)nullptr);
        HIP_THROW(hipGetLastError());
        std::vector<double> rc(DCGS_W);
        HIP_THROW(hipMemcpyAsync(rc.data(), dd, DCGS_W * sizeof(double), hipMemcpyDeviceToHost, s));
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
    res = lsq(jd, g0, y.data());
    if (zkeep) // t = R^{-1} y
      for (int i = jd - 1; i >= 0; --i)
        {
          double t = y[i];
          for (int c = i + 1; c < jd; ++c)
            t -= RR(i, c) * y[c];
          y[i] = t / RR(i, i);
        }
    return jd;
  };

  // r (in column 0 of V) = b - A x
  HIP_THROW(hipMemcpyAsync(vcol(0), b, n * sizeof(double), hipMemcpyDeviceToDevice, s));
  while (!conv && it < desc->max_iterations)
    {
      const double beta = res;
      {
        const double sc = 1.0 / beta;
        RB_THROW(rocblas_dscal(h, (rocblas_int)n, &sc, vcol(0), 1));
      }
      std::fill(g.begin(), g.end(), 0.0);
      g[0]   = beta;
      int jd = 0; // columns of this cycle
      if (dcgs)
        jd = cycle_dcgs(beta);
      else
        {
      // software pipeline: step j + 1 is enqueued before the host waits for
      // step j's Hessenberg column, so the device never idles through the
      // host round trip; when step j converges, the enqueued step j + 1 runs
      // to completion and is discarded (its basis column is never used)
      if (m > 0)
        arnoldi(0);
      for (int j = 0; j < m && it < desc->max_iterations; ++j)
        {
          if (j + 1 < m && it + 1 < desc->max_iterations)
            arnoldi(j + 1);
          HIP_THROW(hipEventSynchronize(ev[j % 2]));
          const double *hc = op->gmres_host + (j % 2) * HC;
          const double  hn = hc[2 * (m + 1)];
          double       *Hj = &H[(size_t)j * (m + 1)];
          for (int i = 0; i <= j; ++i)
            Hj[i] = hc[i] + hc[(m + 1) + i];
          Hj[j + 1] = hn;
          // Givens rotations on the new Hessenberg column
          for (int i = 0; i < j; ++i)
            {
              const double t = cs[i] * Hj[i] + sn[i] * Hj[i + 1];
              Hj[i + 1]      = -sn[i] * Hj[i] + cs[i] * Hj[i + 1];
              Hj[i]          = t;
            }
          const double rr = std::hypot(Hj[j], Hj[j + 1]);
          cs[j]           = rr > 0 ? Hj[j] / rr : 1.0;
          sn[j]           = rr > 0 ? Hj[j + 1] / rr : 0.0;
          Hj[j]           = rr;
          Hj[j + 1]       = 0;
          g[j + 1]        = -sn[j] * g[j];
          g[j]            = cs[j] * g[j];
          ++it;
          ++jd;
          res = std::fabs(g[j + 1]);
          // deal.II checks the GMRES residual estimate every iteration; a
          // lucky breakdown (hn == 0) means the estimate is exact
          if (res <= tol || hn == 0)
            break;
        }
      // y = H^{-1} g (upper triangular), x += M^{-1} V y
      for (int i = jd - 1; i >= 0; --i)
        {
          double t = g[i];
          for (int c = i + 1; c < jd; ++c)
            t -= H[(size_t)c * (m + 1) + i] * y[c];
          y[i] = t / H[(size_t)i * (m + 1) + i];
        }
        }
      HIP_THROW(hipMemcpyAsync(dh.d(), y.data(), jd * sizeof(double), hipMemcpyHostToDevice, s));
      if (jd > 0)
        {
          const double one = 1.0, zero = 0.0;
          if (zkeep)
            RB_THROW(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, jd, &one, Zd,
                                   (rocblas_int)n, dh.d(), 1, &one, x, 1));
          else
            {
              RB_THROW(rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)n, jd, &one, V.d(),
                                     (rocblas_int)n, dh.d(), 1, &zero, w.d(), 1));
              precondition(z.d(), w.d());
              RB_THROW(rocblas_daxpy(h, (rocblas_int)n, &one, z.d(), 1, x, 1));
            }
        }
      conv = res <= tol;
      if (conv || it >= desc->max_iterations)
        break;
      // restart: true residual r = b - A x into column 0
      ++n_rst;
      {
        gls::Section sc("ns::vmult", s);
        gls::op_vmult_device(op, vcol(0), x, s);
      }
      hipLaunchKernelGGL(k_residual, grid1(n), dim3(256), 0, s, vcol(0), b, n);
      HIP_THROW(hipGetLastError());
      res  = nrm2(vcol(0));
      conv = res <= tol;
    }
  op->stage.finish_out(x_, s);
  HIP_THROW(hipStreamSynchronize(s));
  // a resident smoothing sweep that stalled poisoned a V-cycle with NaN:
  // reported here (the multigrid continues with one launch per step)
  if (mg)
    gls::mg_check_stall(mg, "gls_gmres_solve");
  if (result)
    {
      result->n_iterations   = it;
      result->n_restarts     = n_rst;
      result->initial_residual = bnorm;
      result->final_residual = res;
      result->tolerance      = tol;
      result->converged      = conv ? 1 : 0;
    }
  if (!conv)
    throw std::runtime_error("gls_gmres_solve: no convergence in " + std::to_string(it) +
                             " iterations (residual " + std::to_string(res) + " > " +
                             std::to_string(tol) + ")");
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
