// ilu.hip — the device side of the ILU(k) preconditioner (gls_ilu_*):
// dst = U^-1 L^-1 src on FP64 device vectors over the level schedule of
// csrc/ilu_plan.cc (TrilinosWrappers::PreconditionILU::vmult; the reference
// applies Ifpack's sequential solves, preconditioner.cc:5-28).
//
// Storage: each factor's rows level by level (position p holds row order[p],
// its off-diagonal entries rp[p] .. rp[p + 1], columns in the original
// numbering), so the work vector is never permuted.  The work vector is dst
// itself: the forward solve reads src and writes y into dst, the backward
// solve overwrites y_r by (y_r - sum_j u_rj x_j) / u_rr with the stored
// reciprocal pivot, so there is no copy pass and no temporary.
//
// Rows: G lanes per row (a power of two <= 64, one value per factor); a
// group sums its partial dot by xor shuffles in a fixed order and there are
// no atomics, so the result depends on neither the launch shapes nor the
// run: chained and unchained applies are bitwise equal.
//
// Ordering: a wide level is one grid launch over its rows; a run of narrow
// levels is one launch of ONE workgroup (ILU_CHAIN_THREADS) that walks the
// levels with __syncthreads() between them.  Order across workgroups comes
// from the launch order on the stream only: no flags, no waits, no grid
// barrier.  Inside a chain other waves of the same workgroup produce the
// entries a row reads, so the work vector is a plain (non-const, non-
// restrict) pointer read by per-lane vector loads behind the barrier; the
// read-only factor arrays alone are const __restrict__.
//
// The numeric factorisation on the device (gls_ilu_refactor_device,
// gls_ilu_create_device) is csrc/ilu_factor.hip; the object the two files
// share is in csrc/ilu_internal.h.
#include "ilu_internal.h"

#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace gls
{
namespace
{
// one row at scheduled position p; every lane of the group calls it
template <int G, bool LOWER>
__device__ __forceinline__ void
ilu_row(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
        const double *__restrict__ v, const int32_t *__restrict__ order,
        const double *__restrict__ dinv, const double *__restrict__ src, double *x, int32_t p,
        int lane)
{
  double        s  = 0;
  const int32_t k1 = rp[p + 1];
  for (int32_t k = rp[p] + lane; k < k1; k += G)
    s += v[k] * x[ci[k]];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1)
    s += __shfl_xor(s, o);
  if (lane == 0)
    {
      const int32_t r = order[p];
      if (LOWER)
        x[r] = src[r] - s;
      else
        x[r] = (x[r] - s) * dinv[r];
    }
}

// a wide level: positions [p0, p1), one group per row
template <int G, bool LOWER>
__global__ void __launch_bounds__(ILU_WIDE_THREADS)
  k_ilu_level(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
              const double *__restrict__ v, const int32_t *__restrict__ order,
              const double *__restrict__ dinv, const double *__restrict__ src, double *x,
              int32_t p0, int32_t p1)
{
  const int64_t p    = (int64_t)p0 + ((int64_t)blockIdx.x * ILU_WIDE_THREADS + threadIdx.x) / G;
  const int     lane = threadIdx.x & (G - 1);
  if (p < p1) // uniform over a group
    ilu_row<G, LOWER>(rp, ci, v, order, dinv, src, x, (int32_t)p, lane);
}

// a chain: levels [l0, l1) by one workgroup, a barrier after each
template <int G, bool LOWER>
__global__ void __launch_bounds__(ILU_CHAIN_THREADS)
  k_ilu_chain(const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
              const double *__restrict__ v, const int32_t *__restrict__ order,
              const double *__restrict__ dinv, const int32_t *__restrict__ lev_ptr,
              const double *__restrict__ src, double *x, int32_t l0, int32_t l1)
{
  const int     lane = threadIdx.x & (G - 1);
  const int32_t g    = threadIdx.x / G;
  for (int32_t l = l0; l < l1; ++l)
    {
      const int32_t p1 = lev_ptr[l + 1];
      for (int32_t p = lev_ptr[l] + g; p < p1; p += ILU_CHAIN_THREADS / G)
        ilu_row<G, LOWER>(rp, ci, v, order, dinv, src, x, p, lane);
      __syncthreads(); // the level's rows are written and visible to the next
    }
}

template <typename T>
void
upload(T **d, const std::vector<T> &h)
{
  if (!*d)
    HIP_THROW(hipMalloc((void **)d, std::max<size_t>(1, h.size()) * sizeof(T)));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

void
upload_tri(DevTri &D, const IluTri &T, bool values_only)
{
  if (!values_only)
    {
      upload(&D.rp, T.rp);
      upload(&D.ci, T.ci);
      upload(&D.order, T.order);
      upload(&D.lev_ptr, T.lev_ptr);
    }
  upload(&D.v, T.v);
}

void
free_tri(DevTri &D)
{
  (void)hipFree(D.rp), (void)hipFree(D.ci), (void)hipFree(D.order), (void)hipFree(D.lev_ptr),
    (void)hipFree(D.v);
  D = DevTri{};
}

double
wall_ms()
{
  using clk = std::chrono::steady_clock;
  return std::chrono::duration<double, std::milli>(clk::now().time_since_epoch()).count();
}

template <int G, bool LOWER>
void
run_tri(const IluTri &T, const DevTri &D, const double *dinv, const double *src, double *x,
        hipStream_t st)
{
  constexpr int rows_per_block = ILU_WIDE_THREADS / G;
  for (const IluLaunch &q : T.launches)
    if (q.chain)
      hipLaunchKernelGGL((k_ilu_chain<G, LOWER>), dim3(1), dim3(ILU_CHAIN_THREADS), 0, st, D.rp,
                         D.ci, D.v, D.order, dinv, D.lev_ptr, src, x, q.lev0, q.lev1);
    else
      hipLaunchKernelGGL((k_ilu_level<G, LOWER>),
                         dim3((unsigned)((q.pos1 - q.pos0 + rows_per_block - 1) / rows_per_block)),
                         dim3(ILU_WIDE_THREADS), 0, st, D.rp, D.ci, D.v, D.order, dinv, src, x,
                         q.pos0, q.pos1);
}

template <int G>
void
run_both(const IluPlan &P, const DevTri &L, const DevTri &U, const double *dinv,
         const double *src, double *x, hipStream_t st)
{
  run_tri<G, true>(P.L, L, dinv, src, x, st);
  run_tri<G, false>(P.U, U, dinv, src, x, st);
}

// the rows of one exported factor in the original order
void
export_factor(const IluPlan &P, int which, int64_t *nnz, int64_t *row_ptr, int64_t *cols,
              double *vals)
{
  int64_t c = 0;
  for (int64_t i = 0; i < P.n; ++i)
    {
      if (row_ptr)
        row_ptr[i] = c;
      const int64_t k0 = which == 0 ? P.rp[(size_t)i] : P.diag[(size_t)i];
      const int64_t k1 = which == 0 ? P.diag[(size_t)i] : P.rp[(size_t)i + 1];
      for (int64_t k = k0; k < k1; ++k, ++c)
        {
          if (cols)
            cols[c] = P.ci[(size_t)k];
          if (vals)
            vals[c] = P.val[(size_t)k];
        }
    }
  if (row_ptr)
    row_ptr[P.n] = c;
  if (nnz)
    *nnz = c;
}
} // namespace
} // namespace gls

namespace gls
{
// the internal form of gls_ilu_vmult for the multigrid, the AMG and GMRES
void
ilu_apply(glsILU_ *ilu, double *dst, const double *src, hipStream_t st)
{
  if (dst == src)
    throw std::runtime_error("gls_ilu_vmult: dst and src must be distinct");
  if (!ilu->valid)
    throw std::runtime_error("gls_ilu_vmult: the last refactorisation failed");
  const IluPlan &P = ilu->plan;
  switch (P.group)
    {
      case 1: run_both<1>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 2: run_both<2>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 4: run_both<4>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 8: run_both<8>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 16: run_both<16>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 32: run_both<32>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      case 64: run_both<64>(P, ilu->L, ilu->U, ilu->dinv, src, dst, st); break;
      default: throw std::runtime_error("gls_ilu_vmult: no kernel for this group width");
    }
  HIP_THROW(hipGetLastError());
}

int64_t
ilu_size(const glsILU_ *ilu)
{
  return ilu->plan.n;
}
} // namespace gls

extern "C" {

glsStatus
gls_ilu_create(int64_t n, const int64_t *row_ptr, const int64_t *cols, const double *vals,
               const glsILUParams *prm, glsILU *out)
{
  GLS_TRY
  using namespace gls;
  if (!prm || !out)
    throw std::runtime_error("gls_ilu_create: null argument");
  IluParams p;
  p.fill_level = prm->fill_level, p.atol = prm->atol, p.rtol = prm->rtol;
  auto *ilu = new glsILU_();
  struct Guard
  {
    glsILU_ *p;
    ~Guard()
    {
      if (p)
        gls_ilu_destroy(p);
    }
  } guard{ilu};
  ilu->plan = ilu_make_plan(n, row_ptr, cols, vals, p, ilu_tuning_from_env());
  HIP_THROW(hipGetDevice(&ilu->device));
  const double t0 = wall_ms();
  upload_tri(ilu->L, ilu->plan.L, false);
  upload_tri(ilu->U, ilu->plan.U, false);
  upload(&ilu->dinv, ilu->plan.dinv);
  ilu->upload_ms = wall_ms() - t0;
  ilu->valid     = true;
  guard.p        = nullptr;
  *out           = ilu;
  GLS_CATCH
}

glsStatus
gls_ilu_refactor(glsILU ilu, const double *vals)
{
  GLS_TRY
  using namespace gls;
  if (!ilu || !vals)
    throw std::runtime_error("gls_ilu_refactor: null argument");
  DeviceScope ds(ilu->device);
  ilu->valid     = false; // host and device values disagree until the upload below
  ilu->on_device = false;
  ilu_refactor(ilu->plan, vals);
  ilu->plan.symbolic_ms = 0.0;
  // applies in flight on any stream still read the old values
  HIP_THROW(hipDeviceSynchronize());
  const double t0 = wall_ms();
  upload_tri(ilu->L, ilu->plan.L, true);
  upload_tri(ilu->U, ilu->plan.U, true);
  upload(&ilu->dinv, ilu->plan.dinv);
  ilu->upload_ms = wall_ms() - t0;
  ilu->valid     = true;
  GLS_CATCH
}

void
gls_ilu_destroy(glsILU ilu)
{
  if (!ilu)
    return;
  gls::free_tri(ilu->L), gls::free_tri(ilu->U);
  gls::ilu_factor_release(ilu);
  (void)hipFree(ilu->dinv);
  delete ilu;
}

glsStatus
gls_ilu_refactor_device(glsILU ilu, const double *d_vals, void *stream)
{
  GLS_TRY
  if (!ilu || !d_vals)
    throw std::runtime_error("gls_ilu_refactor_device: null argument");
  gls::DeviceScope ds(ilu->device);
  gls::ilu_factor_device(ilu, d_vals, (hipStream_t)stream);
  ilu->plan.symbolic_ms = 0.0;
  GLS_CATCH
}

glsStatus
gls_ilu_create_device(const glsDeviceCSR *A, const glsILUParams *prm, void *stream, glsILU *out)
{
  GLS_TRY
  using namespace gls;
  if (!A || !prm || !out || !A->row_ptr || !A->cols || !A->vals)
    throw std::runtime_error("gls_ilu_create_device: null argument");
  if (A->n <= 0 || A->nnz < 0)
    throw std::runtime_error("gls_ilu_create_device: empty matrix");
  IluParams p;
  p.fill_level = prm->fill_level, p.atol = prm->atol, p.rtol = prm->rtol;
  hipStream_t st = (hipStream_t)stream;
  // the pattern to the host, once (the assembly on `stream` comes first)
  std::vector<int64_t> rp((size_t)A->n + 1), ci((size_t)A->nnz);
  std::vector<int32_t> ci32((size_t)A->nnz);
  HIP_THROW(hipMemcpyAsync(rp.data(), A->row_ptr, rp.size() * sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
  if (A->nnz > 0)
    HIP_THROW(hipMemcpyAsync(ci32.data(), A->cols, ci32.size() * sizeof(int32_t),
                             hipMemcpyDeviceToHost, st));
  HIP_THROW(hipStreamSynchronize(st));
  if (rp[(size_t)A->n] != A->nnz)
    throw std::runtime_error("gls_ilu_create_device: row_ptr[n] != nnz");
  std::copy(ci32.begin(), ci32.end(), ci.begin());
  auto *ilu = new glsILU_();
  struct Guard
  {
    glsILU_ *p;
    ~Guard()
    {
      if (p)
        gls_ilu_destroy(p);
    }
  } guard{ilu};
  ilu->plan = ilu_make_symbolic(A->n, rp.data(), ci.data(), p, ilu_tuning_from_env());
  HIP_THROW(hipGetDevice(&ilu->device));
  upload_tri(ilu->L, ilu->plan.L, false); // the schedule; the values are written on the device
  upload_tri(ilu->U, ilu->plan.U, false);
  upload(&ilu->dinv, ilu->plan.dinv);
  ilu_factor_device(ilu, A->vals, st);
  guard.p = nullptr;
  *out    = ilu;
  GLS_CATCH
}

glsStatus
gls_ilu_factor_info(glsILU ilu, glsILUFactorInfo *info)
{
  GLS_TRY
  if (!ilu || !info)
    throw std::runtime_error("gls_ilu_factor_info: null argument");
  const gls::IluPlan &P = ilu->plan;
  std::memset(info, 0, sizeof(*info));
  info->levels   = (int)P.L.lev_ptr.size() - 1;
  info->launches = (int)P.factor_launches.size();
  for (const gls::IluLaunch &q : P.factor_launches)
    info->chains += q.chain;
  info->narrow = P.factor_narrow, info->group = P.factor_group, info->rows = P.factor_rows;
  info->chain       = P.tuning.factor_chain;
  info->max_row     = P.max_row;
  info->max_row_limit = gls::ILU_FACTOR_MAX_ROW;
  info->device      = ilu->on_device ? 1 : 0;
  info->factor_ms   = ilu->on_device ? ilu->factor_kernels_ms : 0.0;
  GLS_CATCH
}

glsStatus
gls_ilu_vmult(glsILU ilu, double *dst, const double *src, void *stream)
{
  GLS_TRY
  if (!ilu || !dst || !src)
    throw std::runtime_error("gls_ilu_vmult: null argument");
  gls::DeviceScope ds(ilu->device);
  gls::ilu_apply(ilu, dst, src, (hipStream_t)stream);
  GLS_CATCH
}

glsStatus
gls_ilu_info(glsILU ilu, glsILUInfo *info)
{
  GLS_TRY
  if (!ilu || !info)
    throw std::runtime_error("gls_ilu_info: null argument");
  const gls::IluPlan &P = ilu->plan;
  std::memset(info, 0, sizeof(*info));
  info->n = P.n, info->nnz_a = P.nnz_a;
  info->nnz_l = (int64_t)P.L.ci.size(), info->nnz_u = (int64_t)P.U.ci.size() + P.n;
  info->levels_l = (int)P.L.lev_ptr.size() - 1, info->levels_u = (int)P.U.lev_ptr.size() - 1;
  info->launches_l = (int)P.L.launches.size(), info->launches_u = (int)P.U.launches.size();
  info->max_level_rows = std::max(P.L.max_level_rows, P.U.max_level_rows);
  info->group = P.group, info->narrow = P.narrow, info->chain = P.tuning.chain;
  info->min_pivot = P.min_pivot;
  info->symbolic_ms = P.symbolic_ms, info->numeric_ms = P.numeric_ms;
  info->upload_ms = ilu->upload_ms;
  GLS_CATCH
}

glsStatus
gls_ilu_factors(glsILU ilu, int which, int64_t *nnz, int64_t *row_ptr, int64_t *cols,
                double *vals)
{
  GLS_TRY
  if (!ilu || !nnz || which < 0 || which > 1)
    throw std::runtime_error("gls_ilu_factors: bad argument");
  if (!ilu->valid)
    throw std::runtime_error("gls_ilu_factors: the last refactorisation failed");
  if (ilu->on_device && vals) // the values of a device factorisation live there
    {
      gls::DeviceScope ds(ilu->device);
      gls::ilu_factor_download(ilu);
    }
  gls::export_factor(ilu->plan, which, nnz, row_ptr, cols, vals);
  GLS_CATCH
}

glsStatus
gls_ilu_host_factor(int64_t n, const int64_t *row_ptr, const int64_t *cols, const double *vals,
                    const glsILUParams *prm, glsILUHostFactor *out)
{
  GLS_TRY
  using namespace gls;
  if (!prm || !out)
    throw std::runtime_error("gls_ilu_host_factor: null argument");
  IluParams p;
  p.fill_level = prm->fill_level, p.atol = prm->atol, p.rtol = prm->rtol;
  const IluPlan P = ilu_make_plan(n, row_ptr, cols, vals, p, ilu_tuning_from_env());
  out->n          = P.n;
  out->levels_l = (int)P.L.lev_ptr.size() - 1, out->levels_u = (int)P.U.lev_ptr.size() - 1;
  out->launches_l = (int)P.L.launches.size(), out->launches_u = (int)P.U.launches.size();
  out->group = P.group, out->narrow = P.narrow, out->chain = P.tuning.chain;
  out->min_pivot = P.min_pivot;
  export_factor(P, 0, &out->nnz_l, out->l_row_ptr, out->l_cols, out->l_vals);
  export_factor(P, 1, &out->nnz_u, out->u_row_ptr, out->u_cols, out->u_vals);
  const auto copy = [](int32_t *d, const std::vector<int32_t> &s) {
    if (d && !s.empty())
      std::memcpy(d, s.data(), s.size() * sizeof(int32_t));
  };
  copy(out->row_level_l, P.L.level), copy(out->row_level_u, P.U.level);
  copy(out->order_l, P.L.order), copy(out->order_u, P.U.order);
  const auto launches = [](int32_t *d, const IluTri &T) {
    if (d)
      for (const IluLaunch &q : T.launches)
        *d++ = q.pos0, *d++ = q.pos1, *d++ = q.lev0, *d++ = q.lev1, *d++ = q.chain;
  };
  launches(out->launch_l, P.L), launches(out->launch_u, P.U);
  if (out->solve_dst && out->solve_src)
    ilu_host_solve(P, out->solve_dst, out->solve_src);
  GLS_CATCH
}

glsStatus
gls_ilu_factor_host(int64_t n, const int64_t *row_ptr, const int64_t *cols, const double *vals,
                    const glsILUParams *prm, glsILUFactorHost *out)
{
  GLS_TRY
  using namespace gls;
  if (!prm || !out || !vals)
    throw std::runtime_error("gls_ilu_factor_host: null argument");
  IluParams p;
  p.fill_level = prm->fill_level, p.atol = prm->atol, p.rtol = prm->rtol;
  IluPlan P = ilu_make_symbolic(n, row_ptr, cols, p, ilu_tuning_from_env());
  ilu_refactor_scheduled(P, vals);
  out->n        = P.n;
  out->levels   = (int)P.L.lev_ptr.size() - 1;
  out->launches = (int)P.factor_launches.size();
  out->chains   = 0;
  for (const IluLaunch &q : P.factor_launches)
    out->chains += q.chain;
  out->narrow = P.factor_narrow, out->group = P.factor_group, out->rows = P.factor_rows;
  out->chain     = P.tuning.factor_chain;
  out->max_row   = P.max_row;
  out->min_pivot = P.min_pivot;
  export_factor(P, 0, &out->nnz_l, out->l_row_ptr, out->l_cols, out->l_vals);
  export_factor(P, 1, &out->nnz_u, out->u_row_ptr, out->u_cols, out->u_vals);
  if (out->order && !P.L.order.empty())
    std::memcpy(out->order, P.L.order.data(), P.L.order.size() * sizeof(int32_t));
  if (out->row_level && !P.L.level.empty())
    std::memcpy(out->row_level, P.L.level.data(), P.L.level.size() * sizeof(int32_t));
  if (int32_t *d = out->launch)
    for (const IluLaunch &q : P.factor_launches)
      *d++ = q.pos0, *d++ = q.pos1, *d++ = q.lev0, *d++ = q.lev1, *d++ = q.chain;
  GLS_CATCH
}

} // extern "C"
