// ilu_factor.hip — the numeric ILU(k) factorisation on the device
// (gls_ilu_refactor_device, gls_ilu_create_device): the IKJ elimination of
// ilu_refactor (csrc/ilu_plan.cc) over the level schedule of L, fed by a
// device CSR, so the values never visit the host between assembly and apply.
//
// Storage: the plan's pattern (rp / diag int64, ci int32, rows in the
// original order, columns ascending) with the FP64 values `val` on the
// device; a_to_f places the entries of A, from_l / from_u name the entries
// the two scheduled triangles of csrc/ilu.hip copy.
//
// Kernels, all on the caller's stream:
//   k_ilu_load    val = 0; val[a_to_f[k]] = A_vals[k]; Ifpack's diagonal
//                 modification (three launches of one kernel: each phase
//                 needs the one before it complete on the whole grid).
//   k_ilu_factor_level / k_ilu_factor_chain
//                 row i depends on exactly the rows of its L pattern, so the
//                 dependency levels are those of the forward solve: a wide
//                 level is one grid launch with one group of G lanes per row,
//                 a run of narrow levels one launch of ONE workgroup walking
//                 the levels with __syncthreads() between them (IluPlan::
//                 factor_launches).  Order across workgroups comes from the
//                 launch order on the stream only: no flags, no waits, no
//                 grid barrier, no atomics.
//   k_ilu_store / k_ilu_status
//                 the scheduled copies L.v / U.v, dinv = 1 / pivot, and per
//                 block, then over the blocks in a fixed tree order, min
//                 |pivot| and the smallest row whose pivot is zero or not
//                 finite, into a host-mapped status record.
//
// One row: the group stages the row (values and columns) in LDS.  The L
// entries k run serially in ascending column order; every lane forms l =
// row[k] / val[diag[p]] itself (the same division in every lane), then the
// lanes stride over the entries q of U-row p beyond its diagonal, find
// column ci[q] by a binary search in the staged columns beyond k, and do
// row[w] -= l val[q]; columns the row lacks are dropped.  Inside one pivot
// step the targets w are distinct (the columns of a row are), so lanes never
// collide.  At the end the group writes the row back to val.  What a step
// reads from global memory (the pivot, the pivot row's bounds and its first
// entries) is loaded one or two steps ahead: those rows are final.  The step
// is then bound by the instructions of the searches, not by latency: a row
// of the 3-D Q2 matrices has about 260 L entries and pivot rows of about 260
// entries, each of which costs a nine-step search.
//
// Hazard (a), the hand-off of row[k + 1] between pivot steps: the working
// values are in LDS and a group never spans waves (G <= 64 divides the wave,
// groups are aligned), so producer and consumer lanes run in one wave, whose
// LDS operations complete in issue order.  What is left is to keep the
// compiler from moving or caching LDS accesses across the step: a
// wavefront-scope release / acquire fence pair around a wave barrier
// (group_sync below).  No workgroup barrier is needed, and none would be
// legal: rows of one workgroup have different numbers of L entries.
//
// Hazard (b), rows of earlier levels inside a chain were written by other
// waves of the same workgroup: `val` is a plain pointer (no const, no
// __restrict__, hence no scalar or read-only-cache loads), read by per-lane
// vector loads behind the __syncthreads() that ends each level, as the work
// vector of k_ilu_chain is.
//
// Bitwise contract: no product and difference may become an FMA.  The
// compiler contracts __dsub_rn(x, __dmul_rn(l, v)) under its default
// -ffp-contract=fast, and a file-scope contraction pragma did not stop it
// either, so every product passes through mul_rn below: an empty asm that
// takes and returns the product in a register, which the optimiser cannot
// look through.  FP64 division is correctly rounded (its expansion has FMAs
// of its own, which is what makes it so), as on the host, whose loop is
// compiled for baseline x86-64 (no FMA).  Every entry sees the operations of
// ilu_refactor in the same order, so the device factor equals the host factor
// bit for bit, whatever the launch shapes.
#include "ilu_internal.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace gls
{
namespace
{
constexpr int ILU_STORE_THREADS = 256;
constexpr int ILU_STORE_BLOCKS  = 256; // at most; a power of two

// a * b rounded to FP64 on its own: never one half of an FMA
__device__ __forceinline__ double
mul_rn(double a, double b)
{
  double p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// phase 0: val = 0 (fill positions start at zero); 1: the entries of A;
// 2: d <- rtol d + (d < 0 ? -atol : atol) on every diagonal
template <int PHASE>
__global__ void __launch_bounds__(256)
  k_ilu_load(double *val, const double *__restrict__ a_vals, const int64_t *__restrict__ a_to_f,
             const int64_t *__restrict__ diag, int64_t count, double atol, double rtol)
{
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += stride)
    if (PHASE == 0)
      val[k] = 0.0;
    else if (PHASE == 1)
      val[a_to_f[k]] = a_vals[k];
    else
      {
        const double d = val[diag[k]];
        val[diag[k]]   = mul_rn(rtol, d) + (d < 0.0 ? -atol : atol);
      }
}

// LDS accesses of the lanes of one wave, before and after, stay where they
// are written (see hazard (a) above)
__device__ __forceinline__ void
group_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// U entries of a pivot row for this lane, from q on in steps of G, up to
// q_end: columns and values together (one latency, not two)
template <int G, int U>
__device__ __forceinline__ void
load_chunk(const int32_t *__restrict__ ci, const double *val, int64_t q, int64_t q_end,
           int32_t (&c)[U], double (&u)[U])
{
#pragma unroll
  for (int j = 0; j < U; ++j)
    {
      const int64_t qq = q + (int64_t)j * G;
      const bool    in = qq < q_end;
      c[j] = in ? ci[qq] : 0x7fffffff; // no column: never found
      u[j] = in ? val[qq] : 0.0;
    }
}

// row[w] -= l u for the staged columns w beyond k that equal c.  The U
// searches have the same trip count (it depends on k and len alone) and no
// branches, so the dependent LDS reads of one overlap those of the others.
template <int U>
__device__ __forceinline__ void
apply_chunk(double *sv, const int32_t *sc, int32_t k, int32_t len, double l,
            const int32_t (&c)[U], const double (&u)[U])
{
  // the first staged column >= c in [k + 1, len): it lies in [w, w + n]
  // throughout (len > k + 1: the diagonal is beyond k)
  int32_t w[U];
#pragma unroll
  for (int j = 0; j < U; ++j)
    w[j] = k + 1;
  int32_t n = len - (k + 1);
  while (n > 1)
    {
      const int32_t half = n >> 1;
#pragma unroll
      for (int j = 0; j < U; ++j)
        w[j] = sc[w[j] + half - 1] < c[j] ? w[j] + half : w[j];
      n -= half;
    }
#pragma unroll
  for (int j = 0; j < U; ++j)
    {
      w[j] += sc[w[j]] < c[j] ? 1 : 0;
      if (w[j] < len && sc[w[j]] == c[j])
        sv[w[j]] = sv[w[j]] - mul_rn(l, u[j]);
    }
}

// row i by its group of G lanes; sv / sc: the group's staged values and
// columns (capacity: the longest row of the pattern)
template <int G>
__device__ __forceinline__ void
factor_row(const int64_t *__restrict__ rp, const int64_t *__restrict__ diag,
           const int32_t *__restrict__ ci, double *val, int64_t i, double *sv, int32_t *sc,
           int lane)
{
  // entries of a pivot row per lane in flight: long rows (the full wave)
  // take several passes per pivot, short ones would only search for nothing
  constexpr int U   = G == 64 ? 4 : 1;
  const int64_t r0  = rp[i];
  const int32_t len = (int32_t)(rp[i + 1] - r0);
  const int32_t nl  = (int32_t)(diag[i] - r0);
  if (nl == 0) // uniform over the group: nothing to eliminate
    return;
  for (int32_t e = lane; e < len; e += G)
    sv[e] = val[r0 + e], sc[e] = ci[r0 + e];
  group_sync();
  // The pivot rows are final and the staged columns never change, so all a
  // step reads from global memory is fetched ahead of it: the bounds of the
  // pivot row two steps ahead, the pivot and the first chunk of the pivot row
  // one step ahead.  Only row[k] itself waits for step k - 1.
  int64_t dp = diag[sc[0]], q1 = rp[sc[0] + 1];
  int64_t dpn = 0, q1n = 0;
  if (nl > 1)
    dpn = diag[sc[1]], q1n = rp[sc[1] + 1];
  double  piv = val[dp];
  int32_t c[U];
  double  u[U];
  load_chunk<G, U>(ci, val, dp + 1 + lane, q1, c, u);
  for (int32_t k = 0; k < nl; ++k)
    {
      const double l = sv[k] / piv;
      int32_t      cn[U];
      double       un[U], pivn = 0.0;
      int64_t      dpnn = 0, q1nn = 0;
      if (k + 1 < nl)
        {
          pivn = val[dpn];
          load_chunk<G, U>(ci, val, dpn + 1 + lane, q1n, cn, un);
          if (k + 2 < nl)
            dpnn = diag[sc[k + 2]], q1nn = rp[sc[k + 2] + 1];
        }
      if (lane == 0)
        sv[k] = l;
      apply_chunk<U>(sv, sc, k, len, l, c, u);
      for (int64_t q = dp + 1 + lane + (int64_t)U * G; q < q1; q += (int64_t)U * G)
        {
          load_chunk<G, U>(ci, val, q, q1, c, u);
          apply_chunk<U>(sv, sc, k, len, l, c, u);
        }
      group_sync(); // the step's updates before row[k + 1] is read
      dp = dpn, q1 = q1n, piv = pivn, dpn = dpnn, q1n = q1nn;
#pragma unroll
      for (int j = 0; j < U; ++j)
        c[j] = cn[j], u[j] = un[j];
    }
  for (int32_t e = lane; e < len; e += G)
    val[r0 + e] = sv[e];
  group_sync(); // the slot is free for the group's next row
}

// the group's slot of the workgroup's dynamic LDS: values of all groups
// first, then their columns
__device__ __forceinline__ void
row_slot(double *smem, int32_t groups, int32_t stage, int32_t g, double **sv, int32_t **sc)
{
  *sv = smem + (size_t)g * stage;
  *sc = (int32_t *)(smem + (size_t)groups * stage) + (size_t)g * stage;
}

// a wide level: positions [p0, p1), blockDim.x / G rows per workgroup
template <int G>
__global__ void __launch_bounds__(ILU_WIDE_THREADS)
  k_ilu_factor_level(const int64_t *__restrict__ rp, const int64_t *__restrict__ diag,
                     const int32_t *__restrict__ ci, const int32_t *__restrict__ order,
                     double *val, int32_t p0, int32_t p1, int32_t stage)
{
  extern __shared__ double smem[];
  const int32_t groups = (int32_t)blockDim.x / G, g = (int32_t)threadIdx.x / G;
  const int     lane   = threadIdx.x & (G - 1);
  const int64_t p      = (int64_t)p0 + (int64_t)blockIdx.x * groups + g;
  double       *sv;
  int32_t      *sc;
  row_slot(smem, groups, stage, g, &sv, &sc);
  if (p < p1) // uniform over a group
    factor_row<G>(rp, diag, ci, val, order[p], sv, sc, lane);
}

// a chain: levels [l0, l1) by one workgroup of blockDim.x / G groups, a
// barrier after each level
template <int G>
__global__ void __launch_bounds__(ILU_CHAIN_THREADS)
  k_ilu_factor_chain(const int64_t *__restrict__ rp, const int64_t *__restrict__ diag,
                     const int32_t *__restrict__ ci, const int32_t *__restrict__ order,
                     const int32_t *__restrict__ lev_ptr, double *val, int32_t l0, int32_t l1,
                     int32_t stage)
{
  extern __shared__ double smem[];
  const int32_t groups = (int32_t)blockDim.x / G, g = (int32_t)threadIdx.x / G;
  const int     lane   = threadIdx.x & (G - 1);
  double       *sv;
  int32_t      *sc;
  row_slot(smem, groups, stage, g, &sv, &sc);
  for (int32_t l = l0; l < l1; ++l)
    {
      const int32_t p1 = lev_ptr[l + 1];
      for (int32_t p = lev_ptr[l] + g; p < p1; p += groups)
        factor_row<G>(rp, diag, ci, val, order[p], sv, sc, lane);
      __syncthreads(); // the level's rows are written and visible to the next
    }
}

// min |pivot| over the good pivots and the smallest bad row, pairwise
__device__ __forceinline__ void
status_merge(double &m, int64_t &b, double m2, int64_t b2)
{
  m = m2 < m ? m2 : m;
  b = b2 >= 0 && (b < 0 || b2 < b) ? b2 : b;
}

// a fixed tree over the workgroup's threads; the result in thread 0
__device__ __forceinline__ void
status_reduce(double &m, int64_t &b)
{
  __shared__ double  sm[ILU_STORE_THREADS];
  __shared__ int64_t sb[ILU_STORE_THREADS];
  sm[threadIdx.x] = m, sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = ILU_STORE_THREADS / 2; o > 0; o >>= 1)
    {
      if ((int)threadIdx.x < o)
        {
          status_merge(m, b, sm[threadIdx.x + o], sb[threadIdx.x + o]);
          sm[threadIdx.x] = m, sb[threadIdx.x] = b;
        }
      __syncthreads();
    }
}

__global__ void __launch_bounds__(ILU_STORE_THREADS)
  k_ilu_store(const double *__restrict__ val, const int64_t *__restrict__ diag,
              const int64_t *__restrict__ from_l, const int64_t *__restrict__ from_u,
              double *__restrict__ lv, double *__restrict__ uv, double *__restrict__ dinv,
              int64_t n, int64_t nnz_l, int64_t nnz_u, double *__restrict__ part_min,
              int64_t *__restrict__ part_bad)
{
  const int64_t stride = (int64_t)gridDim.x * ILU_STORE_THREADS;
  const int64_t t0     = (int64_t)blockIdx.x * ILU_STORE_THREADS + threadIdx.x;
  for (int64_t k = t0; k < nnz_l; k += stride)
    lv[k] = val[from_l[k]];
  for (int64_t k = t0; k < nnz_u; k += stride)
    uv[k] = val[from_u[k]];
  double  m = HUGE_VAL;
  int64_t b = -1;
  for (int64_t i = t0; i < n; i += stride) // ascending rows: the first bad one stays
    {
      const double piv = val[diag[i]];
      dinv[i]          = 1.0 / piv;
      if (piv == 0.0 || !isfinite(piv))
        b = b < 0 ? i : b;
      else
        m = fabs(piv) < m ? fabs(piv) : m;
    }
  status_reduce(m, b);
  if (threadIdx.x == 0)
    part_min[blockIdx.x] = m, part_bad[blockIdx.x] = b;
}

__global__ void __launch_bounds__(ILU_STORE_THREADS)
  k_ilu_status(const double *__restrict__ val, const int64_t *__restrict__ diag,
               const double *__restrict__ part_min, const int64_t *__restrict__ part_bad,
               int32_t blocks, IluFactorStatus *status)
{
  double  m = HUGE_VAL;
  int64_t b = -1;
  for (int32_t k = threadIdx.x; k < blocks; k += ILU_STORE_THREADS)
    status_merge(m, b, part_min[k], part_bad[k]);
  status_reduce(m, b);
  if (threadIdx.x == 0)
    {
      status->min_pivot = m;
      status->bad_row   = b;
      status->bad_value = b >= 0 ? val[diag[b]] : 0.0;
    }
}

template <typename T>
void
upload_new(T **d, const std::vector<T> &h)
{
  HIP_THROW(hipMalloc((void **)d, std::max<size_t>(1, h.size()) * sizeof(T)));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
}

unsigned
blocks_for(int64_t count, int threads, int most)
{
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(most, (count + threads - 1) / threads));
}

// the device copy of the pattern, once per factor
void
prepare(glsILU_ *ilu)
{
  DevFactor     &F = ilu->F;
  const IluPlan &P = ilu->plan;
  if (F.ready)
    return;
  if (P.max_row > ILU_FACTOR_MAX_ROW)
    throw std::runtime_error("ilu: the longest row of the pattern has " +
                             std::to_string(P.max_row) +
                             " entries, the device factorisation stages at most " +
                             std::to_string(ILU_FACTOR_MAX_ROW) + " (use the host factorisation)");
  const size_t nnz  = P.ci.size();
  const size_t need = nnz * (sizeof(double) + sizeof(int32_t)) +
                      (size_t)(2 * P.n + 1) * sizeof(int64_t) +
                      ((size_t)P.nnz_a + P.L.from.size() + P.U.from.size()) * sizeof(int64_t);
  size_t free_b = 0, total_b = 0;
  HIP_THROW(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b)
    throw std::runtime_error("ilu: the device factorisation's pattern and values need " +
                             std::to_string(need >> 20) + " MB, " + std::to_string(free_b >> 20) +
                             " MB of device memory are free");
  upload_new(&F.rp, P.rp);
  upload_new(&F.diag, P.diag);
  upload_new(&F.ci, P.ci);
  upload_new(&F.a_to_f, P.a_to_f);
  upload_new(&F.from_l, P.L.from);
  upload_new(&F.from_u, P.U.from);
  HIP_THROW(hipMalloc((void **)&F.val, std::max<size_t>(1, nnz) * sizeof(double)));
  F.store_blocks = (int)blocks_for(std::max<int64_t>((int64_t)nnz, P.n), ILU_STORE_THREADS,
                                   ILU_STORE_BLOCKS);
  HIP_THROW(hipMalloc((void **)&F.part_min, (size_t)F.store_blocks * sizeof(double)));
  HIP_THROW(hipMalloc((void **)&F.part_bad, (size_t)F.store_blocks * sizeof(int64_t)));
  HIP_THROW(hipHostMalloc((void **)&F.h_status, sizeof(IluFactorStatus),
                          hipHostMallocMapped | hipHostMallocCoherent));
  HIP_THROW(hipHostGetDevicePointer((void **)&F.d_status, F.h_status, 0));
  for (hipEvent_t &e : F.ev)
    HIP_THROW(hipEventCreate(&e));
  F.ready = true;
}

template <int G>
void
run_factor(const glsILU_ *ilu, hipStream_t st)
{
  const IluPlan   &P     = ilu->plan;
  const DevFactor &F     = ilu->F;
  const int32_t    stage = (int32_t)P.max_row;
  // rows of one workgroup: what its threads and its LDS hold
  const int rows_fit   = std::max(1, ILU_FACTOR_MAX_ROW / (int)P.max_row);
  const int wide_rows  = std::max(1, std::min(ILU_WIDE_THREADS / G, rows_fit));
  const int chain_rows = std::max(1, std::min(ILU_CHAIN_THREADS / G, rows_fit));
  for (const IluLaunch &q : P.factor_launches)
    if (q.chain)
      hipLaunchKernelGGL((k_ilu_factor_chain<G>), dim3(1), dim3((unsigned)(chain_rows * G)),
                         (size_t)chain_rows * stage * ILU_FACTOR_ROW_BYTES, st, F.rp, F.diag, F.ci,
                         ilu->L.order, ilu->L.lev_ptr, F.val, q.lev0, q.lev1, stage);
    else
      hipLaunchKernelGGL((k_ilu_factor_level<G>),
                         dim3((unsigned)((q.pos1 - q.pos0 + wide_rows - 1) / wide_rows)),
                         dim3((unsigned)(wide_rows * G)),
                         (size_t)wide_rows * stage * ILU_FACTOR_ROW_BYTES, st, F.rp, F.diag, F.ci,
                         ilu->L.order, F.val, q.pos0, q.pos1, stage);
}
} // namespace

void
ilu_factor_device(glsILU_ *ilu, const double *d_vals, hipStream_t st)
{
  IluPlan &P = ilu->plan;
  prepare(ilu);
  DevFactor &F = ilu->F;
  ilu->valid   = false;
  const int64_t nnz = (int64_t)P.ci.size();
  HIP_THROW(hipEventRecord(F.ev[0], st));
  hipLaunchKernelGGL((k_ilu_load<0>), dim3(blocks_for(nnz, 256, 1024)), dim3(256), 0, st, F.val,
                     d_vals, F.a_to_f, F.diag, nnz, P.prm.atol, P.prm.rtol);
  hipLaunchKernelGGL((k_ilu_load<1>), dim3(blocks_for(P.nnz_a, 256, 1024)), dim3(256), 0, st,
                     F.val, d_vals, F.a_to_f, F.diag, P.nnz_a, P.prm.atol, P.prm.rtol);
  hipLaunchKernelGGL((k_ilu_load<2>), dim3(blocks_for(P.n, 256, 1024)), dim3(256), 0, st, F.val,
                     d_vals, F.a_to_f, F.diag, P.n, P.prm.atol, P.prm.rtol);
  HIP_THROW(hipEventRecord(F.ev[1], st));
  switch (P.factor_group)
    {
      case 1: run_factor<1>(ilu, st); break;
      case 2: run_factor<2>(ilu, st); break;
      case 4: run_factor<4>(ilu, st); break;
      case 8: run_factor<8>(ilu, st); break;
      case 16: run_factor<16>(ilu, st); break;
      case 32: run_factor<32>(ilu, st); break;
      case 64: run_factor<64>(ilu, st); break;
      default: throw std::runtime_error("gls_ilu_refactor_device: no kernel for this group width");
    }
  HIP_THROW(hipEventRecord(F.ev[2], st));
  hipLaunchKernelGGL(k_ilu_store, dim3((unsigned)F.store_blocks), dim3(ILU_STORE_THREADS), 0, st,
                     F.val, F.diag, F.from_l, F.from_u, ilu->L.v, ilu->U.v, ilu->dinv, P.n,
                     (int64_t)P.L.from.size(), (int64_t)P.U.from.size(), F.part_min, F.part_bad);
  hipLaunchKernelGGL(k_ilu_status, dim3(1), dim3(ILU_STORE_THREADS), 0, st, F.val, F.diag,
                     F.part_min, F.part_bad, (int32_t)F.store_blocks, F.d_status);
  HIP_THROW(hipEventRecord(F.ev[3], st));
  HIP_THROW(hipGetLastError());
  HIP_THROW(hipStreamSynchronize(st));
  float all_ms = 0, rows_ms = 0;
  HIP_THROW(hipEventElapsedTime(&all_ms, F.ev[0], F.ev[3]));
  HIP_THROW(hipEventElapsedTime(&rows_ms, F.ev[1], F.ev[2]));
  P.numeric_ms           = all_ms;
  ilu->factor_kernels_ms = rows_ms;
  ilu->upload_ms         = 0;
  ilu->on_device         = true; // plan.val is stale from here on
  const volatile IluFactorStatus *hs = F.h_status;
  IluFactorStatus                 s;
  s.min_pivot = hs->min_pivot, s.bad_value = hs->bad_value, s.bad_row = hs->bad_row;
  if (s.bad_row >= 0)
    throw std::runtime_error("ilu: zero or non-finite pivot in row " + std::to_string(s.bad_row) +
                             " (value " + std::to_string(s.bad_value) + ")");
  P.min_pivot = s.min_pivot;
  ilu->valid  = true;
}

void
ilu_factor_download(glsILU_ *ilu)
{
  if (!ilu->F.ready || ilu->plan.val.empty())
    return;
  HIP_THROW(hipMemcpy(ilu->plan.val.data(), ilu->F.val, ilu->plan.val.size() * sizeof(double),
                      hipMemcpyDeviceToHost));
}

void
ilu_factor_release(glsILU_ *ilu)
{
  DevFactor &F = ilu->F;
  for (void *p : {(void *)F.rp, (void *)F.diag, (void *)F.a_to_f, (void *)F.from_l,
                  (void *)F.from_u, (void *)F.ci, (void *)F.val, (void *)F.part_min,
                  (void *)F.part_bad})
    if (p)
      (void)hipFree(p);
  if (F.h_status)
    (void)hipHostFree(F.h_status);
  for (hipEvent_t e : F.ev)
    if (e)
      (void)hipEventDestroy(e);
  F = DevFactor{};
}
} // namespace gls
