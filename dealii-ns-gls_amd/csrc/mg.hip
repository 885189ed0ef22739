// mg.hip — geometric multigrid on the GPU: level transfer (MGTwoLevelTransfer
// semantics, main.cc:538-563), damped-Jacobi relaxation smoother with a
// power-iteration relaxation factor (PreconditionRelaxation with
// relaxation = 0, multigrid.cc:281-369 — NOT Chebyshev), and the
// V-cycle of PreconditionMG / Multigrid (multigrid.cc:202-220, 534-548).
//
// Transfer between level l-1 (coarse) and l (fine), per coarse cell, with
// P the 1D interpolation of the parent's Q_k basis to the (2k+1) child
// lattice points:
//   prolongate_add: dst_f += w_f * (P x P x P) (Z_c src_c)
//   restrict_add:   dst_c += Z_c (P x P x P)^T (w_f * src_f)
// Z_c zeroes constrained coarse dofs, w_f = 1/valence on unconstrained fine
// dofs and 0 on constrained ones; interpolate = nodal injection (nested GLL
// nodes, k <= 2).
#include "../../include/gls_op.h"
#include "common.h"
#include "kernels.h"
#include "op_internal.h"
#include "arnoldi.h"
#include "coarse.h"
#include "trace.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

using namespace gls;

namespace
{
constexpr int MAXP = 2 * 3 + 1; // (2k+1) for k <= 3
constexpr int MAXN = 4;
constexpr uint32_t NOT_OWNER = 0x80000000u;

template <typename T>
struct TransferArgs
{
  const uint32_t *coarse_nodes; // [cells_c][nq] node | cmask << 28
  const uint32_t *child;        // [cells_c][nl] fine node ids | NOT_OWNER: every fine
                                // node is owned by one entry (its first coarse cell)
  const T        *weight;       // [n_dofs_f]
  int64_t         n_cells_c;
  T               P[MAXP][MAXN];
  // restriction of a residual whose shared-node reduction is still pending
  // (v_step, FP32 3D brick levels; null: src complete): the fine node's
  // shared index, the residual apply's slots and classes, its src x and b
  const int32_t  *q_index   = nullptr;
  const uint32_t *q_nodes   = nullptr; // shared node | cmask << 28
  const T        *q_slots   = nullptr;
  const T        *q_x       = nullptr;
  const T        *q_b       = nullptr;
  gls::ReduceClasses q_rc{};
  // prolongation of a coarse solution whose last smoothing step's reduction
  // is pending: the coarse node's shared index, that step's slots, its src
  // (the iterate before), b, d (null: 1) and omega
  const int32_t  *p_index   = nullptr;
  const T        *p_slots   = nullptr;
  const T        *p_prev    = nullptr;
  const T        *p_b       = nullptr;
  const T        *p_d       = nullptr;
  T               p_omega   = T(0);
  gls::ReduceClasses p_rc{};
  // deterministic restriction (GLS_DETERMINISTIC): the coarse cells of one
  // colour, one workgroup each (null: workgroup c = coarse cell c)
  const int32_t  *cells     = nullptr;
};

// the relaxation step x_prev + omega d (b - A x_prev) at shared coarse node s
// from the step's partial slots, in k_shared_reduce_cls's order and
// arithmetic (bitwise its result; constrained components keep x_prev)
template <typename T>
__device__ __forceinline__ typename gls::Pack<T>::V
rebuild_relax(const TransferArgs<T> &a, uint32_t s, uint32_t node, uint32_t cm)
{
  using V        = typename gls::Pack<T>::V;
  constexpr int W = gls::Pack<T>::W;
  int           k = 0;
#pragma unroll
  for (int j = 1; j < gls::ReduceClasses::MAX; ++j)
    if (j < a.p_rc.n && s >= a.p_rc.first[j])
      k = j;
  const uint32_t m   = a.p_rc.mult[k];
  const uint32_t b0  = a.p_rc.slot0[k] + (s - a.p_rc.first[k]) * m;
  const V       *pp  = reinterpret_cast<const V *>(a.p_slots);
  V              sum = {};
  uint32_t       i   = 0;
  for (; i + 4 <= m; i += 4)
    {
      const V x0 = pp[b0 + i], x1 = pp[b0 + i + 1], x2 = pp[b0 + i + 2], x3 = pp[b0 + i + 3];
      sum += (x0 + x1) + (x2 + x3);
    }
  if (i + 2 <= m)
    {
      const V x0 = pp[b0 + i], x1 = pp[b0 + i + 1];
      sum += x0 + x1;
      i += 2;
    }
  if (i < m)
    sum += pp[b0 + i];
  const V xs = reinterpret_cast<const V *>(a.p_prev)[node];
  if (cm)
#pragma unroll
    for (int w = 0; w < W; ++w)
      if ((cm >> w) & 1)
        sum[w] = xs[w];
  const V dj = a.p_d ? reinterpret_cast<const V *>(a.p_d)[node] : V{} + T(1);
  return xs + a.p_omega * dj * (reinterpret_cast<const V *>(a.p_b)[node] - sum);
}

// the residual b - A x of shared fine node s from the residual apply's
// partial slots, in k_shared_reduce_cls's order and arithmetic (bitwise its
// result: keep 0, omega 1, d 1; constrained components b - x)
template <typename T>
__device__ __forceinline__ typename gls::Pack<T>::V
rebuild_residual(const TransferArgs<T> &a, uint32_t s)
{
  using V        = typename gls::Pack<T>::V;
  constexpr int W = gls::Pack<T>::W;
  int           k = 0;
#pragma unroll
  for (int j = 1; j < gls::ReduceClasses::MAX; ++j)
    if (j < a.q_rc.n && s >= a.q_rc.first[j])
      k = j;
  const uint32_t m      = a.q_rc.mult[k];
  const uint32_t b0     = a.q_rc.slot0[k] + (s - a.q_rc.first[k]) * m;
  const uint32_t packed = a.q_nodes[s];
  const V       *pp     = reinterpret_cast<const V *>(a.q_slots);
  V              sum    = {};
  uint32_t       i      = 0;
  for (; i + 4 <= m; i += 4)
    {
      const V x0 = pp[b0 + i], x1 = pp[b0 + i + 1], x2 = pp[b0 + i + 2], x3 = pp[b0 + i + 3];
      sum += (x0 + x1) + (x2 + x3);
    }
  if (i + 2 <= m)
    {
      const V x0 = pp[b0 + i], x1 = pp[b0 + i + 1];
      sum += x0 + x1;
      i += 2;
    }
  if (i < m)
    sum += pp[b0 + i];
  const uint32_t node = packed & gls::NODE_MASK, cm = packed >> 28;
  const V        xs   = reinterpret_cast<const V *>(a.q_x)[node];
  if (cm)
#pragma unroll
    for (int w = 0; w < W; ++w)
      if ((cm >> w) & 1)
        sum[w] = xs[w];
  const V dj = V{} + T(1);
  return V{} + T(1) * dj * (reinterpret_cast<const V *>(a.q_b)[node] - sum);
}

// Transfers as sum factorisation over the (2k+1)^dim child lattice of one
// coarse cell: the 1-D interpolation matrix P [(2k+1) x (k+1)] is staged in
// LDS and each lane reads its rows into registers, so every tensor index is a
// compile-time constant of the unrolled sweeps (a dense (2k+1)^dim x
// (k+1)^dim loop indexing the kernel-argument array at run time went
// through scratch: 28.7 us per r2 -> r1 restriction).
// threads per transfer workgroup (one coarse cell): the fine lattice's
// (2k+1)^dim points rounded up to whole waves, at least the coarse cell's
// dofs, at most 256 (3D Q2: 125 points -> 128 threads, twice the resident
// workgroups of a 256-thread block that idles half its lanes)
template <int dim, int k>
constexpr int
transfer_block()
{
  constexpr int nl = ipow(2 * k + 1, dim), nd = ipow(k + 1, dim) * (dim + 1);
  constexpr int m  = nl > nd ? nl : nd;
  return m <= 64 ? 64 : m <= 128 ? 128 : 256;
}

template <int dim, int k, typename T>
__global__ void __launch_bounds__(256)
  k_prolongate(TransferArgs<T> a, T *__restrict__ dst_f, const T *__restrict__ src_c,
               const T *__restrict__ base = nullptr)
{
  constexpr int n = k + 1, nq = ipow(n, dim), nc = dim + 1, L = 2 * k + 1;
  constexpr int nl = ipow(L, dim);
  constexpr int TB  = transfer_block<dim, k>();
  constexpr int NIT = (nl + TB - 1) / TB; // lattice points per thread
  __shared__ T  u[nc][nq];
  __shared__ T  sP[L][n];
  const int64_t c = blockIdx.x;
  const int     t = threadIdx.x;
  // the lattice's fine node ids and their weights / base values do not
  // depend on the coarse gather: issued first, in flight together with it
  // (one memory round trip before the sweeps instead of two)
  uint32_t fe[NIT];
  T        wv[NIT][nc], bv[NIT][nc];
#pragma unroll
  for (int r = 0; r < NIT; ++r)
    {
      const int I = t + r * TB;
      fe[r]       = I < nl ? a.child[c * nl + I] : NOT_OWNER;
    }
#pragma unroll
  for (int r = 0; r < NIT; ++r)
#pragma unroll
    for (int comp = 0; comp < nc; ++comp)
      {
        const size_t j = (size_t)(fe[r] & ~NOT_OWNER) * nc + comp;
        const bool   o = !(fe[r] & NOT_OWNER);
        wv[r][comp]    = o ? a.weight[j] : T(0);
        bv[r][comp]    = o ? (base ? base[j] : dst_f[j]) : T(0);
      }
  if (t < L * n)
    sP[t / n][t % n] = a.P[t / n][t % n];
  if (t < nq)
    {
      const uint32_t packed = a.coarse_nodes[c * nq + t];
      const uint32_t node = packed & NODE_MASK, cm = packed >> 28;
      bool           done = false;
      if constexpr (sizeof(T) == 4 && nc == 4)
        if (a.p_index)
          {
            // pending last smoothing step: shared coarse rows rebuilt
            using V          = typename gls::Pack<T>::V;
            const int32_t si = a.p_index[node];
            const V       x  = si >= 0 ? rebuild_relax(a, (uint32_t)si, node, cm) :
                                         reinterpret_cast<const V *>(src_c)[node];
#pragma unroll
            for (int comp = 0; comp < nc; ++comp)
              u[comp][t] = ((cm >> comp) & 1) ? T(0) : x[comp];
            done = true;
          }
      if (!done)
#pragma unroll
        for (int comp = 0; comp < nc; ++comp)
          u[comp][t] = ((cm >> comp) & 1) ? T(0) : src_c[(size_t)node * nc + comp];
    }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NIT; ++r)
    {
      const int I = t + r * TB;
      if (I >= nl)
        break;
      const int Ix = I % L, Iy = (I / L) % L, Iz = dim == 3 ? I / (L * L) : 0;
      T         px[n], py[n], pz[n];
#pragma unroll
      for (int i = 0; i < n; ++i)
        {
          px[i] = sP[Ix][i];
          py[i] = sP[Iy][i];
          pz[i] = dim == 3 ? sP[Iz][i] : T(0);
        }
      // a fine node shared by several coarse cells is written by its owner
      // only (conforming interpolation: all give the same value), so the
      // update is a plain read-modify-write, no atomics
      if (fe[r] & NOT_OWNER)
        continue;
      const uint32_t fn = fe[r];
#pragma unroll
      for (int comp = 0; comp < nc; ++comp)
        {
          T s = 0;
#pragma unroll
          for (int iz = 0; iz < (dim == 3 ? n : 1); ++iz)
            {
              T sy = 0;
#pragma unroll
              for (int iy = 0; iy < n; ++iy)
                {
                  T sx = 0;
#pragma unroll
                  for (int ix = 0; ix < n; ++ix)
                    sx += px[ix] * u[comp][ix + n * (iy + n * iz)];
                  sy += py[iy] * sx;
                }
              s += (dim == 3 ? pz[iz] : T(1)) * sy;
            }
          const T      w = wv[r][comp];
          const size_t j = (size_t)fn * nc + comp;
          if (base) // out of place: dst = base + w P src
            dst_f[j] = bv[r][comp] + (w != T(0) ? w * s : T(0));
          else if (w != T(0))
            dst_f[j] = bv[r][comp] + w * s;
        }
    }
}

template <int dim, int k, typename T>
__global__ void __launch_bounds__(256)
  k_restrict(TransferArgs<T> a, T *__restrict__ dst_c, const T *__restrict__ src_f)
{
  constexpr int n = k + 1, nq = ipow(n, dim), nc = dim + 1, L = 2 * k + 1;
  constexpr int nl = ipow(L, dim);
  __shared__ T  v[nc][nl];
  __shared__ T  sP[L][n];
  const int64_t c = a.cells ? (int64_t)a.cells[blockIdx.x] : (int64_t)blockIdx.x;
  const int     t = threadIdx.x;
  // this thread's coarse dof (node id, constraint bits) is independent of
  // the fine gather: loaded up front (blockDim >= nq * nc, k <= 2 in 3D)
  constexpr bool ONE = nq * nc <= transfer_block<dim, k>();
  const uint32_t pk0 = ONE && t < nq * nc ? a.coarse_nodes[c * nq + t % nq] : 0u;
  if (t < L * n)
    sP[t / n][t % n] = a.P[t / n][t % n];
  for (int I = t; I < nl; I += blockDim.x)
    {
      // R = P^T of the owner-only prolongation: a shared fine node feeds its
      // owner's coarse dofs only (its other cells' shape functions that are
      // nonzero there are the same shared coarse dofs)
      const uint32_t fe    = a.child[c * nl + I];
      const bool     owner = !(fe & NOT_OWNER);
      const uint32_t fn    = fe & ~NOT_OWNER;
      if constexpr (sizeof(T) == 4 && nc == 4)
        if (a.q_index)
          {
            // pending residual: shared rows rebuilt from the slots
            using V     = typename gls::Pack<T>::V;
            const int32_t si = owner ? a.q_index[fn] : -1;
            const V       r  = si >= 0 ? rebuild_residual(a, (uint32_t)si) :
                               owner  ? reinterpret_cast<const V *>(src_f)[fn] : V{};
            const V       wv = owner ? reinterpret_cast<const V *>(a.weight)[fn] : V{};
#pragma unroll
            for (int comp = 0; comp < nc; ++comp)
              v[comp][I] = wv[comp] * r[comp];
            continue;
          }
#pragma unroll
      for (int comp = 0; comp < nc; ++comp)
        v[comp][I] = owner ? a.weight[(size_t)fn * nc + comp] * src_f[(size_t)fn * nc + comp]
                           : T(0);
    }
  __syncthreads();
  for (int i = t; i < nq * nc; i += blockDim.x)
    {
      const int      ii = i % nq, comp = i / nq;
      const uint32_t packed = ONE ? pk0 : a.coarse_nodes[c * nq + ii];
      const uint32_t node = packed & NODE_MASK, cm = packed >> 28;
      if ((cm >> comp) & 1)
        continue;
      const int ix = ii % n, iy = (ii / n) % n, iz = dim == 3 ? ii / (n * n) : 0;
      T         px[L], py[L], pz[L];
#pragma unroll
      for (int I = 0; I < L; ++I)
        {
          px[I] = sP[I][ix];
          py[I] = sP[I][iy];
          pz[I] = dim == 3 ? sP[I][iz] : T(0);
        }
      const T *vc = v[comp];
      T        s  = 0;
#pragma unroll
      for (int Iz = 0; Iz < (dim == 3 ? L : 1); ++Iz)
        {
          T sy = 0;
#pragma unroll
          for (int Iy = 0; Iy < L; ++Iy)
            {
              T sx = 0;
#pragma unroll
              for (int Ix = 0; Ix < L; ++Ix)
                sx += px[Ix] * vc[Ix + L * (Iy + L * Iz)];
              sy += py[Iy] * sx;
            }
          s += (dim == 3 ? pz[Iz] : T(1)) * sy;
        }
      unsafeAtomicAdd(dst_c + (size_t)node * nc + comp, s);
    }
}

// interpolate_to_mg: coarse GLL node i sits at fine lattice point 2 i (k <= 2)
template <int dim, int k, typename T>
__global__ void
k_interpolate(TransferArgs<T> a, T *__restrict__ dst_c, const T *__restrict__ src_f)
{
  constexpr int n = k + 1, nq = ipow(n, dim), nc = dim + 1, L = 2 * k + 1;
  constexpr int nl = ipow(L, dim);
  const int64_t g  = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.n_cells_c * nq)
    return;
  const int64_t  c  = g / nq;
  const int      i  = (int)(g % nq);
  const int      ix = i % n, iy = (i / n) % n, iz = dim == 3 ? i / (n * n) : 0;
  const int      I  = 2 * ix + L * (2 * iy + L * (dim == 3 ? 2 * iz : 0));
  const uint32_t fn = a.child[c * nl + I] & ~NOT_OWNER;
  const uint32_t cn = a.coarse_nodes[c * nq + i] & NODE_MASK;
#pragma unroll
  for (int comp = 0; comp < nc; ++comp)
    dst_c[(size_t)cn * nc + comp] = src_f[(size_t)fn * nc + comp];
}

// ------------------------------------------------------------ vectors
// PreconditionRelaxation with a diagonal preconditioner:
//   first (zero start): x = omega d . b;  step: x += omega d . (b - t), t = A x
template <typename T>
__global__ void
k_relax(T *__restrict__ x, const T *__restrict__ b, const T *__restrict__ t,
        const T *__restrict__ d, T omega, int first, int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  if (first)
    x[i] = omega * d[i] * b[i];
  else
    x[i] += omega * d[i] * (b[i] - t[i]);
}

// The zero-start relaxation of a level's pre-smoothing with two neighbours of
// the V-cycle folded in: the next coarser defect, which the restriction then
// accumulates into, is zeroed here (zero_words), and on the finest level the
// outer FP64 defect is converted here (copy_to_mg): b = (T) b64, written to
// bout.  One launch instead of three.
template <typename T>
__global__ void
k_relax_first(T *__restrict__ x, const T *__restrict__ b, const T *__restrict__ d, T omega,
              int64_t n, uint32_t *__restrict__ zero, int64_t zero_words,
              const double *__restrict__ b64, T *__restrict__ bout)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < zero_words)
    zero[i] = 0u;
  if (i >= n)
    return;
  T bi;
  if (b64)
    {
      bi      = (T)b64[i];
      bout[i] = bi;
    }
  else
    bi = b[i];
  x[i] = omega * d[i] * bi;
}

// zero fill / copy of the V-cycle's own buffers (kernels)
__global__ void
k_zero(uint32_t *__restrict__ x, int64_t n_words)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words)
    x[i] = 0u;
}

__global__ void
k_copy(uint32_t *__restrict__ y, const uint32_t *__restrict__ x, int64_t n_words)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_words)
    y[i] = x[i];
}

// power iteration step (deal.II power_iteration, see power_iteration_t):
// y = D^{-1} (A x) in place; per-block partial sums of x.y and y.y into
// part[2 block], part[2 block + 1] (no atomics: k_power_finish adds the
// blocks in a fixed order)
template <typename T>
__global__ void __launch_bounds__(256)
  k_power_step(T *__restrict__ y, const T *__restrict__ x, const T *__restrict__ d,
               double *__restrict__ part, int64_t n)
{
  __shared__ double red[2][4];
  const int64_t     i  = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double            xy = 0, yy = 0;
  if (i < n)
    {
      const T v = d[i] * y[i];
      y[i]      = v;
      xy        = (double)x[i] * (double)v;
      yy        = (double)v * (double)v;
    }
  for (int off = 32; off > 0; off >>= 1)
    {
      xy += __shfl_down(xy, off);
      yy += __shfl_down(yy, off);
    }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    {
      red[0][w] = xy;
      red[1][w] = yy;
    }
  __syncthreads();
  if (threadIdx.x == 0)
    {
      part[2 * blockIdx.x]     = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      part[2 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// deal.II set_initial_guess + constraints.set_zero: x_i = i % 11 - mean,
// zero on constrained components; per-block partial sums of x.x for the
// normalisation (k_power_finish)
template <typename T>
__global__ void __launch_bounds__(256)
  k_power_start(T *__restrict__ x, const uint8_t *__restrict__ cmask, int nc, double mean,
                double *__restrict__ part, int64_t n)
{
  __shared__ double red[4];
  const int64_t     i  = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double            xx = 0;
  if (i < n)
    {
      const int64_t node = i / nc;
      const int     c    = (int)(i - node * nc);
      const double  v    = ((cmask[node] >> c) & 1) ? 0.0 : (double)(i % 11) - mean;
      x[i]               = (T)v;
      xx                 = v * v;
    }
  for (int off = 32; off > 0; off >>= 1)
    xx += __shfl_down(xx, off);
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = xx;
  __syncthreads();
  if (threadIdx.x == 0)
    {
      part[2 * blockIdx.x]     = 0.0;
      part[2 * blockIdx.x + 1] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// one workgroup: scal[0] = x.y (the Rayleigh quotient of the normalised x),
// scal[1] = 1 / |y| (0 if y = 0)
__global__ void __launch_bounds__(256)
  k_power_finish(const double *__restrict__ part, int64_t n_blocks, double *__restrict__ scal)
{
  __shared__ double red[2][256];
  double            xy = 0, yy = 0;
  for (int64_t b = threadIdx.x; b < n_blocks; b += 256)
    {
      xy += part[2 * b];
      yy += part[2 * b + 1];
    }
  red[0][threadIdx.x] = xy;
  red[1][threadIdx.x] = yy;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1)
    {
      if ((int)threadIdx.x < s)
        {
          red[0][threadIdx.x] += red[0][threadIdx.x + s];
          red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
      __syncthreads();
    }
  if (threadIdx.x == 0)
    {
      scal[0] = red[0][0];
      scal[1] = red[1][0] > 0 ? 1.0 / sqrt(red[1][0]) : 0.0;
    }
}

// x = scal[1] * y (the scale factor stays on the device: no host round trip
// per power iteration)
template <typename T>
__global__ void
k_scale_dev(T *__restrict__ x, const T *__restrict__ y, const double *__restrict__ scal,
            int64_t n)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    x[i] = (T)(scal[1] * (double)y[i]);
}

} // namespace

namespace gls
{
void
zero_words(void *x, int64_t n_words, hipStream_t s)
{
  hipLaunchKernelGGL(k_zero, g1(n_words), dim3(256), 0, s, (uint32_t *)x, n_words);
  HIP_THROW(hipGetLastError());
}

void
copy_words(void *y, const void *x, int64_t n_words, hipStream_t s)
{
  hipLaunchKernelGGL(k_copy, g1(n_words), dim3(256), 0, s, (uint32_t *)y, (const uint32_t *)x,
                     n_words);
  HIP_THROW(hipGetLastError());
}
} // namespace gls

struct glsMG_
{
  glsMGDesc          desc{};
  // timer-section names of the V-cycle phases per level (multigrid.cc:550-583:
  // gmg::vmult::level_<l>::<phase>; [l][5] = the coarse solve's plain name)
  std::vector<std::vector<std::string>> sec;
  std::vector<glsOp> ops;
  int                prec = GLS_F32, dim = 3, degree = 2, nc = 4;
  std::vector<uint32_t *> d_child;  // level l >= 1: [cells(l-1)][nl]
  std::vector<void *>     d_weight; // level l >= 1: [n_dofs(l)]
  // the weights without node constraints (host) and the fine operator's
  // nc_version they were last uploaded for: gls_mg_setup zeroes the weights of
  // the eliminated fine components when a level's rows changed
  std::vector<std::vector<double>> h_weight;
  std::vector<uint64_t>            weight_nc_version;
  std::vector<void *>     invdiag, sol, def, tmp;
  // deferred shared-node reductions of the smoother (smooth): per level two
  // partial-slot buffers the applies alternate between (beside the
  // operator's own, which the residual and the explicit reductions use);
  // GLS_MG_DEFER=0 reduces after every apply instead
  std::vector<void *>     qslot[2];
  std::vector<double>     omega, lambda;
  // power iteration: per level, block partials | 2 scalars (the levels'
  // estimates run concurrently, gls_mg_setup)
  double                 *d_acc = nullptr;
  std::vector<int64_t>    acc_off; // level l's partials start at d_acc + acc_off[l]
  std::vector<hipStream_t> side;   // setup: one stream per level, joined by events
  std::vector<hipEvent_t>  side_ev;
  double                  P[3][MAXP][MAXN]{}; // 1D prolongation per coarse degree (1, 2)
  bool                    setup_done = false;
  bool                    partitioned = false; // rank-local level operators
  gls::VecStage           stage; // caller layout of gls_mg_vcycle's vectors
  // the coarse solvers built from the coarse matrix (direct, ILU, AMG) and
  // the coarse GMRES (coarse.hip)
  std::unique_ptr<gls::CoarseSolver> coarse;
  // finest-level FP64 defect for the fused copy_to_mg (mg_vcycle_device; null:
  // def[top] already holds the defect)
  const double *top_b64 = nullptr;
  // its FP64 result for the fused copy_from_mg (null: none), and whether the
  // last post-smoothing step wrote it
  double *top_out64      = nullptr;
  bool    top_out64_done = false;
  // the residual of level rq_level whose shared-node reduction the next
  // restriction rebuilds (v_step; rq_level < 0: none): its slots, x and b
  mutable int   rq_level = -1;
  mutable void *rq_slots = nullptr;
  mutable const void *rq_x = nullptr, *rq_b = nullptr;
  // the coarse solution of level pp_level - 1 whose last smoothing step's
  // reduction the next prolongation into level pp_level rebuilds
  mutable int         pp_level = -1;
  mutable const void *pp_slots = nullptr, *pp_prev = nullptr, *pp_b = nullptr,
                     *pp_d = nullptr;
  mutable double      pp_omega = 0.0;

  size_t
  ts() const
  {
    return prec == GLS_F64 ? 8 : 4;
  }
};

namespace
{
template <typename T>
TransferArgs<T>
targs(const glsMG_ *mg, int level)
{
  TransferArgs<T> a;
  a.coarse_nodes = mg->ops[level - 1]->d_nodes;
  a.child        = mg->d_child[level];
  a.weight       = (const T *)mg->d_weight[level];
  a.n_cells_c    = mg->ops[level - 1]->n_cells;
  const int kc   = mg->ops[level - 1]->degree;
  for (int i = 0; i < MAXP; ++i)
    for (int j = 0; j < MAXN; ++j)
      a.P[i][j] = (T)mg->P[kc][i][j];
  if (mg->rq_level == level)
    {
      const glsOp op = mg->ops[level];
      a.q_index      = op->d_shared_index;
      a.q_nodes      = op->d_shared_nodes;
      a.q_slots      = (const T *)mg->rq_slots;
      a.q_x          = (const T *)mg->rq_x;
      a.q_b          = (const T *)mg->rq_b;
      a.q_rc         = op->reduce_classes;
    }
  if (mg->pp_level == level)
    {
      const glsOp oc = mg->ops[level - 1];
      a.p_index      = oc->d_shared_index;
      a.p_slots      = (const T *)mg->pp_slots;
      a.p_prev       = (const T *)mg->pp_prev;
      a.p_b          = (const T *)mg->pp_b;
      a.p_d          = (const T *)mg->pp_d;
      a.p_omega      = (T)mg->pp_omega;
      a.p_rc         = oc->reduce_classes;
    }
  return a;
}

// kind: 0 prolongate_add, 1 restrict_add, 2 interpolate; base (prolongate
// only): dst = base + P src instead of dst += P src
template <int dim, int k, typename T>
void
transfer_t(const glsMG_ *mg, int kind, int level, void *dst, const void *src, hipStream_t s,
           const void *base)
{
  constexpr int nq = ipow(k + 1, dim);
  const auto    a  = targs<T>(mg, level);
  const dim3    grid((unsigned)a.n_cells_c);
  const dim3    tb(transfer_block<dim, k>());
  if (kind == 0)
    hipLaunchKernelGGL((k_prolongate<dim, k, T>), grid, tb, 0, s, a, (T *)dst, (const T *)src,
                       (const T *)base);
  else if (kind == 1 && !gls::op_deterministic(mg->ops[level - 1]))
    hipLaunchKernelGGL((k_restrict<dim, k, T>), grid, tb, 0, s, a, (T *)dst, (const T *)src);
  else if (kind == 1)
    {
      // coarse cell colour by colour: no two workgroups of a launch add to
      // one coarse node, the sums in a fixed order
      glsOp_ *oc = const_cast<glsOp_ *>(mg->ops[level - 1]);
      gls::op_cell_colours(oc);
      for (size_t col = 0; col + 1 < oc->colour_off.size(); ++col)
        {
          auto ac  = a;
          ac.cells = oc->d_colour_cells + oc->colour_off[col];
          hipLaunchKernelGGL((k_restrict<dim, k, T>),
                             dim3((unsigned)(oc->colour_off[col + 1] - oc->colour_off[col])), tb, 0,
                             s, ac, (T *)dst, (const T *)src);
        }
    }
  else
    hipLaunchKernelGGL((k_interpolate<dim, k, T>), g1(a.n_cells_c * nq), dim3(256), 0, s, a,
                       (T *)dst, (const T *)src);
  HIP_THROW(hipGetLastError());
}

void
transfer(const glsMG_ *mg, int kind, int level, void *dst, const void *src, hipStream_t s,
         const void *base = nullptr)
{
  if (level < 1 || level >= (int)mg->ops.size())
    throw std::runtime_error("multigrid transfer: level out of range");
  // node constraints of the coarse level (C_c): the prolongation reads
  // C_c x_c (the source resolved in place and restored), the restriction ends
  // with C_c^T and zero on the eliminated coarse components (dst's eliminated
  // components are zero before: a defect of the constrained operator)
  const glsOp_ *cop = mg->ops[level - 1];
  if (kind == 0)
    gls::nc_resolve(cop, const_cast<void *>(src), true, s);
  // the coarse level's degree: a FE_Q_iso_Q1 coarsest level is Q1 on the
  // sub-cells under Q_k levels (main.cc:436-446)
  const int k = cop->degree;
  if (k != 1 && k != 2)
    throw std::runtime_error("multigrid transfer: degree must be 1 or 2");
  gls::with_real(mg->prec, [&](auto t) {
    gls::with_dim_degree<2>(mg->dim, k, "multigrid transfer", [&](auto d, auto kk) {
      transfer_t<decltype(d)::value, decltype(kk)::value, decltype(t)>(mg, kind, level, dst, src,
                                                                         s, base);
    });
  });
  if (kind == 0)
    gls::nc_restore(cop, const_cast<void *>(src), s);
  else if (kind == 1)
    gls::nc_transpose(cop, dst, nullptr, true, s);
}

// x = omega D^{-1} b (first) or x += omega D^{-1} (b - tmp[level])
void
relax(const glsMG_ *mg, int level, void *x, const void *b, int first, hipStream_t s)
{
  const int64_t n = mg->ops[level]->n_dofs;
  gls::with_real(mg->prec, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_relax<T>, g1(n), dim3(256), 0, s, (T *)x, (const T *)b,
                       (const T *)mg->tmp[level], (const T *)mg->invdiag[level],
                       (T)mg->omega[level], first, n);
  });
  HIP_THROW(hipGetLastError());
}

// what the zero-start relaxation folds in (k_relax_first)
struct FirstRelax
{
  uint32_t     *zero       = nullptr;
  int64_t       zero_words = 0;
  const double *b64        = nullptr; // FP64 defect to convert into b
};

void
relax_first(const glsMG_ *mg, int level, void *x, void *b, const FirstRelax &fr, hipStream_t s)
{
  const int64_t n = mg->ops[level]->n_dofs;
  gls::with_real(mg->prec, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_relax_first<T>, g1(std::max(n, fr.zero_words)), dim3(256), 0, s, (T *)x,
                       (const T *)b, (const T *)mg->invdiag[level], (T)mg->omega[level], n,
                       fr.zero, fr.zero_words, fr.b64, (T *)b);
  });
  HIP_THROW(hipGetLastError());
}

// the last apply of a smoothing sequence whose shared-node reduction is
// still pending (deferred): its slots, its src (the iterate before) and its
// relaxation
struct PendingReduce
{
  const void *slots = nullptr, *src = nullptr, *b = nullptr, *d = nullptr;
  double      omega = 0.0;
  bool        valid = false;
};

bool
defer_reduce(const glsMG_ *mg, int level)
{
  static const bool on = [] {
    const char *e = getenv("GLS_MG_DEFER");
    return !e || std::atoi(e) != 0;
  }();
  return on && gls::deferred_reduce_ok(mg->ops[level]) && mg->qslot[0].size() > (size_t)level &&
         mg->qslot[0][(size_t)level];
}

// deferred smoothing sequences in one resident launch (k_brick_sweeps) where
// the level qualifies: GLS_MG_DEFER unset or >= 2; 1 keeps one launch per
// step (with deferred reductions), 0 reduces after every step
bool
defer_resident()
{
  static const bool on = [] {
    const char *e = getenv("GLS_MG_DEFER");
    return !e || std::atoi(e) >= 2;
  }();
  return on;
}

// PreconditionRelaxation::vmult (zero start) / step, `iters` iterations;
// the result in x.  x_in (step only): the starting iterate is in tmp[level]
// instead of x (the multigrid's out-of-place prolongation put it there).
// fr (zero start only): folded into the first relaxation; false when there
// was none (iters == 0), so the caller does that work itself
// out64 (deferred-reduction levels only): the last step's result also
// written as FP64 by its brick write-out and reduction (*wrote64 = true)
bool
smooth(const glsMG_ *mg, int level, void *x, const void *b, bool zero_start, int iters,
       hipStream_t s, bool start_in_tmp = false, const FirstRelax *fr = nullptr,
       PendingReduce *pend = nullptr, double *out64 = nullptr, bool *wrote64 = nullptr)
{
  auto  first = [&](void *xx) {
    if (fr)
      relax_first(mg, level, xx, (void *)b, *fr, s);
    else
      relax(mg, level, xx, b, 1, s);
  };
  glsOp op    = mg->ops[level];
  void *tmp   = mg->tmp[level];
  if (!gls::fused_relax_ok(op))
    {
      int it = 0;
      if (start_in_tmp)
        {
          const int64_t w = (int64_t)((size_t)op->n_dofs * mg->ts() / 4);
          copy_words(x, tmp, w, s);
        }
      if (zero_start && iters > 0)
        {
          first(x);
          it = 1;
        }
      for (; it < iters; ++it)
        {
          gls::op_vmult_device(op, tmp, x, s);
          relax(mg, level, x, b, 0, s);
        }
      return zero_start && iters > 0;
    }
  // brick operators: the step x + omega D^{-1} (b - A x) is fused into the
  // vmult's write-out (k_brick, k_shared_reduce_cls), ping-ponging between x
  // and tmp; the start buffer is chosen so that the last step lands in x
  // (zero start: the first iterate omega D^{-1} b goes to tmp when the
  // remaining count is odd), a final copy otherwise
  int   it  = 0;
  void *cur = start_in_tmp ? tmp : x;
  if (zero_start && iters > 0)
    {
      cur = ((iters - 1) % 2 == 1) ? tmp : x;
      first(cur);
      it = 1;
    }
  gls::RelaxStep rx;
  rx.b     = b;
  rx.d     = mg->invdiag[level];
  rx.omega = mg->omega[level];
  // deferred reductions: apply j writes its boundary partials to slot
  // buffer j % 2 and skips its reduction; apply j + 1 rebuilds those rows in
  // its gather (and stores them into its src); the last apply's reduction
  // runs explicitly below, or is handed to the caller (pend), whose next
  // apply of the operator to x rebuilds it the same way
  const bool    defer = defer_reduce(mg, level);
  if (!defer || pend || it >= iters)
    out64 = nullptr;
  PendingReduce pr;
  // the steps in one resident launch (k_brick_sweeps) where the level
  // qualifies; the same iterates as the per-step launches below
  if (defer && defer_resident() && iters - it >= 2)
    {
      void          *oth = cur == x ? tmp : x;
      void          *s0  = mg->qslot[it % 2][(size_t)level];
      void          *s1  = mg->qslot[(it + 1) % 2][(size_t)level];
      gls::RelaxStep r   = rx;
      r.out64            = out64;
      const int      ns  = iters - it;
      if (gls::brick_sweeps(op, gls::op_vmult_mode(op), cur, oth, s0, s1, ns, r, s))
        {
          // the last sweep (ns - 1) read v[(ns - 1) % 2] and wrote the other
          const bool even = (ns - 1) % 2 == 0;
          pr  = PendingReduce{even ? s0 : s1, even ? cur : oth, rx.b, rx.d, rx.omega, true};
          cur = even ? oth : cur;
          it  = iters;
        }
    }
  for (; it < iters; ++it)
    {
      void          *oth = cur == x ? tmp : x;
      gls::RelaxStep r   = rx;
      if (it + 1 == iters)
        r.out64 = out64;
      if (defer)
        {
          r.defer   = true;
          r.partial = mg->qslot[it % 2][(size_t)level];
          if (pr.valid)
            {
              r.prev_partial = pr.slots, r.prev_src = pr.src;
              r.prev_b = pr.b, r.prev_d = pr.d, r.prev_omega = pr.omega;
            }
        }
      gls::brick_launch(op, gls::op_vmult_mode(op), oth, cur, 0, op->n_bricks,
                        gls::BRICK_RUN | gls::BRICK_REDUCE, s, &r);
      if (defer)
        pr = PendingReduce{r.partial, cur, rx.b, rx.d, rx.omega, true};
      cur = oth;
    }
  if (pr.valid)
    {
      if (pend && cur == x)
        *pend = pr;
      else
        {
          gls::RelaxStep r = rx;
          r.partial        = const_cast<void *>(pr.slots);
          r.out64          = out64;
          gls::brick_launch(op, gls::op_vmult_mode(op), cur, pr.src, 0, 0, gls::BRICK_REDUCE, s,
                            &r);
        }
    }
  if (cur != x)
    {
      const int64_t w = (int64_t)((size_t)op->n_dofs * mg->ts() / 4);
      copy_words(x, cur, w, s);
    }
  if (wrote64)
    *wrote64 = out64 != nullptr && pr.valid;
  return zero_start && iters > 0;
}

void
residual(const glsMG_ *mg, int level, void *t, const void *b, hipStream_t s)
{
  const int64_t n = mg->ops[level]->n_dofs;
  gls::with_real(mg->prec, [&](auto r) {
    using T = decltype(r);
    hipLaunchKernelGGL(k_residual<T>, g1(n), dim3(256), 0, s, (T *)t, (const T *)b, n);
  });
  HIP_THROW(hipGetLastError());
}

// the coarse "preconditioner" once: sol[0] from def[0] (multigrid.cc:465-489):
// relaxation sweeps (the level smoother), the identity (a copy), or the
// coarse solver object (direct, ILU, AMG)
void
coarse_apply(glsMG_ *mg, hipStream_t s, PendingReduce *pend = nullptr)
{
  switch (mg->coarse->kind())
    {
      case gls::CoarseKind::relaxation:
        smooth(mg, 0, mg->sol[0], mg->def[0], true, mg->desc.coarse_n_iterations, s, false, nullptr,
               pend);
        break;
      case gls::CoarseKind::identity:
        copy_words(mg->sol[0], mg->def[0], (int64_t)((size_t)mg->ops[0]->n_dofs * mg->ts() / 4), s);
        break;
      default:
        mg->coarse->apply(mg->sol[0], (const void *)mg->def[0], s);
    }
}

// Multigrid::level_v_step (deal.II default V-cycle): solution[l] from defect[l]
void v_step_body(glsMG_ *mg, int l, hipStream_t s);
void
v_step(glsMG_ *mg, int l, hipStream_t s)
{
  // a deferred reduction handed to the next transfer (rq_level / pp_level)
  // must not outlive a failed step: a later transfer of that level would read
  // stale slots and vectors
  try
    {
      v_step_body(mg, l, s);
    }
  catch (...)
    {
      mg->rq_level = -1;
      mg->pp_level = -1;
      throw;
    }
}

void
v_step_body(glsMG_ *mg, int l, hipStream_t s)
{
  const std::vector<std::string> &sec = mg->sec[(size_t)l];
  if (l == 0 && mg->desc.coarse_iterate)
    {
      gls::Section sc(sec[5], s);
      mg->coarse->gmres(mg->sol[0], mg->def[0], [&] { coarse_apply(mg, s); }, s);
      return;
    }
  // the last smoothing step's reduction of a level below the finest handed
  // to the prolongation that reads its result (GLS_MG_DEFER=0: off)
  auto hand_over = [&](int lc, const PendingReduce &p) {
    if (!p.valid)
      return;
    mg->pp_level = lc + 1, mg->pp_slots = p.slots, mg->pp_prev = p.src;
    mg->pp_b = p.b, mg->pp_d = p.d, mg->pp_omega = p.omega;
  };
  const bool pro_ok = [&](int lc) {
    return mg->prec == GLS_F32 && mg->dim == 3 && lc + 1 < (int)mg->ops.size() &&
           defer_reduce(mg, lc);
  }(l);
  if (l == 0)
    {
      gls::Section  sc(sec[5], s);
      PendingReduce pc;
      coarse_apply(mg, s, pro_ok ? &pc : nullptr);
      hand_over(0, pc);
      return;
    }
  const int nit = mg->desc.smoothing_n_iterations;
  // pre-smoothing from a zero initial guess (MGSmootherPrecondition::apply);
  // its first relaxation also zeroes the coarser defect for the restriction
  // (and on the finest level converts the outer defect, mg->top_b64)
  FirstRelax fr;
  fr.zero       = (uint32_t *)mg->def[l - 1];
  fr.zero_words = (int64_t)((size_t)mg->ops[l - 1]->n_dofs * mg->ts() / 4);
  fr.b64        = l == (int)mg->ops.size() - 1 ? mg->top_b64 : nullptr;
  PendingReduce pend;
  bool          folded;
  {
    gls::Section sc(sec[0], s);
    folded = smooth(mg, l, mg->sol[l], mg->def[l], true, nit, s, false, &fr, &pend);
    if (!folded && fr.b64)
      {
        const int64_t n = mg->ops[l]->n_dofs;
        hipLaunchKernelGGL((k_convert<double, float>), g1(n), dim3(256), 0, s,
                           (float *)mg->def[l], fr.b64, n);
        HIP_THROW(hipGetLastError());
      }
  }
  // residual t = defect - A solution (fused into the brick vmult's write-out
  // and shared-node reduction for brick operators)
  std::unique_ptr<gls::Section> sc_res(new gls::Section(sec[1], s));
  if (gls::fused_relax_ok(mg->ops[l]))
    {
      gls::RelaxStep rs;
      rs.b     = mg->def[l];
      rs.omega = 1.0;
      rs.keep  = false;
      if (pend.valid) // the pre-smoothing's last reduction, rebuilt in this gather
        {
          rs.prev_partial = pend.slots, rs.prev_src = pend.src;
          rs.prev_b = pend.b, rs.prev_d = pend.d, rs.prev_omega = pend.omega;
        }
      // the residual's own reduction deferred into the restriction's gather
      // (its only reader: the prolongation overwrites tmp afterwards), into
      // the slot buffer the pre-smoothing's pending slots do not occupy
      if (defer_reduce(mg, l) && mg->prec == GLS_F32 && mg->ops[l]->dim == 3)
        {
          void *q0   = mg->qslot[0][(size_t)l], *q1 = mg->qslot[1][(size_t)l];
          rs.defer   = true;
          rs.partial = pend.valid && pend.slots == q0 ? q1 : q0;
        }
      gls::brick_launch(mg->ops[l], gls::op_vmult_mode(mg->ops[l]), mg->tmp[l], mg->sol[l], 0,
                        mg->ops[l]->n_bricks, gls::BRICK_RUN | gls::BRICK_REDUCE, s, &rs);
      if (rs.defer) // (set only once the launch went through)
        mg->rq_level = l, mg->rq_slots = rs.partial, mg->rq_x = mg->sol[l], mg->rq_b = mg->def[l];
    }
  else
    {
      gls::op_vmult_device(mg->ops[l], mg->tmp[l], mg->sol[l], s);
      residual(mg, l, mg->tmp[l], mg->def[l], s);
    }
  sc_res.reset();
  // restrict
  {
    gls::Section sc(sec[2], s);
    if (!folded)
      {
        const int64_t w = (int64_t)((size_t)mg->ops[l - 1]->n_dofs * mg->ts() / 4);
        zero_words(mg->def[l - 1], w, s);
      }
    transfer(mg, 1, l, mg->def[l - 1], mg->tmp[l], s);
  }
  mg->rq_level = -1;
  v_step(mg, l - 1, s);
  // prolongate and add the coarse correction; with an odd number of fused
  // smoothing steps to follow it goes out of place into tmp, so the
  // ping-pong ends in sol without a copy
  const bool odd = gls::fused_relax_ok(mg->ops[l]) && nit % 2 == 1;
  {
    gls::Section sc(sec[3], s);
    if (odd)
      transfer(mg, 0, l, mg->tmp[l], mg->sol[l - 1], s, mg->sol[l]);
    else
      transfer(mg, 0, l, mg->sol[l], mg->sol[l - 1], s);
  }
  mg->pp_level = -1;
  // post-smoothing (MGSmootherPrecondition::smooth -> step); on the finest
  // level its last step also writes the FP64 result (copy_from_mg folded)
  bool          wrote = false;
  PendingReduce pp;
  {
    gls::Section sc(sec[4], s);
    smooth(mg, l, mg->sol[l], mg->def[l], false, nit, s, odd, nullptr, pro_ok ? &pp : nullptr,
           l == (int)mg->ops.size() - 1 ? mg->top_out64 : nullptr, &wrote);
  }
  if (l == (int)mg->ops.size() - 1)
    mg->top_out64_done = wrote;
  hand_over(l, pp);
}

// Relaxation-factor estimate of PreconditionRelaxation with relaxation = 0
// and EigenvalueAlgorithm::power_iteration (multigrid.cc:294-305, 353-369).
// Restates deal.II (>= 9.4, not vendored):
//   internal::PreconditionChebyshevImplementation::set_initial_guess:
//     x_i = i % 11 on the global index, minus the mean; then
//     AdditionalData::constraints.set_zero(x)
//   power_iteration(matrix, x, D^{-1}, eig_cg_n_iterations):
//     x /= |x|; repeat: y = D^{-1} A x; lambda = x . y; x = y / |y|;
//     return |lambda|
//   estimate_eigenvalues: max_eigenvalue_estimate = 1.2 * lambda (safety
//     factor), and PreconditionRelaxation::estimate_eigenvalues then sets
//     omega = 2 / (alpha + max), alpha = max / smoothing_range.
// The index i is this library's dof numbering (node-major), not deal.II's
// DoFHandler numbering, so the start vector is the same formula on a
// different numbering (deviation).  All reductions stay on the
// device; the host reads lambda once after the last iteration.
template <typename T>
void
power_iteration_t(glsMG_ *mg, int l, hipStream_t s)
{
  // enqueues the estimate on s; the Rayleigh quotient x.y of the last step
  // ends in d_acc[acc_off[l] + 2 nb] (gls_mg_setup collects it)
  glsOp         op = mg->ops[l];
  const int64_t n  = op->n_dofs;
  void         *x = mg->sol[l], *y = mg->tmp[l];
  const int64_t nb   = (n + 255) / 256;
  double       *part = mg->d_acc + mg->acc_off[l], *scal = part + 2 * nb;
  // start vector on the device: mean of i % 11 over [0, n) in closed form
  const int64_t q11  = n / 11, r11 = n % 11;
  const double  mean = n > 0 ? (double)(q11 * 55 + r11 * (r11 - 1) / 2) / (double)n : 0.0;
  // "constrained" for the start vector: the Dirichlet mask and the
  // components the node constraints eliminate
  hipLaunchKernelGGL(k_power_start<T>, g1(n), dim3(256), 0, s, (T *)x,
                     op->nc.n ? op->nc.d_cmask_all : op->d_node_cmask, op->dim + 1, mean, part,
                     n);
  hipLaunchKernelGGL(k_power_finish, dim3(1), dim3(256), 0, s, (const double *)part, nb, scal);
  hipLaunchKernelGGL(k_scale_dev<T>, g1(n), dim3(256), 0, s, (T *)x, (const T *)x,
                     (const double *)scal, n);
  HIP_THROW(hipGetLastError());
  HIP_THROW(hipMemsetAsync(scal, 0, 2 * sizeof(double), s));
  for (int it = 0; it < mg->desc.smoothing_eig_n_iterations; ++it)
    {
      gls::op_vmult_device(op, y, x, s);
      hipLaunchKernelGGL(k_power_step<T>, g1(n), dim3(256), 0, s, (T *)y, (const T *)x,
                         (const T *)mg->invdiag[l], part, n);
      hipLaunchKernelGGL(k_power_finish, dim3(1), dim3(256), 0, s, (const double *)part, nb,
                         scal);
      hipLaunchKernelGGL(k_scale_dev<T>, g1(n), dim3(256), 0, s, (T *)x, (const T *)y,
                         (const double *)scal, n);
      HIP_THROW(hipGetLastError());
    }
}

} // namespace

extern "C" {

glsStatus
gls_mg_create(const glsMGDesc *desc, const glsOp *levels, const uint32_t *const *child,
              glsMG *out)
{
  GLS_TRY
  if (!desc || !levels || !out || desc->n_levels < 1)
    throw std::runtime_error("gls_mg_create: invalid arguments");
  auto *mg   = new glsMG_();
  mg->desc   = *desc;
  mg->prec   = levels[0]->prec;
  mg->dim    = levels[0]->dim;
  mg->degree = levels[desc->n_levels - 1]->degree;
  mg->nc     = mg->dim + 1;
  const int nl_levels = desc->n_levels;
  for (int l = 0; l < nl_levels; ++l)
    {
      glsOp op = levels[l];
      // every level shares dim, precision and degree, except that the
      // coarsest may be of lower degree (FE_Q_iso_Q1: Q1 on the sub-cells)
      if (!op || op->prec != mg->prec || op->dim != mg->dim ||
          (l > 0 && op->degree != mg->degree) || op->degree > mg->degree)
        throw std::runtime_error("gls_mg_create: level operators must share dim, degree and "
                                 "precision (the coarsest may be of lower degree)");
      // partitioned (rank-local) level operators: the transfers
      // (prolongate_add / restrict_add / interpolate) and the relaxation
      // step serve the host-driven distributed multigrid (glsdist.py);
      // setup / V-cycle / smooth are single-domain and refuse them
      mg->partitioned = mg->partitioned || op->n_owned_nodes != op->n_nodes;
      mg->ops.push_back(op);
    }
  if (desc->coarse_amg && mg->partitioned)
    throw std::runtime_error("gls_mg_create: the AMG coarse solver is single-domain");
  if (nl_levels > 1 && (!child || mg->degree > 2))
    throw std::runtime_error("gls_mg_create: child lattices required (degree <= 2)");
  // 1D prolongation per coarse degree: parent GLL basis at the child
  // lattice points (for a Q1 coarse level under Q_k: the iso-Q1 embedding)
  for (int k = 1; k <= 2; ++k)
    {
      Basis1D b(k);
      for (int I = 0; I <= 2 * k; ++I)
        {
          const int    c = I / k > 1 ? 1 : I / k;
          const double x = 0.5 * (c + b.nodes[I - c * k]);
          for (int j = 0; j <= k; ++j)
            {
              double v = 1;
              for (int m = 0; m <= k; ++m)
                if (m != j)
                  v *= (x - b.nodes[m]) / (b.nodes[j] - b.nodes[m]);
              mg->P[k][I][j] = v;
            }
        }
    }
  mg->d_child.assign(nl_levels, nullptr);
  mg->d_weight.assign(nl_levels, nullptr);
  mg->h_weight.assign(nl_levels, std::vector<double>());
  mg->weight_nc_version.assign(nl_levels, 0);
  for (int l = 1; l < nl_levels; ++l)
    {
      glsOp         cop = mg->ops[l - 1], fop = mg->ops[l];
      const int     L   = 2 * cop->degree + 1;
      const int     nl  = mg->dim == 3 ? L * L * L : L * L;
      const int64_t nch = cop->n_cells * nl;
      std::vector<uint32_t> ch(child[l], child[l] + nch);
      // a periodic node map of the fine level (glsOpDesc.node_master): the
      // lattices address unknowns, so they go through it before ownership and
      // weights are assigned (no coarse cell's lattice holds a node twice: the
      // coarse operator refused a cell that lists one twice)
      if (!fop->h_master.empty())
        for (uint32_t &fn : ch)
          {
            if ((int64_t)(fn & ~NOT_OWNER) >= fop->n_nodes)
              throw std::runtime_error("gls_mg_create: child lattice node out of range");
            fn = (uint32_t)fop->h_master[fn & ~NOT_OWNER] | (fn & NOT_OWNER);
          }
      std::vector<uint8_t>  seen((size_t)fop->n_nodes, 0);
      // ownership of the fine nodes: the first coarse cell touching a node
      // owns it; a lattice that already carries NOT_OWNER bits (bit 31,
      // e.g. the global-first owners of a partitioned hierarchy) is taken as
      // given
      bool flagged = false;
      for (uint32_t fn : ch)
        flagged = flagged || (fn & NOT_OWNER);
      for (uint32_t &fn : ch)
        {
          if ((int64_t)(fn & ~NOT_OWNER) >= fop->n_nodes)
            throw std::runtime_error("gls_mg_create: child lattice node out of range");
          if (!flagged && seen[fn])
            fn |= NOT_OWNER;
          seen[fn & ~NOT_OWNER] = 1;
        }
      // the transfer kernels walk the coarse operator's cells in its own
      // (possibly brick-discovered) order: rows follow it
      if (!cop->cell_perm.empty())
        {
          std::vector<uint32_t> pc(ch.size());
          for (int64_t c = 0; c < cop->n_cells; ++c)
            std::copy(ch.begin() + gls::ext_cell(cop, c) * nl,
                      ch.begin() + (gls::ext_cell(cop, c) + 1) * nl, pc.begin() + c * nl);
          ch.swap(pc);
        }
      std::vector<double> w((size_t)fop->n_dofs, 0.0);
      for (int64_t nd = 0; nd < fop->n_nodes; ++nd)
        for (int c = 0; c < mg->nc; ++c)
          w[nd * mg->nc + c] = (((fop->h_cmask[nd] >> c) & 1) || !seen[nd]) ? 0.0 : 1.0;
      HIP_THROW(hipMalloc((void **)&mg->d_child[l], nch * sizeof(uint32_t)));
      HIP_THROW(hipMemcpy(mg->d_child[l], ch.data(), nch * sizeof(uint32_t),
                          hipMemcpyHostToDevice));
      mg->h_weight[l] = w;
      gls::upload_real(mg->prec, &mg->d_weight[l], w);
    }
  for (int l = 0; l < nl_levels; ++l)
    {
      const size_t bytes = (size_t)mg->ops[l]->n_dofs * mg->ts();
      void        *p[4];
      for (auto &q : p)
        {
          HIP_THROW(hipMalloc(&q, std::max<size_t>(bytes, 1)));
          HIP_THROW(hipMemset(q, 0, std::max<size_t>(bytes, 1)));
        }
      mg->invdiag.push_back(p[0]);
      mg->sol.push_back(p[1]);
      mg->def.push_back(p[2]);
      mg->tmp.push_back(p[3]);
    }
  mg->omega.assign(nl_levels, 1.0);
  mg->lambda.assign(nl_levels, 0.0);
  for (int l = 0; l < nl_levels; ++l)
    {
      const std::string b = "gmg::vmult::level_" + std::to_string(l);
      mg->sec.push_back({b + "::0_pre_smoother_step", b + "::1_residual_step",
                         b + "::2_restriction", b + "::3_prolongation",
                         b + "::5_post_smoother_step", b});
    }
  int64_t acc_total = 0;
  for (int l = 0; l < nl_levels; ++l)
    {
      mg->acc_off.push_back(acc_total);
      acc_total += 2 * ((mg->ops[l]->n_dofs + 255) / 256) + 2;
    }
  HIP_THROW(hipMalloc((void **)&mg->d_acc, std::max<int64_t>(acc_total, 1) * sizeof(double)));
  mg->coarse = gls::CoarseSolver::create(mg->desc, mg->ops[0], mg->prec, mg->partitioned);
  *out = mg;
  GLS_CATCH
}

void
gls_mg_destroy(glsMG mg)
{
  if (!mg)
    return;
  for (auto *p : mg->d_child)
    if (p)
      (void)hipFree(p);
  for (auto *p : mg->d_weight)
    if (p)
      (void)hipFree(p);
  for (auto *v : {&mg->invdiag, &mg->sol, &mg->def, &mg->tmp, &mg->qslot[0], &mg->qslot[1]})
    for (void *p : *v)
      if (p)
        (void)hipFree(p);
  if (mg->d_acc)
    (void)hipFree(mg->d_acc);
  for (hipStream_t st : mg->side)
    (void)hipStreamDestroy(st);
  for (hipEvent_t ev : mg->side_ev)
    (void)hipEventDestroy(ev);
  mg->stage.release();
  delete mg;
}

glsStatus
gls_mg_setup(glsMG mg, void *stream)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_setup: null handle");
  if (mg->partitioned)
    throw std::runtime_error("gls_mg_setup: partitioned levels are set up by the host-driven "
                             "distributed multigrid (glsdist.py)");
  // the fused and resident smoothers run the cell loop: levels stay matrix-free
  for (size_t l = 0; l < mg->ops.size(); ++l)
    if (mg->ops[l]->matrix_based)
      throw std::runtime_error("gls_mg_setup: level " + std::to_string(l) +
                               " is in matrix-based mode (gls_op_set_matrix_based); level "
                               "operators stay matrix-free");
  mg->coarse->check_operator();
  // node constraints: the transfer weights are zero on the eliminated fine
  // components, as on the Dirichlet ones; rebuilt when a level's rows changed
  for (size_t l = 1; l < mg->ops.size(); ++l)
    {
      const glsOp fop = mg->ops[l];
      if (mg->weight_nc_version[l] == fop->nc_version)
        continue;
      gls::DeviceScope dev(fop->device);
      HIP_THROW(hipStreamSynchronize((hipStream_t)stream));
      std::vector<double> w = mg->h_weight[l];
      for (int64_t i = 0; i < fop->nc.n; ++i)
        w[(size_t)(fop->nc.h_node[(size_t)i] * mg->nc + fop->nc.h_comp[(size_t)i])] = 0.0;
      gls::upload_real(mg->prec, &mg->d_weight[l], w, false);
      mg->weight_nc_version[l] = fop->nc_version;
    }
  // every allocation and launch of the setup (the AMG hierarchy included)
  // on the levels' device; the caller's current device is restored
  gls::DeviceScope dev(mg->ops[0]->device);
  hipStream_t      s  = (hipStream_t)stream;
  gls::Section     sec_("gmg::initialize", s);
  const size_t     nl = mg->ops.size();
  // the smoother's slot buffers for deferred reductions (smooth)
  for (int q = 0; q < 2; ++q)
    {
      mg->qslot[q].resize(nl, nullptr);
      for (size_t l = 0; l < nl; ++l)
        if (!mg->qslot[q][l] && gls::deferred_reduce_ok(mg->ops[l]))
          HIP_THROW(hipMalloc(&mg->qslot[q][l], std::max<size_t>(16, (size_t)mg->ops[l]->n_slots *
                                                                        (mg->dim + 1) * mg->ts())));
    }
  // the levels are independent here: each level's diagonal and power
  // iteration run on a stream of its own (forked from and joined back into
  // s by events), so the small levels' launch-bound steps overlap the fine
  // level's instead of queueing behind them
  if (mg->side.empty())
    for (size_t l = 0; l < nl; ++l)
      {
        hipStream_t st;
        hipEvent_t  ev;
        HIP_THROW(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIP_THROW(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        mg->side.push_back(st);
        mg->side_ev.push_back(ev);
      }
  hipEvent_t fork;
  HIP_THROW(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
  HIP_THROW(hipEventRecord(fork, s));
  std::vector<char> estimate(nl, 0);
  // enqueued finest level first: its kernels (the longest chain) start while
  // the host is still enqueueing the coarser levels' ~100 short launches each
  for (size_t li = nl; li-- > 0;)
    {
      const size_t l  = li;
      hipStream_t  ls = mg->side[l];
      HIP_THROW(hipStreamWaitEvent(ls, fork, 0));
      // compute_inverse_diagonal (multigrid.cc:290-293)
      {
        gls::Section sc("gmg::initialize::smoother::init0", ls);
        gls::op_inverse_diagonal_device(mg->ops[l], mg->invdiag[l], ls);
      }
      // relaxation = 0: omega from the power-iteration estimate of
      // lambda_max(D^-1 A) (power_iteration_t), estimated on the levels
      // above the coarsest one (multigrid.cc:355-358 with
      // compute_evs_n_levels = 0); the coarse level's smoother is used only
      // by the relaxation coarse solve (coarse_n_iterations > 0), which
      // then gets an estimate too
      if (l == 0 && mg->ops.size() > 1 && mg->desc.coarse_n_iterations <= 0 &&
          mg->desc.compute_evs_n_levels <= 0)
        {
          mg->lambda[l] = 0.0;
          mg->omega[l]  = 1.0;
        }
      else
        {
          gls::Section sc("gmg::initialize::smoother::init1", ls);
          gls::with_real(mg->prec,
                         [&](auto t) { power_iteration_t<decltype(t)>(mg, (int)l, ls); });
          estimate[l] = 1;
        }
      HIP_THROW(hipMemsetAsync(mg->sol[l], 0, (size_t)mg->ops[l]->n_dofs * mg->ts(), ls));
      HIP_THROW(hipEventRecord(mg->side_ev[l], ls));
      HIP_THROW(hipStreamWaitEvent(s, mg->side_ev[l], 0));
    }
  HIP_THROW(hipEventDestroy(fork));
  // collect the Rayleigh quotients (one host sync for all levels)
  std::vector<double> lam(nl, 0.0);
  for (size_t l = 0; l < nl; ++l)
    if (estimate[l])
      {
        const int64_t nb = (mg->ops[l]->n_dofs + 255) / 256;
        HIP_THROW(hipMemcpyAsync(&lam[l], mg->d_acc + mg->acc_off[l] + 2 * nb, sizeof(double),
                                 hipMemcpyDeviceToHost, s));
      }
  HIP_THROW(hipStreamSynchronize(s));
  for (size_t l = 0; l < nl; ++l)
    if (estimate[l])
      {
        const double ev_max = 1.2 * std::abs(lam[l]); // estimate_eigenvalues' safety factor
        mg->lambda[l]       = ev_max;
        if (ev_max > 0)
          {
            const double alpha = mg->desc.smoothing_range > 1.0 ?
                                   ev_max / mg->desc.smoothing_range :
                                   0.9 * ev_max;
            mg->omega[l] = 2.0 / (alpha + ev_max);
          }
        else
          mg->omega[l] = 1.0;
      }
  mg->coarse->setup(mg->sol[0], mg->tmp[0], s);
  HIP_THROW(hipStreamSynchronize(s));
  mg->setup_done = true;
  GLS_CATCH
}

glsStatus
gls_mg_set_coarse_direct(glsMG mg, int method, int max_leaf_cells)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_set_coarse_direct: null handle");
  mg->coarse->set_direct(method, max_leaf_cells);
  GLS_CATCH
}

glsStatus
gls_mg_coarse_direct_info(glsMG mg, glsCoarseDirectInfo *info)
{
  GLS_TRY
  if (!mg || !info)
    throw std::runtime_error("gls_mg_coarse_direct_info: null argument");
  mg->coarse->direct_info(info);
  GLS_CATCH
}

glsStatus
gls_mg_get_relaxation(glsMG mg, int level, double *omega, double *lambda_max)
{
  GLS_TRY
  if (!mg || level < 0 || level >= (int)mg->ops.size())
    throw std::runtime_error("gls_mg_get_relaxation: bad level");
  if (omega)
    *omega = mg->omega[level];
  if (lambda_max)
    *lambda_max = mg->lambda[level];
  GLS_CATCH
}

glsStatus
gls_mg_vcycle(glsMG mg, void *dst, const void *src, void *stream)
{
  GLS_TRY
  if (!mg || !dst || !src)
    throw std::runtime_error("gls_mg_vcycle: null argument");
  hipStream_t s = (hipStream_t)stream;
  gls::Section sec_("gmg::vmult", s);
  // a stall of an earlier (asynchronous) V-cycle is reported before this one
  // runs; a stall of this one as soon as its flag is visible (host-layout
  // vectors: at return)
  gls::mg_check_stall(mg, "gls_mg_vcycle");
  const void *x = mg->stage.in_vec(src, 0, s);
  void       *y = mg->stage.out_vec(dst);
  gls::mg_vcycle_device(mg, y, x, s);
  mg->stage.finish_out(dst, s);
  mg->stage.done(s);
  gls::mg_check_stall(mg, "gls_mg_vcycle");
  GLS_CATCH
}

glsStatus
gls_mg_relax(glsMG mg, int level, void *x, const void *b, const void *ax, const void *inv_diag,
             double omega, int zero_start, void *stream)
{
  GLS_TRY
  if (!mg || level < 0 || level >= (int)mg->ops.size() || !x || !b || !inv_diag ||
      (!zero_start && !ax))
    throw std::runtime_error("gls_mg_relax: bad arguments");
  const int64_t n = mg->ops[level]->n_dofs;
  hipStream_t   s = (hipStream_t)stream;
  gls::with_real(mg->prec, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_relax<T>, g1(n), dim3(256), 0, s, (T *)x, (const T *)b, (const T *)ax,
                       (const T *)inv_diag, (T)omega, zero_start ? 1 : 0, n);
  });
  HIP_THROW(hipGetLastError());
  GLS_CATCH
}

glsStatus
gls_mg_set_vector_layout(glsMG mg, int memory, const int64_t *dof_map)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_set_vector_layout: null handle");
  const size_t ts = mg->desc.outer_precision == GLS_F64 ? 8 : mg->ts();
  mg->stage.set(memory, dof_map, mg->ops.back()->n_dofs, ts);
  GLS_CATCH
}

} // extern "C"

namespace gls
{
void
mg_check_outer(glsMG mg, const glsOp_ *op)
{
  if (mg->desc.outer_precision != GLS_F64)
    throw std::runtime_error("gls_gmres_solve: the multigrid's outer_precision must be GLS_F64 "
                             "(PreconditionerGMG::vmult on VectorType<double>)");
  if (mg->ops.empty() || mg->ops.back()->n_dofs != op->n_dofs)
    throw std::runtime_error("gls_gmres_solve: the multigrid's finest level does not match the "
                             "operator's size");
  if (!mg->setup_done)
    throw std::runtime_error("gls_gmres_solve: the multigrid is not set up (gls_mg_setup)");
}

// a resident smoothing sweep of a level stalled since the last check (its
// neighbour brick was not resident: kernels of other streams held CUs): the
// level now runs one launch per step (gls::brick_sweeps); reported once
void
mg_check_stall(glsMG mg, const char *who)
{
  bool stalled = false;
  for (glsOp op : mg->ops)
    stalled = gls::sweep_stalled(op) || stalled;
  if (stalled)
    throw std::runtime_error(std::string(who) +
                             ": a resident smoothing sweep timed out (co-residency of the "
                             "level's bricks lost, INTEGRATION.md §5); the V-cycle it ran in "
                             "returned NaN, the multigrid now runs one launch per smoothing "
                             "step: repeat the computation");
}

bool
mg_is_linear(glsMG mg)
{
  return !mg->desc.coarse_iterate;
}

void
mg_vcycle_device(glsMG mg, void *dst, const void *src, hipStream_t s)
{
  if (!mg->setup_done)
    throw std::runtime_error("gls_mg_vcycle before gls_mg_setup");
  const int     top = (int)mg->ops.size() - 1;
  const int64_t n   = mg->ops[top]->n_dofs;
  const bool    cvt = mg->desc.outer_precision == GLS_F64 && mg->prec == GLS_F32;
  // copy_to_mg: folded into the finest level's first relaxation (v_step)
  // when the V-cycle has a smoothing level on top (the coarse-only hierarchy
  // has no relaxation to fold into)
  const bool folded = cvt && top > 0 && mg->desc.smoothing_n_iterations > 0;
  if (folded)
    {
      mg->top_b64   = (const double *)src;
      mg->top_out64 = (double *)dst;
    }
  else if (cvt)
    hipLaunchKernelGGL((k_convert<double, float>), g1(n), dim3(256), 0, s,
                       (float *)mg->def[top], (const double *)src, n);
  else
    HIP_THROW(hipMemcpyAsync(mg->def[top], src, n * mg->ts(), hipMemcpyDeviceToDevice, s));
  HIP_THROW(hipGetLastError());
  try
    {
      // (a hipGraph replay of the whole cycle, captured once per setup,
      // measured slower than these direct launches -- 0.539 vs 0.484 ms: the
      // cycle's launches run back to back, there is no launch overhead to
      // remove -- and is on the git tag r4-graph-replay)
      v_step(mg, top, s);
    }
  catch (...)
    {
      mg->top_b64   = nullptr;
      mg->top_out64 = nullptr;
      throw;
    }
  const bool done = mg->top_out64 != nullptr && mg->top_out64_done;
  mg->top_b64        = nullptr;
  mg->top_out64      = nullptr;
  mg->top_out64_done = false;
  // copy_from_mg (unless the last post-smoothing step wrote dst itself)
  if (done)
    ;
  else if (cvt)
    hipLaunchKernelGGL((k_convert<float, double>), g1(n), dim3(256), 0, s, (double *)dst,
                       (const float *)mg->sol[top], n);
  else
    HIP_THROW(hipMemcpyAsync(dst, mg->sol[top], n * mg->ts(), hipMemcpyDeviceToDevice, s));
  HIP_THROW(hipGetLastError());
}
} // namespace gls

extern "C" {

glsStatus
gls_mg_coarse_statistics(glsMG mg, int *n_iterations, int *converged)
{
  GLS_TRY
  if (!mg || !n_iterations || !converged)
    throw std::runtime_error("gls_mg_coarse_statistics: null argument");
  mg->coarse->statistics(n_iterations, converged);
  GLS_CATCH
}

glsStatus
gls_mg_set_coarse_ilu(glsMG mg, const glsILUParams *prm)
{
  GLS_TRY
  if (!mg || !prm)
    throw std::runtime_error("gls_mg_set_coarse_ilu: null argument");
  mg->coarse->set_ilu(*prm);
  GLS_CATCH
}

glsStatus
gls_mg_set_coarse_ilu_device(glsMG mg, int on)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_set_coarse_ilu_device: null argument");
  mg->coarse->set_ilu_device(on != 0);
  GLS_CATCH
}

glsStatus
gls_mg_set_coarse_amg_ilu(glsMG mg, const glsAMGIluParams *prm)
{
  GLS_TRY
  if (!mg || !prm)
    throw std::runtime_error("gls_mg_set_coarse_amg_ilu: null argument");
  mg->coarse->set_amg_ilu(*prm);
  GLS_CATCH
}

glsStatus
gls_mg_coarse_ilu(glsMG mg, glsILU *ilu, double *setup_ms)
{
  GLS_TRY
  if (!mg || !ilu)
    throw std::runtime_error("gls_mg_coarse_ilu: null argument");
  *ilu = mg->coarse->ilu(setup_ms);
  GLS_CATCH
}

glsStatus
gls_mg_coarse_amg(glsMG mg, glsAMG *amg, double *setup_ms)
{
  GLS_TRY
  if (!mg || !amg)
    throw std::runtime_error("gls_mg_coarse_amg: null argument");
  *amg = mg->coarse->amg(setup_ms);
  GLS_CATCH
}

glsStatus
gls_mg_coarse_setup_times(glsMG mg, double *ms3, int *n_colors)
{
  GLS_TRY
  if (!mg || !ms3)
    throw std::runtime_error("gls_mg_coarse_setup_times: null argument");
  mg->coarse->setup_times(ms3, n_colors);
  GLS_CATCH
}

glsStatus
gls_mg_prolongate_add(glsMG mg, int level, void *dst_fine, const void *src_coarse,
                      void *stream)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_prolongate_add: null handle");
  transfer(mg, 0, level, dst_fine, src_coarse, (hipStream_t)stream);
  GLS_CATCH
}

glsStatus
gls_mg_restrict_add(glsMG mg, int level, void *dst_coarse, const void *src_fine, void *stream)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_restrict_add: null handle");
  transfer(mg, 1, level, dst_coarse, src_fine, (hipStream_t)stream);
  GLS_CATCH
}

glsStatus
gls_mg_interpolate(glsMG mg, int level, void *dst_coarse, const void *src_fine, void *stream)
{
  GLS_TRY
  if (!mg)
    throw std::runtime_error("gls_mg_interpolate: null handle");
  transfer(mg, 2, level, dst_coarse, src_fine, (hipStream_t)stream);
  GLS_CATCH
}

glsStatus
gls_mg_smooth(glsMG mg, int level, void *x, const void *b, int zero_initial_guess,
              void *stream)
{
  GLS_TRY
  if (!mg || level < 0 || level >= (int)mg->ops.size())
    throw std::runtime_error("gls_mg_smooth: bad arguments");
  if (!mg->setup_done)
    throw std::runtime_error("gls_mg_smooth before gls_mg_setup");
  smooth(mg, level, x, b, zero_initial_guess != 0, mg->desc.smoothing_n_iterations,
         (hipStream_t)stream);
  GLS_CATCH
}

} // extern "C"
