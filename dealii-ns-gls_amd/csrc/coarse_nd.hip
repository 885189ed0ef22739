// coarse_nd.hip — the nested-dissection sparse direct coarse solver: a
// multifrontal factorisation over the plan of coarse_nd.cc with every pivot
// block stored as an explicit inverse, and the solve as two sweeps of ragged
// batched GEMVs (one launch per tree level and direction).
//
// Per tree node t with own dofs I and boundary dofs B the front on I ∪ B is
// the sum of the node's cell blocks (a leaf) or of its children's updates
// (extend-add).  Z = F_II^-1, W = F_BI Z, G = Z F_IB, U = F_BB - F_BI G; U
// goes into the parent's front.  Stored: row-major [Z | -G] and W.
//   forward  (leaves to root):  f = rhs_I + children's f_B;  f_B -= W f_I
//   backward (root to leaves):  x_I = [Z | -G] [f_I ; x_B]
// Everything is summed in a fixed order: no atomics, no grid-wide waits.
#include "../../include/gls_op.h"
#include "coarse_nd.h"
#include "coarse_nd_solver.h"
#include "common.h"

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <string>

namespace gls
{
namespace
{
void
nd_blas(rocblas_status st, const char *what)
{
  if (st != rocblas_status_success)
    throw std::runtime_error(std::string("nested-dissection coarse solver: ") + what +
                             " failed (rocblas status " + std::to_string((int)st) + ")");
}

inline int
pad4(int n)
{
  return (n + 3) / 4 * 4;
}

// device view of a tree node
struct NdDesc
{
  int32_t ni, nb;   // |I|, |B|
  int32_t ni4, nb4; // padded to 4 (the stored rows and the front vector)
  int32_t ldw;      // row stride of W (= ni4); [Z | -G]'s is ni4 + nb4
  int32_t parent, c0, c1;
  int32_t idx;      // [I | B] plan dofs at d_idx + idx; pinv at d_pinv + 2 idx
  int32_t mapo;     // map[nb] at d_map + mapo
  int64_t zg, w;    // element offsets of [Z | -G] and W in the factor store
  int64_t v;        // front vector [f_I (ni4) | f_B (nb4)] at d_v + v
  int64_t f;        // FP64 front (column major, ld ni + nb) at fronts + f
  int64_t wt, gt;   // FP64 W^T and G (both ni x nb, column major) at tmp + wt / gt
};

// ---------------------------------------------------------------- setup
// cell blocks of one colour into the leaves' fronts: cells of a colour share
// no mesh node, so no two threads of a launch touch the same entry; the
// colours run in a fixed order
template <typename TE>
__global__ void
k_nd_scatter(double *__restrict__ fronts, const int64_t *__restrict__ cfront,
             const int32_t *__restrict__ cm, const int32_t *__restrict__ cpos,
             const TE *__restrict__ E, const int32_t *__restrict__ cells, int64_t n_cells,
             int nloc)
{
  const int64_t per = (int64_t)nloc * nloc;
  const int64_t g   = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_cells * per)
    return;
  const int64_t ci = g / per;
  const int     r  = (int)(g - ci * per);
  const int     j = r / nloc, i = r - j * nloc;
  const int64_t c  = cells[ci];
  const int32_t fi = cpos[c * nloc + i], fj = cpos[c * nloc + j];
  if (fi < 0 || fj < 0)
    return;
  fronts[cfront[c] + (int64_t)fj * cm[c] + fi] += (double)E[c * per + r];
}

// extend-add: the update U (the F_BB block of a child's front) into the
// parent's front through the child's map.  One launch covers the nodes
// `list` of one level that are the same child slot of their parents, so no
// two of them share a parent.
__global__ void
k_nd_extend_add(double *__restrict__ fronts, const NdDesc *__restrict__ desc,
                const int32_t *__restrict__ list, const int32_t *__restrict__ maps)
{
  const NdDesc  d  = desc[list[blockIdx.y]];
  const int64_t nb = d.nb;
  const int64_t g  = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nb * nb)
    return;
  const int64_t  j = g / nb, i = g - j * nb;
  const NdDesc   p  = desc[d.parent];
  const int64_t  m = d.ni + d.nb, mp = p.ni + p.nb;
  const int32_t *mp_ = maps + d.mapo;
  fronts[p.f + (int64_t)mp_[j] * mp + mp_[i]] += fronts[d.f + (d.ni + j) * m + d.ni + i];
}

// the stored factors of every node from the FP64 blocks: row-major
// [Z | -G] (row stride ni4 + nb4) and W (row stride ni4), pads zero
template <typename S>
__global__ void
k_nd_store(S *__restrict__ store, const double *__restrict__ fronts,
           const double *__restrict__ tmp, const NdDesc *__restrict__ desc)
{
  const NdDesc  d   = desc[blockIdx.y];
  const int64_t ldr = d.ni4 + d.nb4;
  const int64_t nzg = (int64_t)d.ni * ldr, nw = (int64_t)d.nb * d.ldw;
  const int64_t g   = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < nzg)
    {
      const int64_t i = g / ldr, j = g - i * ldr;
      double        v = 0;
      if (j < d.ni)
        v = fronts[d.f + j * (d.ni + d.nb) + i];
      else if (j >= d.ni4 && j - d.ni4 < d.nb)
        v = -tmp[d.gt + (j - d.ni4) * d.ni + i];
      store[d.zg + g] = (S)v;
    }
  else if (g < nzg + nw)
    {
      const int64_t e = g - nzg, b = e / d.ldw, i = e - b * d.ldw;
      store[d.w + e] = (S)(i < d.ni ? tmp[d.wt + b * d.ni + i] : 0.0);
    }
}

// ---------------------------------------------------------------- solve
// front vectors of one level: f = [rhs on I ; 0] + the children's f_B, the
// first child first (a gather: two siblings never write the same entry)
__global__ void
k_nd_gather(double *__restrict__ v, const double *__restrict__ rhs,
            const NdDesc *__restrict__ desc, const int32_t *__restrict__ list,
            const int32_t *__restrict__ idx, const int32_t *__restrict__ pinv)
{
  const NdDesc d   = desc[list[blockIdx.y]];
  const int    pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (pos >= d.ni4 + d.nb4)
    return;
  // position in I ∪ B of this entry of the padded vector (-1: a pad)
  const int q = pos < d.ni ? pos : (pos >= d.ni4 && pos - d.ni4 < d.nb ? pos - d.ni4 + d.ni : -1);
  double    s = 0;
  if (q >= 0)
    {
      if (q < d.ni)
        s = rhs[idx[d.idx + q]];
      if (d.c0 >= 0)
        {
          const int32_t *pi = pinv + 2 * (int64_t)d.idx;
          const int32_t  k0 = pi[q], k1 = pi[d.ni + d.nb + q];
          if (k0 >= 0)
            {
              const NdDesc c = desc[d.c0];
              s += v[c.v + c.ni4 + k0];
            }
          if (k1 >= 0)
            {
              const NdDesc c = desc[d.c1];
              s += v[c.v + c.ni4 + k1];
            }
        }
    }
  v[d.v + pos] = s;
}

// four consecutive row entries as FP64 (one 16-byte load of FP32, two of FP64)
template <bool NT>
__device__ __forceinline__ void
nd_load4(const float *p, double m[4])
{
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 t = NT ? __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p)) :
                    *reinterpret_cast<const f4 *>(p);
  m[0] = t.x, m[1] = t.y, m[2] = t.z, m[3] = t.w;
}
template <bool NT>
__device__ __forceinline__ void
nd_load4(const double *p, double m[4])
{
  typedef double d2 __attribute__((ext_vector_type(2)));
  const d2 *q = reinterpret_cast<const d2 *>(p);
  const d2  a = NT ? __builtin_nontemporal_load(q) : q[0];
  const d2  b = NT ? __builtin_nontemporal_load(q + 1) : q[1];
  m[0] = a.x, m[1] = a.y, m[2] = b.x, m[3] = b.y;
}

// a0 / a1 += the 4-entry piece at m times the vector entries at x
template <typename S, bool NT, typename X>
__device__ __forceinline__ void
nd_piece(const S *m, const X *x, double &a0, double &a1)
{
  double t[4];
  nd_load4<NT>(m, t);
  a0 += t[0] * x[0] + t[1] * x[1];
  a1 += t[2] * x[2] + t[3] * x[3];
}

// the pieces [c, n) of a row, stride L, times the vector x (piece p at
// x + 4 p): four 16-byte row loads in flight per lane; returns the next c
template <typename S, bool NT, typename X>
__device__ __forceinline__ int
nd_row_part(const S *row, const X *x, int c, int n, int L, double &a0, double &a1)
{
  for (; c + 3 * L < n; c += 4 * L)
    {
      double t[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        nd_load4<NT>(row + 4 * (c + u * L), t[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        {
          const X *xu = x + 4 * (c + u * L);
          a0 += t[u][0] * xu[0] + t[u][1] * xu[1];
          a1 += t[u][2] * xu[2] + t[u][3] * xu[3];
        }
    }
  for (; c < n; c += L)
    nd_piece<S, NT>(row + 4 * c, x + 4 * c, a0, a1);
  return c;
}

// sum over the 1 << lg lanes that share a row (butterfly, fixed order)
__device__ __forceinline__ double
nd_row_sum(double v, int lg)
{
  for (int o = (1 << lg) >> 1; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
  return v;
}

// forward: f_B -= W f_I on the nodes `list` of one level.  A row is shared
// by 1 << lg lanes (a whole wavefront for long rows, several rows per
// wavefront for short ones); each lane takes 16-byte pieces of the row,
// stride 1 << lg, FP64 partial sums, then the butterfly.
template <typename S, bool NT>
__global__ void __launch_bounds__(256)
  k_nd_forward(double *__restrict__ v, const S *__restrict__ store,
               const NdDesc *__restrict__ desc, const int32_t *__restrict__ list, int lg)
{
  const NdDesc d    = desc[list[blockIdx.y]];
  const int    L    = 1 << lg;
  const int    row  = (int)blockIdx.x * (256 >> lg) + ((int)threadIdx.x >> lg);
  const int    lane = threadIdx.x & (L - 1);
  if (row >= d.nb)
    return;
  const S      *w  = store + d.w + (int64_t)row * d.ldw;
  const double *fi = v + d.v;
  double        a0 = 0, a1 = 0;
  nd_row_part<S, NT>(w, fi, lane, d.ni4 >> 2, L, a0, a1);
  const double s = nd_row_sum(a0 + a1, lg);
  if (lane == 0)
    v[d.v + d.ni4 + row] -= s;
}

// backward: x_I = [Z | -G] [f_I ; x_B] on the nodes `list` of one level,
// x_B gathered from the dofs the levels above have solved -- once per
// workgroup into LDS (XLDS; the launch gives nb4 doubles of it), or entry by
// entry from memory where a boundary set is larger than ND_XB_LDS; every row
// writes its dof of the FP64 solution xs and of the level vector sol itself
constexpr int ND_XB_LDS = 6144; // doubles (48 KB)
template <typename S, typename T, bool NT, bool XLDS>
__global__ void __launch_bounds__(256)
  k_nd_backward(const double *__restrict__ v, double *__restrict__ xs, T *__restrict__ sol,
                const int32_t *__restrict__ free, const S *__restrict__ store,
                const NdDesc *__restrict__ desc, const int32_t *__restrict__ list,
                const int32_t *__restrict__ idx, int lg)
{
  extern __shared__ double xb[];
  const NdDesc d    = desc[list[blockIdx.y]];
  const int    L    = 1 << lg;
  const int    row  = (int)blockIdx.x * (256 >> lg) + ((int)threadIdx.x >> lg);
  const int    lane = threadIdx.x & (L - 1);
  // (the whole workgroup leaves, or none of it before the barrier)
  if ((int)blockIdx.x * (256 >> lg) >= d.ni)
    return;
  const int32_t *ib = idx + d.idx + d.ni;
  if constexpr (XLDS)
    {
      for (int j = threadIdx.x; j < d.nb4; j += 256)
        xb[j] = j < d.nb ? xs[ib[j]] : 0.0;
      __syncthreads();
    }
  if (row >= d.ni)
    return;
  const S      *z  = store + d.zg + (int64_t)row * (d.ni4 + d.nb4);
  const double *fi = v + d.v;
  double        a0 = 0, a1 = 0;
  const int     n1 = d.ni4 >> 2, nch = (d.ni4 + d.nb4) >> 2;
  // the Z part, then the -G part: the lanes go on where the Z part ended
  // (c - n1 is this lane's first piece of it)
  int c = nd_row_part<S, NT>(z, fi, lane, n1, L, a0, a1);
  if constexpr (XLDS)
    nd_row_part<S, NT>(z + 4 * n1, xb, c - n1, nch - n1, L, a0, a1);
  else
    for (; c < nch; c += L)
      {
        double    x0[4];
        const int j = 4 * (c - n1);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          x0[u] = j + u < d.nb ? xs[ib[j + u]] : 0.0;
        nd_piece<S, NT>(z + 4 * c, x0, a0, a1);
      }
  const double s = nd_row_sum(a0 + a1, lg);
  if (lane == 0)
    {
      const int32_t dof = idx[d.idx + row];
      xs[dof]           = s;
      sol[free[dof]]    = (T)s;
    }
}

// lanes per row (log2) for rows of `len` entries: one 16-byte piece per lane
// where the row is shorter than a wavefront's pass
int
lanes_log2(int len)
{
  const int pieces = std::max(1, len / 4);
  int       lg     = 3;
  while (lg < 6 && (1 << lg) < pieces)
    ++lg;
  return lg;
}
} // namespace

struct NdSolver
{
  NdPlan              plan;
  std::vector<NdDesc> desc;
  // per level: the nodes (d_list + lvl_off[l], lvl_n[l] of them), split by
  // child slot for the extend-add (slot 0 first), the largest |I| and |B|
  std::vector<int32_t> lvl_off, lvl_n, lvl_n0, lvl_max_ni, lvl_max_nb, lvl_max_m4;
  int64_t front_entries = 0, tmp_entries = 0, store_entries = 0, v_entries = 0;
  NdDesc  *d_desc = nullptr;
  int32_t *d_list = nullptr, *d_idx = nullptr, *d_pinv = nullptr, *d_map = nullptr;
  double  *d_v = nullptr, *d_xs = nullptr;
  void    *d_store = nullptr;
  bool     store_f32 = false, factored = false, nt = false;
  rocblas_int *d_ipiv = nullptr, *d_info = nullptr;
  int32_t     *d_cpos = nullptr, *d_cm = nullptr;
  int64_t     *d_cfront = nullptr;
  int          cpos_nloc = 0;
  double       ms_factor = 0, ms_store = 0;

  ~NdSolver()
  {
    for (void *p : {(void *)d_desc, (void *)d_list, (void *)d_idx, (void *)d_pinv, (void *)d_map,
                    (void *)d_v, (void *)d_xs, d_store, (void *)d_ipiv, (void *)d_info,
                    (void *)d_cpos, (void *)d_cm, (void *)d_cfront})
      if (p)
        (void)hipFree(p);
  }
};

namespace
{
template <typename V>
void
upload(V **dst, const std::vector<V> &h)
{
  HIP_THROW(hipMalloc((void **)dst, std::max<size_t>(1, h.size()) * sizeof(V)));
  if (!h.empty())
    HIP_THROW(hipMemcpy(*dst, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
}
} // namespace

NdSolver *
nd_solver_create(NdPlan plan_in)
{
  std::unique_ptr<NdSolver> S(new NdSolver);
  S->plan            = std::move(plan_in);
  const NdPlan &plan = S->plan;
  const size_t  nt   = plan.nodes.size();
  S->desc.resize(nt);
  std::vector<int32_t> idx, pinv, maps, list;
  int64_t              ipiv_total = 0;
  // level order: the factor store and the front vectors are laid out level
  // by level, the root first
  for (size_t l = 0; l < plan.levels.size(); ++l)
    {
      // slot-0 children first
      std::vector<int32_t> nodes;
      for (int slot = 0; slot < 2; ++slot)
        for (int32_t t : plan.levels[l])
          {
            const int32_t p = plan.nodes[(size_t)t].parent;
            const int     s = p >= 0 && plan.nodes[(size_t)p].child[1] == t ? 1 : 0;
            if (s == slot)
              nodes.push_back(t);
          }
      int n0 = 0, mi = 0, mb = 0, mm = 0;
      for (int32_t t : nodes)
        {
          const NdNode &nd = plan.nodes[(size_t)t];
          NdDesc       &d  = S->desc[(size_t)t];
          d.ni = (int32_t)nd.own.size(), d.nb = (int32_t)nd.boundary.size();
          d.ni4 = pad4(d.ni), d.nb4 = pad4(d.nb), d.ldw = d.ni4;
          d.parent = nd.parent, d.c0 = nd.child[0], d.c1 = nd.child[1];
          d.idx    = (int32_t)idx.size();
          idx.insert(idx.end(), nd.own.begin(), nd.own.end());
          idx.insert(idx.end(), nd.boundary.begin(), nd.boundary.end());
          d.mapo = (int32_t)maps.size();
          maps.insert(maps.end(), nd.map.begin(), nd.map.end());
          d.zg = S->store_entries;
          S->store_entries += (int64_t)d.ni * (d.ni4 + d.nb4);
          d.w = S->store_entries;
          S->store_entries += (int64_t)d.nb * d.ldw;
          d.v = S->v_entries;
          S->v_entries += d.ni4 + d.nb4;
          d.f = S->front_entries;
          S->front_entries += (int64_t)(d.ni + d.nb) * (d.ni + d.nb);
          d.wt = S->tmp_entries;
          d.gt = d.wt + (int64_t)d.ni * d.nb;
          S->tmp_entries += 2 * (int64_t)d.ni * d.nb;
          ipiv_total += d.ni;
          const NdNode *pp = nd.parent >= 0 ? &plan.nodes[(size_t)nd.parent] : nullptr;
          if (!pp || pp->child[0] == t)
            ++n0;
          mi = std::max(mi, (int)d.ni), mb = std::max(mb, (int)d.nb);
          mm = std::max(mm, (int)(d.ni4 + d.nb4));
        }
      S->lvl_off.push_back((int32_t)list.size());
      S->lvl_n.push_back((int32_t)nodes.size());
      S->lvl_n0.push_back(n0);
      S->lvl_max_ni.push_back(mi), S->lvl_max_nb.push_back(mb), S->lvl_max_m4.push_back(mm);
      list.insert(list.end(), nodes.begin(), nodes.end());
    }
  // inverse maps: per parent position the entry of each child's B (-1: none)
  pinv.assign(2 * idx.size(), -1);
  for (size_t t = 0; t < nt; ++t)
    {
      const NdDesc &d = S->desc[t];
      for (int k = 0; k < 2; ++k)
        {
          const int32_t c = k == 0 ? d.c0 : d.c1;
          if (c < 0)
            continue;
          const NdNode &ch = plan.nodes[(size_t)c];
          for (size_t e = 0; e < ch.map.size(); ++e)
            pinv[2 * (size_t)d.idx + (size_t)k * (size_t)(d.ni + d.nb) + (size_t)ch.map[e]] =
              (int32_t)e;
        }
    }
  upload(&S->d_desc, S->desc);
  upload(&S->d_list, list);
  upload(&S->d_idx, idx);
  upload(&S->d_pinv, pinv);
  upload(&S->d_map, maps);
  HIP_THROW(hipMalloc((void **)&S->d_v, std::max<int64_t>(1, S->v_entries) * 8));
  HIP_THROW(hipMalloc((void **)&S->d_xs, std::max<int64_t>(1, plan.n_dofs) * 8));
  HIP_THROW(hipMalloc((void **)&S->d_ipiv, std::max<int64_t>(1, ipiv_total) * sizeof(rocblas_int)));
  HIP_THROW(hipMalloc((void **)&S->d_info, 2 * nt * sizeof(rocblas_int)));
  // the factors are read once per solve, between the fine levels' sweeps:
  // non-temporal loads by default (the V-cycle measured 1% faster with them
  // than with cacheable loads); GLS_COARSE_ND_NT=0: cacheable
  const char *e = getenv("GLS_COARSE_ND_NT");
  S->nt         = !(e && e[0] == '0');
  return S.release();
}

void
nd_solver_destroy(NdSolver *S)
{
  delete S;
}

const NdPlan &
nd_solver_plan(const NdSolver *S)
{
  return S->plan;
}

void
nd_solver_stats(const NdSolver *S, int64_t *stored_entries, int64_t *stored_bytes,
                double *ms_factor, double *ms_store)
{
  *stored_entries = S->store_entries;
  *stored_bytes   = S->store_entries * (S->store_f32 ? 4 : 8);
  *ms_factor      = S->ms_factor;
  *ms_store       = S->ms_store;
}

bool
nd_solver_factor(NdSolver *S, void *blas_, const NdCellBlocks &cb, bool store_f32, void *stream)
{
  hipStream_t    s    = (hipStream_t)stream;
  rocblas_handle blas = (rocblas_handle)blas_;
  const NdPlan  &plan = S->plan;
  const size_t   nt   = plan.nodes.size();
  const auto     t0   = std::chrono::steady_clock::now();
  if (S->d_store && S->store_f32 != store_f32)
    throw std::runtime_error("nested-dissection coarse solver: storage precision changed");
  S->factored = false;
  // the cells' rows and columns in their leaf's front (once: the mesh and
  // the constraints do not change)
  if (!S->d_cpos || S->cpos_nloc != cb.nloc)
    {
      for (void **q : {(void **)&S->d_cpos, (void **)&S->d_cm, (void **)&S->d_cfront})
        if (*q)
          {
            HIP_THROW(hipFree(*q));
            *q = nullptr;
          }
      const int64_t        nc = plan.n_cells;
      std::vector<int32_t> cpos((size_t)nc * cb.nloc, -1), cm((size_t)nc);
      std::vector<int64_t> cfront((size_t)nc);
      for (int64_t c = 0; c < nc; ++c)
        {
          const int64_t ext = cb.cell_caller ? cb.cell_caller[c] : c;
          const int32_t t   = plan.cell_leaf[(size_t)ext];
          const NdNode &nd  = plan.nodes[(size_t)t];
          cm[(size_t)c]     = (int32_t)(nd.own.size() + nd.boundary.size());
          cfront[(size_t)c] = S->desc[(size_t)t].f;
          for (int i = 0; i < cb.nloc; ++i)
            {
              const int32_t dof = cb.cell_dof[(size_t)c * cb.nloc + i];
              if (dof < 0)
                continue;
              auto it = std::lower_bound(nd.own.begin(), nd.own.end(), dof);
              if (it != nd.own.end() && *it == dof)
                {
                  cpos[(size_t)c * cb.nloc + i] = (int32_t)(it - nd.own.begin());
                  continue;
                }
              it = std::lower_bound(nd.boundary.begin(), nd.boundary.end(), dof);
              if (it == nd.boundary.end() || *it != dof)
                throw std::runtime_error("nested-dissection coarse solver: a cell's dof is in "
                                         "neither set of its leaf");
              cpos[(size_t)c * cb.nloc + i] =
                (int32_t)(nd.own.size() + (size_t)(it - nd.boundary.begin()));
            }
        }
      upload(&S->d_cpos, cpos);
      upload(&S->d_cm, cm);
      upload(&S->d_cfront, cfront);
      S->cpos_nloc = cb.nloc;
    }
  // memory: the FP64 fronts and W / G blocks during the setup, the stored
  // factors after it
  const size_t store_bytes = (size_t)std::max<int64_t>(1, S->store_entries) * (store_f32 ? 4 : 8);
  const size_t work_bytes  = (size_t)std::max<int64_t>(1, S->front_entries + S->tmp_entries) * 8;
  {
    size_t free_b = 0, total_b = 0;
    HIP_THROW(hipMemGetInfo(&free_b, &total_b));
    const size_t need = work_bytes + (S->d_store ? 0 : store_bytes);
    if (need > free_b)
      throw std::runtime_error(
        "nested-dissection coarse solver: the factors need " + std::to_string(need >> 20) +
        " MiB of device memory (" + std::to_string(store_bytes >> 20) + " stored, " +
        std::to_string(work_bytes >> 20) + " during the setup), " + std::to_string(free_b >> 20) +
        " MiB are free");
  }
  double *work = nullptr;
  HIP_THROW(hipMalloc((void **)&work, work_bytes));
  double              *fronts = work, *tmp = work + S->front_entries;
  rocblas_atomics_mode am     = rocblas_atomics_allowed;
  rocblas_pointer_mode pm     = rocblas_pointer_mode_host;
  bool                 ok     = true;
  try
    {
      nd_blas(rocblas_get_atomics_mode(blas, &am), "get atomics mode");
      nd_blas(rocblas_get_pointer_mode(blas, &pm), "get pointer mode");
      // run-to-run identical factors: no atomics in the GEMMs
      nd_blas(rocblas_set_atomics_mode(blas, rocblas_atomics_not_allowed), "set atomics mode");
      nd_blas(rocblas_set_pointer_mode(blas, rocblas_pointer_mode_host), "set pointer mode");
      nd_blas(rocblas_set_stream(blas, s), "rocblas_set_stream");
      HIP_THROW(hipMemsetAsync(work, 0, work_bytes, s));
      HIP_THROW(hipMemsetAsync(S->d_info, 0, 2 * nt * sizeof(rocblas_int), s));
      const int64_t per = (int64_t)cb.nloc * cb.nloc;
      for (int k = 0; k < cb.n_colors; ++k)
        {
          const int64_t cnt = cb.color_begin[k + 1] - cb.color_begin[k];
          if (cnt == 0)
            continue;
          const dim3     grid((unsigned)((cnt * per + 255) / 256));
          const int32_t *cells = cb.d_color_cells + cb.color_begin[k];
          if (cb.f64)
            hipLaunchKernelGGL(k_nd_scatter<double>, grid, dim3(256), 0, s, fronts,
                               (const int64_t *)S->d_cfront, (const int32_t *)S->d_cm,
                               (const int32_t *)S->d_cpos, (const double *)cb.blocks, cells, cnt,
                               cb.nloc);
          else
            hipLaunchKernelGGL(k_nd_scatter<float>, grid, dim3(256), 0, s, fronts,
                               (const int64_t *)S->d_cfront, (const int32_t *)S->d_cm,
                               (const int32_t *)S->d_cpos, (const float *)cb.blocks, cells, cnt,
                               cb.nloc);
        }
      HIP_THROW(hipGetLastError());
      const double one = 1.0, zero = 0.0, mone = -1.0;
      int64_t      ipo = 0;
      std::vector<int64_t> ipiv_off(nt, 0);
      for (size_t t = 0; t < nt; ++t)
        ipiv_off[t] = ipo, ipo += S->desc[t].ni;
      for (size_t l = plan.levels.size(); l-- > 0;)
        {
          for (int32_t t : plan.levels[l])
            {
              const NdDesc     &d = S->desc[(size_t)t];
              const rocblas_int ni = d.ni, nb = d.nb, m = d.ni + d.nb;
              if (ni == 0)
                continue;
              double      *F    = fronts + d.f;
              rocblas_int *ipiv = S->d_ipiv + ipiv_off[(size_t)t];
              nd_blas(rocsolver_dgetrf(blas, ni, ni, F, m, ipiv, S->d_info + 2 * t),
                      "rocsolver_dgetrf");
              if (nb > 0)
                {
                  // G = F_II^-1 F_IB and W^T = F_II^-T F_BI^T by solves with
                  // the LU factors, F_BB -= F_BI G: the error of a solve
                  // scales with |G|, that of a product with the explicit
                  // inverse with |Z| |F_IB|, which is larger by up to the
                  // block's condition number
                  double *Wt = tmp + d.wt, *G = tmp + d.gt;
                  HIP_THROW(hipMemcpy2DAsync(G, (size_t)ni * 8, F + (int64_t)ni * m, (size_t)m * 8,
                                             (size_t)ni * 8, (size_t)nb, hipMemcpyDeviceToDevice,
                                             s));
                  nd_blas(rocsolver_dgetrs(blas, rocblas_operation_none, ni, nb, F, m, ipiv, G,
                                           ni),
                          "rocsolver_dgetrs");
                  nd_blas(rocblas_dgeam(blas, rocblas_operation_transpose, rocblas_operation_none,
                                        ni, nb, &one, F + ni, m, &zero, Wt, ni, Wt, ni),
                          "rocblas_dgeam");
                  nd_blas(rocsolver_dgetrs(blas, rocblas_operation_transpose, ni, nb, F, m, ipiv,
                                           Wt, ni),
                          "rocsolver_dgetrs");
                  nd_blas(rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, nb,
                                        nb, ni, &mone, F + ni, m, G, ni, &one,
                                        F + (int64_t)ni * m + ni, m),
                          "rocblas_dgemm");
                }
              // Z = F_II^-1 in place
              nd_blas(rocsolver_dgetri(blas, ni, F, m, ipiv, S->d_info + 2 * t + 1),
                      "rocsolver_dgetri");
            }
          if (l == 0)
            break;
          // the updates into the parents: first children, then second
          const int32_t *list = S->d_list + S->lvl_off[l];
          const int      n0 = S->lvl_n0[l], n1 = S->lvl_n[l] - n0, mb = S->lvl_max_nb[l];
          const unsigned gx = (unsigned)(((int64_t)mb * mb + 255) / 256);
          if (mb > 0 && n0 > 0)
            hipLaunchKernelGGL(k_nd_extend_add, dim3(gx, (unsigned)n0), dim3(256), 0, s, fronts,
                               (const NdDesc *)S->d_desc, list, (const int32_t *)S->d_map);
          if (mb > 0 && n1 > 0)
            hipLaunchKernelGGL(k_nd_extend_add, dim3(gx, (unsigned)n1), dim3(256), 0, s, fronts,
                               (const NdDesc *)S->d_desc, list + n0, (const int32_t *)S->d_map);
          HIP_THROW(hipGetLastError());
        }
      std::vector<rocblas_int> info(2 * nt);
      HIP_THROW(hipMemcpyAsync(info.data(), S->d_info, info.size() * sizeof(rocblas_int),
                               hipMemcpyDeviceToHost, s));
      HIP_THROW(hipStreamSynchronize(s));
      for (rocblas_int i : info)
        ok = ok && i == 0;
      const auto t1 = std::chrono::steady_clock::now();
      S->ms_factor  = std::chrono::duration<double, std::milli>(t1 - t0).count();
      if (ok)
        {
          if (!S->d_store)
            HIP_THROW(hipMalloc(&S->d_store, store_bytes));
          S->store_f32 = store_f32;
          int64_t most = 1;
          for (const NdDesc &d : S->desc)
            most = std::max(most, (int64_t)d.ni * (d.ni4 + d.nb4) + (int64_t)d.nb * d.ldw);
          const dim3 grid((unsigned)((most + 255) / 256), (unsigned)nt);
          if (store_f32)
            hipLaunchKernelGGL(k_nd_store<float>, grid, dim3(256), 0, s, (float *)S->d_store,
                               (const double *)fronts, (const double *)tmp,
                               (const NdDesc *)S->d_desc);
          else
            hipLaunchKernelGGL(k_nd_store<double>, grid, dim3(256), 0, s, (double *)S->d_store,
                               (const double *)fronts, (const double *)tmp,
                               (const NdDesc *)S->d_desc);
          HIP_THROW(hipGetLastError());
          HIP_THROW(hipStreamSynchronize(s));
          S->factored = true;
        }
      S->ms_store = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1)
                      .count();
    }
  catch (...)
    {
      (void)hipStreamSynchronize(s);
      (void)hipFree(work);
      (void)rocblas_set_atomics_mode(blas, am);
      (void)rocblas_set_pointer_mode(blas, pm);
      throw;
    }
  // the FP64 fronts are not needed by the solve
  HIP_THROW(hipFree(work));
  nd_blas(rocblas_set_atomics_mode(blas, am), "set atomics mode");
  nd_blas(rocblas_set_pointer_mode(blas, pm), "set pointer mode");
  return ok;
}

namespace
{
template <typename S, typename T, bool NT>
void
nd_solve_t(NdSolver *N, const double *rhs, T *sol, const int32_t *d_free, hipStream_t s)
{
  const size_t  nl    = N->lvl_n.size();
  const S      *store = (const S *)N->d_store;
  const NdDesc *desc  = N->d_desc;
  for (size_t l = nl; l-- > 0;)
    {
      const int32_t *list = N->d_list + N->lvl_off[l];
      const unsigned ny   = (unsigned)N->lvl_n[l];
      hipLaunchKernelGGL(k_nd_gather, dim3((unsigned)((N->lvl_max_m4[l] + 255) / 256), ny),
                         dim3(256), 0, s, N->d_v, rhs, desc, list, (const int32_t *)N->d_idx,
                         (const int32_t *)N->d_pinv);
      if (N->lvl_max_nb[l] == 0 || N->lvl_max_ni[l] == 0)
        continue;
      const int lg  = lanes_log2(N->lvl_max_ni[l]);
      const int rpb = 256 >> lg;
      hipLaunchKernelGGL((k_nd_forward<S, NT>),
                         dim3((unsigned)((N->lvl_max_nb[l] + rpb - 1) / rpb), ny), dim3(256), 0, s,
                         N->d_v, store, desc, list, lg);
    }
  for (size_t l = 0; l < nl; ++l)
    {
      if (N->lvl_max_ni[l] == 0)
        continue;
      const int32_t *list = N->d_list + N->lvl_off[l];
      const int      lg   = lanes_log2(N->lvl_max_ni[l] + N->lvl_max_nb[l]);
      const int      rpb  = 256 >> lg;
      const dim3     grid((unsigned)((N->lvl_max_ni[l] + rpb - 1) / rpb), (unsigned)N->lvl_n[l]);
      const int      nb4 = pad4(N->lvl_max_nb[l]);
      if (nb4 <= ND_XB_LDS)
        hipLaunchKernelGGL((k_nd_backward<S, T, NT, true>), grid, dim3(256),
                           (size_t)nb4 * sizeof(double), s, (const double *)N->d_v, N->d_xs, sol,
                           d_free, store, desc, list, (const int32_t *)N->d_idx, lg);
      else
        hipLaunchKernelGGL((k_nd_backward<S, T, NT, false>), grid, dim3(256), 0, s,
                           (const double *)N->d_v, N->d_xs, sol, d_free, store, desc, list,
                           (const int32_t *)N->d_idx, lg);
    }
  HIP_THROW(hipGetLastError());
}
} // namespace

void
nd_solver_solve(NdSolver *N, const double *rhs, void *sol, bool sol_f64, const int32_t *d_free,
                void *stream)
{
  if (!N->factored)
    throw std::runtime_error("nested-dissection coarse solver: solve before a successful setup");
  hipStream_t s = (hipStream_t)stream;
#define GLS_ND_SOLVE(S_, T_)                                              \
  (N->nt ? nd_solve_t<S_, T_, true>(N, rhs, (T_ *)sol, d_free, s) :       \
           nd_solve_t<S_, T_, false>(N, rhs, (T_ *)sol, d_free, s))
  if (N->store_f32 && sol_f64)
    GLS_ND_SOLVE(float, double);
  else if (N->store_f32)
    GLS_ND_SOLVE(float, float);
  else if (sol_f64)
    GLS_ND_SOLVE(double, double);
  else
    GLS_ND_SOLVE(double, float);
#undef GLS_ND_SOLVE
}
} // namespace gls

// ------------------------------------------------------------------ C ABI
struct glsNdPlan_
{
  gls::NdPlan plan;
};

extern "C" {
glsStatus
gls_nd_plan_create(const uint32_t *cell_nodes, int64_t n_cells, int nodes_per_cell,
                   int64_t n_nodes, const int32_t *node_dofs, int max_leaf_cells, glsNdPlan *out)
{
  GLS_TRY
  if (!out)
    throw std::runtime_error("gls_nd_plan_create: null output");
  std::unique_ptr<glsNdPlan_> p(new glsNdPlan_);
  p->plan = gls::nd_make_plan(cell_nodes, n_cells, nodes_per_cell, n_nodes, node_dofs,
                              max_leaf_cells);
  *out    = p.release();
  GLS_CATCH
}

void
gls_nd_plan_destroy(glsNdPlan plan)
{
  delete plan;
}

glsStatus
gls_nd_plan_info(glsNdPlan plan, glsNdPlanInfo *info)
{
  GLS_TRY
  if (!plan || !info)
    throw std::runtime_error("gls_nd_plan_info: null argument");
  const gls::NdPlan &p = plan->plan;
  info->n_dofs         = p.n_dofs;
  info->n_tree_nodes   = (int)p.nodes.size();
  info->depth          = p.depth;
  info->sum_own        = p.sum_own;
  info->stored_entries = p.stored;
  info->max_own        = p.max_own;
  info->max_boundary   = p.max_boundary;
  GLS_CATCH
}

glsStatus
gls_nd_plan_node(glsNdPlan plan, int node, glsNdPlanNode *out)
{
  GLS_TRY
  if (!plan || !out || node < 0 || node >= (int)plan->plan.nodes.size())
    throw std::runtime_error("gls_nd_plan_node: bad arguments");
  const gls::NdNode &nd = plan->plan.nodes[(size_t)node];
  out->parent           = nd.parent;
  out->child[0]         = nd.child[0];
  out->child[1]         = nd.child[1];
  out->level            = nd.level;
  out->n_own            = (int)nd.own.size();
  out->n_boundary       = (int)nd.boundary.size();
  out->n_cells          = (int)nd.cells.size();
  out->own              = nd.own.data();
  out->boundary         = nd.boundary.data();
  out->map              = nd.map.data();
  out->cells            = nd.cells.data();
  GLS_CATCH
}
}
