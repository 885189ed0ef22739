// ilu-apply: time gls_ilu_vmult (csrc/ilu.hip) on matrices shaped like the
// Q1 coarse system matrices -- kron(node stencil, dense b x b): the 2-D
// 9-point stencil with b = 3 and the 3-D 27-point stencil with b = 4 -- with
// ILU(0) and ILU(1), against
//   (a) the same kernels with one launch per level (GLS_ILU_CHAIN=0) and
//   (b) rocSPARSE csrsv (analysis once, L then U) on the same factors,
// and check that the three results agree.
//
//   ilu-apply [reps per window (100)] [windows (7)]
//
// Per variant the windows alternate (chained, per-level, rocSPARSE, chained,
// ...); a window is `reps` applies between two device events; the table
// gives the median window's microseconds per apply.  Output: one markdown
// table row per matrix and fill level (profiles/ilu/README.md keeps a run).
#include "gls_op.h"

#include <hip/hip_runtime.h>
#include <rocsparse/rocsparse.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#define HIP_OK(e)                                                                    \
  do                                                                                 \
    {                                                                                \
      const hipError_t e_ = (e);                                                     \
      if (e_ != hipSuccess)                                                          \
        throw std::runtime_error(std::string(#e) + ": " + hipGetErrorString(e_));    \
    }                                                                                \
  while (0)
#define SP_OK(e)                                                                     \
  do                                                                                 \
    {                                                                                \
      if ((e) != rocsparse_status_success)                                           \
        throw std::runtime_error(std::string(#e) + " failed");                       \
    }                                                                                \
  while (0)
#define GLS_OK(e)                                                                    \
  do                                                                                 \
    {                                                                                \
      if ((e) != 0)                                                                  \
        throw std::runtime_error(std::string(#e) + ": " + gls_last_error());         \
    }                                                                                \
  while (0)

struct Csr
{
  int64_t              n = 0;
  std::vector<int64_t> rp, ci;
  std::vector<double>  v;
};

// nodes on an m^dim grid, every node coupled to its 3^dim neighbours, b dofs
// per node: nonsymmetric values from a fixed sequence, diagonally dominant
static Csr
stencil_block(int dim, int m, int b)
{
  Csr       A;
  const int mz = dim == 3 ? m : 1;
  A.n          = (int64_t)m * m * mz * b;
  A.rp.push_back(0);
  uint64_t state = 0x9e3779b97f4a7c15ull;
  auto     rnd   = [&]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) / (double)(1ull << 53) * 2.0 - 1.0;
  };
  for (int z = 0; z < mz; ++z)
    for (int y = 0; y < m; ++y)
      for (int x = 0; x < m; ++x)
        for (int c = 0; c < b; ++c)
          {
            const int64_t row   = (((int64_t)z * m + y) * m + x) * b + c;
            double        sum   = 0;
            size_t        dpos  = 0;
            for (int dz = (dim == 3 ? -1 : 0); dz <= (dim == 3 ? 1 : 0); ++dz)
              for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                  {
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx < 0 || xx >= m || yy < 0 || yy >= m || zz < 0 || zz >= mz)
                      continue;
                    const int64_t nb = ((int64_t)zz * m + yy) * m + xx;
                    for (int d = 0; d < b; ++d)
                      {
                        const int64_t col = nb * b + d;
                        const double  v   = rnd();
                        if (col == row)
                          dpos = A.ci.size();
                        else
                          sum += std::fabs(v);
                        A.ci.push_back(col);
                        A.v.push_back(v);
                      }
                  }
            A.v[dpos] = sum + 1.0;
            A.rp.push_back((int64_t)A.ci.size());
          }
  return A;
}

struct DevFactor // one triangular factor for rocSPARSE
{
  rocsparse_int        n = 0, nnz = 0;
  rocsparse_int       *rp = nullptr, *ci = nullptr;
  double              *v = nullptr;
  rocsparse_mat_descr  descr = nullptr;
  rocsparse_mat_info   info  = nullptr;
  void                *buffer = nullptr;
};

static DevFactor
upload_factor(rocsparse_handle h, glsILU ilu, int which, int64_t n)
{
  int64_t nnz = 0;
  GLS_OK(gls_ilu_factors(ilu, which, &nnz, nullptr, nullptr, nullptr));
  std::vector<int64_t> rp((size_t)n + 1), ci((size_t)nnz);
  std::vector<double>  v((size_t)nnz);
  GLS_OK(gls_ilu_factors(ilu, which, &nnz, rp.data(), ci.data(), v.data()));
  std::vector<rocsparse_int> rp32(rp.begin(), rp.end()), ci32(ci.begin(), ci.end());
  DevFactor                  F;
  F.n = (rocsparse_int)n, F.nnz = (rocsparse_int)nnz;
  HIP_OK(hipMalloc((void **)&F.rp, rp32.size() * sizeof(rocsparse_int)));
  HIP_OK(hipMalloc((void **)&F.ci, std::max<size_t>(1, ci32.size()) * sizeof(rocsparse_int)));
  HIP_OK(hipMalloc((void **)&F.v, std::max<size_t>(1, v.size()) * sizeof(double)));
  HIP_OK(hipMemcpy(F.rp, rp32.data(), rp32.size() * sizeof(rocsparse_int), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(F.ci, ci32.data(), ci32.size() * sizeof(rocsparse_int), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(F.v, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
  SP_OK(rocsparse_create_mat_descr(&F.descr));
  SP_OK(rocsparse_set_mat_fill_mode(F.descr, which == 0 ? rocsparse_fill_mode_lower :
                                                           rocsparse_fill_mode_upper));
  SP_OK(rocsparse_set_mat_diag_type(F.descr, which == 0 ? rocsparse_diag_type_unit :
                                                           rocsparse_diag_type_non_unit));
  SP_OK(rocsparse_create_mat_info(&F.info));
  size_t bytes = 0;
  SP_OK(rocsparse_dcsrsv_buffer_size(h, rocsparse_operation_none, F.n, F.nnz, F.descr, F.v, F.rp,
                                     F.ci, F.info, &bytes));
  HIP_OK(hipMalloc(&F.buffer, std::max<size_t>(bytes, 8)));
  SP_OK(rocsparse_dcsrsv_analysis(h, rocsparse_operation_none, F.n, F.nnz, F.descr, F.v, F.rp,
                                  F.ci, F.info, rocsparse_analysis_policy_force,
                                  rocsparse_solve_policy_auto, F.buffer));
  return F;
}

static void
free_factor(DevFactor &F)
{
  (void)hipFree(F.rp), (void)hipFree(F.ci), (void)hipFree(F.v), (void)hipFree(F.buffer);
  if (F.info)
    rocsparse_destroy_mat_info(F.info);
  if (F.descr)
    rocsparse_destroy_mat_descr(F.descr);
  F = DevFactor{};
}

static double
rel_diff(const std::vector<double> &a, const std::vector<double> &b)
{
  double d = 0, s = 0;
  for (size_t i = 0; i < a.size(); ++i)
    d += (a[i] - b[i]) * (a[i] - b[i]), s += b[i] * b[i];
  return std::sqrt(d / std::max(s, 1e-300));
}

static int
run(const char *name, const Csr &A, int fill, double atol, int reps, int windows)
{
  const int64_t      n = A.n;
  const glsILUParams prm{fill, atol, 1.0};
  glsILU             chained = nullptr, perlevel = nullptr;
  setenv("GLS_ILU_CHAIN", "1", 1);
  GLS_OK(gls_ilu_create(n, A.rp.data(), A.ci.data(), A.v.data(), &prm, &chained));
  setenv("GLS_ILU_CHAIN", "0", 1);
  GLS_OK(gls_ilu_create(n, A.rp.data(), A.ci.data(), A.v.data(), &prm, &perlevel));
  unsetenv("GLS_ILU_CHAIN");
  glsILUInfo ic, ip;
  GLS_OK(gls_ilu_info(chained, &ic));
  GLS_OK(gls_ilu_info(perlevel, &ip));
  hipStream_t st = nullptr;
  HIP_OK(hipStreamCreate(&st));
  rocsparse_handle h = nullptr;
  SP_OK(rocsparse_create_handle(&h));
  SP_OK(rocsparse_set_stream(h, st));
  DevFactor L = upload_factor(h, chained, 0, n), U = upload_factor(h, chained, 1, n);
  std::vector<double> b((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    b[(size_t)i] = 1.0 + 0.5 * std::sin(0.37 * (double)i);
  double *src = nullptr, *dst = nullptr, *tmp = nullptr;
  HIP_OK(hipMalloc((void **)&src, (size_t)n * 8));
  HIP_OK(hipMalloc((void **)&dst, (size_t)n * 8));
  HIP_OK(hipMalloc((void **)&tmp, (size_t)n * 8));
  HIP_OK(hipMemcpy(src, b.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  const double one     = 1.0;
  auto         apply   = [&](int variant) {
    if (variant == 0)
      GLS_OK(gls_ilu_vmult(chained, dst, src, st));
    else if (variant == 1)
      GLS_OK(gls_ilu_vmult(perlevel, dst, src, st));
    else
      {
        SP_OK(rocsparse_dcsrsv_solve(h, rocsparse_operation_none, L.n, L.nnz, &one, L.descr, L.v,
                                     L.rp, L.ci, L.info, src, tmp, rocsparse_solve_policy_auto,
                                     L.buffer));
        SP_OK(rocsparse_dcsrsv_solve(h, rocsparse_operation_none, U.n, U.nnz, &one, U.descr, U.v,
                                     U.rp, U.ci, U.info, tmp, dst, rocsparse_solve_policy_auto,
                                     U.buffer));
      }
  };
  // results (also the warm-up of every variant)
  std::vector<double> x[3];
  for (int v = 0; v < 3; ++v)
    {
      HIP_OK(hipMemsetAsync(dst, 0xff, (size_t)n * 8, st));
      for (int i = 0; i < 3; ++i)
        apply(v);
      HIP_OK(hipStreamSynchronize(st));
      x[v].resize((size_t)n);
      HIP_OK(hipMemcpy(x[v].data(), dst, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
  const bool   bitwise = x[0] == x[1];
  const double dsp     = rel_diff(x[0], x[2]);
  const bool   agree   = bitwise && dsp < 1e-11;
  hipEvent_t   e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  std::vector<double> us[3];
  for (int w = 0; w < windows; ++w)
    for (int v = 0; v < 3; ++v)
      {
        HIP_OK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i)
          apply(v);
        HIP_OK(hipEventRecord(e1, st));
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        us[v].push_back(1e3 * (double)ms / reps);
      }
  auto med = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
  };
  auto spread = [](std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return (v.back() - v.front()) / v[v.size() / 2];
  };
  std::printf("| %s | %lld | ILU(%d) | %lld | %d / %d | %d | %d / %d | %d / %d | %.1f | %.1f | "
              "%.1f | %.2f | %.2f | %.0f %% | %s, %.1e |\n",
              name, (long long)n, fill, (long long)(ic.nnz_l + ic.nnz_u), ic.levels_l, ic.levels_u,
              ic.group, ic.launches_l, ic.launches_u, ip.launches_l, ip.launches_u, med(us[0]),
              med(us[1]), med(us[2]), med(us[1]) / med(us[0]), med(us[2]) / med(us[0]),
              100.0 * std::max({spread(us[0]), spread(us[1]), spread(us[2])}),
              bitwise ? "bitwise" : "DIFFER", dsp);
  std::fflush(stdout);
  (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
  (void)hipFree(src), (void)hipFree(dst), (void)hipFree(tmp);
  free_factor(L), free_factor(U);
  rocsparse_destroy_handle(h);
  (void)hipStreamDestroy(st);
  gls_ilu_destroy(chained), gls_ilu_destroy(perlevel);
  return agree ? 0 : 1;
}

int
main(int argc, char **argv)
{
  const int reps    = argc > 1 ? std::atoi(argv[1]) : 100;
  const int windows = argc > 2 ? std::atoi(argv[2]) : 7;
  if (reps < 1 || windows < 1)
    {
      std::fprintf(stderr, "usage: ilu-apply [reps per window] [windows]\n");
      return 2;
    }
  int bad = 0;
  try
    {
      int ndev = 0;
      HIP_OK(hipGetDeviceCount(&ndev));
      if (ndev < 1)
        throw std::runtime_error("no GPU");
      std::printf("| matrix | n | fill | nnz(L+U) | levels L / U | G | launches chained L / U | "
                  "launches per level L / U | chained us | per-level us | rocSPARSE us | "
                  "per-level / chained | rocSPARSE / chained | max spread | chained vs per-level, "
                  "vs rocSPARSE |\n");
      std::printf("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n");
      struct Case
      {
        const char *name;
        int         dim, m, b;
      };
      const Case cases[] = {{"2-D 9-pt 20x20 x3", 2, 20, 3},  {"2-D 9-pt 41x41 x3", 2, 41, 3},
                            {"2-D 9-pt 80x80 x3", 2, 80, 3},  {"3-D 27-pt 8^3 x4", 3, 8, 4},
                            {"3-D 27-pt 13^3 x4", 3, 13, 4}, {"3-D 27-pt 16^3 x4", 3, 16, 4}};
      for (const Case &c : cases)
        {
          const Csr A = stencil_block(c.dim, c.m, c.b);
          bad += run(c.name, A, 0, 1e-12, reps, windows);
          bad += run(c.name, A, 1, 1e-6, reps, windows);
        }
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "ilu-apply: %s\n", e.what());
      return 2;
    }
  std::printf("\n%d disagreements\n", bad);
  return bad == 0 ? 0 : 1;
}
