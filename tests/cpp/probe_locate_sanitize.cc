// probe_locate_sanitize.cc — the probe's point location
// (dealii-ns-gls_amd/csrc/probe_locate.cc, host only) under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Built by tests/test_probe_locate.py with the
// ROCm clang for the host, together with host/mesh.cc and probe_locate.cc;
// locates the pressure-probe points (-+D/2, 0[, 0]) of the r0 cylinder meshes
// (shared mesh nodes: at least two cells each, reference points that
// reproduce the point) and interior / face / vertex / outside points of the
// r1 hypercube.  Any sanitizer report fails the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dealii-ns-gls_amd/csrc/probe_locate.h"
#include "../../include/gls_mesh.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do                                                              \
    {                                                             \
      if (!(c))                                                   \
        {                                                         \
          std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
          ++fails;                                                \
        }                                                         \
    }                                                             \
  while (0)

// the pairs of every point map back onto the point
static void
check_pairs(glsMesh *m, const std::vector<double> &pts, const gls::ProbePairs &pp)
{
  const int       dim = gls_mesh_dim(m), k = gls_mesh_degree(m), n = k + 1;
  const int       nq = dim == 3 ? n * n * n : n * n;
  const uint32_t *cn = gls_mesh_cell_nodes(m);
  const double   *X  = gls_mesh_node_coords(m);
  double          nodes[4];
  gls::gll_nodes(k, nodes);
  const int64_t np = (int64_t)pts.size() / dim;
  CHECK((int64_t)pp.off.size() == np + 1);
  CHECK(pp.xi.size() == pp.cell.size() * (size_t)dim);
  for (int64_t p = 0; p < np; ++p)
    for (int64_t j = pp.off[(size_t)p]; j < pp.off[(size_t)p + 1]; ++j)
      {
        const int64_t c = pp.cell[(size_t)j];
        CHECK(c >= 0 && c < gls_mesh_n_cells(m));
        double x[3] = {0, 0, 0};
        for (int i = 0; i < nq; ++i)
          {
            const int ia[3] = {i % n, (i / n) % n, i / (n * n)};
            double    ph    = 1;
            for (int e = 0; e < dim; ++e)
              {
                const double t = pp.xi[(size_t)j * dim + e];
                CHECK(t >= 0.0 && t <= 1.0);
                double v = 1;
                for (int q = 0; q < n; ++q)
                  if (q != ia[e])
                    v *= (t - nodes[q]) / (nodes[ia[e]] - nodes[q]);
                ph *= v;
              }
            for (int d = 0; d < dim; ++d)
              x[d] += ph * X[(size_t)cn[c * nq + i] * dim + d];
          }
        for (int d = 0; d < dim; ++d)
          CHECK(std::fabs(x[d] - pts[(size_t)p * dim + d]) < 1e-6);
      }
}

static gls::ProbePairs
locate(glsMesh *m, const std::vector<double> &pts)
{
  gls::ProbePairs pp;
  const int       dim = gls_mesh_dim(m);
  gls::locate_points(dim, gls_mesh_degree(m), gls_mesh_n_cells(m), gls_mesh_cell_nodes(m),
                     gls_mesh_n_nodes(m), gls_mesh_node_coords(m), (int64_t)pts.size() / dim,
                     pts.data(), pp);
  check_pairs(m, pts, pp);
  return pp;
}

int
main()
{
  for (int dim = 2; dim <= 3; ++dim)
    for (int k = 1; k <= 2; ++k)
      {
        glsMesh *m = nullptr;
        CHECK(gls_mesh_cylinder(dim, k, 0, dim == 2 ? 2.2 : 2.5, 0.41, dim == 2 ? 0.2 : 0.5, 0.1,
                                0.005, &m) == 0);
        if (!m)
          continue;
        std::vector<double> pts((size_t)2 * dim, 0.0);
        pts[0]                  = -0.05;
        pts[(size_t)dim]        = +0.05;
        const gls::ProbePairs pp = locate(m, pts);
        for (int p = 0; p < 2; ++p)
          CHECK(pp.off[(size_t)p + 1] - pp.off[(size_t)p] >= 2);
        std::printf("cylinder dim %d Q%d: %lld + %lld cells\n", dim, k,
                    (long long)(pp.off[1] - pp.off[0]), (long long)(pp.off[2] - pp.off[1]));
        gls_mesh_destroy(m);
      }
  {
    glsMesh *m = nullptr;
    CHECK(gls_mesh_hypercube(3, 2, 1, &m) == 0);
    if (m)
      {
        const std::vector<double> pts = {0.3,  0.2,  0.7, 0.81, 0.44, 0.13, 0.26, 0.77, 0.9,
                                         0.5,  0.3,  0.2, 0.5,  0.5,  0.5,  2.0,  0.5,  0.5};
        const gls::ProbePairs     pp = locate(m, pts);
        const int64_t             want[6] = {1, 1, 1, 2, 8, 0};
        for (int p = 0; p < 6; ++p)
          CHECK(pp.off[(size_t)p + 1] - pp.off[(size_t)p] == want[p]);
        // no points, and no cells
        gls::ProbePairs none;
        gls::locate_points(3, 2, gls_mesh_n_cells(m), gls_mesh_cell_nodes(m), gls_mesh_n_nodes(m),
                           gls_mesh_node_coords(m), 0, nullptr, none);
        CHECK(none.off.size() == 1 && none.cell.empty());
        gls::locate_points(3, 2, 0, nullptr, gls_mesh_n_nodes(m), gls_mesh_node_coords(m), 6,
                           pts.data(), none);
        CHECK(none.off.size() == 7 && none.cell.empty());
        bool thrown = false;
        try
          {
            gls::locate_points(4, 2, 0, nullptr, 0, nullptr, 0, nullptr, none);
          }
        catch (const std::exception &)
          {
            thrown = true;
          }
        CHECK(thrown);
        gls_mesh_destroy(m);
      }
  }
  std::printf("probe location sanitizer run: %d failures\n", fails);
  return fails ? 1 : 0;
}
