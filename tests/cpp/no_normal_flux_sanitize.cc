// no_normal_flux_sanitize.cc — gls_mesh_no_normal_flux (host/mesh.cc) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Built by
// tests/test_slip_constraints.py with the ROCm clang for the host, together
// with host/mesh.cc: the rows of the cylinder on the 2D and 3D cylinder
// meshes (count, then fill, into exactly sized arrays), with and without a
// Dirichlet id, a planar id, the hypercube (no curved id at all) and the
// refusal of a corner inside one id.  Any sanitizer report fails the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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

static int64_t
rows(glsMesh *m, uint32_t slip, uint32_t vel, bool with_normals)
{
  const int dim = gls_mesh_dim(m);
  int64_t   n   = -1;
  CHECK(gls_mesh_no_normal_flux(m, slip, vel, &n, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(n >= 0);
  if (n <= 0)
    return n;
  std::vector<int64_t> nodes((size_t)n);
  std::vector<int32_t> comp((size_t)n);
  std::vector<double>  coef((size_t)n * dim), nrm((size_t)n * dim);
  int64_t              n2 = -1;
  CHECK(gls_mesh_no_normal_flux(m, slip, vel, &n2, nodes.data(), comp.data(), coef.data(),
                                with_normals ? nrm.data() : nullptr) == 0);
  CHECK(n2 == n);
  const double *X = gls_mesh_node_coords(m);
  for (int64_t i = 0; i < n; ++i)
    {
      CHECK(nodes[i] >= 0 && nodes[i] < gls_mesh_n_nodes(m));
      CHECK(i == 0 || nodes[i] > nodes[i - 1]);
      CHECK(comp[i] >= 0 && comp[i] < dim);
      CHECK(coef[(size_t)i * dim + comp[i]] == 0.0);
      if (with_normals)
        {
          // radial on the cylinder (axis through the origin)
          const double x = X[nodes[i] * dim], y = X[nodes[i] * dim + 1], r = std::hypot(x, y);
          const double d = nrm[(size_t)i * dim] * x / r + nrm[(size_t)i * dim + 1] * y / r;
          CHECK(std::abs(std::abs(d) - 1.0) < 1e-13);
        }
    }
  return n;
}

int
main()
{
  const uint32_t cyl = 1u << GLS_BID_CYLINDER;
  for (int dim = 2; dim <= 3; ++dim)
    for (int degree = 1; degree <= 2; ++degree)
      {
        glsMesh *m = nullptr;
        CHECK(gls_mesh_cylinder(dim, degree, dim == 2 ? 1 : 0, dim == 2 ? 2.2 : 2.5, 0.41,
                                dim == 2 ? 0.2 : 0.5, 0.1, 0.005, &m) == 0);
        if (!m)
          continue;
        const int64_t n = rows(m, cyl, 0, true);
        CHECK(n > 0);
        CHECK(rows(m, cyl, 0, false) == n);
        CHECK(rows(m, cyl, cyl, true) == 0);       // the id itself Dirichlet
        CHECK(rows(m, 0x78u, 0, true) == 0);       // planar walls 3..6
        if (dim == 3)
          CHECK(rows(m, cyl, 1u << 5 | 1u << 6, true) < n);
        gls_mesh_destroy(m);
      }
  {
    glsMesh *m = nullptr;
    CHECK(gls_mesh_hypercube(3, 2, 1, &m) == 0);
    if (m)
      {
        CHECK(rows(m, 1u, 0, true) == 0);
        gls_mesh_destroy(m);
      }
  }
  {
    // a quadrilateral with a 45-degree corner between two faces of id 7
    const double  v[8]  = {0, 0, 2, 0, 0, 1, 1, 1};
    const int32_t c[4]  = {0, 1, 2, 3};
    const int32_t bf[4] = {0, 1, 1, 3};
    const int32_t id[2] = {7, 7};
    glsMesh      *m     = nullptr;
    CHECK(gls_mesh_from_coarse(2, 2, 1, 4, v, 1, c, 2, bf, id, &m) == 0);
    if (m)
      {
        int64_t n = 0;
        CHECK(gls_mesh_no_normal_flux(m, 1u << 7, 0, &n, nullptr, nullptr, nullptr, nullptr) != 0);
        CHECK(std::strstr(gls_mesh_last_error(), "corner") != nullptr);
        gls_mesh_destroy(m);
      }
  }
  int64_t n = 0;
  CHECK(gls_mesh_no_normal_flux(nullptr, 1, 0, &n, nullptr, nullptr, nullptr, nullptr) != 0);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
