// periodic_sanitize.cc — gls_mesh_periodic_nodes (host/mesh.cc) under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Built by
// tests/test_periodic_mesh.py with the ROCm clang for the host, together with
// host/mesh.cc: the y (and z) walls of the 2D and 3D cylinder meshes paired
// into an exactly sized map, idempotence, the chains of the 3D edges, no pair
// at all, and each refusal (direction out of range, a curved id, unequal
// counts, a node without partner, null arguments).  Any sanitizer report fails
// the run.
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

// the map of the pairs; returns the number of slaves (-1: refused)
static int64_t
pairs(glsMesh *m, int n, const int32_t *a, const int32_t *b, const int32_t *dir)
{
  const int            dim = gls_mesh_dim(m);
  const int64_t        nn  = gls_mesh_n_nodes(m);
  std::vector<int64_t> master((size_t)nn, -7);
  if (gls_mesh_periodic_nodes(m, n, a, b, dir, master.data()) != 0)
    return -1;
  const double   *X   = gls_mesh_node_coords(m);
  const uint32_t *bid = gls_mesh_node_boundary(m);
  int64_t         ns  = 0;
  for (int64_t i = 0; i < nn; ++i)
    {
      const int64_t r = master[(size_t)i];
      CHECK(r >= 0 && r < nn);
      if (r < 0 || r >= nn)
        continue;
      CHECK(master[(size_t)r] == r);
      if (r == i)
        continue;
      ++ns;
      // the slave lies on an eliminated id; it and its master differ only in
      // the paired directions
      uint32_t on_b = 0;
      bool     free_dir[3] = {false, false, false};
      for (int p = 0; p < n; ++p)
        {
          on_b |= (bid[i] >> b[p]) & 1u;
          free_dir[dir[p]] = true;
        }
      CHECK(on_b);
      for (int d = 0; d < dim; ++d)
        if (!free_dir[d])
          CHECK(std::abs(X[i * dim + d] - X[r * dim + d]) < 1e-8);
    }
  return ns;
}

int
main()
{
  const int32_t a[2] = {3, 5}, b[2] = {4, 6}, dir[2] = {1, 2};
  for (int dim = 2; dim <= 3; ++dim)
    for (int degree = 1; degree <= 2; ++degree)
      {
        glsMesh *m = nullptr;
        CHECK(gls_mesh_cylinder(dim, degree, dim == 2 ? 1 : 0, dim == 2 ? 2.2 : 2.5, 0.41,
                                dim == 2 ? 0.2 : 0.5, 0.1, 0.005, &m) == 0);
        if (!m)
          continue;
        const int64_t ny = pairs(m, 1, a, b, dir);
        CHECK(ny > 0);
        CHECK(pairs(m, 0, nullptr, nullptr, nullptr) == 0);
        if (dim == 3)
          {
            const int64_t nz  = pairs(m, 1, a + 1, b + 1, dir + 1);
            const int64_t nyz = pairs(m, 2, a, b, dir);
            CHECK(nz > 0);
            // the nodes on both eliminated walls are counted once
            CHECK(nyz > ny && nyz > nz && nyz < ny + nz);
          }
        // refusals
        const int32_t bad_dir = dim, cyl = GLS_BID_CYLINDER, in = GLS_BID_INFLOW, three = 3;
        CHECK(pairs(m, 1, a, b, &bad_dir) == -1);
        CHECK(std::strstr(gls_mesh_last_error(), "direction") != nullptr);
        CHECK(pairs(m, 1, &cyl, b, dir) == -1);
        CHECK(std::strstr(gls_mesh_last_error(), "curved") != nullptr);
        // inflow against a y-wall: other counts (or, if equal, no partner)
        CHECK(pairs(m, 1, &in, b, dir) == -1);
        // the right ids in the wrong direction: no partner
        const int32_t zero = 0;
        CHECK(pairs(m, 1, a, b, &zero) == -1);
        CHECK(std::strstr(gls_mesh_last_error(), "partner") != nullptr);
        CHECK(pairs(m, 1, &three, &three, dir) == -1);
        std::vector<int64_t> master((size_t)gls_mesh_n_nodes(m));
        CHECK(gls_mesh_periodic_nodes(m, 1, nullptr, b, dir, master.data()) != 0);
        CHECK(gls_mesh_periodic_nodes(m, 1, a, b, dir, nullptr) != 0);
        gls_mesh_destroy(m);
      }
  CHECK(gls_mesh_periodic_nodes(nullptr, 0, nullptr, nullptr, nullptr, nullptr) != 0);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
