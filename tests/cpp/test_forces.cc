// test_forces.cc — drag / lift and probe through the C++ facade
// (include/gls_operator.hpp: set_force_faces, surface_force,
// set_probe_points, probe) on the r0 cylinder mesh:
//   p = x, u = 0 on the cylinder's faces gives F = -A_h e_x (A_h: the
//   discrete cylinder's cross-section, times the height in 3D; argv[3]),
//   and the probe at (-D/2, 0[, 0]) returns p = -D/2.
// usage: test_forces dim degree A_h      exit 0 = pass
#include "gls_mesh.h"
#include "gls_operator.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

int
main(int argc, char **argv)
{
  if (argc < 4)
    {
      std::fprintf(stderr, "usage: %s dim degree A_h\n", argv[0]);
      return 2;
    }
  const int    dim = std::atoi(argv[1]), degree = std::atoi(argv[2]);
  const double A_h = std::atof(argv[3]), D = 0.1;
  glsMesh     *mesh = nullptr;
  if (gls_mesh_cylinder(dim, degree, 0, dim == 2 ? 2.2 : 2.5, 0.41, dim == 2 ? 0.2 : 0.5, D, 0.005,
                        &mesh))
    {
      std::fprintf(stderr, "mesh: %s\n", gls_mesh_last_error());
      return 2;
    }
  const int64_t nc = gls_mesh_n_cells(mesh), nn = gls_mesh_n_nodes(mesh);
  const int     n = degree + 1, nq = dim == 3 ? n * n * n : n * n, ncomp = dim + 1;
  std::vector<uint8_t> cmask((size_t)nn, 0);
  std::vector<double>  meas((size_t)nc), hmin((size_t)nc);
  int                  brick[3] = {0, 0, 0};
  if (gls_mesh_cell_measure(mesh, meas.data(), hmin.data()) || gls_mesh_brick(mesh, brick))
    {
      std::fprintf(stderr, "mesh: %s\n", gls_mesh_last_error());
      return 2;
    }
  const uint32_t *cn = gls_mesh_cell_nodes(mesh), *nb = gls_mesh_node_boundary(mesh);
  const double   *X  = gls_mesh_node_coords(mesh);

  // the cell faces whose nodes all lie on the cylinder (boundary id 2)
  std::vector<int64_t> cells;
  std::vector<int32_t> faces;
  for (int64_t c = 0; c < nc; ++c)
    for (int fn = 0; fn < 2 * dim; ++fn)
      {
        const int ax = fn / 2, side = fn % 2;
        bool      all = true;
        for (int i = 0; i < nq && all; ++i)
          {
            const int ia[3] = {i % n, (i / n) % n, i / (n * n)};
            if (ia[ax] == side * degree)
              all = (nb[cn[c * nq + i]] >> GLS_BID_CYLINDER) & 1u;
          }
        if (all)
          {
            cells.push_back(c);
            faces.push_back(fn);
          }
      }
  std::printf("dim %d Q%d: %lld cells, %zu cylinder faces\n", dim, degree, (long long)nc,
              cells.size());

  glsOpDesc d{};
  d.dim           = dim;
  d.degree        = degree;
  d.precision     = GLS_F64;
  d.n_cells       = nc;
  d.n_nodes       = nn;
  d.n_owned_nodes = nn;
  d.cell_nodes    = cn;
  d.node_coords   = X;
  d.node_cmask    = cmask.data();
  d.cell_measure  = meas.data();
  d.cell_hmin     = hmin.data();
  for (int i = 0; i < 3; ++i)
    d.brick[i] = brick[i];

  int fails = 0;
  try
    {
      gls::Operator op(d);
      op.set_vector_layout(GLS_MEM_HOST);
      std::vector<double> v((size_t)nn * ncomp, 0.0);
      for (int64_t i = 0; i < nn; ++i)
        v[(size_t)i * ncomp + dim] = X[i * dim];

      bool thrown = false;
      try
        {
          (void)op.surface_force(v.data());
        }
      catch (const gls::Error &e)
        {
          thrown = true;
          std::printf("error path ok: %s\n", e.what());
        }
      fails += !thrown;

      gls::Parameters prm;
      prm.nu = 1e-3;
      op.set_parameters(prm);
      op.set_force_faces(cells, faces, X);
      const auto F = op.surface_force(v.data());
      double     err = std::fabs(F[0] + A_h);
      for (int c = 1; c < dim; ++c)
        err = std::fmax(err, std::fabs(F[c]));
      std::printf("F = (%.15e, %.15e, %.15e), -A_h = %.15e, rel err %.2e\n", F[0], F[1], F[2],
                  -A_h, err / A_h);
      fails += !(err <= 1e-12 * A_h);
      const auto pf = op.surface_force_faces(dim, v.data());
      double     sum = 0;
      for (size_t f = 0; f < cells.size(); ++f)
        sum += pf[f * dim];
      fails += !(std::fabs(sum - F[0]) <= 1e-14 * A_h);

      std::vector<double> pts((size_t)dim, 0.0);
      pts[0]           = -D / 2;
      const auto found = op.set_probe_points(dim, pts, X);
      const auto val   = op.probe(v.data());
      std::printf("probe at (-D/2, 0): %lld cells, p = %.15e\n", (long long)found[0], val[dim]);
      fails += !(found[0] >= 2);
      fails += !(std::fabs(val[dim] + D / 2) <= 1e-12 * D);
      for (int c = 0; c < dim; ++c)
        fails += !(val[c] == 0.0);
    }
  catch (const std::exception &e)
    {
      std::fprintf(stderr, "exception: %s\n", e.what());
      ++fails;
    }
  gls_mesh_destroy(mesh);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
