"""The numpy restatement of the drag / lift integral and the point probe
(tests/forces_ref.py, after simulation.cc:451-541) pinned by known answers,
the deck's force scaling and the CylinderPostprocess file format.  No GPU.

Error scale of a force: S = sum over faces and face points of |f|, the sum
of the absolute per-point contributions (closed-surface sums cancel)."""
import functools

import numpy as np
import pytest

import forces_ref as fr
import glsmesh as gm
from helpers import deck


@functools.lru_cache(maxsize=None)
def _cyl(dim, k, r=0):
    mesh = gm.cylinder(dim, k, r)
    cells, faces = gm.boundary_faces(mesh, 2)
    return mesh, cells, faces


def _field(mesh, p=None, G=None):
    """dof vector of u = G x, p = p(x)."""
    X = np.asarray(mesh.coords)
    v = np.zeros((mesh.n_nodes, mesh.dim + 1))
    if G is not None:
        v[:, :mesh.dim] = X @ np.asarray(G).T
    if p is not None:
        v[:, mesh.dim] = p(X)
    return v.ravel()


_G = {2: np.array([[0.3, -1.1], [0.7, 0.45]]),
      3: np.array([[0.3, -1.1, 0.2], [0.7, 0.45, -0.6], [-0.9, 0.25, 0.8]])}


@pytest.mark.parametrize("dim,k", [(2, 1), (2, 2), (3, 2)])
def test_constant_pressure_closed_surface(dim, k):
    mesh, cells, faces = _cyl(dim, k)
    assert len(cells) == (8 if dim == 2 else 32) and np.all(faces == 0)
    F, S = fr.total_force(mesh, cells, faces, _field(mesh, p=lambda X: np.ones(len(X))), 1e-3)
    print(f"dim {dim} Q{k}: |F| {np.abs(F).max():.2e}, S {S:.3e}")
    assert np.abs(F).max() <= 1e-14


@pytest.mark.parametrize("dim,k", [(2, 1), (2, 2), (3, 2)])
def test_linear_pressure_gives_hole_measure(dim, k):
    mesh, cells, faces = _cyl(dim, k)
    A = fr.hole_measure(mesh)
    for axis in range(2):
        F, _ = fr.total_force(mesh, cells, faces, _field(mesh, p=lambda X: X[:, axis]), 1e-3)
        want = np.zeros(dim)
        want[axis] = -A
        err = np.abs(F - want).max() / A
        print(f"dim {dim} Q{k} p = x_{axis}: F {F}, A_h {A:.12e}, rel err {err:.2e}")
        assert err <= 1e-12


def test_hole_measure_converges():
    exact = np.pi * 0.1 ** 2 / 4
    e0 = fr.hole_measure(_cyl(2, 2, 0)[0]) / exact - 1
    e1 = fr.hole_measure(_cyl(2, 2, 1)[0]) / exact - 1
    print(f"A_h / (pi D^2 / 4) - 1: Q2 r0 {e0:.2e}, Q2 r1 {e1:.2e}")
    assert abs(e1) < abs(e0)


@pytest.mark.parametrize("dim,k", [(2, 1), (2, 2), (3, 2)])
def test_linear_velocity_closed_surface(dim, k):
    mesh, cells, faces = _cyl(dim, k)
    F, S = fr.total_force(mesh, cells, faces,
                          _field(mesh, p=lambda X: np.full(len(X), 0.8), G=_G[dim]), 0.37)
    print(f"dim {dim} Q{k}: |F| {np.abs(F).max():.2e}, S {S:.3e}")
    assert np.abs(F).max() <= 1e-14 * S


def test_linear_velocity_per_face_2d():
    """F_face = sigma . perp(chord), sigma = -p0 I + nu (G + G^T), chord =
    last minus first face node, perp(a, b) = (b, -a): exact for a polynomial
    face curve.  The test of the viscous term."""
    mesh, cells, faces = _cyl(2, 2)
    p0, nu, G = 0.8, 0.37, _G[2]
    pf, sf = fr.surface_force(mesh, cells, faces,
                              _field(mesh, p=lambda X: np.full(len(X), p0), G=G), nu)
    sigma = -p0 * np.eye(2) + nu * (G + G.T)
    n = mesh.degree + 1
    X = np.asarray(mesh.coords)
    for f, (c, fn) in enumerate(zip(cells, faces)):
        assert fn == 0
        line = np.asarray(mesh.cell_nodes[c], dtype=np.int64).reshape(n, n)[:, 0]  # x = 0
        chord = X[line[-1]] - X[line[0]]
        want = sigma @ np.array([chord[1], -chord[0]])
        err = np.abs(pf[f] - want).max()
        print(f"face {f}: F {pf[f]}, want {want}, err {err:.2e}, S_face {sf[f]:.3e}")
        assert err <= 1e-12 * sf[f]


def test_hypercube_all_faces_linear_pressure():
    mesh = gm.hypercube(3, 2, 1)
    cells, faces = gm.boundary_faces(mesh, 0)
    assert len(cells) == 24 and set(faces.tolist()) == set(range(6))
    F, _ = fr.total_force(mesh, cells, faces, _field(mesh, p=lambda X: X[:, 0]), 1e-3)
    print("F", F)
    assert np.abs(F - np.array([1.0, 0.0, 0.0])).max() <= 1e-12


@pytest.mark.parametrize("dim", [2, 3])
def test_rotated_shuffled_mesh_matches_base(dim):
    mesh, cells, faces = _cyl(dim, 2)
    sm = gm.ShuffledMesh(mesh, seed=3, rotate=True)
    sc, sf = gm.boundary_faces(sm, 2)
    assert set(sf.tolist()) == set(range(2 * dim)), sf
    vec = np.random.default_rng(5).standard_normal(mesh.n_dofs)
    svec = vec.reshape(-1, dim + 1)[sm.node_old].ravel()
    F0, S = fr.total_force(mesh, cells, faces, vec, 0.01)
    F1, _ = fr.total_force(sm, sc, sf, svec, 0.01)
    print(f"dim {dim}: |F1 - F0| {np.abs(F1 - F0).max():.2e}, S {S:.3e}")
    assert np.abs(F1 - F0).max() <= 1e-13 * S


def test_probe_points_are_shared_nodes():
    for dim, k in [(2, 1), (2, 2), (3, 1), (3, 2)]:
        mesh = _cyl(dim, k)[0]
        d = deck("input_turek_2D_Re20_stat.json" if dim == 2 else "input_turek_3D_Re100.json")
        pts = d.pressure_probe_points(mesh)
        vec = np.random.default_rng(6).standard_normal(mesh.n_dofs)
        vals, cnt = fr.probe(mesh, pts, vec)
        X = np.asarray(mesh.coords)
        for p, v, c in zip(pts, vals, cnt):
            node = int(np.argmin(((X - p) ** 2).sum(axis=1)))
            assert np.linalg.norm(X[node] - p) <= 1e-15
            assert c >= 2
            assert np.abs(v - vec.reshape(-1, dim + 1)[node]).max() <= 1e-12


def test_deck_force_scaling():
    want = {"input_turek_2D_Re20_stat.json": 500.0,
            "input_turek_2D_Re100.json": 20.0,
            "input_turek_3D_Re100.json": 2 / (0.1 * 0.41),
            "input_hoffmann_3D_Re3900.json": 2 / (0.1 * 39 ** 2 * 0.41)}
    for name, w in want.items():
        d = deck(name)
        mesh = _cyl(d.dim, 1)[0]
        got = d.force_scaling(mesh)
        print(name, got, w)
        assert abs(got - w) <= 1e-12 * w
        cells, faces = d.cylinder_faces(mesh)
        assert np.array_equal(cells, _cyl(d.dim, 1)[1])
        pts = d.pressure_probe_points(mesh)
        assert pts.shape == (2, d.dim) and pts[0, 0] == -0.05 and pts[1, 0] == 0.05
        assert not pts[:, 1:].any()


def test_cylinder_postprocess_file(tmp_path):
    import glssolvers

    class StubOperator:
        dim = 2

        def set_force_faces(self, cells, face_no, n_q_1d=3):
            self.n_faces, self.n_q_1d = len(cells), n_q_1d

        def set_probe_points(self, xyz):
            return np.full(len(xyz), 2)

        def surface_force(self, vec):
            return np.array([0.011, -0.002])

        def probe(self, vec):
            return np.array([[0.0, 0.0, 0.25], [0.0, 0.0, 0.125]])

    d = deck("input_turek_2D_Re20_stat.json")
    mesh = _cyl(2, 1)[0]
    path = tmp_path / "run_drag_lift_pressure.m"
    op = StubOperator()
    post = glssolvers.CylinderPostprocess(op, d, mesh, str(path))
    assert op.n_faces == 8 and op.n_q_1d == 3
    out = post(0.5, np.zeros(3))
    assert out == pytest.approx((5.5, -1.0, 0.125), rel=1e-14)
    assert len(path.read_text().splitlines()) == 1  # flushed after the call
    post(1.0, np.zeros(3))
    post.t = 1.5
    post(np.zeros(3))  # the NonLinearSolverBase.postprocess form
    lines = path.read_text().splitlines()
    assert len(lines) == 3
    for line, t in zip(lines, (0.5, 1.0, 1.5)):
        cols = line.split("\t")
        assert len(cols) == 4
        assert [float(c) for c in cols] == pytest.approx([t, 5.5, -1.0, 0.125], rel=1e-5)
