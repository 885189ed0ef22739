"""No-normal-flux constraints on curved boundaries, host side
(gls_mesh_no_normal_flux, Mesh.node_constraints, Deck.node_constraints) and
the numpy reference of the constrained operator (tests/slip_ref.py).

The cylinder's averaged normal must be the radial direction to 1e-13
(rounding of the Q_k map's derivatives; 1.5e-15 measured), coef must equal
the numpy restatement of the rule to 1e-14, and the reference's
C^T A C must equal the dense product assembled from cell matrices to 1e-12."""
import os
import subprocess

import numpy as np
import pytest

import glsmesh as gm
import slip_ref
from helpers import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# (dim, degree, n_ref, cells, cylinder nodes)
MESHES = [(2, 1, 1, 352, 16), (2, 2, 0, 88, 16), (2, 2, 1, 352, 32), (3, 2, 0, 400, 144),
          (3, 1, 1, 3200, 144)]


@pytest.fixture(scope="module", params=MESHES, ids=lambda m: "%dD_Q%d_r%d" % m[:3])
def cyl(request):
    dim, degree, n_ref, n_cells, n_rows = request.param
    mesh = gm.cylinder(dim, degree, n_ref)
    assert mesh.n_cells == n_cells
    return mesh, n_rows, mesh.node_constraints([2]), slip_ref.normals(mesh, 2)


def test_normals_are_radial(cyl):
    mesh, n_rows, (nodes, comp, coef, nrm), _ = cyl
    assert len(nodes) == n_rows
    assert np.all(np.diff(nodes) > 0)  # one row per node, ascending
    assert np.array_equal(nodes, np.nonzero((mesh.node_boundary >> 2) & 1)[0])
    x = mesh.coords[nodes][:, :2]
    r = x / np.linalg.norm(x, axis=1)[:, None]
    err = np.minimum(np.abs(nrm[:, :2] - r).max(axis=1), np.abs(nrm[:, :2] + r).max(axis=1))
    print("max normal error", err.max())
    assert err.max() <= 1e-13
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() <= 1e-15
    if mesh.dim == 3:
        assert np.all(nrm[:, 2] == 0.0)
        assert np.all(coef[:, 2] == 0.0)


def test_comp_and_tie_rule(cyl):
    mesh, _, (nodes, comp, coef, nrm), _ = cyl
    assert set(np.unique(comp)) <= {0, 1}
    a = np.abs(nrm[:, :2])
    tie = np.abs(a[:, 0] - a[:, 1]) <= 1e-10 * a.max(axis=1)
    # the 45-degree nodes: 4 in 2D, 4 per z-line in 3D; the lowest component wins
    per_line = 4
    lines = 1 if mesh.dim == 2 else len(np.unique(np.round(mesh.coords[nodes][:, 2], 12)))
    assert tie.sum() == per_line * lines
    assert np.all(comp[tie] == 0)
    assert np.all(comp[~tie] == np.argmax(a[~tie], axis=1))
    assert np.all(coef[np.arange(len(nodes)), comp] == 0.0)
    # u . n = 0 for u = C u
    u = np.random.default_rng(0).standard_normal(nrm.shape)
    u[np.arange(len(nodes)), comp] = np.einsum("ie,ie->i", coef, u)
    assert np.abs(np.einsum("ie,ie->i", u, nrm)).max() <= 1e-14 * np.abs(u).max()


def test_coef_matches_numpy_rule(cyl):
    mesh, _, (nodes, comp, coef, nrm), (rn, rc, rk, rnrm, min_dot) = cyl
    assert np.array_equal(nodes, rn)
    assert np.array_equal(comp, rc)
    assert np.abs(coef - rk).max() <= 1e-14
    assert np.abs(nrm - rnrm).max() <= 1e-14
    print("smallest face . average", min_dot)
    assert min_dot >= 0.98


def test_dirichlet_and_planar_ids():
    mesh = gm.cylinder(3, 2, 0)
    # planar ids give no rows; nodes of a velocity Dirichlet id have none
    assert len(mesh.node_constraints([3, 4, 5, 6])[0]) == 0
    assert len(mesh.node_constraints([0, 1])[0]) == 0
    assert len(mesh.node_constraints([2], [2])[0]) == 0
    nodes = mesh.node_constraints([2], [5, 6])[0]
    full = mesh.node_constraints([2])[0]
    on_wall = ((mesh.node_boundary[full] >> 5) | (mesh.node_boundary[full] >> 6)) & 1
    assert on_wall.sum() > 0
    assert np.array_equal(nodes, full[on_wall == 0])
    # the mask call still refuses the curved id
    with pytest.raises(RuntimeError, match="not an axis-aligned planar wall"):
        mesh.constraint_mask([], [], [2])


def test_deck_wiring():
    d = gm.read_deck(f"{gm.DECK_DIR}/input_hoffmann_3D_Re3900.json")
    mesh = d.mesh(0)
    assert len(d.node_constraints(mesh)[0]) == 0  # cylinder no-slip: Dirichlet
    d.no_slip_cylinder = False
    nodes, comp, coef = d.node_constraints(mesh)
    assert len(nodes) > 0
    cmask = d.mask(mesh)
    assert not np.any((cmask[nodes] >> comp) & 1)
    vel, p, slip = d.boundary_descriptor()
    assert 2 in slip
    with pytest.raises(RuntimeError, match="not an axis-aligned planar wall"):
        mesh.constraint_mask(vel, p, slip)
    with pytest.raises(NotImplementedError):
        d.node_constraints(gm.IsoQ1Mesh(mesh))


def _one_quad(v, faces):
    return dict(vertices=np.asarray(v, dtype=np.float64),
                cells=np.array([[0, 1, 2, 3]], dtype=np.int32),
                bfaces=np.asarray(faces, dtype=np.int32),
                bids=np.full(len(faces), 7, dtype=np.int32))


def test_corner_inside_one_id_is_refused():
    """The rule refuses a node where a face normal has n_face . n < 0.5 with
    the averaged normal n, i.e. faces whose normals are more than 120 degrees
    apart.  Two faces of one id at 90 degrees give n_face . n = cos 45 =
    0.7071 at their common node, which that condition accepts; a corner the
    condition does catch is the 45-degree corner below (normals 135 degrees
    apart, n_face . n = cos 67.5 = 0.383).  Both are pinned."""
    # lower and right side of a quadrilateral with a 45-degree corner at (2, 0)
    sharp = _one_quad([[0, 0], [2, 0], [0, 1], [1, 1]], [[0, 1], [1, 3]])
    mesh = gm.from_coarse(sharp, 2, 1)
    with pytest.raises(RuntimeError, match=r"node \d+ is a corner"):
        mesh.node_constraints([7])
    # lower and right side of a unit square turned by 30 degrees: a 90-degree corner
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[c, -s], [s, c]])
    sq = np.array([[0.0, 0], [1, 0], [0, 1], [1, 1]]) @ R.T
    mesh = gm.from_coarse(_one_quad(sq, [[0, 1], [1, 3]]), 2, 1)
    nodes, comp, coef, nrm = mesh.node_constraints([7])
    assert len(nodes) == 9
    corner = np.argmin(np.linalg.norm(mesh.coords[nodes] - sq[1], axis=1))
    n1, n2 = R @ [0.0, -1.0], R @ [1.0, 0.0]
    assert abs(nrm[corner] @ n1 - np.sqrt(0.5)) <= 1e-14
    assert abs(nrm[corner] @ n2 - np.sqrt(0.5)) <= 1e-14
    # one oblique face alone is smooth: the normal is the face's
    mesh = gm.from_coarse(_one_quad(sq, [[0, 1]]), 2, 1)
    nodes, comp, coef, nrm = mesh.node_constraints([7])
    assert len(nodes) == 5 and np.all(comp == 1)
    assert np.abs(nrm - n1).max() <= 1e-14


@pytest.fixture(scope="module")
def q2r0():
    case = slip_ref.slip_case("input_turek_2D_Re20_stat.json", 0, fe_degree=2)
    assert case.mesh.n_cells == 88 and len(case.rows.nodes) == 16
    o = case.oracle()
    A = slip_ref.dense_matrix(o, case.mesh, case.cmask)
    return case, o, A


def test_ref_dense_oracle_agree(q2r0):
    case, o, A = q2r0
    assert rel_err(A @ case.src, o.vmult(case.src)) <= 1e-12


def test_ref_vmult_is_dense_product(q2r0):
    case, o, A = q2r0
    M = slip_ref.dense_constrained(A, case.rows)
    assert rel_err(slip_ref.vmult(o, case.rows, case.src), M @ case.src) <= 1e-12
    assert np.all(M[case.rows.elim, case.rows.elim] == 1.0)
    d = slip_ref.diagonal(o, case.rows, case.mesh)
    assert rel_err(d, np.diag(M)) <= 1e-12


def test_ref_distribute_and_transpose(q2r0):
    case, o, A = q2r0
    rows = case.rows
    x, y = case.src, case.u_star
    u = rows.distribute(x, case.cmask).reshape(-1, case.dim + 1)
    _, _, _, nrm = case.mesh.node_constraints([2])
    un = np.einsum("ie,ie->i", u[rows.nodes][:, :case.dim], nrm)
    assert np.abs(un).max() <= 1e-14 * np.abs(u).max()
    # (y, C x) = (C^T y, x) for x with zero eliminated entries (C ignores them)
    x0 = np.array(x)
    x0[rows.elim] = 0.0
    assert abs(y @ rows.resolve(x0) - rows.transpose(y) @ x0) <= 1e-13 * abs(y @ x0)
    Cm = rows.dense(len(x))
    assert np.abs(Cm @ x - rows.resolve(x)).max() <= 1e-14
    yz = Cm.T @ y
    assert np.abs(yz - rows.transpose(y)).max() <= 1e-14


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_no_normal_flux_asan_ubsan(tmp_path):
    exe = str(tmp_path / "no_normal_flux_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "no_normal_flux_sanitize.cc"),
           os.path.join(ROOT, "dealii-ns-gls_amd", "host", "mesh.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "0 failures" in out


def test_ids_are_treated_one_at_a_time():
    """Several ids in one call: only the faces of one id enter a node's
    normal (as the reference calls compute_no_normal_flux_constraints once
    per id); a node on two curved ids would need two rows and is refused."""
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[c, -s], [s, c]])
    sq = np.array([[0.0, 0], [1, 0], [0, 1], [1, 1]]) @ R.T
    coarse = _one_quad(sq, [[0, 1], [1, 3]])
    coarse["bids"] = np.array([7, 8], dtype=np.int32)
    mesh = gm.from_coarse(coarse, 2, 1)
    assert (mesh.nonplanar_ids >> 7) & 1 and (mesh.nonplanar_ids >> 8) & 1
    n7 = mesh.node_constraints([7])[3]
    n8 = mesh.node_constraints([8])[3]
    assert np.abs(n7 - R @ [0.0, -1.0]).max() <= 1e-14  # no blending at the corner
    assert np.abs(n8 - R @ [1.0, 0.0]).max() <= 1e-14
    with pytest.raises(RuntimeError, match=r"node \d+ lies on two curved slip boundary ids"):
        mesh.node_constraints([7, 8])
    # the cylinder with the planar walls in the same call: the cylinder's rows
    cyl = gm.cylinder(2, 2, 0)
    a, b = cyl.node_constraints([2]), cyl.node_constraints([2, 3, 4])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert cyl.nonplanar_ids == 1 << 2
