"""Drag / lift and pressure-drop evaluation on the device (csrc/forces.hip:
gls_op_surface_force, gls_op_probe and their gls_dist_* forms) against the
numpy restatement tests/forces_ref.py of simulation.cc:451-541.

Error scale of a force: S = sum over faces and face points of |f| (a closed
surface's sum cancels).  Parity tolerances are the project's: 1e-12 S for
FP64 vectors, 2e-5 S for FP32 ones."""
import functools

import numpy as np
import pytest

import forces_ref as fr
import glsmesh as gm

pytestmark = pytest.mark.gpu

NU = 0.01


@functools.lru_cache(maxsize=None)
def _mesh(kind, dim, k):
    """(mesh, cells, face_no) of the force faces: the cylinder's (r0), those
    of its seed-3 rotated shuffle, or every boundary face of the hypercube
    (r1)."""
    if kind == "cube":
        mesh = gm.hypercube(dim, k, 1)
        return (mesh,) + tuple(gm.boundary_faces(mesh, 0))
    mesh = gm.cylinder(dim, k, 0)
    if kind == "shuffled":
        mesh = gm.ShuffledMesh(mesh, seed=3, rotate=True)
    return (mesh,) + tuple(gm.boundary_faces(mesh, 2))


@functools.lru_cache(maxsize=None)
def _vec(kind, dim, k):
    v = np.random.default_rng(17).standard_normal(_mesh(kind, dim, k)[0].n_dofs)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _ref(kind, dim, k, n_q_1d=3):
    mesh, cells, faces = _mesh(kind, dim, k)
    pf, sf = fr.surface_force(mesh, cells, faces, _vec(kind, dim, k), NU, n_q_1d)
    return pf, float(sf.sum())


def _op(mesh, prec="f64", brick=None, nu=NU):
    import glsamd
    op = glsamd.NavierStokesOperator(mesh, np.zeros(mesh.n_nodes, dtype=np.uint8), prec,
                                     brick=brick)
    op.set_parameters(nu=nu)
    return op


CASES = [("cylinder", 2, 1, 3), ("cylinder", 2, 2, 3), ("cylinder", 3, 1, 3),
         ("cylinder", 3, 2, 3), ("shuffled", 2, 2, 3), ("shuffled", 3, 2, 3),
         ("cube", 2, 3, 3), ("cube", 3, 3, 3), ("cube", 3, 2, 3),
         ("cylinder", 3, 2, 2), ("cylinder", 3, 2, 4)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind,dim,k,n_q_1d", CASES)
def test_force_parity(kind, dim, k, n_q_1d, prec):
    mesh, cells, faces = _mesh(kind, dim, k)
    if kind == "cube":
        assert set(faces.tolist()) == set(range(2 * dim))
    if kind == "shuffled":
        assert set(faces.tolist()) == set(range(2 * dim))
    ref_faces, S = _ref(kind, dim, k, n_q_1d)
    op = _op(mesh, prec)
    op.set_force_faces(cells, faces, n_q_1d)
    x = op._dev(np.array(_vec(kind, dim, k)))
    total = op.surface_force(x)
    per_face = op.surface_force_faces(x)
    e_tot = np.abs(total - ref_faces.sum(axis=0)).max()
    e_face = np.abs(per_face - ref_faces).max()
    print(f"{kind} dim {dim} Q{k} nq {n_q_1d} {prec}: {len(cells)} faces, S {S:.3e}, "
          f"total err {e_tot:.2e}, per-face err {e_face:.2e}, brick {op.brick_shape}")
    tol = (1e-12 if prec == "f64" else 2e-5) * S
    assert per_face.shape == (len(cells), dim)
    assert e_tot <= tol and e_face <= tol


def test_repeatable_and_cell_order_independent():
    mesh, cells, faces = _mesh("cylinder", 3, 2)
    vec = np.array(_vec("cylinder", 3, 2))
    op = _op(mesh)
    op.set_force_faces(cells, faces)
    x = op._dev(vec)
    a, b = op.surface_force(x), op.surface_force(x)
    assert a.tobytes() == b.tobytes()
    assert op.surface_force_faces(x).tobytes() == op.surface_force_faces(x).tobytes()
    op0 = _op(mesh, brick=(0, 0, 0))
    op0.set_force_faces(cells, faces)
    assert op0.brick_shape == (0, 0, 0)
    c = op0.surface_force(op0._dev(vec))
    print("default brick", op.brick_shape, a, "per-cell", c)
    assert a.tobytes() == c.tobytes()
    # the discovered cell order of a shuffled copy of the same cells
    sm = gm.ShuffledMesh(mesh, seed=1, rotate=False)
    sc, sf = gm.boundary_faces(sm, 2)
    ops = _op(sm)
    ops.set_force_faces(sc, sf)
    svec = vec.reshape(-1, 4)[sm.node_old].ravel()
    per = ops.surface_force_faces(ops._dev(svec))
    base = op.surface_force_faces(x)
    order = {int(sm.cell_order[c_]): i for i, c_ in enumerate(sc)}
    same = np.array([per[order[int(c_)]] for c_ in cells])
    assert same.tobytes() == base.tobytes()


@pytest.mark.parametrize("dim", [2, 3])
def test_known_answer_linear_pressure(dim):
    mesh, cells, faces = _mesh("cylinder", dim, 2)
    A = fr.hole_measure(mesh)
    v = np.zeros((mesh.n_nodes, dim + 1))
    v[:, dim] = np.asarray(mesh.coords)[:, 0]
    op = _op(mesh)
    op.set_force_faces(cells, faces)
    F = op.surface_force(op._dev(v.ravel()))
    want = np.zeros(dim)
    want[0] = -A
    err = np.abs(F - want).max() / A
    print(f"dim {dim}: F {F}, A_h {A:.12e}, rel err {err:.2e}")
    assert err <= 1e-12


def test_vector_layout_host_permuted():
    mesh, cells, faces = _mesh("cylinder", 3, 2)
    vec = np.array(_vec("cylinder", 3, 2))
    _, S = _ref("cylinder", 3, 2)
    op = _op(mesh)
    op.set_force_faces(cells, faces)
    pts = np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0]])
    op.set_probe_points(pts)
    x = op._dev(vec)
    F, P = op.surface_force(x), op.probe(x)
    perm = np.random.default_rng(5).permutation(mesh.n_dofs).astype(np.int64)
    oph = _op(mesh)
    oph.set_force_faces(cells, faces)
    oph.set_probe_points(pts)
    oph.set_vector_layout("host", perm)
    hv = np.ascontiguousarray(vec[perm])
    Fh, Ph = oph.surface_force(hv), oph.probe(hv)
    print("device", F, "host + dof_map", Fh)
    assert np.abs(Fh - F).max() <= 1e-14 * S
    assert np.abs(oph.surface_force_faces(hv) - op.surface_force_faces(x)).max() <= 1e-14 * S
    assert np.abs(Ph - P).max() <= 1e-14 * np.abs(P).max()


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("dim,k", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_probe_cylinder_points(dim, k, prec):
    import glsmesh
    mesh = _mesh("cylinder", dim, k)[0]
    deck = glsmesh.Deck(name="probe", dim=dim)
    pts = deck.pressure_probe_points(mesh)
    vec = np.array(_vec("cylinder", dim, k))
    op = _op(mesh, prec)
    found = op.set_probe_points(pts)
    vals = op.probe(op._dev(vec))
    X = np.asarray(mesh.coords)
    tol = 1e-12 if prec == "f64" else 2e-6
    for p, v, c in zip(pts, vals, found):
        node = int(np.argmin(((X - p) ** 2).sum(axis=1)))
        want = vec.reshape(-1, dim + 1)[node]
        err = np.abs(v - want).max() / np.abs(want).max()
        print(f"dim {dim} Q{k} {prec}: point {p}, {c} cells, rel err {err:.2e}")
        assert c >= 2
        assert err <= tol
    ref_vals, ref_cnt = fr.probe(mesh, pts, vec)
    assert np.array_equal(found, ref_cnt)


def test_probe_hypercube_points():
    mesh = _mesh("cube", 3, 2)[0]
    X = np.asarray(mesh.coords)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    v = np.stack([x * y, z * z, x, x * x * y - z * z], axis=1).ravel()
    pts = np.array([[0.3, 0.2, 0.7], [0.81, 0.44, 0.13], [0.26, 0.77, 0.9],
                    [0.5, 0.3, 0.2],        # on a cell face
                    [0.5, 0.5, 0.5],        # on a vertex
                    [2.0, 0.5, 0.5]])       # outside
    op = _op(mesh)
    found = op.set_probe_points(pts)
    vals = op.probe(op._dev(v))
    print("cells found", found)
    assert found.tolist() == [1, 1, 1, 2, 8, 0]
    px, py, pz = pts[:5, 0], pts[:5, 1], pts[:5, 2]
    want = np.stack([px * py, pz * pz, px, px * px * py - pz * pz], axis=1)
    err = np.abs(vals[:5] - want).max()
    print(f"max err {err:.2e}")
    assert err <= 1e-12
    assert not vals[5].any()
    ref_vals, ref_cnt = fr.probe(mesh, pts, v)
    assert np.array_equal(found, ref_cnt) and np.abs(vals - ref_vals).max() <= 1e-12


def test_cylinder_postprocess_on_device(tmp_path):
    """glssolvers.CylinderPostprocess end to end on the Turek 2D deck's r0
    mesh: c_D, c_L from the reference force and the deck's scaling, dp from
    the nodal pressures at the two probe points, one line per call."""
    import glssolvers
    from helpers import deck
    d = deck("input_turek_2D_Re100.json")
    mesh = d.mesh(0)
    op = _op(mesh, nu=d.nu)
    vec = np.random.default_rng(23).standard_normal(mesh.n_dofs)
    path = tmp_path / "turek_drag_lift_pressure.m"
    post = glssolvers.CylinderPostprocess(op, d, mesh, str(path))
    c_d, c_l, dp = post(0.25, op._dev(vec))
    cells, faces = d.cylinder_faces(mesh)
    F, S = fr.total_force(mesh, cells, faces, vec, d.nu)
    vals, _ = fr.probe(mesh, d.pressure_probe_points(mesh), vec)
    scale = d.force_scaling(mesh)
    print(f"c_D {c_d:.6e}, c_L {c_l:.6e}, dp {dp:.6e}; reference {F * scale}, "
          f"{vals[0, 2] - vals[1, 2]:.6e}")
    assert abs(c_d - F[0] * scale) <= 1e-12 * S * scale
    assert abs(c_l - F[1] * scale) <= 1e-12 * S * scale
    assert abs(dp - (vals[0, 2] - vals[1, 2])) <= 1e-12 * np.abs(vals).max()
    post(0.5, op._dev(vec))
    lines = path.read_text().splitlines()
    assert len(lines) == 2 and all(len(ln.split("\t")) == 4 for ln in lines)
    assert float(lines[0].split("\t")[0]) == 0.25


def test_errors():
    import glsamd
    mesh, cells, faces = _mesh("cylinder", 2, 2)
    op = _op(mesh)
    x = op.initialize_dof_vector()
    with pytest.raises(glsamd.GlsError, match="before gls_op_set_force_faces"):
        op.surface_force(x)
    with pytest.raises(glsamd.GlsError, match="before gls_op_set_probe_points"):
        op.probe(x)
    bad = faces.copy()
    bad[1] = 2 * mesh.dim
    with pytest.raises(glsamd.GlsError, match="bad cell or face number"):
        op.set_force_faces(cells, bad)
    with pytest.raises(glsamd.GlsError, match="bad cell or face number"):
        op.set_force_faces(np.array([mesh.n_cells]), np.array([0]))
    with pytest.raises(glsamd.GlsError, match="before gls_op_set_force_faces"):
        op.surface_force(x)  # a rejected list is not a list
    with pytest.raises(glsamd.GlsError, match="n_q_1d"):
        op.set_force_faces(cells, faces, 5)
    fresh = glsamd.NavierStokesOperator(mesh, np.zeros(mesh.n_nodes, dtype=np.uint8), "f64")
    fresh.set_force_faces(cells, faces)
    with pytest.raises(glsamd.GlsError, match="nu is not set"):
        fresh.surface_force(x)
    # an empty list is a list: zero force
    op.set_force_faces(cells, faces)
    op.set_force_faces(cells[:0], faces[:0])
    assert not op.surface_force(x).any()
    iso = gm.IsoQ1Mesh(mesh)
    opm = _op(iso)
    with pytest.raises(glsamd.GlsError, match="mapping_points"):
        opm.set_force_faces(cells[:0], faces[:0])


def test_partitioned_group():
    import glsdist
    mesh, cells, faces = _mesh("cylinder", 3, 2)
    vec = np.array(_vec("cylinder", 3, 2))
    _, S = _ref("cylinder", 3, 2)
    pts = np.array([[-0.05, 0.0, 0.0], [0.05, 0.0, 0.0], [0.3, 0.01, 0.02]])
    op = _op(mesh)
    op.set_force_faces(cells, faces)
    op.set_probe_points(pts)
    x = op._dev(vec)
    F, P = op.surface_force(x), op.probe(x)
    # two contiguous cell ranges that both touch the cylinder
    bounds = [0, int(cells[len(cells) // 2]), mesh.n_cells]
    parts = glsdist.build_partitions(mesh, 2, bounds)
    cmask = np.zeros(mesh.n_nodes, dtype=np.uint8)
    ranks = [glsdist.RankOperator(mesh, cmask, p, "f64") for p in parts]
    native = []
    for r in ranks:
        native.append(r.eng.partitioned(r.part, group=native[0] if native else None))
    n_local = []
    for r in ranks:
        sel = (cells >= r.part.cell_begin) & (cells < r.part.cell_end)
        n_local.append(int(sel.sum()))
        r.op.set_parameters(nu=NU)
        r.op.set_force_faces(cells[sel] - r.part.cell_begin, faces[sel])
        r.op.set_probe_points(pts)
    print("faces per rank", n_local)
    assert all(n > 0 for n in n_local) and sum(n_local) == len(cells)
    vs = [r.local_from_global(vec) for r in ranks]
    for r, v in zip(ranks, vs):
        v[r.n_owned_dofs:].zero_()  # the calls import the ghosts
    out = glsdist.run_threaded(2, lambda r: (native[r].surface_force(vs[r]),
                                             native[r].probe(vs[r])))
    for r, (Fr, Pr) in enumerate(out):
        print(f"rank {r}: |F - F1| {np.abs(Fr - F).max():.2e}, |P - P1| {np.abs(Pr - P).max():.2e}")
        assert np.abs(Fr - F).max() <= 1e-13 * S
        assert np.abs(Pr - P).max() <= 1e-12 * np.abs(P).max()
