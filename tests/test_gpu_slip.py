"""Node constraints (no-normal-flux rows on the curved cylinder) on the GPU
against the numpy restatement tests/slip_ref.py on top of the oracle (TEST
INFRASTRUCTURE), fed the library's own (nodes, comp, coef).

Tolerances are the project's (test_gpu_parity): FP64 relative l2 1e-12, FP32
2e-5; the diagonals 10 times that, as there."""
import numpy as np
import pytest

import glsmesh as gm
import slip_ref
from helpers import Case, deck, rel_err

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}

RE20, RE100_3D, RE3900 = ("input_turek_2D_Re20_stat.json", "input_turek_3D_Re100.json",
                          "input_hoffmann_3D_Re3900.json")
# name, n_ref, overrides: 2D Q1 r1, 2D Q2 r0 / r1, 3D Q2 r0 (400 cells: one round of bricks)
SHAPES = {"2d_q1_r1": (RE20, 1, dict(fe_degree=1)), "2d_q2_r0": (RE20, 0, dict(fe_degree=2)),
          "2d_q2_r1": ("input_turek_2D_Re100.json", 1, dict(fe_degree=2)),
          "turek3d_r0": (RE100_3D, 0, {}), "re3900_r0": (RE3900, 0, {})}
_cache = {}


def _np(t):
    return t.double().cpu().numpy()


def ref_case(shape, fixed=False):
    """The case, its oracle and the reference results, computed once."""
    key = (shape, fixed)
    if key not in _cache:
        name, n_ref, over = SHAPES[shape]
        over = dict(over, nonlinear_solver="Picard") if fixed else over
        case = slip_ref.slip_case(name, n_ref, **over)
        assert len(case.rows.nodes) > 0
        o = case.oracle()
        g = deck(name).constraint_values(case.mesh, 0.02)
        ref = dict(vmult=slip_ref.vmult(o, case.rows, case.src),
                   res=slip_ref.residual(o, case.rows, case.u_star, case.cmask, g),
                   plain=slip_ref.residual_plain(o, case.rows, case.u_star),
                   rhs=slip_ref.residual(o, case.rows, np.zeros(case.n_dofs), case.cmask, g),
                   diag=slip_ref.diagonal(o, case.rows, case.mesh), g=g)
        ref["inv"] = np.where(np.abs(ref["diag"]) > 1e-10, 1.0 / ref["diag"], 1.0)
        _cache[key] = (case, ref)
    return _cache[key]


@pytest.mark.parametrize("fixed", [False, True], ids=["newton", "fixed"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_against_slip_ref(shape, prec, fixed):
    import torch
    case, ref = ref_case(shape, fixed)
    op = slip_ref.gpu(case, prec)
    assert op.n_node_constraints[0] == len(case.rows.nodes)
    assert op.n_node_constraints[1] >= 2
    op.set_constraint_values(ref["g"])
    src = op._dev(case.src)
    keep = src.clone()
    out = {k: op.initialize_dof_vector() for k in ("vmult", "res", "plain", "rhs", "diag", "inv")}
    op.vmult(out["vmult"], src)
    op.evaluate_residual(out["res"], op._dev(case.u_star))
    op.evaluate_residual_plain(out["plain"], op._dev(case.u_star))
    op.evaluate_rhs(out["rhs"])
    op.compute_diagonal(out["diag"])
    op.compute_inverse_diagonal(out["inv"])
    torch.cuda.synchronize()
    assert torch.equal(src, keep)  # the source is restored bit for bit
    err = {k: rel_err(_np(v), ref[k]) for k, v in out.items()}
    print(shape, prec, "fixed" if fixed else "newton", err)
    for k in ("vmult", "res", "plain", "rhs"):
        assert err[k] < TOL[prec], k
    for k in ("diag", "inv"):
        assert err[k] < TOL[prec] * 10, k
    elim = case.rows.elim
    assert np.all(_np(out["vmult"])[elim] == _np(src)[elim])  # identity rows
    for k in ("res", "plain", "rhs"):
        assert np.all(_np(out[k])[elim] == 0.0)
    assert np.all(_np(out["diag"])[elim] == 1.0) and np.all(_np(out["inv"])[elim] == 1.0)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_per_cell_path_3d(prec):
    import torch
    case, ref = ref_case("re3900_r0")
    op = slip_ref.gpu(case, prec, brick=(0, 0, 0))
    assert op.brick_shape == (0, 0, 0)
    dst, inv = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(dst, op._dev(case.src))
    op.compute_inverse_diagonal(inv)
    torch.cuda.synchronize()
    assert rel_err(_np(dst), ref["vmult"]) < TOL[prec]
    assert rel_err(_np(inv), ref["inv"]) < TOL[prec] * 10


@pytest.mark.parametrize("shape", ["2d_q2_r1", "re3900_r0"])
def test_deterministic_repeats_bitwise(shape):
    import torch
    case, ref = ref_case(shape)
    op = slip_ref.gpu(case, "f64", deterministic=True)
    src = op._dev(case.src)
    a, b = op.initialize_dof_vector(), op.initialize_dof_vector()
    da, db = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(a, src)
    op.compute_inverse_diagonal(da)
    op.vmult(b, src)
    op.compute_inverse_diagonal(db)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(da, db)
    assert rel_err(_np(a), ref["vmult"]) < TOL["f64"]


def test_distribute():
    import torch
    case, ref = ref_case("2d_q2_r0")
    op = slip_ref.gpu(case, "f64")
    op.set_constraint_values(ref["g"])
    x = op._dev(case.src)
    op.distribute(x)
    y = op._dev(case.src)
    op.distribute(y, homogeneous=True)
    torch.cuda.synchronize()
    assert np.abs(_np(x) - case.rows.distribute(case.src, case.cmask, ref["g"])).max() <= 1e-15
    assert np.abs(_np(y) - case.rows.distribute(case.src, case.cmask)).max() <= 1e-15
    _, _, _, nrm = case.mesh.node_constraints([2])
    u = _np(y).reshape(-1, case.dim + 1)[case.rows.nodes][:, :case.dim]
    assert np.abs(np.einsum("ie,ie->i", u, nrm)).max() <= 1e-14 * np.abs(u).max()


def _axis_rows(mesh, cmask, bits):
    """The components `bits` of the mask as node-constraint rows with zero
    coefficients, on the nodes where exactly one of them is set (one row per
    node); returns (mask without them, rows)."""
    cm = np.asarray(cmask)
    nodes, comp = [], []
    out = cm.copy()
    for c in range(mesh.dim):
        if not (bits >> c) & 1:
            continue
        sel = np.nonzero(((cm >> c) & 1 == 1) & (cm == (1 << c)))[0]
        nodes += list(sel)
        comp += [c] * len(sel)
        out[sel] &= ~np.uint8(1 << c)
    order = np.argsort(nodes)
    nodes = np.asarray(nodes, dtype=np.int64)[order]
    comp = np.asarray(comp, dtype=np.int32)[order]
    return out, (nodes, comp, np.zeros((len(nodes), mesh.dim)))


@pytest.mark.parametrize("kind", ["hypercube", "cylinder_walls"])
def test_two_constraint_paths_agree(kind):
    """An axis-normal constraint as rows with zero coefficients equals the
    same component in the Dirichlet mask."""
    import glsamd
    import torch
    d = deck(RE3900 if kind == "cylinder_walls" else RE20)
    if kind == "hypercube":
        mesh = gm.hypercube(2, 2, 2)
        # u_y fixed on y = 0 / 1, u_x on x = 0 / 1 (both at the corners)
        x = mesh.coords
        cmask = (((np.abs(x[:, 1] - 0.5) == 0.5) * 2) | ((np.abs(x[:, 0] - 0.5) == 0.5) * 1))
        cmask = cmask.astype(np.uint8)
    else:
        d.no_slip_wall = False
        mesh = d.mesh(0)
        vel, p, slip = d.boundary_descriptor()
        cmask = mesh.constraint_mask(vel, p, slip)
    params, w = d.operator_parameters()
    case = Case(mesh, cmask, params, w)
    reduced, rows = _axis_rows(mesh, cmask, (1 << mesh.dim) - 1)
    assert len(rows[0]) > 0
    a = case.gpu("f64")
    case.cmask = reduced
    b = case.gpu("f64")
    b.set_node_constraints(*rows)
    src = a._dev(case.src)
    ya, yb, da, db = (a.initialize_dof_vector() for _ in range(4))
    a.vmult(ya, src)
    b.vmult(yb, src)
    a.compute_diagonal(da)
    b.compute_diagonal(db)
    torch.cuda.synchronize()
    assert rel_err(_np(yb), _np(ya)) < 1e-12
    assert rel_err(_np(db), _np(da)) < 1e-12


@pytest.mark.parametrize("outflow", ["cut", "nitsche"])
def test_with_outflow_faces(outflow):
    import torch
    case = slip_ref.slip_case(RE20, 1, outflow=outflow)
    assert case.outflow is not None
    o = case.oracle(outflow=case.outflow)
    op = slip_ref.gpu(case, "f64")
    assert op.n_outflow_faces[0] > 0
    dst, dg = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(dst, op._dev(case.src))
    op.compute_diagonal(dg)
    torch.cuda.synchronize()
    assert rel_err(_np(dst), slip_ref.vmult(o, case.rows, case.src)) < 1e-12
    assert rel_err(_np(dg), slip_ref.diagonal(o, case.rows, case.mesh)) < 1e-11


def test_error_paths():
    import glsamd
    case, ref = ref_case("2d_q2_r0")
    nodes, comp, coef = case.node_constraints
    op = slip_ref.gpu(case, "f64")
    x, y = op._dev(case.src), op.initialize_dof_vector()
    with pytest.raises(glsamd.GlsError, match="vmult_cells.*node constraints"):
        op.vmult_cells(y, x, 0, case.mesh.n_cells)
    with pytest.raises(glsamd.GlsError, match="ascending"):
        op.set_node_constraints(nodes[::-1], comp[::-1], coef[::-1])
    with pytest.raises(glsamd.GlsError, match="ascending"):
        op.set_node_constraints(nodes[[0, 0]], comp[[0, 0]], coef[[0, 0]])
    assert op.n_node_constraints[0] == len(nodes)  # a refused call changes nothing
    # comp in the node's Dirichlet mask; a coefficient on a Dirichlet component
    wall = np.nonzero(np.asarray(case.cmask) == 3)[0][:1]
    with pytest.raises(glsamd.GlsError, match="Dirichlet mask"):
        op.set_node_constraints(wall, [0], [[0.0, 0.0]])
    half = np.nonzero(np.asarray(case.cmask) == 4)[0]
    if len(half):  # outflow pressure node: free velocity
        with pytest.raises(glsamd.GlsError, match="coef\\[comp\\]"):
            op.set_node_constraints(half[:1], [0], [[1.0, 0.0]])
    with pytest.raises(glsamd.GlsError, match="velocity component"):
        op.set_node_constraints(nodes[:1], [case.dim], coef[:1])
    # a non-zero constraint value on a Dirichlet component of a node with a row
    mesh3 = gm.cylinder(3, 2, 0)
    d = deck(RE3900)
    d.no_slip_cylinder, d.no_slip_wall = False, False
    cm3 = d.mask(mesh3)
    n3, c3, k3 = d.node_constraints(mesh3)
    on_wall = np.nonzero((cm3[n3] >> 2) & 1)[0]
    assert len(on_wall) > 0
    params, w = d.operator_parameters()
    c = Case(mesh3, cm3, params, w)
    c.outflow, c.node_constraints = None, (n3, c3, k3)
    op3 = slip_ref.gpu(c, "f64")
    g = np.zeros(c.n_dofs)
    g[n3[on_wall[0]] * 4 + 2] = 1.0
    with pytest.raises(glsamd.GlsError, match="non-zero constraint value"):
        op3.set_constraint_values(g)
    op3.set_constraint_values(np.zeros(c.n_dofs))
    # cleared rows: the plain operator again
    op.set_node_constraints([], [], [])
    assert op.n_node_constraints == (0, 0)
    op.vmult_cells(y, x, 0, case.mesh.n_cells)
