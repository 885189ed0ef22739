"""Periodic node identification (glsOpDesc.node_master) on the GPU against
the numpy restatement tests/periodic_ref.py on top of the oracle (TEST
INFRASTRUCTURE), which runs over the caller's connectivity.

Tolerances are the project's (test_gpu_parity): FP64 relative l2 1e-12, FP32
2e-5; the diagonals 10 times that, as there.  Every case runs with the
declared brick, with discovered bricks ("auto") and with the per-cell kernel.

The slave entries of the source vectors and of the linearization point are
NaN in every call: no entry point reads them.  vmult's row of a slave is the
identity, so dst holds the source's NaN there; every other entry, and every
entry of the residuals and diagonals, must be finite."""
import numpy as np
import pytest

import forces_ref as fr
import glsmesh as gm
import periodic_ref as pr
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}
RE100, SHAPES, _cache = pr.RE100, pr.SHAPES, pr._cache
ref_case, _gpu, _np, _poison = pr.ref_case, pr.gpu_poisoned, pr.to_np, pr.poison
BRICKS = {"declared": None, "auto": "auto", "percell": (0, 0, 0)}


@pytest.mark.parametrize("brick", list(BRICKS))
@pytest.mark.parametrize("fixed", [False, True], ids=["newton", "fixed"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_operator_against_periodic_ref(shape, prec, fixed, brick):
    import torch
    case, ref = ref_case(shape, fixed)
    pm = case.pm
    op = _gpu(case, prec, BRICKS[brick])
    if brick == "declared":
        assert op.brick_shape != (0, 0, 0)  # the brick kernels run
    if brick == "percell":
        assert op.brick_shape == (0, 0, 0)
    op.set_constraint_values(_poison(pm, ref["g"]))
    src = op._dev(_poison(pm, case.src))
    lin = op._dev(_poison(pm, case.u_star))
    out = {k: op.initialize_dof_vector() for k in ("vmult", "res", "plain", "rhs", "diag", "inv")}
    op.vmult(out["vmult"], src)
    op.evaluate_residual(out["res"], lin)
    op.evaluate_residual_plain(out["plain"], lin)
    op.evaluate_rhs(out["rhs"])
    op.compute_diagonal(out["diag"])
    op.compute_inverse_diagonal(out["inv"])
    u_max = op.get_max_u(lin)
    torch.cuda.synchronize()
    got = {k: _np(v) for k, v in out.items()}
    # the identity rows of the slaves hand the source's NaN through; nothing else is NaN
    assert np.all(np.isnan(got["vmult"][pm.sdofs]))
    got["vmult"][pm.sdofs] = case.src[pm.sdofs]
    for k, v in got.items():
        assert np.all(np.isfinite(v)), k
    assert np.isfinite(u_max)
    err = {k: rel_err(got[k], ref[k]) for k in got}
    print(shape, prec, "fixed" if fixed else "newton", brick, op.brick_shape, err)
    for k in ("vmult", "res", "plain", "rhs"):
        assert err[k] < TOL[prec], k
    for k in ("diag", "inv"):
        assert err[k] < TOL[prec] * 10, k
    f = pr.fixed_dofs(pm, case.rows)
    keep = f & ~pm.is_slave_dof
    if case.rows is not None:
        assert op.n_node_constraints[0] == len(case.rows.nodes) > 0
    assert np.all(got["vmult"][keep] == _np(src)[keep])  # identity rows
    for k in ("res", "plain", "rhs"):
        assert np.all(got[k][f] == 0.0)
    assert np.all(got["diag"][f] == 1.0) and np.all(got["inv"][f] == 1.0)


def test_period_of_one_cell_is_refused():
    import glsamd
    case = pr.box_case((2, 1), 2, 0, "y")
    with pytest.raises(glsamd.GlsError, match=r"cell 0 lists node \d+ twice under node_master"):
        pr.gpu(case, "f64")


def test_map_is_validated():
    import glsamd
    case, _ = ref_case("a_2d_q1")
    m = case.mesh
    bad = case.node_master.copy()
    bad[0] = m.n_nodes
    with pytest.raises(glsamd.GlsError, match=r"node_master\[0\] out of range"):
        glsamd.NavierStokesOperator(m, case.cmask, "f64", node_master=bad)
    s = case.pm.slaves[0]
    free = [i for i in range(m.n_nodes) if case.node_master[i] == i and i != case.node_master[s]]
    bad = case.node_master.copy()
    bad[free[0]] = s  # a master that is a slave
    with pytest.raises(glsamd.GlsError, match="not idempotent"):
        glsamd.NavierStokesOperator(m, case.cmask, "f64", node_master=bad)
    with pytest.raises(glsamd.GlsError, match="partitioned"):
        glsamd.NavierStokesOperator(m, case.cmask, "f64", node_master=case.node_master,
                                    n_owned_nodes=m.n_nodes - 1)


@pytest.mark.parametrize("shape", ["b_2d_q2_brick_period", "c_3d_q2_yz", "d_3d_q2_brick_period",
                                   "e_cylinder", "e_cylinder_slip"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_deterministic_repeats_bitwise(shape, prec):
    import torch
    case, ref = ref_case(shape)
    op = _gpu(case, prec, deterministic=True)
    src = op._dev(case.pm.resolve(case.src))
    a, b = op.initialize_dof_vector(), op.initialize_dof_vector()
    da, db = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(a, src)
    op.compute_inverse_diagonal(da)
    op.vmult(b, src)
    op.compute_inverse_diagonal(db)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(da, db)
    want = ref["vmult"].copy()
    want[case.pm.sdofs] = case.pm.resolve(case.src)[case.pm.sdofs]
    assert rel_err(_np(a), want) < TOL[prec]


@pytest.mark.parametrize("shape", ["c_3d_q2_yz", "e_cylinder", "e_cylinder_slip"])
def test_distribute(shape):
    import torch
    case, ref = ref_case(shape)
    pm = case.pm
    op = _gpu(case, "f64")
    op.set_constraint_values(_poison(pm, ref["g"]))
    x = op._dev(_poison(pm, case.src))
    op.distribute(x)
    y = op._dev(_poison(pm, case.src))
    op.distribute(y, homogeneous=True)
    torch.cuda.synchronize()
    # (with rows: the coefficient sums round as the kernel's do or one ulp off)
    tol = 0.0 if case.rows is None else 1e-15
    assert np.abs(_np(x) - pr.distribute(pm, case.src, ref["g"], case.rows)).max() <= tol
    assert np.abs(_np(y) - pr.distribute(pm, case.src, None, case.rows)).max() <= tol
    assert np.array_equal(_np(x)[pm.sdofs], _np(x)[pm.mdofs])


def test_node_constraint_row_on_a_slave_is_refused():
    import glsamd
    case, _ = ref_case("e_cylinder")
    op = _gpu(case, "f64")
    s = int(case.pm.slaves[len(case.pm.slaves) // 2])
    assert case.pm.op_mask[case.node_master[s]] == 0  # a free master: the row is legal there
    coef = np.zeros((1, 2))
    with pytest.raises(glsamd.GlsError, match=rf"node {s} is a slave of the periodic node map"):
        op.set_node_constraints(np.array([s]), np.array([1], dtype=np.int32), coef)
    op.set_node_constraints(np.array([case.node_master[s]]), np.array([1], dtype=np.int32), coef)
    assert op.n_node_constraints[0] == 1


# ------------------------------------------------ (f) the shift known answer
def _shift_setup(dims, periodic):
    """A box periodic in every direction, Q2, r1, uniform cells; fields built
    from the node coordinates; the node permutation of a shift by one cell
    along y (masters onto masters)."""
    case = pr.box_case(dims, 2, 1, periodic)
    m, pm = case.mesh, case.pm
    assert not case.cmask.any()
    L = np.array([float(n) for n in dims])
    h = 0.5  # one cell of the once refined unit coarse cells
    # nodes lie on the lattice of spacing h / 2; positions modulo the period
    per = (4 * L).astype(np.int64)
    key = lambda X: [tuple(r) for r in np.round(X * 4).astype(np.int64) % per]
    masters = np.nonzero(pm.master == np.arange(m.n_nodes))[0]
    at = {k: n for k, n in zip(key(m.coords[masters]), masters)}
    assert len(at) == len(masters)
    moved = m.coords[masters].copy()
    moved[:, 1] += h
    perm = np.array([at[k] for k in key(moved)])  # master at x -> master at x + h e_y
    assert sorted(perm) == sorted(masters)
    X = m.coords / L * 2 * np.pi
    nc = m.dim + 1

    def field(seed, scale):
        v = np.zeros((m.n_nodes, nc))
        for c in range(nc):
            ph = 0.3 * seed + 0.7 * c
            v[:, c] = scale * (np.sin(X[:, 0] + ph) * np.cos(2 * X[:, 1] - ph) + 0.25 * c
                               + (np.sin(X[:, 2] + 2 * ph) if m.dim == 3 else 0.0))
        return v.ravel()

    def shift(v):
        w = np.zeros((m.n_nodes, nc))
        w[perm] = np.asarray(v).reshape(-1, nc)[masters]
        return pm.resolve(w.ravel())

    return case, masters, perm, field, shift


@pytest.mark.parametrize("brick", list(BRICKS))
@pytest.mark.parametrize("dims,periodic", [((2, 2), "xy"), ((2, 2, 2), "xyz")], ids=["2d", "3d"])
def test_shift_by_one_cell(dims, periodic, brick):
    """Independent of the oracle: on a uniform, fully periodic box the operator
    commutes with the shift by one cell, to 1e-12 (FP64 summation order)."""
    import torch
    key = ("shift", dims)
    if key not in _cache:
        _cache[key] = _shift_setup(dims, periodic)
    case, masters, perm, field, shift = _cache[key]
    pm, nc = case.pm, case.dim + 1
    u_star, src = field(1, 1.0), field(2, 0.5)
    hist = [field(3 + i, 1.0) for i in range(len(case.hist))]
    outs = []
    for mv in (lambda v: v, shift):
        op = pr.gpu(case, "f64", brick=BRICKS[brick], u_star=_poison(pm, mv(u_star)),
                    hist=[_poison(pm, mv(h)) for h in hist])
        dst, res = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.vmult(dst, op._dev(_poison(pm, mv(src))))
        op.evaluate_residual_plain(res, op._dev(_poison(pm, mv(u_star))))
        torch.cuda.synchronize()
        outs.append((_np(dst).reshape(-1, nc), _np(res).reshape(-1, nc)))
    for k, name in enumerate(("vmult", "residual")):
        plain, moved = outs[0][k][masters], outs[1][k][perm]
        assert np.all(np.isfinite(plain)) and np.linalg.norm(plain) > 0
        e = rel_err(moved, plain)
        print(dims, brick, name, e)
        assert e < 1e-12, name


# ------------------------------------------------------- forces and the probe
def test_surface_force_and_probe():
    """On (e), fed the distributed vector with NaN on the slaves: the dofs are
    read through the map, the geometry through the caller's connectivity."""
    case, _ = ref_case("e_cylinder")
    m, pm = case.mesh, case.pm
    nu = case.params["nu"]
    v = pm.resolve(np.random.default_rng(5).standard_normal(m.n_dofs))
    cells, faces = gm.boundary_faces(m, 2)
    ref_faces, scale = fr.surface_force(m, cells, faces, v, nu, 3)
    S = float(scale.sum())
    # points in the cells under the eliminated wall, on it, on its master wall,
    # and in front of and behind the cylinder (centred at the origin, radius 0.05)
    (x0, y0), (x1, y1) = m.coords.min(axis=0), m.coords.max(axis=0)
    at = lambda t: x0 + t * (x1 - x0)
    pts = np.array([[at(0.4), y1 - 1e-3], [at(0.6), y1], [at(0.8), y1 - 0.02], [at(0.5), y0],
                    [-0.06, 0.0], [0.06, 0.0]])
    want, count = fr.probe(m, pts, v)
    assert np.all(count >= 1)
    for prec in ("f64", "f32"):
        op = _gpu(case, prec)
        op.set_force_faces(cells, faces, 3)
        x = op._dev(_poison(pm, v))
        total = op.surface_force(x)
        found = op.set_probe_points(pts)
        assert np.all(found >= 1)
        got = op.probe(x)
        e_f = np.abs(total - ref_faces.sum(axis=0)).max() / S
        e_p = np.abs(got - want).max() / np.abs(want).max()
        print(prec, "force", e_f, "probe", e_p)
        assert e_f < TOL[prec] and e_p < TOL[prec]


# ------------------------------------------------------ vmult_cells with a map
@pytest.mark.parametrize("shape", ["b_2d_q2_brick_period", "c_3d_q2_yz"])
@pytest.mark.parametrize("brick", ["declared", "percell"])
def test_vmult_cells_goes_through_the_map(shape, brick):
    """The cell contributions of all cells into a zero vector, then the
    identity rows: vmult."""
    import torch
    case, ref = ref_case(shape)
    pm = case.pm
    op = _gpu(case, "f64", BRICKS[brick])
    src = op._dev(_poison(pm, case.src))
    dst = op.initialize_dof_vector()
    dst.zero_()
    op.vmult_cells(dst, src, 0, case.mesh.n_cells)
    op.apply_identity_rows(dst, src)
    torch.cuda.synchronize()
    keep = ~pm.is_slave_dof
    assert rel_err(_np(dst)[keep], ref["vmult"][keep]) < TOL["f64"]


def test_mapping_points_with_a_map_are_refused_by_the_library():
    """An FE_Q_iso_Q1 level (glsOpDesc.mapping_points) with node_master: the
    Python layer refuses it, and so does gls_op_create for any other caller."""
    import ctypes as C
    import glsamd
    case, _ = ref_case("b_2d_q2_brick_period")
    m = case.mesh
    with pytest.raises(NotImplementedError, match="FE_Q_iso_Q1"):
        glsamd.NavierStokesOperator(gm.IsoQ1Mesh(m), case.cmask, "f64",
                                    node_master=case.node_master)
    meas, hmin = m.cell_measure()
    keep = [np.ascontiguousarray(m.cell_nodes, dtype=np.uint32),
            np.ascontiguousarray(m.coords), np.ascontiguousarray(case.cmask, dtype=np.uint8),
            np.ascontiguousarray(meas), np.ascontiguousarray(hmin),
            np.ascontiguousarray(m.coords[m.cell_nodes]),  # the cells' own Q2 points
            np.ascontiguousarray(case.node_master, dtype=np.int64)]
    d = glsamd.OpDesc(m.dim, m.degree, glsamd.GLS_F64, m.n_cells, m.n_nodes, m.n_nodes,
                      keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data,
                      keep[3].ctypes.data, keep[4].ctypes.data, (C.c_int * 3)(0, 0, 0))
    d.mapping_degree, d.mapping_points = m.degree, keep[5].ctypes.data
    d.node_master = keep[6].ctypes.data
    h = C.c_void_p()
    assert glsamd.lib().gls_op_create(C.byref(d), C.byref(h)) != 0
    assert b"node_master with mapping_points" in glsamd.lib().gls_last_error()
