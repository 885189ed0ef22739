"""GPU parity at the (dim, degree) pairs the decks never reach -- (2,3), (3,1)
and (3,3) -- against the CPU oracle on the curved hyper cube of warped.py,
with (3,2), (2,2) and (2,1) as controls of the harness itself.

Every operator kernel is instantiated for six (dim, degree) pairs; the decks
are 2D Q1 / 3D Q2 (a few tests override to 2D Q2).  The other three have the
thread maps least like the tuned 3D Q2 one (3D Q3: one cell per wavefront, 3D
Q1: eight, 2D Q3: four) and run on the brick kernels' generic paths.

Meshes are the smallest that reach each structure (at most 64 cells / 8788
dofs); flat_axis keeps the cells of one half exactly Cartesian so both
geometry classes of the operator run in one mesh (flat_axis=0: mixed inside
bricks and wavefronts; flat_axis=2 at n_ref 2: whole bricks of either class).

Covered per pair, FP64 and FP32: vmult and residual in the four operator modes
on the default brick and the per-cell kernel, smaller bricks, partial
workgroups (cells dropped from the list), shuffled and rotated cells with
discovered bricks, the deterministic accumulation, the per-q tables, both
diagonals, get_max_u, the element and system matrices, the weak outflow
faces; and that two Q3 multigrid levels are refused.

Measured on an MI355X (worst block over all meshes and modes): FP64 1.2e-14
(3,3), 7.6e-15 (2,3), 1.6e-15 (3,1); FP32 7.5e-7, 9.2e-7, 5.7e-7; with
outflow faces (residual at the linearization point, where the time terms
cancel) FP32 up to 6.1e-6, the Q2 control 7.2e-6.

Tolerances: the project's, FP64 1e-12 and FP32 2e-5 relative l2 -- applied to
every solution component's block (dst[c::nc]) on its own, and inside it to
three disjoint node sets: nodes interior to one cell, nodes shared by cells of
one brick, nodes on brick boundaries (a wrong write-out or reduction of the
few shared nodes cannot hide under the interior ones).  Constrained rows:
vmult hands src through exactly; in the residual they match the oracle to
1e-12 of the vector's norm."""
import functools

import numpy as np
import pytest

import glsmesh as gm
from helpers import Case, deck, rel_err
from shuffle import ShuffledMesh, check_tiling
from test_oracle_kat import _assemble
from warped import WarpedMesh, drop_middle, position_mask

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}
PRECS = ["f64", "f32"]

# id: dim, degree, n_ref, flat_axis
MESHES = {
    "q3_2d": (2, 3, 2, 0),        # 4 cells per wave, one 13x13 lattice
    "q3_2d_r1": (2, 3, 1, 0),     # one 2x2 brick (the n_ref 2 order tiles no 2x2)
    "q3_3d_r1": (3, 3, 1, 0),     # 1 cell per wave, two rounds in one brick
    "q3_3d_r2": (3, 3, 2, 0),     # several bricks, shared brick-boundary nodes
    "q3_3d_r2_z": (3, 3, 2, 2),   # ... whole bricks Cartesian or curved
    "q1_3d_r2": (3, 1, 2, 0),     # 8 cells per wave
    "q1_3d_r2_z": (3, 1, 2, 2),
    # one wave, workgroup 3/4 idle.  The only interior node of this mesh sits
    # on X_0 = 1/2 and belongs to all 8 cells, so no warp gives it both
    # geometry classes: flat_axis=0 leaves it all Cartesian, None all curved
    "q1_3d_r1": (3, 1, 1, 0),
    "q1_3d_r1_w": (3, 1, 1, None),
    "ctl_q2_3d": (3, 2, 1, 0),    # controls: pairs the suite already trusts
    "ctl_q2_2d": (2, 2, 2, 0),
    "ctl_q1_2d": (2, 1, 2, 0),
}
DECK = {2: "input_turek_2D_Re100.json", 3: "input_hoffmann_3D_Re3900.json"}
# the four parameter sets of test_gpu_parity.py (deck default: Newton, BDF2,
# q-wise delta), same overrides as its test_vmult_variants
PSETS = {
    "default": {},
    "fixed": dict(nonlinear_solver="Picard"),
    "cellwise": dict(cell_wise_stabilization=True),
    "theta": dict(time_integration="theta", theta=0.5, consider_time_derivative=False,
                  nonlinear_solver="Picard"),
}


def _np(t):
    return t.double().cpu().numpy()


def _parameters(dim, pset):
    d = deck(DECK[dim])
    for k, v in PSETS[pset].items():
        setattr(d, k, v)
    return d.operator_parameters(2.5e-4)


@functools.lru_cache(maxsize=None)
def _base(dim, k, n_ref):
    return gm.hypercube(dim, k, n_ref)


class Ref:
    """One mesh + parameter set: the inputs of helpers.Case and the oracle's
    results, computed once and shared (never written to)."""

    def __init__(self, mesh, cmask, pset):
        params, w = _parameters(mesh.dim, pset)
        self.case = Case(mesh, cmask, params, w, u_inf=1.0)
        self.o = self.case.oracle()
        self.vmult = self.o.vmult(self.case.src)
        self.residual = self.o.evaluate_residual(self.case.src)
        for v in (self.vmult, self.residual):
            v.setflags(write=False)
        nc = mesh.dim + 1
        self.constrained = np.zeros(mesh.n_dofs, bool)
        for comp in range(nc):
            self.constrained[comp::nc] = (cmask >> comp) & 1

    @functools.cached_property
    def inverse_diagonal(self):
        return self.o.inverse_diagonal()

    @functools.cached_property
    def diagonal(self):
        return self.o.diagonal()


@functools.lru_cache(maxsize=None)
def ref_of(mesh_id, pset, keep=None, order=None):
    """keep: that many cells, the others dropped from the middle of the list;
    order: all cells, listed brick by brick for bricks of that shape."""
    dim, k, n_ref, flat = MESHES[mesh_id]
    base = _base(dim, k, n_ref)
    kept = None if keep is None else drop_middle(base.n_cells, keep)
    if order is not None:
        kept = _brick_major(WarpedMesh(base), order)
    mesh = WarpedMesh(base, flat_axis=flat, keep=kept)
    return Ref(mesh, position_mask(mesh.ref_coords), pset)


def node_classes(mesh, op):
    """Disjoint node sets by how the running kernel shares them: interior to
    one cell, shared by cells of one brick, on a brick boundary (from
    cell_permutation() and brick_shape; the per-cell kernel is bricks of one
    cell), and the nodes no cell lists."""
    perm = np.asarray(op.cell_permutation())  # internal cell -> caller cell
    cpb = int(np.prod(op.brick_shape)) if op.brick_shape != (0, 0, 0) else 1
    brick = np.empty(mesh.n_cells, np.int64)
    brick[perm] = np.arange(mesh.n_cells) // cpb
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    n_cell = np.bincount(cn.ravel(), minlength=mesh.n_nodes)
    pairs = np.unique(np.stack([cn.ravel(), np.repeat(brick, cn.shape[1])], axis=1), axis=0)
    n_brick = np.bincount(pairs[:, 0], minlength=mesh.n_nodes)
    cls = {"interior": np.nonzero(n_cell == 1)[0],
           "in_brick": np.nonzero((n_cell > 1) & (n_brick == 1))[0],
           "brick_boundary": np.nonzero(n_brick > 1)[0],
           "untouched": np.nonzero(n_cell == 0)[0]}
    assert sum(len(v) for v in cls.values()) == mesh.n_nodes
    return cls


def check_vector(label, got, ref, mesh, classes, prec, scale=1):
    """Relative l2 of every component block, whole and per node class; the
    rows of untouched nodes equal the oracle's exactly.  Prints the worst."""
    nc = mesh.dim + 1
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = TOL[prec] * scale
    assert np.all(np.isfinite(got)), label
    errs = {}
    for comp in range(nc):
        errs[f"all/c{comp}"] = rel_err(got[comp::nc], ref[comp::nc])
        for name in ("interior", "in_brick", "brick_boundary"):
            idx = classes[name] * nc + comp
            if len(idx):
                errs[f"{name}/c{comp}"] = rel_err(got[idx], ref[idx])
    worst = max(errs, key=errs.get)
    print(f"DEG {label} worst {worst} {errs[worst]:.3e} whole {rel_err(got, ref):.3e}")
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, (label, bad)
    if len(classes["untouched"]):
        idx = (classes["untouched"][:, None] * nc + np.arange(nc)).ravel()
        want = ref[idx] if prec == "f64" else ref[idx].astype(np.float32).astype(np.float64)
        assert np.array_equal(got[idx], want), label
    return errs[worst]


def check_operator(label, r, op, prec, residual=True, diagonal=False):
    """vmult (+ residual, + diagonals) of one operator against the shared
    reference, by component and node class; constrained rows separately."""
    import torch
    case, mesh = r.case, r.case.mesh
    cls = node_classes(mesh, op)
    src = op._dev(case.src)
    dst = op.initialize_dof_vector()
    for _ in range(2):  # a repeated apply overwrites dst completely
        op.vmult(dst, src)
    res = op.initialize_dof_vector()
    if residual:
        op.evaluate_residual_plain(res, src)
    torch.cuda.synchronize()
    got = _np(dst)
    check_vector(f"{label} vmult", got, r.vmult, mesh, cls, prec)
    assert np.array_equal(got[r.constrained], _np(src)[r.constrained]), label
    if residual:
        got = _np(res)
        check_vector(f"{label} residual", got, r.residual, mesh, cls, prec)
        assert (np.abs(got - r.residual)[r.constrained].max(initial=0.0)
                <= 1e-12 * np.linalg.norm(r.residual)), label
    if diagonal:
        inv, dg = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.compute_inverse_diagonal(inv)
        op.compute_diagonal(dg)
        torch.cuda.synchronize()
        # the bound of test_gpu_parity.test_inverse_diagonal
        check_vector(f"{label} inverse_diagonal", _np(inv), r.inverse_diagonal, mesh, cls,
                     prec, 10)
        check_vector(f"{label} diagonal", _np(dg), r.diagonal, mesh, cls, prec, 10)
        assert np.all(_np(inv)[r.constrained] == 1.0) and np.all(_np(dg)[r.constrained] == 1.0)
    return cls


# ------------------------------------------------------------ operator paths
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pset", list(PSETS))
@pytest.mark.parametrize("mesh_id", list(MESHES))
def test_operator_paths(mesh_id, pset, prec):
    """vmult and the residual on the default brick and on the per-cell kernel."""
    r = ref_of(mesh_id, pset)
    mesh = r.case.mesh
    op = r.case.gpu(prec)
    assert op.brick_shape != (0, 0, 0)
    # a cell is Cartesian exactly where the warp left its nodes in place
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    n_flat = int(np.all(mesh.coords[cn] == mesh.ref_coords[cn], axis=(1, 2)).sum())
    assert op.geometry_counts() == (mesh.n_cells - n_flat, n_flat)
    if not mesh_id.startswith("q1_3d_r1"):
        assert 0 < n_flat < mesh.n_cells  # both geometry classes in one mesh
    cls = check_operator(f"{mesh_id} {pset} {prec} brick{op.brick_shape}", r, op, prec)
    if op.brick_shape[0] * op.brick_shape[1] * op.brick_shape[2] < mesh.n_cells:
        assert len(cls["brick_boundary"]) > 0
    pc = r.case.gpu(prec, brick=(0, 0, 0))
    assert pc.brick_shape == (0, 0, 0)
    check_operator(f"{mesh_id} {pset} {prec} percell", r, pc, prec)


# ------------------------------------------------------------ smaller bricks
def _tiles(mesh, shape):
    """Whether consecutive cells of the mesh's order form bricks of `shape`."""
    try:
        check_tiling(mesh.cell_nodes, mesh.dim, mesh.degree, shape, np.arange(mesh.n_cells))
    except AssertionError:
        return False
    return True


SMALL = {3: [(2, 2, 1), (2, 1, 1), (1, 1, 1)], 2: [(2, 2, 1), (4, 2, 1)]}


def _brick_major(mesh, shape):
    """The mesh's cells in the order that tiles bricks of `shape`: bricks
    lexicographic, cells lexicographic inside a brick."""
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    per_dir = round(mesh.n_cells ** (1.0 / mesh.dim))
    c = np.floor(mesh.ref_coords[cn].mean(axis=1) * per_dir).astype(np.int64)
    c = np.concatenate([c, np.zeros((len(c), 3 - mesh.dim), np.int64)], axis=1)
    b, i = c // np.array(shape), c % np.array(shape)
    return np.lexsort((i[:, 0], i[:, 1], i[:, 2], b[:, 0], b[:, 1], b[:, 2]))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mesh_id,shape", [
    pytest.param(m, s, id=f"{m}-{s[0]}x{s[1]}x{s[2]}") for m, (d, _, r, _) in MESHES.items()
    for s in SMALL[d] if np.prod(s) <= 2 ** (r * d)])
def test_smaller_bricks(mesh_id, shape, prec):
    """Smaller bricks change the round count and the shared-node structure;
    each gives the same operator.  A shape the mesh's cell order does not tile
    (the generator orders cells lexicographically inside 4 x 4 (x 2) bricks,
    which no 2 x 2 brick tiles) is refused by the library; the shape then
    runs on the same cells listed brick by brick."""
    import glsamd
    r = ref_of(mesh_id, "default")
    if not _tiles(r.case.mesh, shape):
        with pytest.raises(glsamd.GlsError, match="do not form the declared bricks"):
            r.case.gpu(prec, brick=shape)
        r = ref_of(mesh_id, "default", order=shape)
        assert _tiles(r.case.mesh, shape)
    op = r.case.gpu(prec, brick=shape)
    assert op.brick_shape == shape
    check_operator(f"{mesh_id} default {prec} brick{shape}", r, op, prec)


# ------------------------------------------------- workgroup tails, per-cell
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mesh_id,n_keep", [("q3_3d_r1", 7), ("q3_2d", 13), ("q1_3d_r2", 61)])
def test_percell_tails(mesh_id, n_keep, prec):
    """Cells dropped from the middle of the list: the last workgroup of the
    per-cell kernel is partial and its cells are not contiguous in the mesh."""
    r = ref_of(mesh_id, "default", n_keep)
    assert r.case.mesh.n_cells == n_keep
    op = r.case.gpu(prec)
    assert op.brick_shape == (0, 0, 0)
    cls = check_operator(f"{mesh_id} keep{n_keep} {prec} percell", r, op, prec, diagonal=True)
    assert (len(cls["untouched"]) > 0) == (r.case.mesh.degree > 1)


# ------------------------------------------------ deterministic accumulation
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mesh_id", ["q3_2d", "q3_3d_r2", "q1_3d_r2", "ctl_q2_3d"])
def test_deterministic(mesh_id, prec):
    """GLS_DETERMINISTIC (the brick kernels' barrier-ordered accumulation,
    an instantiation of its own per (dim, degree)): the same operator, and
    bitwise the same from run to run."""
    import torch
    r = ref_of(mesh_id, "default")
    op = r.case.gpu(prec)
    op.set_parameters(**r.case.params, deterministic=True)
    assert op.brick_shape != (0, 0, 0)
    check_operator(f"{mesh_id} default {prec} brick-det", r, op, prec, diagonal=True)
    src = op._dev(r.case.src)
    a, b = op.initialize_dof_vector(), op.initialize_dof_vector()
    da, db = op.initialize_dof_vector(), op.initialize_dof_vector()
    op.vmult(a, src)
    op.compute_inverse_diagonal(da)
    op.vmult(b, src)
    op.compute_inverse_diagonal(db)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(da, db)


# ---------------------------------------------------------------- cell order
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mesh_id,seed", [("q3_3d_r1", 5), ("q3_2d", 9)])
def test_shuffled_rotated_cells(mesh_id, seed, prec):
    """Arbitrary cell order and per-cell orientation: the bricks are
    discovered (the measures and the mask follow the permutation)."""
    warped = ref_of(mesh_id, "default").case.mesh
    sm = ShuffledMesh(warped, seed, rotate=True)
    meas, hmin = warped.cell_measure()
    assert np.array_equal(sm.cell_measure()[0], meas[sm.cell_order])
    r = Ref(sm, position_mask(warped.ref_coords)[sm.node_old], "default")
    op = r.case.gpu(prec, brick="auto")
    assert op.brick_shape != (0, 0, 0)
    check_operator(f"{mesh_id} shuffled {prec} brick{op.brick_shape}", r, op, prec,
                   diagonal=True)
    # the bricks' internal cell order is not the caller's; per-cell results
    # come back in the caller's
    perm = np.asarray(op.cell_permutation())
    assert sorted(perm.tolist()) == list(range(sm.n_cells)) and np.any(perm != np.arange(sm.n_cells))
    E = op.element_matrices()
    errs = [rel_err(E[c], r.o.cell_matrix(c)) for c in range(sm.n_cells)]
    print(f"DEG {mesh_id} shuffled {prec} element_matrices {max(errs):.3e}")
    assert max(errs) < TOL[prec]
    if prec == "f64":
        t, cw = op.download_tables()
        t_ref, cw_ref = r.o.tables()
        assert rel_err(t, t_ref) < 1e-13 and rel_err(cw, cw_ref) < 1e-13


# ----------------------------------------------- the other device quantities
GROUPS = lambda dim: {"delta1": [0], "delta2": [1], "U": range(2, 2 + dim),  # noqa: E731
                      "gradU": range(2 + dim, 2 + dim + dim * dim),
                      "gradP": range(2 + dim + dim * dim, 2 + 2 * dim + dim * dim),
                      "Ut_old": range(2 + 2 * dim + dim * dim, 2 + 3 * dim + dim * dim)}


@pytest.mark.parametrize("pset", ["default", "cellwise"])
@pytest.mark.parametrize("mesh_id", list(MESHES))
def test_tables(mesh_id, pset):
    r = ref_of(mesh_id, pset)
    t_ref, cw_ref = r.o.tables()
    for brick in (None, (0, 0, 0)):
        t, cw = r.case.gpu("f64", brick=brick).download_tables()
        # the bound of test_gpu_parity.test_tables_producers
        assert rel_err(t, t_ref) < 1e-13 and rel_err(cw, cw_ref) < 1e-13
        errs = {g: rel_err(t[:, :, list(f)], t_ref[:, :, list(f)])
                for g, f in GROUPS(r.case.dim).items()}
        print(f"DEG {mesh_id} {pset} f64 tables brick={brick}", errs)
        for g in errs:  # every field group by itself
            assert errs[g] < TOL["f64"], g


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pset", ["default", "cellwise"])
@pytest.mark.parametrize("mesh_id", list(MESHES))
def test_diagonals_and_max_u(mesh_id, pset, prec):
    import torch
    r = ref_of(mesh_id, pset)
    mesh = r.case.mesh
    for brick in (None, (0, 0, 0)):
        op = r.case.gpu(prec, brick=brick)
        cls = node_classes(mesh, op)
        inv, dg = op.initialize_dof_vector(), op.initialize_dof_vector()
        op.compute_inverse_diagonal(inv)
        op.compute_diagonal(dg)
        torch.cuda.synchronize()
        label = f"{mesh_id} {pset} {prec} {'percell' if brick else 'brick'}"
        # the bound of test_gpu_parity.test_inverse_diagonal
        check_vector(f"{label} inverse_diagonal", _np(inv), r.inverse_diagonal, mesh, cls,
                     prec, 10)
        check_vector(f"{label} diagonal", _np(dg), r.diagonal, mesh, cls, prec, 10)
        assert np.all(_np(inv)[r.constrained] == 1.0) and np.all(_np(dg)[r.constrained] == 1.0)
        for v in (r.case.u_star, r.case.src):
            got, want = op.get_max_u(op._dev(v)), r.o.get_max_u(v)
            print(f"DEG {label} get_max_u {abs(got - want) / want:.3e}")
            # the bound of test_gpu_layout.test_get_max_u
            assert abs(got - want) < (1e-13 if prec == "f64" else 1e-6) * want


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pset", ["default", "cellwise"])
@pytest.mark.parametrize("mesh_id", list(MESHES))
def test_element_matrices(mesh_id, pset, prec):
    """Every cell's element matrix, in the caller's cell order, per cell in
    the Frobenius norm."""
    r = ref_of(mesh_id, pset)
    op = r.case.gpu(prec)
    E = op.element_matrices()
    assert E.shape[0] == op.n_cells
    assert sorted(op.cell_permutation().tolist()) == list(range(op.n_cells))
    errs = np.array([rel_err(E[c], r.o.cell_matrix(c)) for c in range(op.n_cells)])
    print(f"DEG {mesh_id} {pset} {prec} element_matrices worst cell {errs.argmax()} "
          f"{errs.max():.3e}")
    assert errs.max() < TOL[prec]


@pytest.mark.parametrize("pset", ["default", "cellwise"])
@pytest.mark.parametrize("mesh_id", [m for m, (d, k, n, _) in MESHES.items()
                                     if (k * 2 ** n + 1) ** d * (d + 1) <= 1372])
def test_system_matrix(mesh_id, pset):
    """The assembled CSR against the densely assembled oracle matrix (bounds
    of test_gpu_system_matrix.py)."""
    r = ref_of(mesh_id, pset)
    mesh = r.case.mesh
    A = r.case.gpu("f64").system_matrix()
    assert A.shape == (mesh.n_dofs, mesh.n_dofs) and np.all(np.diff(A.indptr) > 0)
    ref = _assemble(r.o, mesh, r.case.cmask)
    err = rel_err(A.toarray(), ref)
    print(f"DEG {mesh_id} {pset} f64 system_matrix {err:.3e}")
    assert err < TOL["f64"]
    assert rel_err(A @ r.case.src, r.vmult) < TOL["f64"]
    assert rel_err(A.diagonal(), r.diagonal) < TOL["f64"]


# ------------------------------------------------------- weak outflow faces
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["cut", "nitsche"])
@pytest.mark.parametrize("mesh_id", ["q3_2d", "q3_3d_r1", "q1_3d_r2", "ctl_q2_3d"])
def test_outflow_faces(mesh_id, kind, prec):
    """The weak outflow face terms (their kernels take the degree at run
    time) on the face X_0 = 1 of the curved cells, as test_gpu_outflow.py on
    the decks: vmult, residual and the diagonal with the faces, brick and
    per-cell kernels; backflow through half of the faces for "cut", a
    non-zero target for "nitsche".  The pressure is free on the outflow."""
    import torch
    mesh = ref_of(mesh_id, "default").case.mesh
    dim, nc = mesh.dim, mesh.dim + 1
    X = mesh.ref_coords
    cmask = position_mask(X) & np.uint8((1 << dim) - 1)
    cells = np.nonzero(np.abs(X[np.asarray(mesh.cell_nodes, dtype=np.int64)][:, :, 0].max(axis=1)
                              - 1.0) < 1e-12)[0]
    of = (cells, np.ones(len(cells), np.int32), kind)  # face 2 * axis + side = 1
    params, w = _parameters(dim, "default")
    case = Case(mesh, cmask, params, w, u_inf=1.0)
    if kind == "cut":
        case.u_star[0::nc] -= 4.0 * (X[:, 1] > 0.5)
    o, plain = case.oracle(outflow=of), case.oracle()
    pts = o.outflow_face_points()
    assert np.allclose(pts[:, :, 0], 1.0, atol=1e-14)
    g = np.zeros_like(pts)
    g[:, :, 0] = 1.0 + pts[:, :, 1] * (1.0 - pts[:, :, 1])
    o.set_outflow_target(g)
    ref = {"vmult": o.vmult(case.src), "residual": o.evaluate_residual(case.u_star),
           "inverse_diagonal": o.inverse_diagonal()}
    # the face terms are a visible part of the operator
    assert rel_err(ref["vmult"], plain.vmult(case.src)) > 1e-6
    for brick in (None, (0, 0, 0)):
        op = case.gpu(prec, brick=brick, outflow=of)
        assert op.n_outflow_faces[0] == len(cells)
        assert rel_err(op.outflow_face_points(), pts) < 1e-14
        op.set_outflow_target(g)
        out = {k: op.initialize_dof_vector() for k in ref}
        op.vmult(out["vmult"], op._dev(case.src))
        op.evaluate_residual_plain(out["residual"], op._dev(case.u_star))
        op.compute_inverse_diagonal(out["inverse_diagonal"])
        torch.cuda.synchronize()
        cls = node_classes(mesh, op)
        label = f"{mesh_id} outflow-{kind} {prec} {'percell' if brick else 'brick'}"
        check_vector(f"{label} vmult", _np(out["vmult"]), ref["vmult"], mesh, cls, prec)
        check_vector(f"{label} residual", _np(out["residual"]), ref["residual"], mesh, cls, prec)
        # the assembled diagonal (1 / inverse), as test_gpu_outflow.py
        check_vector(f"{label} diagonal", 1 / _np(out["inverse_diagonal"]),
                     1 / ref["inverse_diagonal"], mesh, cls, prec, 10)


# ------------------------------------------------------------ Q3 multigrid
def test_q3_multigrid_is_refused():
    """The multigrid transfers exist for degree <= 2: two Q3 levels are
    refused by gls_mg_create (before any multigrid kernel runs)."""
    import glsamd
    meshes = [gm.hypercube(2, 3, 0), gm.hypercube(2, 3, 1)]
    masks = [position_mask(m.coords) for m in meshes]
    params, w = _parameters(2, "default")
    case = Case(meshes[1], masks[1], params, w)
    with pytest.raises(glsamd.GlsError, match=r"degree <= 2"):
        glsamd.build_gmg(meshes, masks, params, case.u_star, case.hist, w)
