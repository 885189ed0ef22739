"""Node constraints in the assembled system matrix (host and device: C^T A C
on the pattern of A), what it feeds (matrix-based vmult, ILU-preconditioned
GMRES, the Newton solve) and the refusals, against tests/slip_ref.py.

Tolerances: the project's for an assembled matrix against vmult, relative l2
1e-12 in FP64 and 2e-5 in FP32 (tests/test_gpu_system_matrix.py)."""
import numpy as np
import pytest

import glsinputs as gi
import slip_ref
from helpers import deck, rel_err
from test_gpu_slip import RE20, ref_case, _np

pytestmark = pytest.mark.gpu


def _device_csr(op):
    import scipy.sparse as sp
    rp, ci, va = (t.cpu().numpy() for t in op.system_matrix_device())
    return sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(op.n_dofs, op.n_dofs))


@pytest.mark.parametrize("shape", ["2d_q1_r1", "2d_q2_r0", "re3900_r0"])
def test_system_matrix_is_ctac(shape):
    import torch
    case, ref = ref_case(shape)
    op = slip_ref.gpu(case, "f64")
    plain = slip_ref.gpu(case, "f64")
    plain.set_node_constraints([], [], [])
    A0 = plain.system_matrix()
    A = op.system_matrix()
    D = _device_csr(op)
    # the pattern does not change
    assert np.array_equal(A.indptr, A0.indptr) and np.array_equal(A.indices, A0.indices)
    assert np.array_equal(D.indptr, A.indptr) and np.array_equal(D.indices, A.indices)
    x = gi.rnd(7, case.n_dofs)
    want = slip_ref.vmult(case.oracle(), case.rows, x)
    assert rel_err(A @ x, want) < 1e-12
    assert rel_err(D @ x, want) < 1e-12
    assert rel_err(D.data, A.data) < 1e-12
    elim = case.rows.elim
    for M in (A, D):
        assert np.all(M.diagonal()[elim] == 1.0)
        assert np.all(abs(M[elim]).sum(axis=1) == 1.0)       # unit rows
        assert np.all(abs(M[:, elim]).sum(axis=0) == 1.0)    # and columns
    assert rel_err(A.diagonal(), ref["diag"]) < 1e-12
    # matrix-based vmult equals the matrix-free one
    src = op._dev(x)
    free = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(True)
    mb = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(False)
    torch.cuda.synchronize()
    assert rel_err(_np(mb), _np(free)) < 1e-12
    assert np.array_equal(_np(mb)[elim], x[elim])


def test_system_matrix_device_f32_operator():
    case, ref = ref_case("re3900_r0")
    op = slip_ref.gpu(case, "f32")
    D = _device_csr(op)
    x = gi.rnd(7, case.n_dofs)
    assert rel_err(D @ x, slip_ref.vmult(case.oracle(), case.rows, x)) < 2e-5
    assert np.all(D.diagonal()[case.rows.elim] == 1.0)


def test_gmres_ilu_2d():
    import torch
    import glsamd
    import glssolvers
    case, ref = ref_case("2d_q2_r1")
    op = slip_ref.gpu(case, "f64")
    A = op.system_matrix()
    b = gi.rnd(31, case.n_dofs)
    b[np.asarray(A.diagonal() == 1.0) & (np.diff(A.indptr) == 1)] = 0.0  # Dirichlet rows
    b[case.rows.elim] = 0.0
    for device in (False, True):
        prec = glssolvers.MatrixPreconditioner(op, "ILU", device=device)
        prec.initialize()
        solver = glsamd.LinearSolverGMRES(op, prec, relative_tolerance=1e-8,
                                          absolute_tolerance=0.0)
        x = torch.zeros(case.n_dofs, dtype=torch.float64, device="cuda")
        solver.solve(x, torch.from_numpy(b).cuda())
        got = x.cpu().numpy()
        print("GMRES + ILU, device =", device, solver.last["n_iterations"], "iterations")
        assert solver.last["converged"] == 1
        r = b - slip_ref.vmult(case.oracle(), case.rows, got)
        assert np.linalg.norm(r) <= 1.01e-8 * np.linalg.norm(b)
        assert np.all(got[case.rows.elim] == 0.0)


def test_newton_stationary_re20_slip_cylinder():
    """The stationary 2D Re20 deck with the cylinder on slip at r1 through
    wire_newton (ILU of C^T A C as the preconditioner): converges to the
    deck's Newton tolerance and u . n = 0 on the cylinder."""
    import torch
    import glsamd
    import glssolvers as gs
    d = deck(RE20)
    d.no_slip_cylinder = False
    mesh = d.mesh(1)
    cmask = d.mask(mesh)
    nodes, comp, coef = d.node_constraints(mesh)
    normals = mesh.node_constraints([2], d.boundary_descriptor()[0])[3]
    params, w = d.operator_parameters()
    g = d.constraint_values(mesh, 0.0)
    op = glsamd.NavierStokesOperator(mesh, cmask, "f64", node_constraints=(nodes, comp, coef))
    op.set_parameters(**params)
    op.set_constraint_values(g)
    sol = op.initialize_dof_vector()
    op.distribute(sol)  # the start value carries the Dirichlet values
    op.set_linearization_point(sol)
    if params["order"] > 0:
        op.set_previous_solution([sol] * (params["order"] + 1), w)
    pre = gs.MatrixPreconditioner(op, "ILU", fill_level=1)
    lin = glsamd.LinearSolverGMRES(op, pre, n_max_iterations=1000, relative_tolerance=1e-4)
    newton = gs.wire_newton(gs.NonLinearSolverNewton(inexact_newton=False,
                                                     newton_tolerance=1e-7), op, cmask, lin, pre)
    n_it = newton.solve(sol)
    torch.cuda.synchronize()
    print("newton steps", n_it, "residuals", newton.history)
    assert newton.history[-1] <= 1e-7 < newton.history[0]
    op.distribute(sol)
    u = _np(sol).reshape(-1, 3)
    un = np.einsum("ie,ie->i", u[nodes][:, :2], normals)
    print("max |u.n|", np.abs(un).max(), "max |u|", np.abs(u[:, :2]).max())
    assert np.abs(u[nodes][:, :2]).max() > 1e-3  # the cylinder is not no-slip
    assert np.abs(un).max() <= 1e-12 * np.abs(u[:, :2]).max()
    con = ((cmask[:, None] >> np.arange(3)[None, :]) & 1).astype(bool).ravel()
    assert np.array_equal(_np(sol)[con], g[con])


def test_refusals_name_what_is_unsupported():
    import glsamd
    case, ref = ref_case("2d_q2_r0")
    op = slip_ref.gpu(case, "f32")
    # (the direct coarse solvers: tests/test_gpu_slip_mg.py)
    # partitioned operators
    import ctypes as C
    desc = glsamd.DistDesc()
    desc.rank, desc.world = 0, 1
    h = C.c_void_p()
    rc = glsamd.lib().gls_dist_create(op.h, C.byref(desc), C.byref(h))
    assert rc != 0 and b"node constraints" in glsamd.lib().gls_last_error()
