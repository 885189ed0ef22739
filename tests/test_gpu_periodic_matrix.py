"""A periodic node map in the assembled system matrix (host and device) and
what it feeds (matrix-based vmult, ILU-preconditioned GMRES), against the dense
C^T A C of tests/periodic_ref.py.

Tolerances: the project's for an assembled matrix against vmult, relative l2
1e-12 in FP64 and 2e-5 in FP32 (tests/test_gpu_system_matrix.py)."""
import numpy as np
import pytest

import glsinputs as gi
import periodic_ref as pr
from helpers import rel_err

ref_case, _gpu, _np, _poison = pr.ref_case, pr.gpu_poisoned, pr.to_np, pr.poison

pytestmark = pytest.mark.gpu


def _device_csr(op):
    import scipy.sparse as sp
    rp, ci, va = (t.cpu().numpy() for t in op.system_matrix_device())
    return sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(op.n_dofs, op.n_dofs))


@pytest.mark.parametrize("brick", [None, (0, 0, 0)], ids=["declared", "percell"])
@pytest.mark.parametrize("shape", ["a_2d_q1", "c_3d_q2_yz", "d_3d_q2_brick_period"])
def test_system_matrix_is_ctac(shape, brick):
    import torch
    case, ref = ref_case(shape)
    pm = case.pm
    op = _gpu(case, "f64", brick)
    want = pr.dense_constrained(pr.oracle(case), case.mesh, pm)
    A = op.system_matrix()
    D = _device_csr(op)
    assert np.array_equal(D.indptr, A.indptr) and np.array_equal(D.indices, A.indices)
    # host and device assemblies are bitwise equal
    assert np.array_equal(D.data, A.data)
    scale = np.abs(want).max()
    err = np.abs(A.toarray() - want).max() / scale
    print(shape, "max entry error / max entry", err)
    assert err < 1e-12
    assert rel_err(A.toarray(), want) < 1e-12
    f = np.nonzero(pm.fixed)[0]
    for M in (A, D):
        assert np.all(M.diagonal()[f] == 1.0)
        assert np.all(np.diff(M.indptr)[f] == 1)              # unit rows, present in the pattern
        assert np.all(abs(M[:, f]).sum(axis=0) == 1.0)        # and columns
    assert rel_err(A.diagonal(), ref["diag"]) < 1e-12
    # matrix-based vmult equals the matrix-free one; no slave entry is read
    x = gi.rnd(7, case.n_dofs)
    src = op._dev(_poison(pm, x))
    free = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(True)
    mb = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(False)
    torch.cuda.synchronize()
    keep = ~pm.is_slave_dof
    assert np.all(np.isfinite(_np(mb)[keep]))
    assert rel_err(_np(mb)[keep], _np(free)[keep]) < 1e-12
    assert rel_err(_np(mb)[keep], (want @ x)[keep]) < 1e-12


def test_system_matrix_device_f32_operator():
    case, ref = ref_case("c_3d_q2_yz")
    op = _gpu(case, "f32")
    D = _device_csr(op)
    want = pr.dense_constrained(pr.oracle(case), case.mesh, case.pm)
    assert rel_err(D.toarray(), want) < 2e-5
    assert np.all(D.diagonal()[case.pm.fixed] == 1.0)


def test_gmres_ilu_cylinder():
    import torch
    import glsamd
    import glssolvers
    case, ref = ref_case("e_cylinder")
    pm = case.pm
    op = _gpu(case, "f64")
    o = pr.oracle(case)
    b = gi.rnd(31, case.n_dofs)
    b[pm.fixed] = 0.0
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
        r = b - pr.vmult(o, pm, got)
        assert np.linalg.norm(r) <= 1.01e-8 * np.linalg.norm(b)
        assert np.all(got[pm.fixed] == 0.0)
        # distribute makes the solution periodic
        op.distribute(x, homogeneous=True)
        torch.cuda.synchronize()
        assert np.array_equal(_np(x), pm.resolve(got))


def test_partitioned_operators_are_refused():
    import ctypes as C
    import glsamd
    case, ref = ref_case("a_2d_q1")
    op = _gpu(case, "f32")
    desc = glsamd.DistDesc()
    desc.rank, desc.world = 0, 1
    h = C.c_void_p()
    rc = glsamd.lib().gls_dist_create(op.h, C.byref(desc), C.byref(h))
    assert rc != 0 and b"periodic node map" in glsamd.lib().gls_last_error()
