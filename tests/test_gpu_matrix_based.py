"""The matrix-based operator mode (gls_op_set_matrix_based: vmult is the SpMV
k_csr_vmult of the device system matrix; NavierStokesOperatorMatrixBased,
operator_ns.cc:1525-1590) against the matrix-free vmult of the same operator
and against scipy on the host matrix.

Tolerances: the project's for an assembled matrix against vmult
(tests/test_gpu_system_matrix.py): relative l2 1e-12 in FP64, 2e-5 in FP32;
constrained entries exactly src."""
import numpy as np
import pytest

import glsinputs as gi
import matrix_cases as mc
from helpers import rel_err

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}


def _np(t):
    return t.double().cpu().numpy()


def _constrained(case):
    nc = case.dim + 1
    cm = np.asarray(case.cmask, dtype=np.int64)
    return ((np.repeat(cm, nc) >> np.tile(np.arange(nc), len(cm))) & 1) == 1


@pytest.mark.parametrize("key", mc.CASES)
def test_matrix_based_vmult(key):
    import torch
    b = mc.built(key)
    case, A = b["case"], b["A"]
    prec = key.split("-")[1]
    op = mc.make_op(key)
    src = op._dev(case.src)
    free = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(True)
    mb = op.vmult(op.initialize_dof_vector(), src).clone()
    again = op.vmult(op.initialize_dof_vector(), src).clone()
    down = op.vmult_interface_down(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(False)
    off = op.vmult(op.initialize_dof_vector(), src).clone()
    torch.cuda.synchronize()
    err = rel_err(_np(mb), _np(free))
    print(f"{key}: matrix-based vs matrix-free vmult rel l2 {err:.3e}")
    assert err < TOL[prec]
    con = _constrained(case)
    assert con.any() and torch.equal(mb[torch.from_numpy(con).cuda()],
                                     src[torch.from_numpy(con).cuda()])
    assert torch.equal(mb, again) and torch.equal(mb, down)  # two applies bitwise equal
    if prec == "f64":
        e2 = rel_err(_np(mb), A @ case.src)
        print(f"{key}: matrix-based vmult vs scipy A_host @ src rel l2 {e2:.3e}")
        assert e2 < 1e-12
    assert rel_err(_np(off), _np(free)) < TOL[prec]  # bitwise: the deterministic test below


@pytest.mark.parametrize("key", ["re3900_r0-f64-newton", "re100_r1-f32-picard"])
def test_switching_off_restores_matrix_free_bitwise(key):
    """the matrix-free result after the mode was on and off again is bitwise
    the one before (GLS_DETERMINISTIC: without it two matrix-free vmults of a
    brick operator differ in the order of their atomic sums anyway)"""
    import torch
    case = mc.built(key)["case"]
    prec = key.split("-")[1]
    op = case.gpu(prec)
    op.set_parameters(**dict(case.params, deterministic=True))
    op.set_linearization_point(case.u_star)
    if case.params["order"] > 0:
        op.set_previous_solution(case.hist, case.weights)
    src = op._dev(case.src)
    before = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(True)
    mb = op.vmult(op.initialize_dof_vector(), src).clone()
    op.set_matrix_based(False)
    after = op.vmult(op.initialize_dof_vector(), src).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    assert rel_err(_np(mb), _np(before)) < TOL[prec]


def test_host_vector_layout():
    """host memory and the caller's dof numbering (gls_op_set_vector_layout):
    caller dof i is node-major dof dof_map[i]"""
    key = "re20_r0-f64-newton"
    b = mc.built(key)
    case, A = b["case"], b["A"]
    op = mc.make_op(key)
    perm = np.random.default_rng(3).permutation(case.n_dofs).astype(np.int64)
    op.set_vector_layout("host", perm)
    src = np.ascontiguousarray(case.src[perm])
    free, mb = np.zeros(case.n_dofs), np.zeros(case.n_dofs)
    op.vmult(free, src)
    op.set_matrix_based(True)
    op.vmult(mb, src)
    ref = (A @ case.src)[perm]
    print(f"host layout: vs matrix-free {rel_err(mb, free):.3e}, vs scipy {rel_err(mb, ref):.3e}")
    assert rel_err(free, ref) < 1e-12
    assert rel_err(mb, free) < 1e-12 and rel_err(mb, ref) < 1e-12
    con = _constrained(case)[perm]
    assert np.array_equal(mb[con], src[con])


def test_gmres_matrix_based_and_timer_tally():
    """gls_gmres_solve_prec with an ILU of op.system_matrix() on Turek-2D
    Re100 r1: the matrix-based and the matrix-free operator converge to
    solutions that agree to 10 x the solver's relative tolerance; the tally
    shows the vmults and one assembly per linearization point."""
    import torch
    import glsamd
    key = "re100_r1-f64-newton"
    b0 = mc.built(key)
    case, A = b0["case"], b0["A"]
    op = mc.make_op(key)
    rtol = 1e-8
    b = gi.rnd(41, case.n_dofs)
    b[_constrained(case)] = 0.0
    ilu = glsamd.ILU(A)
    solver = glsamd.LinearSolverGMRES(op, ilu, relative_tolerance=rtol, absolute_tolerance=0.0)
    bd = torch.from_numpy(b).cuda()
    x_free = torch.zeros_like(bd)
    solver.solve(x_free, bd)
    assert solver.last["converged"] == 1
    was = glsamd.timer_enable(True)
    try:
        glsamd.timer_reset()
        op.set_matrix_based(True)
        op.set_linearization_point(case.u_star)
        x_mb = torch.zeros_like(bd)
        solver.solve(x_mb, bd)
        assert solver.last["converged"] == 1
        n_its = solver.last["n_iterations"]
        t = glsamd.timer_sections()
        assert t["ns::vmult"]["calls"] >= n_its
        assert t["ns::initialize_system_matrix"]["calls"] == 1
        solver.solve(torch.zeros_like(bd), bd)  # the same point: no new assembly
        assert glsamd.timer_sections()["ns::initialize_system_matrix"]["calls"] == 1
        op.set_linearization_point(case.u_star)
        solver.solve(torch.zeros_like(bd), bd)
        assert glsamd.timer_sections()["ns::initialize_system_matrix"]["calls"] == 2
    finally:
        glsamd.timer_enable(was)
        glsamd.timer_reset()
    got, ref = x_mb.cpu().numpy(), x_free.cpu().numpy()
    print(f"GMRES + ILU(0): matrix-based vs matrix-free solution rel l2 {rel_err(got, ref):.3e} "
          f"({n_its} iterations)")
    assert np.linalg.norm(b - A @ got) <= 1.01 * rtol * np.linalg.norm(b)
    assert rel_err(got, ref) < 10 * rtol


def test_refusals():
    import glsamd
    key = "re20_r0-f64-newton"
    case = mc.built(key)["case"]
    L = glsamd.lib()
    # a level operator of a multigrid in matrix-based mode
    op = mc.make_op(key)
    mg = glsamd.Multigrid([op], [], coarse_n_iterations=-1, outer_precision="f64")
    op.set_matrix_based(True)
    with pytest.raises(glsamd.GlsError, match="matrix-based"):
        mg.setup()
    op.set_matrix_based(False)
    mg.setup()
    # a partitioned operator
    part = glsamd.NavierStokesOperator(case.mesh, case.cmask, "f64",
                                       n_owned_nodes=case.mesh.n_nodes - 1,
                                       brick=(0, 0, 0))
    assert L.gls_op_set_matrix_based(part.h, 1) != 0
    assert "single-domain" in L.gls_last_error().decode()
    m = glsamd.DeviceCSR()
    import ctypes as C
    assert L.gls_op_system_matrix_device(part.h, C.byref(m), glsamd._stream()) != 0
    assert "single-domain" in L.gls_last_error().decode()
    # matrix-based before a linearization point, then vmult
    fresh = glsamd.NavierStokesOperator(case.mesh, case.cmask, "f64")
    fresh.set_parameters(**case.params)
    fresh.set_matrix_based(True)
    dst, src = fresh.initialize_dof_vector(), fresh._dev(case.src)
    assert L.gls_op_vmult(fresh.h, glsamd._ptr(dst), glsamd._ptr(src), glsamd._stream()) != 0
    assert "set_linearization_point" in L.gls_last_error().decode()
    assert L.gls_op_system_matrix_device(fresh.h, C.byref(m), glsamd._stream()) != 0
    assert "set_linearization_point" in L.gls_last_error().decode()
    assert L.gls_op_invalidate_system(None) != 0
