"""The multigrid over levels with a periodic node map against
periodic_ref.PeriodicOracleGMG, the oracle multigrid with the wrapped level
operators, diagonals and transfers (TEST INFRASTRUCTURE).

Tolerances are the project's (tests/test_gpu_mg.py, test_gpu_slip_mg.py):
transfers 1e-12 / 2e-5, one V-cycle 1e-9 with FP64 levels and 5e-4 with FP32
levels (the FP32 cycle on the GPU's own FP32 inverse diagonals, as there), the
power iteration's eigenvalue estimate to 1e-3 relative."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import glsinputs as gi
import periodic_ref as pr
from helpers import rel_err

pytestmark = pytest.mark.gpu

RE100_2D, RE3900 = "input_turek_2D_Re100.json", "input_hoffmann_3D_Re3900.json"
# 2D Q2 r0..r2, y periodic; 3D Q2 r0..r1, y and z periodic (400 / 3,200 cells)
HIERARCHIES = {"2d_q2_r0_r2": (RE100_2D, 3, dict(fe_degree=2)), "3d_q2_r0_r1": (RE3900, 2, {})}
_cache = {}


def _np(t):
    return t.double().cpu().numpy()


def inputs(key):
    """The hierarchy and its inputs (no reference)."""
    name, n_levels, over = HIERARCHIES[key]
    d, meshes, cm, masters, params, w = pr.periodic_hierarchy(name, n_levels, **over)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, params["order"])
    nc = meshes[-1].dim + 1
    slave = np.repeat(masters[-1] != np.arange(meshes[-1].n_nodes), nc)
    return dict(meshes=meshes, cm=cm, masters=masters, params=params, w=w, u=u, hist=hist,
                slave_dofs=slave)


def hierarchy(key):
    """inputs(key) with the reference multigrid (10 coarse sweeps), built once."""
    if key not in _cache:
        h = inputs(key)
        ref = pr.PeriodicOracleGMG(h["meshes"], h["cm"], h["masters"], h["params"], h["u"],
                                   h["hist"], h["w"], coarse_iters=10)
        assert all(len(pm.slaves) > 0 for pm in ref.pms)
        h.update(ref=ref, lam=[ref.estimate(l) for l in range(len(h["meshes"]))],
                 invdiag=[x.copy() for x in ref.invdiag])
        _cache[key] = h
    return _cache[key]


def build(h, prec, coarse_n_iterations=10, **kw):
    import glsamd
    poison = lambda v: np.where(h["slave_dofs"], np.nan, v)  # slave entries are never read
    return glsamd.build_gmg(h["meshes"], h["cm"], dict(h["params"], **kw.pop("params", {})),
                            poison(h["u"]), [poison(x) for x in h["hist"]], h["w"],
                            precision=prec, node_master=h["masters"],
                            coarse_n_iterations=coarse_n_iterations, outer_precision="f64", **kw)


def _rhs(h, seed=11):
    """A right-hand side that is zero on the identity rows of the fine level."""
    m = h["meshes"][-1]
    b = gi.rnd(seed, m.n_dofs)
    b[pr.Map(m.dim, h["masters"][-1], h["cm"][-1]).fixed] = 0.0
    return b


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("key", list(HIERARCHIES))
def test_transfers_relaxation_vcycle(key, prec):
    import torch
    h = hierarchy(key)
    ref, meshes, pms = h["ref"], h["meshes"], h["ref"].pms
    tol = 1e-9 if prec == "f64" else 5e-4
    mg, ops = build(h, prec)
    L = len(meshes) - 1
    for l in range(1, L + 1):
        xc = gi.rnd(20 + l, meshes[l - 1].n_dofs)
        dst = ops[l].initialize_dof_vector()
        mg.prolongate_add(l, dst, ops[l - 1]._dev(np.where(pms[l - 1].is_slave_dof, np.nan, xc)))
        want = np.zeros(meshes[l].n_dofs)
        ref.prolongate_add(l, want, xc)
        rf = gi.rnd(30 + l, meshes[l].n_dofs)
        rc = ops[l - 1].initialize_dof_vector()
        mg.restrict_add(l, rc, ops[l]._dev(np.where(pms[l].is_slave_dof, np.nan, rf)))
        wantc = np.zeros(meshes[l - 1].n_dofs)
        ref.restrict_add(l, wantc, rf)
        torch.cuda.synchronize()
        ep, er = rel_err(_np(dst), want), rel_err(_np(rc), wantc)
        print(key, prec, "level", l, "prolongate", ep, "restrict", er)
        assert ep < (1e-12 if prec == "f64" else 2e-5)
        assert er < (1e-12 if prec == "f64" else 2e-5)
        assert np.all(_np(dst)[pms[l].fixed] == 0.0)   # zero weights on slaves and Dirichlet dofs
        assert np.all(_np(rc)[pms[l - 1].fixed] == 0.0)
    for l in range(L + 1):
        omega, lam = mg.relaxation(l)
        print(key, prec, "level", l, "lambda", lam, "reference", h["lam"][l], "omega", omega)
        assert abs(lam - h["lam"][l]) < 1e-3 * h["lam"][l], (l, lam, h["lam"][l])
        omega_ref = 2.0 / (h["lam"][l] / ref.range + h["lam"][l])
        assert abs(omega - omega_ref) < 1e-3 * omega_ref, (l, omega, omega_ref)
    ref.set_omega([mg.relaxation(l)[0] for l in range(L + 1)])
    for l in range(L + 1):
        if prec == "f32":  # the algorithm on the GPU's own FP32 level diagonals
            dl = ops[l].initialize_dof_vector()
            ops[l].compute_inverse_diagonal(dl)
            ref.invdiag[l] = _np(dl)
        else:
            ref.invdiag[l] = h["invdiag"][l]
    b = _rhs(h)
    src = torch.from_numpy(b).cuda()
    dst = torch.zeros_like(src)
    mg.vcycle(dst, src)
    again = torch.zeros_like(src)
    mg.vcycle(again, src)
    torch.cuda.synchronize()
    err = rel_err(_np(dst), ref.vcycle(b))
    print(key, prec, "V-cycle rel err", err)
    assert err < tol
    assert rel_err(_np(again), _np(dst)) < tol
    stats = [op.sweep_stats() for op in ops]
    print(key, prec, "resident launches / spin-bound waits per level:", stats)
    assert all(s[1] == 0 for s in stats)
    if prec == "f32" and meshes[0].dim == 3:
        # the small periodic levels keep the resident sweeps
        assert stats[0][0] > 0 and stats[1][0] > 0, stats


def test_dense_direct_coarse_solve_3d():
    """The Re3900 deck's coarse solver: the dense direct solve assembles over
    the algebraic connectivity, slaves constrained."""
    import torch
    h = hierarchy("3d_q2_r0_r1")
    ref, meshes = h["ref"], h["meshes"]
    mg, ops = build(h, "f32", coarse_n_iterations=-1)
    L = len(meshes) - 1
    ref.set_omega([mg.relaxation(l)[0] for l in range(L + 1)])
    for l in range(L + 1):
        dl = ops[l].initialize_dof_vector()
        ops[l].compute_inverse_diagonal(dl)
        ref.invdiag[l] = _np(dl)
    b = _rhs(h)
    src = torch.from_numpy(b).cuda()
    dst = torch.zeros_like(src)
    mg.vcycle(dst, src)
    torch.cuda.synchronize()
    ref.coarse_iters = -1  # the reference's direct coarse solve
    try:
        want = ref.vcycle(b)
    finally:
        ref.coarse_iters = 10
    err = rel_err(_np(dst), want)
    print("V-cycle with the dense direct coarse solve, rel err", err)
    assert err < 5e-4


def test_nd_coarse_solver_refuses_by_name():
    import glsamd
    h = hierarchy("3d_q2_r0_r1")
    with pytest.raises(glsamd.GlsError, match=r'"nd" coarse solver does not take .* periodic'):
        build(h, "f32", coarse_n_iterations=-1, coarse_direct="nd")


def test_iso_q1_levels_are_refused():
    h = hierarchy("2d_q2_r0_r2")
    with pytest.raises(NotImplementedError, match="FE_Q_iso_Q1"):
        build(h, "f32", coarse_iso_q1=True)


def test_deterministic_vcycle_equals_per_launch_steps():
    """Resident sweeps on the periodic levels against one launch per step
    (GLS_MG_DEFER=1, a child process): bitwise equal in deterministic mode."""
    import torch
    h = hierarchy("3d_q2_r0_r1")
    mg, ops = build(h, "f32", params=dict(deterministic=True))
    b = _rhs(h, 41)
    x = torch.zeros(len(b), dtype=torch.float64, device="cuda")
    mg.vcycle(x, torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    stats = [op.sweep_stats() for op in ops]
    assert all(s[0] > 0 and s[1] == 0 for s in stats), stats
    code = f"""
import sys, numpy as np, torch
sys.path[:0] = {sys.path!r}
from test_gpu_periodic_mg import inputs, build, _rhs
h = inputs("3d_q2_r0_r1")
mg, ops = build(h, "f32", params=dict(deterministic=True))
b = _rhs(h, 41)
x = torch.zeros(len(b), dtype=torch.float64, device="cuda")
mg.vcycle(x, torch.from_numpy(b).cuda())
torch.cuda.synchronize()
assert all(op.sweep_stats()[0] == 0 for op in ops)
np.save(sys.argv[1], x.cpu().numpy())
"""
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "launches.npy")
        r = subprocess.run([sys.executable, "-c", code, f], env=dict(os.environ, GLS_MG_DEFER="1"),
                           capture_output=True, text=True, timeout=180,
                           cwd=os.path.dirname(__file__))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        per_launch = np.load(f)
    assert np.array_equal(_np(x), per_launch)


def test_gmres_gmg_3d_r1():
    """GMRES with the FP32 GMG on the 3D r1 periodic Newton system to reltol
    1e-8, against periodic_ref's right-preconditioned GMRES(28) on the
    reference operator with the same preconditioner (the GPU's V-cycle); the
    tolerances of tests/test_gpu_slip_mg.py."""
    import torch
    import glsamd
    h = hierarchy("3d_q2_r0_r1")
    meshes, ref = h["meshes"], h["ref"]
    L = len(meshes) - 1
    pm = ref.pms[L]
    mg, ops = build(h, "f32")
    A = glsamd.NavierStokesOperator(meshes[L], h["cm"][L], "f64", node_master=h["masters"][L])
    A.set_parameters(**h["params"])
    A.set_linearization_point(h["u"])
    A.set_previous_solution(h["hist"], h["w"])
    n = meshes[L].n_dofs
    b = _rhs(h, 41)
    solver = glsamd.LinearSolverGMRES(A, mg, relative_tolerance=1e-8, absolute_tolerance=0.0)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    solver.solve(x, torch.from_numpy(b).cuda())
    got = x.cpu().numpy()
    assert solver.last["converged"] == 1

    def M(v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        assert v.size == n
        src = torch.from_numpy(v).cuda()
        dst = torch.zeros(n, dtype=torch.float64, device="cuda")
        mg.vcycle(dst, src)
        return dst.cpu().numpy()

    op_ref = ref.ops[L]
    want, its = pr.gmres_right(op_ref.vmult, M, b, 1e-8)
    print("GMRES + GMG, periodic 3D r1:", solver.last["n_iterations"], "iterations,",
          "restatement", its, "solution rel err", rel_err(got, want))
    assert np.linalg.norm(b - op_ref.vmult(got)) <= 1.01e-8 * np.linalg.norm(b)
    assert abs(solver.last["n_iterations"] - its) <= 1
    assert rel_err(got, want) < 1e-6
    assert np.all(got[pm.fixed] == 0.0)
