"""The multigrid over levels with node constraints (slip cylinder on every
level) against slip_ref.SlipOracleGMG, the oracle multigrid with the wrapped
level operators, diagonals and transfers (TEST INFRASTRUCTURE).

Tolerances are the project's (tests/test_gpu_mg.py, test_a_gpu_configs.py):
transfers and one V-cycle 1e-9 with FP64 levels and 5e-4 with FP32 levels
(the FP32 cycle on the GPU's own FP32 inverse diagonals, as there), the
power iteration's eigenvalue estimate to 1e-3 relative."""
import numpy as np
import pytest

import glsinputs as gi
import slip_ref
from helpers import rel_err

pytestmark = pytest.mark.gpu

RE100_2D, RE3900 = "input_turek_2D_Re100.json", "input_hoffmann_3D_Re3900.json"
# 2D Q2 r0..r2 and 3D Q2 r0..r1
HIERARCHIES = {"2d_q2_r0_r2": (RE100_2D, 3, dict(fe_degree=2)), "3d_q2_r0_r1": (RE3900, 2, {})}
_cache = {}


def _np(t):
    return t.double().cpu().numpy()


def hierarchy(key):
    """The hierarchy, its inputs and the reference multigrid, built once."""
    if key not in _cache:
        name, n_levels, over = HIERARCHIES[key]
        d, meshes, cm, rows, ncs, params, w = slip_ref.slip_hierarchy(name, n_levels, **over)
        assert all(len(r.nodes) > 0 for r in rows)
        u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
        hist = gi.history(u, params["order"])
        ref = slip_ref.SlipOracleGMG(meshes, cm, rows, params, u, hist, w, coarse_iters=10)
        _cache[key] = dict(meshes=meshes, cm=cm, rows=rows, ncs=ncs, params=params, w=w, u=u,
                           hist=hist, ref=ref, lam=[ref.estimate(l) for l in range(n_levels)],
                           invdiag=[x.copy() for x in ref.invdiag])
    return _cache[key]


def build(h, prec, **kw):
    import glsamd
    return glsamd.build_gmg(h["meshes"], h["cm"], h["params"], h["u"], h["hist"], h["w"],
                            precision=prec, node_constraints=h["ncs"], coarse_n_iterations=10,
                            outer_precision="f64", **kw)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("key", list(HIERARCHIES))
def test_transfers_relaxation_vcycle(key, prec):
    import torch
    h = hierarchy(key)
    ref, meshes, rows = h["ref"], h["meshes"], h["rows"]
    tol = 1e-9 if prec == "f64" else 5e-4
    mg, ops = build(h, prec)
    L = len(meshes) - 1
    # transfers
    for l in range(1, L + 1):
        xc = gi.rnd(20 + l, meshes[l - 1].n_dofs)
        dst = ops[l].initialize_dof_vector()
        src = ops[l - 1]._dev(xc)
        keep = src.clone()
        mg.prolongate_add(l, dst, src)
        want = np.zeros(meshes[l].n_dofs)
        ref.prolongate_add(l, want, xc)
        rf = gi.rnd(30 + l, meshes[l].n_dofs)
        rc = ops[l - 1].initialize_dof_vector()
        mg.restrict_add(l, rc, ops[l]._dev(rf))
        wantc = np.zeros(meshes[l - 1].n_dofs)
        ref.restrict_add(l, wantc, rf)
        torch.cuda.synchronize()
        assert torch.equal(src, keep)  # the coarse source is restored
        ep, er = rel_err(_np(dst), want), rel_err(_np(rc), wantc)
        print(key, prec, "level", l, "prolongate", ep, "restrict", er)
        assert ep < (1e-12 if prec == "f64" else 2e-5)
        assert er < (1e-12 if prec == "f64" else 2e-5)
        assert np.all(_np(dst)[rows[l].elim] == 0.0)   # zero weights on eliminated fine dofs
        assert np.all(_np(rc)[rows[l - 1].elim] == 0.0)
    # relaxation factors
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
    # one V-cycle with coarse sweeps
    b = gi.rnd(11, meshes[L].n_dofs)
    b[rows[L].elim] = 0.0
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
    # no resident sweep ran on a level with rows
    for l in range(L + 1):
        assert ops[l].sweep_stats()[0] == 0


def test_setup_rereads_the_rows():
    """rows set after the multigrid was created are picked up by setup():
    the transfer weights of the eliminated fine components become zero"""
    import glsamd
    import torch
    h = hierarchy("2d_q2_r0_r2")
    meshes, rows = h["meshes"], h["rows"]
    mg, ops = glsamd.build_gmg(meshes, h["cm"], h["params"], h["u"], h["hist"], h["w"],
                               precision="f64", coarse_n_iterations=10, outer_precision="f64")
    xc = ops[0]._dev(gi.rnd(21, meshes[0].n_dofs))
    before = ops[1].initialize_dof_vector()
    mg.prolongate_add(1, before, xc)
    for op, nc in zip(ops, h["ncs"]):
        op.set_node_constraints(*nc)
    mg.setup()
    after = ops[1].initialize_dof_vector()
    mg.prolongate_add(1, after, xc)
    torch.cuda.synchronize()
    assert np.any(_np(before)[rows[1].elim] != 0.0)
    assert np.all(_np(after)[rows[1].elim] == 0.0)
    want = np.zeros(meshes[1].n_dofs)
    h["ref"].prolongate_add(1, want, _np(xc))
    assert rel_err(_np(after), want) < 1e-12


def test_gmres_gmg_3d_r1():
    """GMRES with the FP32 GMG on the 3D r1 slip-cylinder Newton system to
    reltol 1e-8, against slip_ref's right-preconditioned GMRES(28) on
    slip_ref's operator with the same preconditioner (the GPU's V-cycle)."""
    import torch
    import glsamd
    h = hierarchy("3d_q2_r0_r1")
    meshes, rows, ref = h["meshes"], h["rows"], h["ref"]
    L = len(meshes) - 1
    mg, ops = build(h, "f32")
    A = glsamd.NavierStokesOperator(meshes[L], h["cm"][L], "f64", node_constraints=h["ncs"][L])
    A.set_parameters(**h["params"])
    A.set_linearization_point(h["u"])
    A.set_previous_solution(h["hist"], h["w"])
    n = meshes[L].n_dofs
    b = gi.rnd(41, n)
    con = ((np.asarray(h["cm"][L])[:, None] >> np.arange(4)[None, :]) & 1).astype(bool).ravel()
    b[con] = 0.0
    b[rows[L].elim] = 0.0
    solver = glsamd.LinearSolverGMRES(A, mg, relative_tolerance=1e-8, absolute_tolerance=0.0)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    solver.solve(x, torch.from_numpy(b).cuda())
    got = x.cpu().numpy()
    assert solver.last["converged"] == 1

    def M(v):
        # FP64 vectors of the operator's size only: the V-cycle reads and
        # writes n doubles whatever it is handed
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        assert v.size == n
        src = torch.from_numpy(v).cuda()
        dst = torch.zeros(n, dtype=torch.float64, device="cuda")
        mg.vcycle(dst, src)
        return dst.cpu().numpy()

    op_ref = ref.ops[L]
    want, its = slip_ref.gmres_right(op_ref.vmult, M, b, 1e-8)
    count = [its]
    print("GMRES + GMG, slip cylinder 3D r1:", solver.last["n_iterations"], "iterations,",
          "restatement", count[0], "solution rel err", rel_err(got, want))
    assert np.linalg.norm(b - op_ref.vmult(got)) <= 1.01e-8 * np.linalg.norm(b)
    assert abs(solver.last["n_iterations"] - count[0]) <= 1
    assert rel_err(got, want) < 1e-6
    assert np.all(got[rows[L].elim] == 0.0)


def test_direct_coarse_solvers_refuse_rows():
    import glsamd
    h3 = hierarchy("3d_q2_r0_r1")
    op = glsamd.NavierStokesOperator(h3["meshes"][0], h3["cm"][0], "f32",
                                     node_constraints=h3["ncs"][0])
    op.set_parameters(**h3["params"])
    op.set_linearization_point(gi.linearization_point(h3["meshes"][0].n_nodes, 3, 1.0))
    op.set_previous_solution(gi.history(gi.linearization_point(h3["meshes"][0].n_nodes, 3, 1.0),
                                        h3["params"]["order"]), h3["w"])
    mg = glsamd.Multigrid([op], [], outer_precision="f64", coarse_n_iterations=-1)
    with pytest.raises(glsamd.GlsError, match="dense Schur-complement direct coarse solver"):
        mg.setup()
    mg = glsamd.Multigrid([op], [], outer_precision="f64", coarse_n_iterations=-1,
                          coarse_direct="nd")
    with pytest.raises(glsamd.GlsError, match="nested-dissection .* direct coarse solver"):
        mg.setup()
    # coarse sweeps on the same operator are fine
    glsamd.Multigrid([op], [], outer_precision="f64", coarse_n_iterations=10).setup()
