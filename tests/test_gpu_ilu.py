"""The ILU(k) preconditioner on the device (csrc/ilu.hip, gls_ilu_*) and its
three uses -- AMG smoother / coarsest solve, coarse solver of the multigrid,
outer preconditioner of GMRES -- against tests/ilu_ref.py, the numpy
restatement (Ifpack itself is not available: the restatement is the pin).

The matrices reach every kernel path: one level (diagonal), n not a multiple
of the group width, a factor that is one chain (tridiagonal: 257 levels of
one row), a wide first level followed by chains (Dirichlet rows), rows
shorter and longer than the group, and forced group widths 1 / 4 / 64."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import glsinputs as gi
import ilu_ref as R
from helpers import deck, deck_case, rel_err

pytestmark = pytest.mark.gpu


# name -> (matrix, fill level, atol, rtol, extra environment)
CASES = {
    "diagonal5": (lambda: sp.diags([[2.0, -3.0, 0.5, 4.0, -1.5]], [0]).tocsr(), 0, 1e-12, 1.0, {}),
    "tridiagonal257": (lambda: R.tridiagonal(257), 0, 1e-12, 1.0, {}),
    "poisson12_k0": (lambda: R.poisson(12), 0, 1e-12, 1.0, {}),
    "poisson12_k1": (lambda: R.poisson(12), 1, 1e-6, 1.0, {}),
    "poisson12_k2": (lambda: R.poisson(12), 2, 1e-6, 1.0, {}),
    "poisson33_k0": (lambda: R.poisson(33), 0, 1e-12, 1.0, {}),
    "poisson33_k1": (lambda: R.poisson(33), 1, 1e-6, 1.0, {}),
    "poisson33_k2": (lambda: R.poisson(33), 2, 1e-6, 1.0, {}),
    "block3_k1": (R.block3, 1, 1e-6, 1.0, {}),
    "block4_3d_k1": (lambda: R.stencil_block((5, 5, 5), 4), 1, 1e-6, 1.0, {}),
    "dirichlet_k1": (lambda: R.with_dirichlet(R.poisson(12)), 1, 1e-12, 1.0,
                     {"GLS_ILU_NARROW": "16"}),
    # rows longer than the group (several passes), shorter than it, one lane
    "block3_k1_group4": (R.block3, 1, 1e-6, 1.0, {"GLS_ILU_GROUP": "4"}),
    "poisson12_k1_group64": (lambda: R.poisson(12), 1, 1e-6, 1.0, {"GLS_ILU_GROUP": "64"}),
    "poisson12_k0_group1": (lambda: R.poisson(12), 0, 1e-12, 1.0, {"GLS_ILU_GROUP": "1"}),
    # every level wide
    "block3_k0_narrow1": (R.block3, 0, 1e-12, 1.0, {"GLS_ILU_NARROW": "1"}),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(A, b, the restatement's U^-1 L^-1 b), computed once"""
    make, k, atol, rtol, _ = CASES[name]
    A = make()
    b = gi.rnd(21, A.shape[0])
    ref = R.ILURef(A, k, atol, rtol).vmult(b)
    ref.setflags(write=False)
    return A, b, ref


def _apply(ilu, b):
    import torch
    src = torch.from_numpy(b).cuda()
    dst = torch.full_like(src, float("nan"))
    ilu.vmult(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(b))  # src untouched
    return dst.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_vmult_equals_restatement(name, monkeypatch):
    import glsamd
    _, k, atol, rtol, env = CASES[name]
    A, b, ref = _case(name)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    out = {}
    for chain in ("1", "0"):
        monkeypatch.setenv("GLS_ILU_CHAIN", chain)  # read when the factor is created
        ilu = glsamd.ILU(A, k, atol, rtol)
        info = ilu.info()
        assert info["chain"] == int(chain) and info["n"] == A.shape[0]
        if chain == "0":
            assert info["launches_l"] == info["levels_l"] and info["launches_u"] == info["levels_u"]
        x1, x2 = _apply(ilu, b), _apply(ilu, b)
        err = rel_err(x1, ref)
        print(f"{name} chain={chain}: n {info['n']}, group {info['group']}, narrow "
              f"{info['narrow']}, levels {info['levels_l']}/{info['levels_u']}, launches "
              f"{info['launches_l']}/{info['launches_u']}, rel err {err:.2e}")
        assert err < 1e-12
        assert np.array_equal(x1, x2)  # two applies of one object: bitwise
        out[chain] = (x1, info)
    assert np.array_equal(out["1"][0], out["0"][0])  # chained == unchained, bitwise
    i1 = out["1"][1]
    if name == "tridiagonal257":
        assert i1["levels_l"] == 257 and i1["launches_l"] == 1 and i1["launches_u"] == 1
    if name == "diagonal5":
        assert i1["levels_l"] == 1 and i1["levels_u"] == 1 and i1["nnz_l"] == 0
    if name == "dirichlet_k1":  # a wide level, then chains
        assert 1 < i1["launches_l"] < i1["levels_l"] and i1["max_level_rows"] > 16
    if name == "block3_k0_narrow1":
        assert i1["launches_l"] > 1
    if "group" in name:
        assert i1["group"] == int(env["GLS_ILU_GROUP"])


def test_factors_equal_host_factor():
    import glsamd
    A, _, _ = _case("block3_k1")
    ilu = glsamd.ILU(A, 1, 1e-6, 1.0)
    L, U = ilu.factors()
    h = glsamd.ilu_host_factor(A, 1, 1e-6, 1.0)
    for got, ref in ((L, h["L"]), (U, h["U"])):
        assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
        assert np.array_equal(got.data, ref.data)
    info = ilu.info()
    assert info["nnz_l"] == L.nnz and info["nnz_u"] == U.nnz and info["nnz_a"] == A.nnz
    assert info["levels_l"] == 102 and info["levels_u"] == 102
    assert info["min_pivot"] == np.min(np.abs(U.diagonal()))


def test_refactor_equals_fresh_create():
    import glsamd
    A, b, _ = _case("poisson33_k1")
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.3 * np.sin(np.arange(A.nnz)))
    ilu = glsamd.ILU(A, 1, 1e-6, 1.0)
    assert ilu.info()["symbolic_ms"] > 0
    _apply(ilu, b)
    ilu.refactor(A2)
    assert ilu.info()["symbolic_ms"] == 0
    fresh = glsamd.ILU(A2, 1, 1e-6, 1.0)
    assert np.array_equal(_apply(ilu, b), _apply(fresh, b))
    for got, ref in zip(ilu.factors(), fresh.factors()):
        assert np.array_equal(got.data, ref.data)
    assert rel_err(_apply(ilu, b), R.ILURef(A2, 1, 1e-6, 1.0).vmult(b)) < 1e-12
    with pytest.raises(glsamd.GlsError):
        ilu.refactor(np.zeros(3))
    plain = glsamd.ILU(A, 1, 0.0, 1.0)  # atol 0: nothing keeps a zero diagonal away from zero
    with pytest.raises(glsamd.GlsError, match="pivot in row 0"):
        plain.refactor(np.zeros(A.nnz))  # an error, no silent repair
    with pytest.raises(glsamd.GlsError, match="refactorisation failed"):
        _apply(plain, b)
    plain.refactor(A)
    assert np.all(np.isfinite(_apply(plain, b)))


def test_vmult_refuses_aliased_vectors():
    import torch
    import glsamd
    A, b, _ = _case("poisson12_k0")
    ilu = glsamd.ILU(A)
    v = torch.from_numpy(b).cuda()
    with pytest.raises(glsamd.GlsError, match="distinct"):
        ilu.vmult(v, v)


# ---- the deck matrix: Turek-2D Re100, r1, FP64 (n = 1230), small pivots
@functools.lru_cache(maxsize=None)
def _deck_matrix(n_ref):
    case = deck_case("input_turek_2D_Re100.json", n_ref)
    op = case.gpu("f64")
    A = op.system_matrix()
    A.sort_indices()
    return case, op, A


def _deck_tolerance(A, k, atol, b):
    """the restatement in float64 and in np.longdouble: 100 x their
    difference, at most 1e-8"""
    x64 = R.solve(*R.factor(A, k, atol, 1.0), b)
    xl = R.solve(*R.factor(A, k, atol, 1.0, np.longdouble), b)
    floor = float(np.linalg.norm((xl - x64).astype(np.float64)) / np.linalg.norm(x64))
    return x64, floor, min(100.0 * floor, 1e-8)


@pytest.mark.parametrize("k,atol", [(0, 1e-12), (1, 1e-6)])
def test_deck_matrix_vmult(k, atol):
    """Deck ILU(0) / atol 1e-12 and the AMG's ILU(1) / atol 1e-6 on the Re100
    r1 system matrix (min |u_ii| about 1.4e-4).  The tolerance is 100 x the
    float64 - longdouble difference of the restatement, capped at 1e-8.
    Measured floors: 4.05e-16 (ILU(0)) and 1.31e-15 (ILU(1)), so the bounds
    are 4.05e-14 and 1.31e-13; the device solve differed from the restatement
    by 2.2e-16 and 2.5e-16."""
    import glsamd
    _, _, A = _deck_matrix(1)
    assert A.shape[0] == 1230
    b = gi.rnd(22, A.shape[0])
    ref, floor, tol = _deck_tolerance(A, k, atol, b)
    ilu = glsamd.ILU(A, k, atol, 1.0)
    info = ilu.info()
    err = rel_err(_apply(ilu, b), ref)
    print(f"ILU({k}) atol {atol}: floor {floor:.2e}, tol {tol:.2e}, err {err:.2e}, min pivot "
          f"{info['min_pivot']:.2e}, levels {info['levels_l']}/{info['levels_u']}, launches "
          f"{info['launches_l']}/{info['launches_u']}, nnz {info['nnz_l'] + info['nnz_u']}")
    assert err < tol


# ---- AMG with ILU smoothing and an ILU coarsest solve
def _amg_pair(A, **prm):
    import glsamd
    ref = R.AMGRefILU(A, ilu_fill=1, ilu_atol=1e-6, ilu_rtol=1.0, **prm)
    amg = glsamd.AMG(A, smoother_type="ILU", coarse_type="ILU", ilu_fill=1, ilu_atol=1e-6,
                     ilu_rtol=1.0, **prm)
    assert amg.info()["sizes"] == ref.info()["sizes"]
    assert ref.info()["levels"] >= 2
    return amg, ref


def test_amg_ilu_poisson():
    A = R.poisson(40)
    amg, ref = _amg_pair(A, block_size=1, threshold=0.0, coarse_max_size=100)
    b = gi.rnd(5, A.shape[0])
    err = rel_err(_apply(amg, b), ref.vmult(b))
    print(f"AMG-ILU Poisson 40: sizes {ref.info()['sizes']}, rel err {err:.2e}")
    assert err < 1e-10


def test_amg_ilu_mixed_forms_poisson():
    """ILU smoother with the dense coarsest solve, and Chebyshev smoothing
    with an ILU coarsest solve"""
    import glsamd
    A = R.poisson(40)
    b = gi.rnd(5, A.shape[0])
    prm = dict(block_size=1, threshold=0.0, coarse_max_size=100)
    for st, ct in (("ILU", "direct"), ("Chebyshev", "ILU")):
        ref = R.AMGRefILU(A, smoother_ilu=st == "ILU", coarse_ilu=ct == "ILU", **prm)
        amg = glsamd.AMG(A, smoother_type=st, coarse_type=ct, **prm)
        assert rel_err(_apply(amg, b), ref.vmult(b)) < 1e-10, (st, ct)


def test_amg_ilu_deck_matrix():
    """The deck's non-default AMG parameters with ILU(1) / atol 1e-6 on the
    Re100 r1 matrix (coarse_max_size 100 forces levels): the hierarchy equals
    the restatement's, one V-cycle within the deck tolerance of
    test_deck_matrix_vmult for ILU(1) on this right-hand side (measured floor
    7.9e-16, bound 7.9e-14, V-cycle difference 2.0e-15)."""
    d = deck("input_turek_2D_Re100.json")
    _, _, A = _deck_matrix(1)
    prm = dict(d.amg_parameters(), coarse_max_size=100)
    if d.amg_ilu_parameters() is None:  # the Re100 deck keeps ML's defaults
        prm.update(block_size=3, threshold=1e-14, elliptic=False)
    amg, ref = _amg_pair(A, **prm)
    b = gi.rnd(23, A.shape[0])
    _, floor, tol = _deck_tolerance(A, 1, 1e-6, b)
    err = rel_err(_apply(amg, b), ref.vmult(b))
    print(f"AMG-ILU deck: sizes {ref.info()['sizes']}, floor {floor:.2e}, tol {tol:.2e}, "
          f"err {err:.2e}")
    assert err < tol


# ---- the multigrid with the ILU coarse solver: Turek-2D Re100, r0 .. r1, FP32
@functools.lru_cache(maxsize=None)
def _mg_inputs():
    d = deck("input_turek_2D_Re100.json")
    meshes = [d.mesh(r) for r in range(2)]
    vel, p, slip = d.boundary_descriptor()
    cm = [m.constraint_mask(vel, p, slip) for m in meshes]
    params, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, params["order"])
    return d, meshes, cm, params, w, u, hist, gi.rnd(11, meshes[-1].n_dofs)


def _deck_ilu(d):
    d.raw["gmg coarse grid solver"] = "ILU"
    return d.coarse_ilu_parameters()


def _vcycle(mg, b):
    import torch
    src = torch.from_numpy(b).cuda()
    dst = torch.zeros_like(src)
    mg.vcycle(dst, src)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def test_mg_coarse_ilu_iterated():
    """coarse GMRES preconditioned by the ILU at reltol 1e-6: the V-cycle of
    the oracle multigrid with an exact coarse solve, within the 5e-4 of
    test_gpu_vcycle_coarse_gmres_amg"""
    import glsamd
    from mg_ref import OracleGMG
    d, meshes, cm, params, w, u, hist, b = _mg_inputs()
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                               coarse_iterate=True, coarse_reltol=1e-6, coarse_maxiter=2000,
                               coarse_n_iterations=0, coarse_ilu=_deck_ilu(d))
    got = _vcycle(mg, b)
    it, conv = mg.coarse_statistics()
    assert conv and it > 0
    info, setup_ms = mg.coarse_ilu()
    assert info["n"] == meshes[0].n_dofs and setup_ms > 0 and info["symbolic_ms"] > 0
    ref = OracleGMG(meshes, cm, params, u, hist, w, coarse_iters=-1)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    err = rel_err(got, ref.vcycle(b))
    print(f"coarse GMRES + ILU(0): {it} iterations, V-cycle vs exact coarse solve {err:.2e}")
    assert err < 5e-4


def test_mg_coarse_ilu_once_and_refactor():
    """coarse_iterate off: the factor applied once to the restricted defect
    (the oracle multigrid with the restatement as its coarse solver).  A
    second setup at a new linearisation point refactors (no symbolic phase)
    and equals a fresh build."""
    import torch
    import glsamd
    from mg_ref import OracleGMG
    d, meshes, cm, params, w, u, hist, b = _mg_inputs()
    oracle_params = params
    params = dict(params, deterministic=True)  # the two builds are compared below
    kw = dict(precision="f32", coarse_iterate=False, coarse_n_iterations=0,
              coarse_ilu=_deck_ilu(d))
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w, **kw)
    got = _vcycle(mg, b)
    ref = OracleGMG(meshes, cm, oracle_params, u, hist, w, coarse_iters=0)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    A0 = ops[0].system_matrix()
    ilu0 = R.ILURef(A0, 0, 1e-12, 1.0)
    ref.coarse_precondition = ilu0.vmult
    err = rel_err(got, ref.vcycle(b))
    print(f"ILU(0) once as the coarse solver: V-cycle vs restatement {err:.2e}")
    assert err < 5e-4
    # a new linearisation point on every level, then setup again
    u2 = 0.7 * u + 0.05 * np.cos(np.arange(u.shape[0]))
    mg2, ops2 = glsamd.build_gmg(meshes, cm, params, u2, hist, w, **kw)
    vecs = [ops[-1]._dev(u2)]
    for l in range(len(ops) - 1, 0, -1):
        v = ops[l - 1].initialize_dof_vector()
        mg.interpolate(l, v, vecs[0])
        vecs.insert(0, v)
    for op, v in zip(ops, vecs):
        op.set_linearization_point(v)
    torch.cuda.synchronize()
    mg.setup()
    info, _ = mg.coarse_ilu()
    assert info["symbolic_ms"] == 0 and info["numeric_ms"] > 0  # refactored, not recreated
    assert mg2.coarse_ilu()[0]["symbolic_ms"] > 0
    assert abs(ops[0].system_matrix() - A0).max() > 0
    # FP32 levels: equal up to the round-off of the level arithmetic
    assert rel_err(_vcycle(mg, b), _vcycle(mg2, b)) < 1e-6


def test_mg_coarse_ilu_refusals():
    import glsamd
    d, meshes, cm, params, w, u, hist, b = _mg_inputs()
    mg, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                             coarse_n_iterations=2)
    prm = glsamd.ilu_params()
    import ctypes as C
    assert glsamd.lib().gls_mg_set_coarse_ilu(mg.h, C.byref(prm)) != 0  # after setup
    assert b"before gls_mg_setup" in glsamd.lib().gls_last_error()
    with pytest.raises(glsamd.GlsError, match="AMG"):
        glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                         coarse_iterate=True, coarse_amg=d.amg_parameters(),
                         coarse_ilu=dict(fill_level=0))
    with pytest.raises(glsamd.GlsError, match="not the AMG"):
        glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                         coarse_amg_ilu=dict(fill_level=1))


def test_mg_coarse_amg_ilu():
    """the coarse AMG in its ILU form inside the multigrid: the coarse GMRES
    converges and the V-cycle is the exact-coarse-solve one"""
    import glsamd
    from mg_ref import OracleGMG
    d, meshes, cm, params, w, u, hist, b = _mg_inputs()
    amg = dict(block_size=3, threshold=1e-14, smoother_sweeps=2, coarse_max_size=100,
               elliptic=False, max_levels=10)
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                               coarse_iterate=True, coarse_reltol=1e-6, coarse_maxiter=2000,
                               coarse_amg=amg,
                               coarse_amg_ilu=dict(smoother_ilu=True, coarse_ilu=True,
                                                   fill_level=1, atol=1e-6, rtol=1.0))
    got = _vcycle(mg, b)
    it, conv = mg.coarse_statistics()
    info, _ = mg.coarse_amg()
    print(f"coarse GMRES + AMG(ILU): {it} iterations, hierarchy {info['sizes']}")
    assert conv and it > 0 and info["levels"] >= 2
    ref = OracleGMG(meshes, cm, params, u, hist, w, coarse_iters=-1)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    assert rel_err(got, ref.vcycle(b)) < 5e-4


# ---- outer GMRES: Re100 r0, FP64 (n = 351)
def _gmres_counting(A, b, M, rtol=1e-8):
    """right-preconditioned restarted GMRES(28) as gls_gmres_solve runs it
    (solver_l.cc:45-74): x, iterations"""
    n = A.shape[0]
    count = [0]

    def cb(_):
        count[0] += 1
    AM = spla.LinearOperator((n, n), matvec=lambda v: A @ M(v))
    y, info = spla.gmres(AM, b, restart=28, rtol=rtol, atol=0.0, maxiter=50, callback=cb,
                         callback_type="pr_norm")
    assert info == 0
    return M(y), count[0]


def test_gmres_ilu_preconditioner():
    import torch
    import glsamd
    case, op, A = _deck_matrix(0)
    assert A.shape[0] == 351
    b = gi.rnd(31, A.shape[0])
    b[np.asarray(A.diagonal() == 1.0) & (np.diff(A.indptr) == 1)] = 0.0  # constrained rows
    ilu = glsamd.ILU(A)  # the deck's "preconditioner": "ILU": ILU(0), atol 1e-12, rtol 1
    solver = glsamd.LinearSolverGMRES(op, ilu, relative_tolerance=1e-8, absolute_tolerance=0.0)
    x = torch.zeros(A.shape[0], dtype=torch.float64, device="cuda")
    solver.solve(x, torch.from_numpy(b).cuda())
    got = x.cpu().numpy()
    assert solver.last["converged"] == 1
    assert np.linalg.norm(b - A @ got) <= 1.01e-8 * np.linalg.norm(b)
    ref, its = _gmres_counting(A, b, R.ILURef(A, 0, 1e-12, 1.0).vmult)
    print(f"GMRES + ILU(0): {solver.last['n_iterations']} iterations (restatement {its}), "
          f"solution vs restatement {rel_err(got, ref):.2e}")
    assert rel_err(got, ref) < 1e-6
    assert abs(solver.last["n_iterations"] - its) <= 2


def test_gmres_amg_preconditioner_and_class():
    """GLS_PREC_AMG, and the glssolvers class that assembles and (re)factors"""
    import torch
    import glsamd
    import glssolvers
    case, op, A = _deck_matrix(0)
    b = gi.rnd(32, A.shape[0])
    for kind, prm in (("ILU", {}), ("AMG", dict(block_size=3, threshold=1e-14, elliptic=False,
                                                 coarse_max_size=100))):
        prec = glssolvers.MatrixPreconditioner(op, kind, **prm)
        prec.initialize()
        prec.initialize()  # ILU: a refactorisation on the same pattern
        if kind == "ILU":
            assert prec.preconditioner.info()["symbolic_ms"] == 0
        solver = glsamd.LinearSolverGMRES(op, prec, relative_tolerance=1e-8,
                                          absolute_tolerance=0.0)
        x = torch.zeros(A.shape[0], dtype=torch.float64, device="cuda")
        solver.solve(x, torch.from_numpy(b).cuda())
        got = x.cpu().numpy()
        print(f"GMRES + {kind}: {solver.last['n_iterations']} iterations")
        assert np.linalg.norm(b - A @ got) <= 1.01e-8 * np.linalg.norm(b)


def test_gmres_prec_mg_is_gmres_solve():
    """gls_gmres_solve_prec with GLS_PREC_MG gives bitwise the result of
    gls_gmres_solve, with a multigrid and with none"""
    import ctypes as C
    import torch
    import glsamd
    d, meshes, cm, params, w, u, hist, _ = _mg_inputs()
    params = dict(params, deterministic=True)  # repeated solves bitwise equal
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                               coarse_n_iterations=-1)
    op = glsamd.NavierStokesOperator(meshes[-1], cm[-1], "f64")
    op.set_parameters(**params)
    op.set_linearization_point(u)
    op.set_previous_solution(hist, w)
    b = torch.from_numpy(gi.rnd(33, op.n_dofs)).cuda()
    desc = glsamd.GMRESDesc(30, 200, 0.0, 1e-8)
    L = glsamd.lib()
    for prec in (mg.h, None):
        xs = []
        for new in (False, True):
            x = torch.zeros_like(b)
            res = glsamd.GMRESResult()
            if new:
                rc = L.gls_gmres_solve_prec(op.h, glsamd.GLS_PREC_MG, prec, C.byref(desc),
                                            glsamd._ptr(x), glsamd._ptr(b), C.byref(res),
                                            glsamd._stream())
            else:
                rc = L.gls_gmres_solve(op.h, prec, C.byref(desc), glsamd._ptr(x), glsamd._ptr(b),
                                       C.byref(res), glsamd._stream())
            # the multigrid converges; without a preconditioner the 200
            # iterations run out, with the same iterate from both entry points
            assert (rc == 0) == (prec is not None), L.gls_last_error()
            xs.append((x.cpu().numpy(), res.n_iterations, res.final_residual))
        assert xs[0][1:] == xs[1][1:] and np.array_equal(xs[0][0], xs[1][0])
        assert np.all(np.isfinite(xs[0][0])) and np.any(xs[0][0] != 0)
    x = torch.zeros_like(b)
    assert L.gls_gmres_solve_prec(op.h, 7, None, C.byref(desc), glsamd._ptr(x), glsamd._ptr(b),
                                  None, glsamd._stream()) != 0
    assert L.gls_gmres_solve_prec(op.h, glsamd.GLS_PREC_ILU, None, C.byref(desc), glsamd._ptr(x),
                                  glsamd._ptr(b), None, glsamd._stream()) != 0
