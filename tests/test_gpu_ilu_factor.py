"""The numeric ILU(k) factorisation on the device (csrc/ilu_factor.hip:
gls_ilu_refactor_device, gls_ilu_create_device) against the host
factorisation, which it must equal bit for bit, and its three users: the
operator path (ILU.from_operator), the multigrid's coarse ILU and the GMRES
preconditioner class.

The matrices are those of tests/test_gpu_ilu.py plus a nonsymmetric one.  They
reach rows without L entries (diagonal5), one chain of 257 one-row levels,
fill positions A does not have (k >= 1), rows longer than a wave (block4_3d:
108 entries of A, 252 of the ILU(1) pattern), wide and
chained levels in one factor (dirichlet_k1 with a narrow threshold of 16, and
block3_k0 with a threshold of 1), every level with more than one
row wide (GLS_ILU_FACTOR_NARROW=1) and groups narrower and wider than the
rows (GLS_ILU_GROUP 4 on block3, 64 on poisson12)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

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
                     {"GLS_ILU_FACTOR_NARROW": "16"}),
    "nonsymmetric_k1": (R.nonsymmetric, 1, 1e-6, 1.1, {}),
    # every level with more than one row is a grid launch
    "block3_k0_narrow1": (R.block3, 0, 1e-12, 1.0, {"GLS_ILU_FACTOR_NARROW": "1"}),
    # the group narrower than the rows (several passes) and wider than them
    "block3_k1_group4": (R.block3, 1, 1e-6, 1.0, {"GLS_ILU_GROUP": "4"}),
    "poisson12_k1_group64": (lambda: R.poisson(12), 1, 1e-6, 1.0, {"GLS_ILU_GROUP": "64"}),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(A, A2 with new values on the pattern, b, the restatement's apply of
    A2's factor to b), computed once"""
    make, k, atol, rtol, _ = CASES[name]
    A = make().tocsr()
    A.sort_indices()
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.3 * np.sin(np.arange(A.nnz)))
    b = gi.rnd(21, A.shape[0])
    ref = R.ILURef(A2, k, atol, rtol).vmult(b)
    ref.setflags(write=False)
    return A, A2, b, ref


def _apply(ilu, b):
    import torch
    src = torch.from_numpy(b).cuda()
    dst = torch.full_like(src, float("nan"))
    ilu.vmult(dst, src)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_factors(got, ref):
    for g, r in zip(got, ref):
        assert np.array_equal(g.indptr, r.indptr) and np.array_equal(g.indices, r.indices)
        assert np.array_equal(_bits(g.data), _bits(r.data))


def _clean(monkeypatch):
    for v in ("GLS_ILU_FACTOR_CHAIN", "GLS_ILU_FACTOR_NARROW", "GLS_ILU_GROUP", "GLS_ILU_CHAIN",
              "GLS_ILU_NARROW"):
        monkeypatch.delenv(v, raising=False)


# ---- 1. bitwise factor, 2. repeatability
@pytest.mark.parametrize("name", list(CASES))
def test_device_factor_is_bitwise_the_host_factor(name, monkeypatch):
    import torch
    import glsamd
    _, k, atol, rtol, env = CASES[name]
    A, A2, b, ref = _case(name)
    _clean(monkeypatch)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    fresh = glsamd.ILU(A2, k, atol, rtol)  # the host factorisation of the new values
    want, x_want, host_info = fresh.factors(), _apply(fresh, b), fresh.info()
    d_vals = torch.from_numpy(A2.data).cuda()
    infos = {}
    for chain in ("1", "0"):
        monkeypatch.setenv("GLS_ILU_FACTOR_CHAIN", chain)  # read when the factor is created
        ilu = glsamd.ILU(A, k, atol, rtol)
        assert ilu.factor_info()["device"] == 0
        ilu.refactor_device(d_vals)
        fi, info = ilu.factor_info(), ilu.info()
        infos[chain] = fi
        print(f"{name} chain={chain}: n {info['n']}, group {fi['group']}, rows {fi['rows']}, "
              f"narrow {fi['narrow']}, levels {fi['levels']}, launches {fi['launches']} "
              f"({fi['chains']} chains), longest row {fi['max_row']}, device "
              f"{info['numeric_ms']:.3f} ms (rows {fi['factor_ms']:.3f} ms)")
        assert fi["device"] == 1 and fi["chain"] == int(chain)
        if chain == "0":
            assert fi["launches"] == fi["levels"] and fi["chains"] == 0
        got = ilu.factors()
        _same_factors(got, want)
        x = _apply(ilu, b)
        assert np.array_equal(_bits(x), _bits(x_want))
        assert rel_err(x, ref) < 1e-12
        assert info["min_pivot"] == host_info["min_pivot"]
        assert info["symbolic_ms"] == 0 and info["upload_ms"] == 0 and info["numeric_ms"] > 0
        # the same values again: bitwise the same factor
        ilu.refactor_device(d_vals)
        _same_factors(ilu.factors(), got)
        # and back on the host path
        ilu.refactor(A)
        assert ilu.factor_info()["device"] == 0
        h = glsamd.ilu_host_factor(A, k, atol, rtol)
        _same_factors(ilu.factors(), (h["L"], h["U"]))
    i1 = infos["1"]
    if name == "diagonal5":
        assert i1["levels"] == 1 and i1["max_row"] == 1
    if name == "tridiagonal257":
        assert i1["levels"] == 257 and i1["launches"] == 1 and i1["chains"] == 1
    if name == "block4_3d_k1":
        assert i1["max_row"] >= 108 and i1["group"] == 64
    if name == "dirichlet_k1":  # wide and chained levels in one factor
        assert 0 < i1["chains"] < i1["launches"] < i1["levels"]
    if name == "block3_k0_narrow1":
        assert i1["narrow"] == 1 and i1["launches"] > i1["chains"] > 0
    if name == "block3_k1_group4":
        assert i1["group"] == 4 < i1["max_row"]
    if name == "poisson12_k1_group64":
        assert i1["group"] == 64 > i1["max_row"]


# ---- 3. bad pivots are error statuses of finite kernels
def test_bad_pivot_is_an_error_and_recoverable(monkeypatch):
    import torch
    import glsamd
    _clean(monkeypatch)
    A, A2, b, _ = _case("poisson33_k1")
    plain = glsamd.ILU(A, 1, 0.0, 1.0)  # atol 0: nothing keeps a zero diagonal away from zero
    with pytest.raises(glsamd.GlsError, match="pivot in row 0"):
        plain.refactor_device(torch.zeros(A.nnz, dtype=torch.float64, device="cuda"))
    with pytest.raises(glsamd.GlsError, match="refactorisation failed"):
        _apply(plain, b)
    with pytest.raises(glsamd.GlsError, match="refactorisation failed"):
        plain.factors()
    plain.refactor_device(torch.from_numpy(A2.data).cuda())
    assert np.all(np.isfinite(_apply(plain, b)))
    with pytest.raises(glsamd.GlsError, match="pivot in row 0"):
        plain.refactor_device(torch.zeros(A.nnz, dtype=torch.float64, device="cuda"))
    plain.refactor(A)  # the host path repairs it too
    assert np.all(np.isfinite(_apply(plain, b)))
    # unit diagonal and unit off-diagonals: u_11 = 1 - 1 * 1
    T = R.tridiagonal(257)
    tri = glsamd.ILU(T, 0, 0.0, 1.0)
    with pytest.raises(glsamd.GlsError, match="pivot in row 1"):
        tri.refactor_device(torch.ones(T.nnz, dtype=torch.float64, device="cuda"))
    with pytest.raises(glsamd.GlsError, match="refactorisation failed"):
        _apply(tri, gi.rnd(3, 257))
    tri.refactor_device(torch.from_numpy(np.ascontiguousarray(T.data, dtype=np.float64)).cuda())
    assert np.all(np.isfinite(_apply(tri, gi.rnd(3, 257))))


# ---- 4. wrong arguments
def test_wrong_values_are_refused(monkeypatch):
    import torch
    import glsamd
    _clean(monkeypatch)
    A, A2, b, _ = _case("poisson12_k1")
    ilu = glsamd.ILU(A, 1, 1e-6, 1.0)
    with pytest.raises(glsamd.GlsError):
        ilu.refactor_device(torch.zeros(A.nnz - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(glsamd.GlsError):
        ilu.refactor_device(A2.data)  # a host array
    with pytest.raises(glsamd.GlsError):
        ilu.refactor_device(torch.from_numpy(A2.data))  # a host tensor
    with pytest.raises(glsamd.GlsError):
        ilu.refactor_device(torch.zeros(A.nnz, dtype=torch.float32, device="cuda"))
    assert ilu.factor_info()["device"] == 0 and np.all(np.isfinite(_apply(ilu, b)))


# ---- 5. the operator path: Turek-2D Re100, r1, FP64 (n = 1230)
@functools.lru_cache(maxsize=None)
def _deck_operator():
    case = deck_case("input_turek_2D_Re100.json", 1)
    return case, case.gpu("f64")


def _device_matrix(op):
    rp, ci, va = (t.cpu().numpy() for t in op.system_matrix_device())
    n = rp.shape[0] - 1
    return sp.csr_matrix((va, ci.astype(np.int64), rp), shape=(n, n))


def _deck_tolerance(A, k, atol, b):
    """the rule of test_gpu_ilu.test_deck_matrix_vmult: the restatement in
    float64 and in np.longdouble; 100 x their difference, at most 1e-8"""
    x64 = R.solve(*R.factor(A, k, atol, 1.0), b)
    xl = R.solve(*R.factor(A, k, atol, 1.0, np.longdouble), b)
    floor = float(np.linalg.norm((xl - x64).astype(np.float64)) / np.linalg.norm(x64))
    return x64, floor, min(100.0 * floor, 1e-8)


@pytest.mark.parametrize("k,atol", [(0, 1e-12), (1, 1e-6)])
def test_operator_path(k, atol, monkeypatch):
    import torch
    import glsamd
    _clean(monkeypatch)
    case, op = _deck_operator()
    op.set_linearization_point(case.u_star)
    A = _device_matrix(op)
    assert A.shape[0] == 1230
    ilu = glsamd.ILU.from_operator(op, k, atol)
    fi, info = ilu.factor_info(), ilu.info()
    assert fi["device"] == 1 and info["symbolic_ms"] > 0 and info["upload_ms"] == 0
    host = glsamd.ILU(A, k, atol, 1.0)
    _same_factors(ilu.factors(), host.factors())
    assert info["min_pivot"] == host.info()["min_pivot"]
    b = gi.rnd(22, A.shape[0])
    ref, floor, tol = _deck_tolerance(A, k, atol, b)
    err = rel_err(_apply(ilu, b), ref)
    print(f"ILU({k}) atol {atol} from the operator: floor {floor:.2e}, tol {tol:.2e}, err "
          f"{err:.2e}, min pivot {info['min_pivot']:.2e}, levels {fi['levels']}, launches "
          f"{fi['launches']} ({fi['chains']} chains), longest row {fi['max_row']}, device "
          f"{info['numeric_ms']:.3f} ms (rows {fi['factor_ms']:.3f} ms)")
    assert err < tol
    assert np.array_equal(_bits(_apply(ilu, b)), _bits(_apply(host, b)))
    # a second linearisation point: the refactorisation equals a fresh factor
    u2 = 0.7 * case.u_star + 0.05 * np.cos(np.arange(case.u_star.shape[0]))
    op.set_linearization_point(u2)
    torch.cuda.synchronize()
    ilu.refactor_from_operator(op)
    assert ilu.info()["symbolic_ms"] == 0
    fresh = glsamd.ILU.from_operator(op, k, atol)
    _same_factors(ilu.factors(), fresh.factors())
    A2 = _device_matrix(op)
    assert abs(A2 - A).max() > 0
    _same_factors(ilu.factors(), glsamd.ILU(A2, k, atol, 1.0).factors())
    op.set_linearization_point(case.u_star)


# ---- 6. the multigrid's coarse ILU on the device: Turek-2D Re100, r0 .. r1, FP32
@functools.lru_cache(maxsize=None)
def _mg_inputs():
    d = deck("input_turek_2D_Re100.json")
    meshes = [d.mesh(r) for r in range(2)]
    vel, p, slip = d.boundary_descriptor()
    cm = [m.constraint_mask(vel, p, slip) for m in meshes]
    params, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, params["order"])
    d.raw["gmg coarse grid solver"] = "ILU"
    return d.coarse_ilu_parameters(), meshes, cm, params, w, u, hist, gi.rnd(11, meshes[-1].n_dofs)


def _vcycle(mg, b):
    import torch
    src = torch.from_numpy(b).cuda()
    dst = torch.zeros_like(src)
    mg.vcycle(dst, src)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def test_mg_coarse_ilu_on_the_device(monkeypatch):
    import torch
    import glsamd
    from mg_ref import OracleGMG
    _clean(monkeypatch)
    deck_ilu, meshes, cm, params, w, u, hist, b = _mg_inputs()
    oracle_params = params
    params = dict(params, deterministic=True)  # builds are compared below
    kw = dict(precision="f32", coarse_iterate=False, coarse_n_iterations=0)
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w,
                               coarse_ilu=dict(**deck_ilu, device=True), **kw)
    info, setup_ms = mg.coarse_ilu()
    assert info["n"] == meshes[0].n_dofs and setup_ms > 0
    assert info["symbolic_ms"] > 0 and info["upload_ms"] == 0
    got = _vcycle(mg, b)
    ref = OracleGMG(meshes, cm, oracle_params, u, hist, w, coarse_iters=0)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    ref.coarse_precondition = R.ILURef(ops[0].system_matrix(), deck_ilu["fill_level"],
                                       deck_ilu["atol"], deck_ilu["rtol"]).vmult
    err = rel_err(got, ref.vcycle(b))
    host, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, coarse_ilu=dict(deck_ilu), **kw)
    assert host.coarse_ilu()[0]["upload_ms"] > 0  # the host path, as before
    diff = rel_err(got, _vcycle(host, b))
    print(f"coarse ILU on the device: V-cycle vs restatement {err:.2e}, vs the host path "
          f"{diff:.2e}, setup {setup_ms:.2f} ms (host path {host.coarse_ilu()[1]:.2f} ms)")
    assert err < 5e-4
    assert diff < 1e-6
    # a new linearisation point on every level, then setup again
    u2 = 0.7 * u + 0.05 * np.cos(np.arange(u.shape[0]))
    mg2, _ = glsamd.build_gmg(meshes, cm, params, u2, hist, w,
                              coarse_ilu=dict(**deck_ilu, device=True), **kw)
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
    assert info["symbolic_ms"] == 0 and info["numeric_ms"] > 0 and info["upload_ms"] == 0
    assert mg2.coarse_ilu()[0]["symbolic_ms"] > 0
    assert rel_err(_vcycle(mg, b), _vcycle(mg2, b)) < 1e-6
    # the switch: before the first setup only, and only with the coarse ILU
    L = glsamd.lib()
    assert L.gls_mg_set_coarse_ilu_device(mg.h, 1) != 0
    assert b"before gls_mg_setup" in L.gls_last_error()
    other, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                                coarse_n_iterations=2)
    assert L.gls_mg_set_coarse_ilu_device(other.h, 1) != 0
    assert b"gls_mg_set_coarse_ilu first" in L.gls_last_error()


# ---- 7. GMRES with the device-built preconditioner: Re100 r1, FP64
def test_gmres_with_the_device_preconditioner(monkeypatch):
    import torch
    import glsamd
    import glssolvers
    _clean(monkeypatch)
    case, op = _deck_operator()
    op.set_linearization_point(case.u_star)
    A = op.system_matrix()
    A.sort_indices()
    b = gi.rnd(31, A.shape[0])
    b[np.asarray(A.diagonal() == 1.0) & (np.diff(A.indptr) == 1)] = 0.0  # constrained rows
    its = {}
    for device in (True, False):
        prec = glssolvers.MatrixPreconditioner(op, "ILU", device=device)
        prec.initialize()
        prec.initialize()  # a refactorisation on the same pattern
        assert prec.preconditioner.info()["symbolic_ms"] == 0
        assert prec.preconditioner.factor_info()["device"] == int(device)
        solver = glsamd.LinearSolverGMRES(op, prec, relative_tolerance=1e-8,
                                          absolute_tolerance=0.0)
        x = torch.zeros(A.shape[0], dtype=torch.float64, device="cuda")
        solver.solve(x, torch.from_numpy(b).cuda())
        got = x.cpu().numpy()
        assert solver.last["converged"] == 1
        res = np.linalg.norm(b - A @ got) / np.linalg.norm(b)
        its[device] = solver.last["n_iterations"]
        print(f"GMRES + ILU(0), device={device}: {its[device]} iterations, residual {res:.2e}")
        assert res <= 1.01e-8
    print(f"iterations: device path {its[True]}, host path {its[False]}")
    with pytest.raises(ValueError):
        glssolvers.MatrixPreconditioner(op, "AMG", device=True)
