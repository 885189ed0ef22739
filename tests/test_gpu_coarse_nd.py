"""The nested-dissection form of the direct coarse solver
(Multigrid(coarse_direct="nd"), csrc/coarse_nd.hip): one-level solves against
numpy and against the dense solver, V-cycles against the oracle multigrid,
refactorisation with the plan reused, a shuffled cell order, the error paths.
Every test checks coarse_direct_info()["method"] == "nd": a silent fallback to
the dense solver cannot pass.

Tolerances are those of the dense solver's tests: the one-level solve 1e-10
(FP64) / 2e-4 (FP32) relative l2 (test_gpu_system_matrix.py::
test_direct_coarse_solve), the V-cycle against the oracle multigrid 1e-9 (FP64
levels) / 5e-4 (FP32 levels) (test_a_gpu_configs.py).  The 3D residual may be
10x the dense solver's: pivoting is confined to the pivot blocks."""
import numpy as np
import pytest

import glsinputs as gi
from helpers import deck, deck_case, rel_err
from mg_ref import OracleGMG

pytestmark = pytest.mark.gpu
RE3900 = "input_hoffmann_3D_Re3900.json"


def _np(t):
    return t.double().cpu().numpy()


def _solve(mg, b):
    import torch
    x = torch.zeros(len(b), dtype=torch.float64, device="cuda")
    mg.vcycle(x, torch.from_numpy(b).cuda())
    torch.cuda.synchronize()
    return _np(x)


def _one_level(op, direct, leaf=None):
    import glsamd
    mg = glsamd.Multigrid([op], [], coarse_n_iterations=-1, outer_precision="f64",
                          coarse_direct=direct, coarse_leaf_cells=leaf)
    mg.setup()
    info = mg.coarse_direct_info()
    assert info["method"] == direct and info["requested"] == direct, info
    return mg, info


@pytest.mark.parametrize("name,n_ref", [("input_turek_2D_Re100.json", 1),
                                        ("input_turek_2D_Re20_stat.json", 1)])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_nd_coarse_solve(name, n_ref, prec):
    """One-level multigrid = the coarse solve alone, against a dense solve of
    the assembled FP64 system matrix: Q1 (nothing condensed) and Q2 (cell
    interiors condensed), 12 cells per leaf (at least three tree levels)."""
    case = deck_case(name, n_ref)
    op = case.gpu(prec)
    A = case.gpu("f64").system_matrix().toarray()
    b = np.random.default_rng(5).standard_normal(op.n_dofs)
    ref = np.linalg.solve(A, b)
    mg, info = _one_level(op, "nd", 12)
    assert info["depth"] >= 3 and info["tree_nodes"] >= 7, info
    assert 0 < info["stored_entries"] < info["nf"] ** 2
    err = rel_err(_solve(mg, b), ref)
    dense, _ = _one_level(op, "dense")
    err_dense = rel_err(_solve(dense, b), ref)
    print(f"{name} {prec}: nd rel err {err:.2e} (dense {err_dense:.2e}), nf {info['nf']}, "
          f"{info['tree_nodes']} tree nodes, depth {info['depth']}, stored "
          f"{info['stored_entries']} entries")
    assert err < (1e-10 if prec == "f64" else 2e-4)
    # repeatable bit for bit
    assert np.array_equal(_solve(mg, b), _solve(mg, b))


@pytest.mark.parametrize("shuffled", [False, True])
def test_nd_residual_re3900_r0(shuffled):
    """Re3900 r0 (400 Q2 cells, 12,606 condensed free dofs), FP64, the same
    right-hand side through both solvers: ||A x - b|| / ||b|| with A x by the
    FP64 vmult at most 10x the dense solver's.  shuffled: the cells in a
    random order (brick discovery permutes them internally once more)."""
    import torch
    if shuffled:
        from shuffle import ShuffledMesh
        from test_brick_discovery import _case
        case = _case(ShuffledMesh(deck(RE3900).mesh(0), seed=11), RE3900)
    else:
        case = deck_case(RE3900, 0)
    op = case.gpu("f64")
    b = np.random.default_rng(7).standard_normal(op.n_dofs)

    def residual(x):
        ax = op.initialize_dof_vector()
        op.vmult(ax, torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        return np.linalg.norm(_np(ax) - b) / np.linalg.norm(b)

    mg, info = _one_level(op, "nd")
    assert info["depth"] >= 3, info
    r_nd = residual(_solve(mg, b))
    del mg
    dense, _ = _one_level(op, "dense")
    r_dense = residual(_solve(dense, b))
    print(f"Re3900 r0 FP64 (shuffled {shuffled}): residual nd {r_nd:.2e}, dense {r_dense:.2e}; "
          f"nd: {info}")
    assert r_nd <= 10 * r_dense


@pytest.fixture(scope="module")
def re3900_r0_r1():
    d = deck(RE3900)
    meshes = [d.mesh(r) for r in range(2)]
    vel, p, slip = d.boundary_descriptor()
    cm = [m.constraint_mask(vel, p, slip) for m in meshes]
    params, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, 3, d.u_max)
    hist = gi.history(u, params["order"])
    ref = OracleGMG(meshes, cm, params, u, hist, w, coarse_iters=-1)
    return meshes, cm, params, w, u, hist, ref


@pytest.mark.parametrize("prec,tol", [("f64", 1e-9), ("f32", 5e-4)])
def test_nd_vcycle_re3900(re3900_r0_r1, prec, tol):
    """The V-cycle on Re3900 r0..r1 with the nd coarse solve against the
    oracle multigrid (its own FP64 diagonals and FP64 LU of its coarse
    matrix; only the relaxation factors are shared)."""
    import glsamd
    meshes, cm, params, w, u, hist, ref = re3900_r0_r1
    b = gi.rnd(11, meshes[-1].n_dofs)
    mg, ops = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision=prec,
                               coarse_n_iterations=-1, coarse_direct="nd")
    info = mg.coarse_direct_info()
    assert info["method"] == "nd", info
    y = _solve(mg, b)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    err = rel_err(y, ref.vcycle(b))
    dense, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision=prec,
                                coarse_n_iterations=-1)
    assert dense.coarse_direct_info()["method"] == "dense"
    diff = rel_err(y, _solve(dense, b))
    print(f"Re3900 r0..r1 {prec} nd-coarse V-cycle rel err {err:.2e}, to the dense-coarse "
          f"V-cycle {diff:.2e}")
    assert err < tol


def test_nd_vcycle_deterministic_bitwise(re3900_r0_r1):
    import glsamd
    meshes, cm, params, w, u, hist, _ = re3900_r0_r1
    b = gi.rnd(41, meshes[-1].n_dofs)
    mg, ops = glsamd.build_gmg(meshes, cm, dict(params, deterministic=True), u, hist, w,
                               precision="f32", coarse_n_iterations=-1, coarse_direct="nd")
    assert mg.coarse_direct_info()["method"] == "nd"
    y1, y2, y3 = _solve(mg, b), _solve(mg, b), _solve(mg, b)
    assert np.array_equal(y1, y2) and np.array_equal(y1, y3)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_nd_refactorisation(prec):
    """setup() after a second set_linearization_point reuses the plan
    (plan_ms == 0) and gives bitwise what a fresh object set up at that point
    gives."""
    case = deck_case("input_turek_2D_Re20_stat.json", 1)
    u2 = 0.5 * case.u_star + 0.1 * gi.rnd(3, case.n_dofs)
    b = np.random.default_rng(9).standard_normal(case.n_dofs)
    op = case.gpu(prec)
    mg, info = _one_level(op, "nd", 12)
    assert info["plan_ms"] > 0
    x1 = _solve(mg, b)
    op.set_linearization_point(op._dev(u2))
    mg.setup()
    info2 = mg.coarse_direct_info()
    assert info2["method"] == "nd" and info2["plan_ms"] == 0, info2
    assert info2["stored_entries"] == info["stored_entries"]
    x2 = _solve(mg, b)
    assert not np.array_equal(x1, x2)
    op_f = case.gpu(prec)
    op_f.set_linearization_point(op_f._dev(u2))
    fresh, _ = _one_level(op_f, "nd", 12)
    assert np.array_equal(x2, _solve(fresh, b))


def test_nd_error_paths():
    import glsamd
    case = deck_case("input_turek_2D_Re100.json", 1)
    op = case.gpu("f64")
    with pytest.raises(glsamd.GlsError):  # not the direct coarse solver
        glsamd.Multigrid([op], [], coarse_n_iterations=10, coarse_direct="nd")
    with pytest.raises(glsamd.GlsError):
        glsamd.Multigrid([op], [], coarse_n_iterations=0, coarse_direct="nd")
    mg, _ = _one_level(op, "nd", 12)
    with pytest.raises(glsamd.GlsError):  # after setup
        mg.set_coarse_direct("dense")
    with pytest.raises(glsamd.GlsError):
        mg.set_coarse_direct("nd", 30)
    assert mg.coarse_direct_info()["method"] == "nd"
