"""The brick kernels' prologue (csrc/brick_entry.inc, brick_setup.inc,
brick_body.inc, brick.h load_lane): the per-brick record read by a scalar
load, scalar bases + 32-bit lane offsets of the streamed loads, the
branch-free gather with clamped lanes, the coefficient tables' device image
and the quadrature weights by selects.  Oracle comparison as in
tests/test_gpu_parity.py (FP64 relative l2 <= 1e-12, FP32 <= 2e-5), on the
smallest shapes that reach each path:

* Re3900 r0 / r1: one-layer bricks, Cartesian and curved (mixed launch,
  both 4-wave bodies);
* bricks (4,2,1) and (4,1,1): lattices of 135 and 81 nodes in a 256-thread
  workgroup, so most gather lanes are clamped.  These shapes are sub-bricks
  of the mesh order from r2 on only (an r1 coarse cell holds 2x2x2 cells:
  gls_op_create refuses them there), so they run at r2, in both precisions
  (tests/test_gpu_parity.py::test_vmult_headline_r2 has them in FP64), and r1
  runs its own sub-bricks (2,1,1) and (1,1,1): 45 and 27 lattice nodes;
* Turek-2D with 8x8 bricks (r3: an r2 coarse cell holds 4x4 cells, so its
  bricks are 4x4), 289 lattice nodes = two lattice chunks per thread,
  the second one 33 live lanes; 7 cells per wavefront, so the last round has
  wavefronts with one live cell slot and wavefronts past the brick's end;
* fixed-point and residual modes (the bodies that prefetch the next round);
* the sphere deck at refinement 0 (every brick curved);
* two-layer bricks (GLS_TWO_LAYER=1);
* a vmult in two brick ranges (brick_begin != 0) against the single launch;
* a V-cycle over Re3900 r0..r1 in FP32 (deferred-reduction gather and the
  resident sweeps kernel, which share the prologue).
"""
import functools

import numpy as np
import pytest

import glsinputs as gi
from helpers import deck, deck_case, rel_err

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}
RE3900 = "input_hoffmann_3D_Re3900.json"


def _np(t):
    return t.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name, n_ref, picard=False, residual=True):
    """(case, oracle vmult of case.src, oracle residual at u_star or None):
    computed once per configuration, shared by the tests, never modified."""
    over = dict(nonlinear_solver="Picard") if picard else {}
    case = deck_case(name, n_ref, **over)
    o = case.oracle()
    ref = o.vmult(case.src)
    ref.setflags(write=False)
    res = None
    if residual:
        res = o.evaluate_residual(case.u_star)
        res.setflags(write=False)
    return case, ref, res


def _vmult(case, prec, brick=None):
    import torch
    op = case.gpu(prec, brick=brick)
    dst = op.initialize_dof_vector()
    src = op._dev(case.src)
    for _ in range(2):  # repeated applies overwrite dst completely
        op.vmult(dst, src)
    torch.cuda.synchronize()
    return op, _np(dst)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n_ref", [0, 1])
def test_newton_re3900(n_ref, prec):
    case, ref, _ = _case(RE3900, n_ref, residual=False)
    _, got = _vmult(case, prec)
    err = rel_err(got, ref)
    print(f"Re3900 r{n_ref} {prec}: rel l2 {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n_ref,brick", [(1, (2, 1, 1)), (1, (1, 1, 1)), (2, (4, 2, 1)),
                                         (2, (4, 1, 1))])
def test_newton_small_lattices(n_ref, brick, prec):
    case, ref, _ = _case(RE3900, n_ref, residual=False)
    op, got = _vmult(case, prec, brick=brick)
    assert tuple(op.brick_shape) == brick
    err = rel_err(got, ref)
    print(f"Re3900 r{n_ref} brick {brick} {prec}: rel l2 {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_turek2d_two_lattice_chunks(prec):
    case, ref, _ = _case("input_turek_2D_Re100.json", 3, residual=False)
    op, got = _vmult(case, prec, brick=(8, 8, 1))
    bs = list(op.brick_shape)
    assert (2 * bs[0] + 1) * (2 * bs[1] + 1) > 256, bs  # two lattice chunks per thread
    err = rel_err(got, ref)
    print(f"Turek-2D r3 bricks {bs} {prec}: rel l2 {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_fixed_point_and_residual_re3900_r0(prec):
    import torch
    case, ref, res_ref = _case(RE3900, 0, picard=True)
    op, got = _vmult(case, prec)
    res = op.initialize_dof_vector()
    op.evaluate_residual_plain(res, op._dev(case.u_star))
    torch.cuda.synchronize()
    e_v, e_r = rel_err(got, ref), rel_err(_np(res), res_ref)
    print(f"Re3900 r0 fixed point {prec}: vmult {e_v:.3e}, residual {e_r:.3e}")
    assert e_v < TOL[prec]
    assert e_r < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_sphere_all_curved(prec):
    case, ref, _ = _case("input_sphere_amg.json", 0, residual=False)
    op, got = _vmult(case, prec)
    n_gen, n_cart = op.geometry_counts()
    assert n_cart == 0 and n_gen == op.n_cells
    err = rel_err(got, ref)
    print(f"sphere r0 {prec}: rel l2 {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_two_layer_bricks(prec, monkeypatch):
    monkeypatch.setenv("GLS_TWO_LAYER", "1")
    case, ref, _ = _case(RE3900, 1, residual=False)
    op, got = _vmult(case, prec)
    assert list(op.brick_shape)[2] == 2, list(op.brick_shape)
    err = rel_err(got, ref)
    print(f"Re3900 r1 two-layer {prec}: rel l2 {err:.3e}")
    assert err < TOL[prec]


@pytest.mark.parametrize("deterministic", [True, False])
def test_two_brick_ranges(deterministic):
    """The partitioned operator's schedule on one member: bricks [0, b), the
    (empty) boundary range, bricks [b, n) and the reduce, against the single
    launch over [0, n).  With the deterministic lattice accumulation the two
    are the same sums in the same order: bitwise equal.  Otherwise they differ
    by the order of the LDS atomic adds of at most 8 cells per lattice node:
    a few units of 2^-53 per entry, 1e-14 in the relative l2 norm (the bound of
    tests/test_dist.py::test_rccl_world1_native)."""
    import torch
    import glsdist
    case, ref, _ = _case(RE3900, 1, residual=False)
    g = glsdist.LocalGroup(case.mesh, case.cmask, 1, engine="gpu", native=True)
    g.setup(dict(case.params, deterministic=deterministic), case.u_star, case.hist, case.weights)
    srcs = g.scatter(case.src)
    dsts = [r.new_vector() for r in g.ranks]
    g.vmult(dsts, srcs)
    one = g.ranks[0].new_vector()
    g.ranks[0].eng.op.vmult(one, srcs[0])
    torch.cuda.synchronize()
    split = g.gather(dsts)
    whole = g.gather([one])
    if deterministic:
        assert torch.equal(split, whole)
    else:
        assert rel_err(_np(split), _np(whole)) < 1e-14
    assert rel_err(_np(split), ref) < TOL["f64"]


def test_vcycle_re3900_f32():
    """One V-cycle over Re3900 r0..r1, FP32 levels, coarse solve 10 relaxation
    sweeps, against the oracle multigrid at the tolerance of
    tests/test_gpu_mg.py::test_relaxation_and_vcycle (5e-4)."""
    import torch
    import glsamd
    from mg_ref import OracleGMG
    d = deck(RE3900)
    meshes = [d.mesh(r) for r in range(2)]
    vel, p, slip = d.boundary_descriptor()
    cmasks = [m.constraint_mask(vel, p, slip) for m in meshes]
    params, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, params["order"])
    mg, ops = glsamd.build_gmg(meshes, cmasks, params, u, hist, w, precision="f32",
                               coarse_n_iterations=10)
    ref = OracleGMG(meshes, cmasks, params, u, hist, w, coarse_iters=10)
    ref.set_omega([mg.relaxation(l)[0] for l in range(len(meshes))])
    for l in range(len(meshes)):  # the GPU's own FP32 level diagonals (test_gpu_mg.py)
        dl = ops[l].initialize_dof_vector()
        ops[l].compute_inverse_diagonal(dl)
        ref.invdiag[l] = _np(dl)
    b = gi.rnd(11, meshes[-1].n_dofs)
    src = torch.from_numpy(b).cuda()
    dst = torch.zeros_like(src)
    mg.vcycle(dst, src)
    torch.cuda.synchronize()
    err = rel_err(_np(dst), ref.vcycle(b))
    print(f"Re3900 r0..r1 FP32 V-cycle: rel l2 {err:.3e}")
    assert err < 5e-4
