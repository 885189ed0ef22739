"""Store policies of the brick write-out and the shared-node reduction
(GLS_STORE_POLICY, csrc/kernels.h StorePolicy): plain, non-temporal or
write-through 16-byte stores at three store sites -- the partial-slot rows
and the exclusive dst / out64 rows of k_brick, the rows of
k_shared_reduce_cls -- write-through with whole FP64 rows per instruction
(lane pairs exchange halves) at the first two, and non-temporal slot loads in
the reduction.  The library's defaults (the variable unset) are compared too.

A policy changes when a row's bytes leave the L2, never their value: in
deterministic mode every combination gives bitwise the all-plain result, and
the all-write-through result is within the suite's parity tolerance of the
CPU oracle (FP64 1e-12, FP32 2e-5 relative l2).

Meshes: hypercube(3, 2, 3) (512 cells, 32 bricks of 4x4x1, shared nodes of
multiplicity 2, 4 and 8, Dirichlet rows) and the curved cylinder(3, 2, 1) with
discovered bricks; a two-level FP32 multigrid on hypercube r1..r2 for the
fused Jacobi write-out, the residual, the deferred reduction and out64."""
import functools
import itertools

import numpy as np
import pytest

import glsinputs as gi
import glsmesh as gm
from helpers import Case, deck, rel_err
from warped import position_mask

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}
DECK = "input_hoffmann_3D_Re3900.json"
# every combination of the three store sites, the slot loads non-temporal on
# top of all-plain and all-write-through stores, and the paired-lane form of
# the write-through stores of the brick write-out
POLICIES = (["".join(p) for p in itertools.product("pnw", repeat=3)] + ["pppn", "wwwn"]
            + ["rpp", "prp", "rrw", "rnr"])  # r: write-through, whole FP64 rows per instruction


def _np(t):
    return t.double().cpu().numpy()


class Ref:
    """One mesh: the case and the oracle's vmult and residual, computed once
    and shared (never written to)."""

    def __init__(self, mesh, cmask, brick, u_inf):
        params, w = deck(DECK).operator_parameters(2.5e-4)
        self.case, self.brick = Case(mesh, cmask, params, w, u_inf=u_inf), brick
        o = self.case.oracle()
        self.vmult = o.vmult(self.case.src)
        self.residual = o.evaluate_residual(self.case.src)
        for v in (self.vmult, self.residual):
            v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ref_of(kind):
    if kind == "hypercube":
        mesh = gm.hypercube(3, 2, 3)
        return Ref(mesh, position_mask(mesh.coords), None, 1.0)
    d = deck(DECK)
    mesh = gm.cylinder(3, 2, 1)
    vel, p, slip = d.boundary_descriptor()
    return Ref(mesh, mesh.constraint_mask(vel, p, slip), "auto", d.u_max)


def _apply(r, prec, policy, monkeypatch):
    """(vmult, residual) of a deterministic operator created under `policy`
    (None: the variable unset, the library's defaults)."""
    import torch
    if policy is None:
        monkeypatch.delenv("GLS_STORE_POLICY", raising=False)
    else:
        monkeypatch.setenv("GLS_STORE_POLICY", policy)
    op = r.case.gpu(prec, brick=r.brick)
    op.set_parameters(**r.case.params, deterministic=True)
    assert op.brick_shape != (0, 0, 0)
    if r.brick is None:
        assert op.brick_shape == (4, 4, 1)  # the hypercube: 32 one-layer bricks
    src = op._dev(r.case.src)
    dst, res = op.initialize_dof_vector(), op.initialize_dof_vector()
    for _ in range(2):  # a repeated apply overwrites dst completely
        op.vmult(dst, src)
    op.evaluate_residual_plain(res, src)
    torch.cuda.synchronize()
    return dst, res


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["hypercube", "cylinder"])
def test_policies_bitwise_and_parity(kind, prec, monkeypatch):
    import torch
    r = ref_of(kind)
    if kind == "hypercube":
        assert r.case.mesh.n_cells == 512
    dst0, res0 = _apply(r, prec, "ppp", monkeypatch)
    for policy in POLICIES[1:] + [None]:
        dst, res = _apply(r, prec, policy, monkeypatch)
        assert torch.equal(dst, dst0), (kind, prec, policy, "vmult")
        assert torch.equal(res, res0), (kind, prec, policy, "residual")
        if policy == "www":
            ev, er = rel_err(_np(dst), r.vmult), rel_err(_np(res), r.residual)
            print(f"STP {kind} {prec} www: vmult {ev:.3e} residual {er:.3e}")
            assert ev < TOL[prec] and er < TOL[prec]


def test_bad_policy_is_refused(monkeypatch):
    import glsamd
    r = ref_of("hypercube")
    for bad in ["w", "wwx", "wwww", "pppnn", "pppr"]:
        monkeypatch.setenv("GLS_STORE_POLICY", bad)
        with pytest.raises(glsamd.GlsError, match="GLS_STORE_POLICY"):
            r.case.gpu("f64")


def test_vcycle_bitwise(monkeypatch):
    """One deterministic V-cycle of a two-level FP32 multigrid (hypercube
    r1..r2; the fine level's 4x4x1 bricks run one launch per smoothing step:
    fused Jacobi write-out, deferred reductions, out64, the residual): all
    write-through equals all plain bitwise."""
    import torch
    import glsamd
    meshes = [gm.hypercube(3, 2, 1), gm.hypercube(3, 2, 2)]
    cmasks = [position_mask(m.coords) for m in meshes]
    params, w = deck(DECK).operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, 3, 1.0)
    hist = gi.history(u, params["order"])
    b = torch.from_numpy(gi.rnd(41, meshes[-1].n_dofs)).cuda()

    def cycle(policy):
        monkeypatch.setenv("GLS_STORE_POLICY", policy)
        mg, ops = glsamd.build_gmg(meshes, cmasks, dict(params, deterministic=True), u, hist, w,
                                   precision="f32")
        assert ops[-1].brick_shape == (4, 4, 1)
        x = torch.zeros(meshes[-1].n_dofs, dtype=torch.float64, device="cuda")
        mg.vcycle(x, b)
        torch.cuda.synchronize()
        return x

    x0 = cycle("ppp")
    assert torch.all(torch.isfinite(x0)) and float(x0.abs().max()) > 0
    for policy in ["www", "wwwn", "wpw", "rrw"]:
        assert torch.equal(cycle(policy), x0), policy
