"""Batched LDS reads of the brick kernels' cell rounds (GLS_STAGE_BATCH,
csrc/brick.h stage_batch, csrc/brick_rounds.inc): a stage's coefficient row
and the lines of every pack are issued together and consumed in the order of
issue.  The order of the loads changes, the arithmetic does not -- every value
keeps its FMA chain -- so

* with deterministic=True every result is bitwise what the kernels gave
  before the batches existed: the SHA-256 of its bytes equals the digest in
  tests/golden/stage_batches/digests.json, recorded on an MI355X from the
  library of the commit before (record_golden below; the commit is named in
  profiles/stage_batch/README.md);
* in the default mode (LDS atomics in arrival order) the results are within
  the suite's tolerance of the CPU oracle, relative l2 1e-12 (FP64) and 2e-5
  (FP32).

The default build batches the gradient and the two-pack sweeps of the FP64
kernels; both checks cover them.  The batched x S^T sweep in front of the LDS
atomics (bit 4, off by default) exists only in the non-deterministic kernels
-- the deterministic ones accumulate cell by cell between barriers -- so in a
build with that bit it is covered by the parity check alone; the batched Dq^T
exchange (bit 2 without bit 1) is in no default kernel either.

Meshes, the smallest that reach each body of the 3D Q2 kernels with both
rounds of a 4x4x1 brick (16 cells, 8 per round):
  cart      hypercube(3, 2, 3): 32 Cartesian bricks, the stand-alone GEO_CART kernel
  mixed     the same, warped where X_0 > 1/2: Cartesian and curved bricks in one
            launch (GEO_ANY, both bodies)
  curved    the same, warped everywhere: GEO_GEN
  cylinder  cylinder(3, 2, 1), discovered 2x2x2 bricks: a single round of 8 cells
Operators: the Re3900 deck's parameters; Newton vmult, fixed-point (Picard)
vmult and evaluate_residual_plain, FP64 and FP32.

Recording (on the GPU, with GLS_AMD_LIB naming the library to record from):
  GLS_RECORD_GOLDEN=1 python tests/test_gpu_stage_batches.py [digests.json]
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the recorder runs outside pytest: conftest.py's paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "dealii-ns-gls_amd", "python"), os.path.join(_root, "oracle"),
               os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, _p)

import glsmesh as gm
from helpers import Case, deck, rel_err
from warped import WarpedMesh, position_mask

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-12, "f32": 2e-5}
DECK = "input_hoffmann_3D_Re3900.json"
KINDS = ["cart", "mixed", "curved", "cylinder"]
PRECS = ["f64", "f32"]
MODES = {"newton": {}, "fixed": dict(nonlinear_solver="Picard")}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_batches",
                      "digests.json")


def _np(t):
    return t.double().cpu().numpy()


def _parameters(mode):
    d = deck(DECK)
    for k, v in MODES[mode].items():
        setattr(d, k, v)
    return d.operator_parameters(2.5e-4)


@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """(mesh, constraint mask, brick argument, u_inf)"""
    if kind == "cylinder":
        d = deck(DECK)
        mesh = gm.cylinder(3, 2, 1)
        vel, p, slip = d.boundary_descriptor()
        return mesh, mesh.constraint_mask(vel, p, slip), "auto", d.u_max
    base = gm.hypercube(3, 2, 3)
    if kind == "cart":
        return base, position_mask(base.coords), None, 1.0
    mesh = WarpedMesh(base, flat_axis=0 if kind == "mixed" else None)
    return mesh, position_mask(mesh.ref_coords), None, 1.0


class Ref:
    """One mesh and mode: the case and the oracle's vmult (and, for the
    Newton parameters, residual), computed once and shared (never written to)."""

    def __init__(self, kind, mode):
        mesh, cmask, self.brick, u_inf = _mesh(kind)
        params, w = _parameters(mode)
        self.case = Case(mesh, cmask, params, w, u_inf=u_inf)
        o = self.case.oracle()
        self.vmult = o.vmult(self.case.src)
        self.vmult.setflags(write=False)
        self.residual = None
        if mode == "newton":
            self.residual = o.evaluate_residual(self.case.src)
            self.residual.setflags(write=False)


@functools.lru_cache(maxsize=None)
def ref_of(kind, mode):
    return Ref(kind, mode)


def _case_of(kind, mode, with_oracle):
    if with_oracle:
        r = ref_of(kind, mode)
        return r.case, r.brick
    mesh, cmask, brick, u_inf = _mesh(kind)
    params, w = _parameters(mode)
    return Case(mesh, cmask, params, w, u_inf=u_inf), brick


def _results(kind, prec, deterministic, with_oracle=True):
    """{"newton": vmult, "fixed": vmult, "residual": evaluate_residual_plain}
    of operators on mesh `kind` (device tensors)."""
    import torch
    out = {}
    for mode in MODES:
        case, brick = _case_of(kind, mode, with_oracle)
        op = case.gpu(prec, brick=brick)
        op.set_parameters(**case.params, deterministic=deterministic)
        if kind == "cylinder":
            assert op.brick_shape == (2, 2, 2)
        else:
            assert case.mesh.n_cells == 512 and op.brick_shape == (4, 4, 1)
        src = op._dev(case.src)
        dst = op.initialize_dof_vector()
        for _ in range(2):  # a repeated apply overwrites dst completely
            op.vmult(dst, src)
        out[mode] = dst
        if mode == "newton":
            res = op.initialize_dof_vector()
            op.evaluate_residual_plain(res, src)
            out["residual"] = res
    torch.cuda.synchronize()
    return out


def _digests(kind, prec, with_oracle=True):
    got = _results(kind, prec, True, with_oracle)
    return {f"{kind}/{prec}/{what}": hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
            for what, t in got.items()}


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_deterministic_bitwise_golden(kind, prec):
    golden = _golden()
    for key, digest in _digests(kind, prec, with_oracle=False).items():
        assert digest == golden[key], key


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_default_mode_parity(kind, prec):
    got = _results(kind, prec, False)
    want = {"newton": ref_of(kind, "newton").vmult, "fixed": ref_of(kind, "fixed").vmult,
            "residual": ref_of(kind, "newton").residual}
    errs = {what: rel_err(_np(got[what]), want[what]) for what in want}
    print(f"STAGE_BATCH {kind} {prec}: " + " ".join(f"{w} {e:.3e}" for w, e in errs.items()))
    for what, e in errs.items():
        assert e < TOL[prec], (kind, prec, what, e)


def record_golden(path=GOLDEN):
    """The digests of every case, computed twice from freshly created
    operators; the two recordings must agree."""
    assert os.environ.get("GLS_RECORD_GOLDEN") == "1", "set GLS_RECORD_GOLDEN=1 to record"
    runs = []
    for _ in range(2):
        d = {}
        for kind in KINDS:
            for prec in PRECS:
                d.update(_digests(kind, prec, with_oracle=False))
        runs.append(d)
    assert runs[0] == runs[1], "two recordings differ"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(runs[0], f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(runs[0])} digests from {os.environ.get('GLS_AMD_LIB', 'the built library')}"
          f" into {path}")


if __name__ == "__main__":
    record_golden(*sys.argv[1:2])
