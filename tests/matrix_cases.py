"""Shared cases of tests/test_gpu_assemble.py and tests/test_gpu_matrix_based.py:
per case the operator, the host system matrix (gls_op_system_matrix) and
max |E| over its element matrices, computed once and left unchanged.  Tests
that change an operator's state build their own through make_op()."""
import numpy as np

import glsmesh as gm
from helpers import Case, deck, deck_case

RE20, RE100, RE3900 = ("input_turek_2D_Re20_stat.json", "input_turek_2D_Re100.json",
                       "input_hoffmann_3D_Re3900.json")
# Re20_stat r0: 88 cells, Q2, five cells around some nodes; Re100 r1: Q1;
# Re3900 r0: 400 cells, 3D Q2, up to 10 cells per node
MESHES = {"re20_r0": (RE20, 0), "re100_r1": (RE100, 1), "re3900_r0": (RE3900, 0)}
CASES = [f"{m}-{prec}-{variant}" for m in MESHES for prec in ("f64", "f32")
         for variant in ("newton", "picard")] + ["outflow-f64-newton", "shuffled-f64-newton"]

_cases, _built = {}, {}


def _case(key):
    """(Case, outflow descriptor or None) of a case key, cached by mesh and variant"""
    mesh, prec, variant = key.split("-")
    ck = (mesh, variant)
    if ck in _cases:
        return _cases[ck]
    over = {} if variant == "newton" else dict(nonlinear_solver="Picard")
    outflow = None
    if mesh == "outflow":
        # as tests/test_gpu_outflow.py: cut faces with backflow through part of them
        case = deck_case(RE3900, 0, outflow_bc="cut")
        cells, fno = gm.boundary_faces(case.mesh, 1)
        assert len(cells) > 0
        nc, x = case.dim + 1, case.mesh.coords
        scale = 1.0 + np.abs(case.u_star[0::nc]).max()
        case.u_star[0::nc] -= 2.0 * scale * (x[:, 1] > np.median(x[:, 1]))
        outflow = (cells, fno, "cut")
    elif mesh == "shuffled":
        # as tests/test_gpu_system_matrix.py: bricks discovered, cells permuted inside
        from shuffle import ShuffledMesh
        d = deck(RE3900)
        mesh = ShuffledMesh(d.mesh(1), seed=11)
        params, w = d.operator_parameters(2.5e-4)
        case = Case(mesh, mesh.constraint_mask(*d.boundary_descriptor()), params, w,
                    u_inf=d.u_max)
    else:
        case = deck_case(*MESHES[mesh], **over)
    _cases[ck] = (case, outflow)
    return _cases[ck]


def make_op(key):
    """a fresh operator of the case, linearised at case.u_star"""
    case, outflow = _case(key)
    prec = key.split("-")[1]
    return case.gpu(prec, outflow=outflow) if outflow is not None else case.gpu(prec)


def built(key):
    """dict(case, op, A, emax): the shared, read-only state of a case"""
    if key not in _built:
        case, _ = _case(key)
        op = make_op(key)
        A = op.system_matrix()
        A.sort_indices()
        emax = float(np.abs(op.element_matrices()).max())
        _built[key] = dict(case=case, op=op, A=A, emax=emax)
    return _built[key]
