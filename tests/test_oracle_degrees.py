"""The oracle at the (dim, degree) pairs its other known-answer tests reach
only on affine cells: (2,3), (3,1) and (3,3) on the curved hyper cube of
warped.py.  The identities are those of test_oracle_kat.py (KAT-1, KAT-3) with
their tolerances; they pin the reference side of test_gpu_degrees.py."""
import numpy as np
import pytest

import glsinputs as gi
import glsmesh as gm
from test_oracle_kat import _assemble, _const_field, _op
from warped import WarpedMesh, drop_middle, position_mask

PAIRS = [(2, 3, 2), (3, 1, 2), (3, 3, 1)]  # dim, degree, n_ref
IDS = ["q3_2d", "q1_3d", "q3_3d"]


def _mesh(dim, k, n_ref, flat_axis, keep=None):
    return WarpedMesh(gm.hypercube(dim, k, n_ref), flat_axis=flat_axis, keep=keep)


@pytest.mark.parametrize("dim,k,n_ref", PAIRS, ids=IDS)
@pytest.mark.parametrize("flat_axis", [0, None])
@pytest.mark.parametrize("increment_form", [True, False])
def test_partition_of_unity(dim, k, n_ref, flat_axis, increment_form):
    mesh = _mesh(dim, k, n_ref, flat_axis)
    op, _ = _op(mesh, increment_form=increment_form)
    U = _const_field(mesh, [1.3, -0.4, 0.7][:dim] + [2.0])
    op.set_linearization_point(U)
    op.set_previous_solution([U, np.zeros_like(U), np.zeros_like(U)], [150.0, 0.0, 0.0])
    cvec = [0.3, 0.8, -0.5][:dim] + [0.0]
    dst = op.vmult(_const_field(mesh, cvec))
    vol = op.geometry()[:, :, 0].sum()
    nc = dim + 1
    for c in range(dim):
        assert abs(dst[c::nc].sum() - 150.0 * cvec[c] * vol) < 1e-11 * max(1, abs(150 * vol))
    assert abs(dst[dim::nc].sum()) < 1e-12


@pytest.mark.parametrize("dim,k,n_ref", PAIRS, ids=IDS)
@pytest.mark.parametrize("flat_axis", [0, None])
@pytest.mark.parametrize("cell_wise", [False, True])
def test_matrix_consistency(dim, k, n_ref, flat_axis, cell_wise):
    mesh = _mesh(dim, k, n_ref, flat_axis)
    cmask = position_mask(mesh.ref_coords)
    op, _ = _op(mesh, cmask, cell_wise_stabilization=cell_wise)
    u = gi.linearization_point(mesh.n_nodes, mesh.dim, 2.0)
    op.set_linearization_point(u)
    op.set_previous_solution(gi.history(u, 2), [150.0, -200.0, 50.0])
    A = _assemble(op, mesh, cmask)
    x = gi.src_vector(mesh.n_dofs)
    assert np.allclose(A @ x, op.vmult(x), rtol=0, atol=1e-11 * np.abs(A @ x).max())
    inv = op.inverse_diagonal()
    dg = np.diag(A)
    ref = np.where(np.abs(dg) > 1e-10, 1.0 / np.where(dg == 0, 1, dg), 1.0)
    assert np.allclose(inv, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dim,k,n_ref", PAIRS, ids=IDS)
@pytest.mark.parametrize("flat_axis", [0, None])
def test_geometry(dim, k, n_ref, flat_axis):
    """det J of the Q_k map has degree 2k-1 per direction in 2D, which
    QGauss(k+1) integrates exactly: the warped cells tile the unit square.
    In 3D (degree 3k-1) the rule is inexact."""
    mesh = _mesh(dim, k, n_ref, flat_axis)
    op, _ = _op(mesh)
    jxw = op.geometry()[:, :, 0]
    assert jxw.min() > 0
    assert abs(jxw.sum() - 1.0) < (1e-13 if dim == 2 else 1e-6)
    if flat_axis is not None:
        # cells left of X_a = 1/2 are the undisplaced ones
        lo = mesh.ref_coords[np.asarray(mesh.cell_nodes, dtype=np.int64)][:, :, flat_axis]
        flat = lo.max(axis=1) <= 0.5 + 1e-12
        assert flat.any() and not flat.all()
        assert np.array_equal(mesh.coords[np.asarray(mesh.cell_nodes)[flat]],
                              mesh.ref_coords[np.asarray(mesh.cell_nodes)[flat]])
    # the per-cell factor of the measures reaches the oracle's inputs
    meas, hmin = mesh.cell_measure()
    m0, h0 = mesh.base.cell_measure()
    assert np.ptp(meas / m0) > 0.1 and np.allclose((hmin / h0) ** dim, meas / m0)


@pytest.mark.parametrize("dim,k,n_ref,n_keep", [(3, 3, 1, 7), (2, 3, 2, 13), (3, 1, 2, 61)],
                         ids=["q3_3d", "q3_2d", "q1_3d"])
def test_keep(dim, k, n_ref, n_keep):
    """Cells dropped from the middle of the list: rows of the nodes no kept
    cell touches are 0 in vmult and the residual, 1 in the inverse diagonal."""
    base = gm.hypercube(dim, k, n_ref)
    keep = drop_middle(base.n_cells, n_keep)
    mesh = WarpedMesh(base, flat_axis=0, keep=keep)
    assert mesh.n_cells == n_keep and mesh.brick() == (0, 0, 0)
    assert mesh.n_nodes == base.n_nodes
    cmask = position_mask(mesh.ref_coords)
    op, _ = _op(mesh, cmask)
    u = gi.linearization_point(mesh.n_nodes, dim, 1.0)
    op.set_linearization_point(u)
    op.set_previous_solution(gi.history(u, 2), [150.0, -200.0, 50.0])
    x = gi.src_vector(mesh.n_dofs)
    nc = dim + 1
    free = np.repeat(~mesh.touched_nodes(), nc)
    for comp in range(nc):  # an untouched node on a constrained face is an identity row
        free[comp::nc] &= ((cmask >> comp) & 1) == 0
    # (a dropped Q1 cell leaves no node untouched: all are its neighbours' too)
    assert (free.sum() > 0) == (k > 1)
    A = _assemble(op, mesh, cmask)
    assert np.allclose(A @ x, op.vmult(x), rtol=0, atol=1e-11 * np.abs(A @ x).max())
    assert np.all(op.vmult(x)[free] == 0)
    assert np.all(op.evaluate_residual(x)[free] == 0)
    assert np.all(op.inverse_diagonal()[free] == 1)
    # the kept cells' rows are those of the full mesh's cells
    full, _ = _op(WarpedMesh(base, flat_axis=0), cmask)
    full.set_linearization_point(u)
    full.set_previous_solution(gi.history(u, 2), [150.0, -200.0, 50.0])
    for i in (0, n_keep // 2, n_keep - 1):
        assert np.array_equal(op.cell_matrix(i), full.cell_matrix(int(keep[i])))
