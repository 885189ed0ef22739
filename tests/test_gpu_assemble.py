"""The system matrix assembled on the device (gls_op_system_matrix_device,
csrc/assemble.hip) against the host assembly of the same operator
(gls_op_system_matrix): equal pattern, values within the bound below; the
result independent of the chunk of cells, repeatable bit for bit, and renewed
when the linearization point changes.

Tolerance (derived, not measured): both paths add the same FP64 addends (the
element-matrix entries, converted to double for FP32 operators) in different
orders, at most V = 10 per entry on these meshes.  Two orderings of a sum of
V terms bounded by max|E| differ by at most 2 (V-1) eps V max|E| ~ 2e-14
max|E|; the tolerance 1e-13 max|E| leaves a factor of 5."""
import numpy as np
import pytest

import matrix_cases as mc

pytestmark = pytest.mark.gpu
TOL = 1e-13


def _host(t):
    return t.cpu().numpy()


def _check_against_host(key, dev, what=""):
    b = mc.built(key)
    A, emax = b["A"], b["emax"]
    rp, ci, va = (_host(t) for t in dev)
    assert rp.dtype == np.int64 and ci.dtype == np.int32 and va.dtype == np.float64
    assert np.array_equal(rp, A.indptr)
    assert np.array_equal(ci, A.indices)
    err = float(np.abs(va - A.data).max())
    print(f"{key}{what}: nnz {A.nnz}, max|E| {emax:.3e}, max |vals_dev - vals_host| {err:.3e} "
          f"= {err / emax:.2e} max|E| (bound {TOL:.0e})")
    assert err <= TOL * emax
    return va


@pytest.mark.parametrize("key", mc.CASES)
def test_device_csr_equals_host_csr(key):
    if key.startswith("shuffled"):
        assert mc.built(key)["op"].brick_shape != (0, 0, 0)
    _check_against_host(key, mc.built(key)["op"].system_matrix_device())


def test_chunked_assembly(monkeypatch):
    """88 cells in chunks of 7 (the last one partial): bitwise the unchunked
    result, and on its own within the bound of the host matrix."""
    key = "re20_r0-f64-newton"
    op = mc.make_op(key)
    assert op.n_cells == 88
    monkeypatch.delenv("GLS_ASSEMBLE_CHUNK_CELLS", raising=False)
    whole = _host(op.system_matrix_device()[2])
    monkeypatch.setenv("GLS_ASSEMBLE_CHUNK_CELLS", "7")
    op.invalidate_system()
    dev = op.system_matrix_device()
    chunked = _check_against_host(key, dev, " (chunks of 7 cells)")
    assert np.array_equal(chunked, whole)
    monkeypatch.setenv("GLS_ASSEMBLE_CHUNK_CELLS", "1")
    op.invalidate_system()
    assert np.array_equal(_host(op.system_matrix_device()[2]), whole)
    import glsamd
    monkeypatch.setenv("GLS_ASSEMBLE_CHUNK_CELLS", "0")
    op.invalidate_system()
    with pytest.raises(glsamd.GlsError, match="GLS_ASSEMBLE_CHUNK_CELLS"):
        op.system_matrix_device()


@pytest.mark.parametrize("key", ["re20_r0-f64-newton", "re3900_r0-f32-newton"])
def test_repeated_assembly_is_bitwise_equal(key):
    op = mc.make_op(key)
    first = _host(op.system_matrix_device()[2])
    op.invalidate_system()
    again = _host(op.system_matrix_device()[2])
    assert np.array_equal(first, again)
    assert np.any(first != 0)


def test_invalidation():
    key = "re100_r1-f64-newton"
    case = mc.built(key)["case"]
    op = mc.make_op(key)
    raw = op.system_matrix_device_raw()
    assert op.system_matrix_device_raw() == raw  # valid: the same pointers, no assembly
    before = _host(op.system_matrix_device()[2])
    _check_against_host(key, op.system_matrix_device())
    # another linearization point: new values, again the host path's
    u2 = case.u_star * 0.5 + 0.1 * np.cos(np.arange(case.n_dofs))
    op.set_linearization_point(u2)
    dev = op.system_matrix_device()
    after = _host(dev[2])
    assert np.any(after != before)
    A2 = op.system_matrix()
    A2.sort_indices()
    emax = float(np.abs(op.element_matrices()).max())
    assert np.array_equal(_host(dev[1]), A2.indices)
    err = float(np.abs(after - A2.data).max())
    print(f"after set_linearization_point: {err / emax:.2e} max|E|")
    assert err <= TOL * emax
    # back: the first matrix bit for bit
    op.set_linearization_point(case.u_star)
    assert np.array_equal(_host(op.system_matrix_device()[2]), before)
