"""The ILU(k) host plan (csrc/ilu_plan.cc through gls_ilu_host_factor, host
only) against tests/ilu_ref.py: the restatement's known answers, then the
library's pattern, values, row levels and launch plan on the same matrices,
the error paths, and the planner under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import glsinputs as gi
import ilu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _stationary_iteration(A, M, b, n):
    x = np.zeros_like(b)
    res = []
    for _ in range(n):
        x = x + M.vmult(b - A @ x)
        res.append(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    return res


# ---- the restatement's known answers
def test_ref_tridiagonal_is_exact():
    A = R.tridiagonal(37)
    L, U = R.factor(A, 0)
    x = gi.rnd(1, 37)
    got = R.solve(L, U, A @ x)
    assert np.max(np.abs(got - x)) / np.max(np.abs(x)) < 1e-13


def test_ref_full_fill_is_exact():
    A = R.poisson(5)
    L, U = R.factor(A, A.shape[0])
    x = gi.rnd(2, A.shape[0])
    assert np.max(np.abs(R.solve(L, U, A @ x) - x)) < 1e-13
    full = (L + sp.identity(25)) @ U
    assert abs(full - A).max() < 1e-13


@pytest.mark.parametrize("m", [6, 12])
def test_ref_poisson_fill_and_levels(m):
    A = R.poisson(m)
    for k, n_levels in ((0, 2 * m - 1), (1, 3 * m - 2), (2, 4 * m - 3)):
        L, U = R.factor(A, k)
        if k == 0:
            assert L.nnz + U.nnz == A.nnz
        if k == 1:
            assert L.nnz + U.nnz - A.nnz == 2 * (m - 1) ** 2
        ll, lu = R.levels(L, U)
        assert ll.max() + 1 == n_levels and lu.max() + 1 == n_levels


def test_ref_block3_levels():
    A = R.block3()
    assert A.shape[0] == 432
    for k, n_levels in ((0, 69), (1, 102)):
        ll, lu = R.levels(*R.factor(A, k))
        assert ll.max() + 1 == n_levels and lu.max() + 1 == n_levels


def test_ref_amg_ilu_poisson_converges():
    """AMG with ILU(1) smoothing and an ILU(1) coarsest solve as a stationary
    iteration on Poisson: the criterion of test_ref_poisson_converges."""
    A = R.poisson(40)
    M = R.AMGRefILU(A, block_size=1, threshold=0.0, coarse_max_size=100)
    assert M.info()["levels"] >= 2
    res = _stationary_iteration(A, M, gi.rnd(3, A.shape[0]), 8)
    assert res[-1] < 1e-3 and res[-1] / res[-2] < 0.5


# ---- the library's plan against the restatement
CASES = {
    "poisson12_k0": (lambda: R.poisson(12), 0, 0.0, 1.0),
    "poisson12_k1": (lambda: R.poisson(12), 1, 0.0, 1.0),
    "poisson12_k2": (lambda: R.poisson(12), 2, 0.0, 1.0),
    "block3_k0": (R.block3, 0, 1e-12, 1.0),
    "block3_k1": (R.block3, 1, 1e-6, 1.0),
    "dirichlet_k1": (lambda: R.with_dirichlet(R.poisson(12)), 1, 1e-12, 1.0),
    "nonsymmetric_k1": (R.nonsymmetric, 1, 1e-6, 1.1),
}


def _same_pattern(a, b):
    return np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


@pytest.mark.parametrize("name", list(CASES))
def test_host_factor_equals_restatement(name):
    import glsamd
    make, k, atol, rtol = CASES[name]
    A = make()
    L, U = R.factor(A, k, atol, rtol)
    b = gi.rnd(4, A.shape[0])
    h = glsamd.ilu_host_factor(A, k, atol, rtol, solve=b)
    assert _same_pattern(h["L"], L) and _same_pattern(h["U"], U)
    for got, ref in ((h["L"], L), (h["U"], U)):
        if ref.nnz:
            assert np.max(np.abs(got.data - ref.data) / np.maximum(np.abs(ref.data), 1e-300)) < 1e-13
    ll, lu = R.levels(L, U)
    assert np.array_equal(h["level_l"], ll) and np.array_equal(h["level_u"], lu)
    assert h["levels_l"] == ll.max() + 1 and h["levels_u"] == lu.max() + 1
    assert abs(h["min_pivot"] - np.min(np.abs(U.diagonal()))) <= 1e-13 * h["min_pivot"]
    ref = R.solve(L, U, b)
    assert np.linalg.norm(h["solve"] - ref) / np.linalg.norm(ref) < 1e-12


def test_host_factor_diagonal_modification_sign():
    """rtol a_ii + sign(a_ii) atol: negative diagonals move away from zero too"""
    import glsamd
    A = sp.diags([[-2.0, 3.0, -0.5, 4.0]], [0]).tocsr()
    h = glsamd.ilu_host_factor(A, 0, 0.25, 1.5)
    assert np.allclose(h["U"].diagonal(), [-3.25, 4.75, -1.0, 6.25], rtol=0, atol=1e-15)


def _check_schedule(h, which, chain_allowed):
    T = h["L" if which == "l" else "U"]
    order, level, launches = h["order_" + which], h["level_" + which], h["launch_" + which]
    n = T.shape[0]
    assert np.array_equal(np.sort(order), np.arange(n))  # every row exactly once
    done = np.zeros(n, dtype=bool)
    pos = lev = 0
    for p0, p1, l0, l1, chain in launches:
        assert p0 == pos and l0 == lev and p1 > p0 and l1 > l0
        assert chain_allowed or not chain
        assert chain or l1 == l0 + 1  # a wide launch holds one level
        rows = order[p0:p1]
        assert level[rows].min() == l0 and level[rows].max() == l1 - 1
        assert np.all(np.diff(level[rows]) >= 0)  # level by level
        for l in range(l0, l1):  # the levels in turn (a barrier between them)
            cur = rows[level[rows] == l]
            if chain:
                assert len(cur) <= h["narrow"]
            for r in cur:
                dep = T.indices[T.indptr[r]:T.indptr[r + 1]]
                dep = dep[dep != r]
                assert np.all(done[dep]), (which, r)
            done[cur] = True
        pos, lev = p1, l1
    assert pos == n and lev == h["levels_" + which]


@pytest.mark.parametrize("chain", ["1", "0"])
@pytest.mark.parametrize("name", ["poisson12_k1", "block3_k1", "dirichlet_k1", "nonsymmetric_k1"])
def test_launch_plan(name, chain, monkeypatch):
    import glsamd
    monkeypatch.setenv("GLS_ILU_CHAIN", chain)
    if name == "dirichlet_k1":
        monkeypatch.setenv("GLS_ILU_NARROW", "16")  # a wide first level, then chains
    make, k, atol, rtol = CASES[name]
    h = glsamd.ilu_host_factor(make(), k, atol, rtol)
    assert h["chain"] == int(chain)
    for which in "lu":
        _check_schedule(h, which, chain == "1")
        if chain == "0":
            assert h["launches_" + which] == h["levels_" + which]
        else:
            assert h["launches_" + which] < h["levels_" + which]
    if name == "dirichlet_k1" and chain == "1":
        assert h["launch_l"][0][4] == 0 and h["launch_l"][1][4] == 1


def test_tridiagonal_is_one_chain(monkeypatch):
    import glsamd
    monkeypatch.delenv("GLS_ILU_CHAIN", raising=False)
    h = glsamd.ilu_host_factor(R.tridiagonal(257), 0, 0.0, 1.0)
    assert h["levels_l"] == 257 and h["launches_l"] == 1 and h["launches_u"] == 1
    assert h["group"] == 4  # the smallest group for one entry per row


def test_deck_helpers():
    from helpers import deck
    d = deck("input_turek_2D_Re20_stat.json")
    assert d.amg_ilu_parameters() == dict(smoother_ilu=True, coarse_ilu=True, fill_level=1,
                                          atol=1e-6, rtol=1.0)
    assert d.coarse_ilu_parameters() is None
    d.raw["gmg coarse grid solver"] = "ILU"
    assert d.coarse_ilu_parameters() == dict(fill_level=0, atol=1e-12, rtol=1.0)
    assert deck("input_turek_2D_Re100.json").amg_ilu_parameters() is None


# ---- error paths (the raw entry point: the Python wrapper sorts columns)
def _raw(n, rp, ci, va, k=0, atol=0.0, rtol=1.0):
    import glsamd
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    va = np.asarray(va, np.float64)
    prm = glsamd.ILUParams(k, atol, rtol)
    f = glsamd.ILUHostFactor()
    rc = glsamd.lib().gls_ilu_host_factor(n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data,
                                          C.byref(prm), C.byref(f))
    return rc, glsamd.lib().gls_last_error().decode()


def test_zero_pivot_names_the_row():
    A = sp.csr_matrix(np.array([[2.0, 1.0, 0.0], [4.0, 2.0, 1.0], [0.0, 1.0, 3.0]]))
    rc, msg = _raw(3, A.indptr, A.indices, A.data)
    assert rc != 0 and "pivot" in msg and "row 1" in msg
    with pytest.raises(ZeroDivisionError, match="row 1"):
        R.factor(A, 0)
    # the same matrix with atol: no error
    rc, msg = _raw(3, A.indptr, A.indices, A.data, atol=1e-6)
    assert rc == 0, msg


def test_unsorted_columns_and_empty_matrix_refused():
    rc, msg = _raw(2, [0, 2, 4], [1, 0, 0, 1], [1.0, 2.0, 1.0, 2.0])
    assert rc != 0 and "not sorted" in msg
    rc, msg = _raw(2, [0, 2, 4], [0, 0, 0, 1], [1.0, 2.0, 1.0, 2.0])
    assert rc != 0 and "not sorted" in msg  # a repeated column
    rc, msg = _raw(0, [0], [], [])
    assert rc != 0 and "empty" in msg
    rc, msg = _raw(2, [0, 1, 2], [0, 5], [1.0, 1.0])
    assert rc != 0 and "out of range" in msg


def test_scipy_spilu_agrees_where_ilu_is_exact():
    """an outside check of the restatement itself: with full fill it equals
    scipy's sparse LU solve on a nonsymmetric matrix"""
    A = R.nonsymmetric(40)
    L, U = R.factor(A, 40)
    b = gi.rnd(6, 40)
    ref = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(R.solve(L, U, b) - ref) / np.linalg.norm(ref) < 1e-11


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_ilu_plan_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ilu_plan_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "dealii-ns-gls_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "ilu_plan_sanitize.cc"),
           os.path.join(ROOT, "dealii-ns-gls_amd", "csrc", "ilu_plan.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    print(out)
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "0 failures" in out
