"""The host side of the device ILU(k) factorisation (csrc/ilu_plan.cc through
gls_ilu_factor_host, host only): the factor launch plan over the level
schedule of L and ilu_refactor_scheduled, the emulation of what the device
does, which must equal the row-by-row factorisation bit for bit; then the
planner under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone
program."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ilu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# name -> (matrix, fill level, atol, rtol)
CASES = {
    "tridiagonal257": (lambda: R.tridiagonal(257), 0, 1e-12, 1.0),
    "poisson12_k0": (lambda: R.poisson(12), 0, 0.0, 1.0),
    "poisson12_k1": (lambda: R.poisson(12), 1, 0.0, 1.0),
    "poisson12_k2": (lambda: R.poisson(12), 2, 0.0, 1.0),
    "block3_k1": (R.block3, 1, 1e-6, 1.0),
    "block4_3d_k1": (lambda: R.stencil_block((5, 5, 5), 4), 1, 1e-6, 1.0),
    "dirichlet_k1": (lambda: R.with_dirichlet(R.poisson(12)), 1, 1e-12, 1.0),
    "nonsymmetric_k1": (R.nonsymmetric, 1, 1e-6, 1.1),
    "diagonal5": (lambda: sp.diags([[2.0, -3.0, 0.5, 4.0, -1.5]], [0]).tocsr(), 0, 1e-12, 1.0),
}


def _clean(monkeypatch):
    for v in ("GLS_ILU_FACTOR_CHAIN", "GLS_ILU_FACTOR_NARROW", "GLS_ILU_GROUP", "GLS_ILU_CHAIN",
              "GLS_ILU_NARROW"):
        monkeypatch.delenv(v, raising=False)


def _bitwise(a, b):
    return (np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
            and np.array_equal(a.data.view(np.int64), b.data.view(np.int64)))


def _check_launches(f, chain_allowed):
    """every row in exactly one launch, after every row of its L pattern;
    the launches tile positions and levels; a wide launch holds one level"""
    L, order, level, launches = f["L"], f["order"], f["level"], f["launch"]
    n = L.shape[0]
    assert len(launches) == f["launches"]
    count = np.zeros(n, dtype=int)
    done = np.zeros(n, dtype=bool)
    pos = lev = chains = 0
    for p0, p1, l0, l1, chain in launches:
        assert p0 == pos and l0 == lev and p1 > p0 and l1 > l0
        assert chain_allowed or not chain
        assert chain or l1 == l0 + 1
        chains += int(chain)
        rows = order[p0:p1]
        count[rows] += 1
        assert level[rows].min() == l0 and level[rows].max() == l1 - 1
        assert np.all(np.diff(level[rows]) >= 0)
        for l in range(l0, l1):  # the levels in turn (a barrier between them)
            cur = rows[level[rows] == l]
            if chain:
                assert len(cur) <= f["narrow"]
            else:
                assert len(cur) > f["narrow"] or not chain_allowed
            for r in cur:
                assert np.all(done[L.indices[L.indptr[r]:L.indptr[r + 1]]]), r
            done[cur] = True
        pos, lev = p1, l1
    assert pos == n and lev == f["levels"] and chains == f["chains"]
    assert np.all(count == 1)


@pytest.mark.parametrize("name", list(CASES))
def test_scheduled_factor_is_bitwise_the_host_factor(name, monkeypatch):
    import glsamd
    _clean(monkeypatch)
    make, k, atol, rtol = CASES[name]
    A = make()
    h = glsamd.ilu_host_factor(A, k, atol, rtol)
    f = glsamd.ilu_factor_host(A, k, atol, rtol)
    assert _bitwise(f["L"], h["L"]) and _bitwise(f["U"], h["U"])
    assert f["min_pivot"] == h["min_pivot"]
    assert f["levels"] == h["levels_l"] and np.array_equal(f["level"], h["level_l"])
    assert np.array_equal(f["order"], h["order_l"])
    assert f["max_row"] == np.diff((h["L"] + h["U"]).tocsr().indptr).max()
    assert f["chain"] == 1 and f["narrow"] == f["rows"] >= 1
    assert f["group"] in (1, 2, 4, 8, 16, 32, 64) and f["rows"] * f["group"] <= 1024
    assert f["rows"] * f["max_row"] * 12 <= 64 * 1024  # the staged rows fit the LDS
    _check_launches(f, True)


@pytest.mark.parametrize("name", list(CASES))
def test_factor_launch_tuning(name, monkeypatch):
    import glsamd
    _clean(monkeypatch)
    make, k, atol, rtol = CASES[name]
    A = make()
    ref = glsamd.ilu_host_factor(A, k, atol, rtol)
    monkeypatch.setenv("GLS_ILU_FACTOR_CHAIN", "0")
    f = glsamd.ilu_factor_host(A, k, atol, rtol)
    assert f["chain"] == 0 and f["chains"] == 0 and f["launches"] == f["levels"]
    _check_launches(f, False)
    assert _bitwise(f["L"], ref["L"]) and _bitwise(f["U"], ref["U"])
    monkeypatch.setenv("GLS_ILU_FACTOR_CHAIN", "1")
    monkeypatch.setenv("GLS_ILU_FACTOR_NARROW", "1")
    f = glsamd.ilu_factor_host(A, k, atol, rtol)
    assert f["narrow"] == 1
    _check_launches(f, True)
    rows_of_level = np.bincount(f["level"], minlength=f["levels"])
    for p0, p1, l0, l1, chain in f["launch"]:
        if rows_of_level[l0] > 1:  # every level with more than one row is wide
            assert not chain and l1 == l0 + 1 and p1 - p0 == rows_of_level[l0]
        else:
            assert chain and np.all(rows_of_level[l0:l1] == 1)
    assert _bitwise(f["L"], ref["L"]) and _bitwise(f["U"], ref["U"])
    # the solves' plan is untouched by the factorisation's variables
    again = glsamd.ilu_host_factor(A, k, atol, rtol)
    assert np.array_equal(again["launch_l"], ref["launch_l"])
    assert np.array_equal(again["launch_u"], ref["launch_u"])


def test_tridiagonal_factor_is_one_chain(monkeypatch):
    import glsamd
    _clean(monkeypatch)
    f = glsamd.ilu_factor_host(R.tridiagonal(257), 0, 1e-12, 1.0)
    assert f["levels"] == 257 and f["launches"] == 1 and f["chains"] == 1 and f["max_row"] == 3


def test_forced_group_is_taken(monkeypatch):
    import glsamd
    _clean(monkeypatch)
    A = R.block3()
    free = glsamd.ilu_factor_host(A, 1, 1e-6, 1.0)
    assert free["group"] == min(64, 2 * glsamd.ilu_host_factor(A, 1, 1e-6, 1.0)["group"])
    for g in (1, 4, 64):
        monkeypatch.setenv("GLS_ILU_GROUP", str(g))
        f = glsamd.ilu_factor_host(A, 1, 1e-6, 1.0)
        assert f["group"] == g and _bitwise(f["L"], free["L"]) and _bitwise(f["U"], free["U"])


def test_unit_tridiagonal_names_row_1(monkeypatch):
    """unit diagonal, unit off-diagonals, atol 0: u_11 = 1 - 1 * 1 = 0; both
    host factorisations name that row"""
    import glsamd
    _clean(monkeypatch)
    n = 9
    A = sp.diags([np.ones(n - 1), np.ones(n), np.ones(n - 1)], [-1, 0, 1]).tocsr()
    with pytest.raises(glsamd.GlsError, match="pivot in row 1"):
        glsamd.ilu_host_factor(A, 0, 0.0, 1.0)
    with pytest.raises(glsamd.GlsError, match="pivot in row 1"):
        glsamd.ilu_factor_host(A, 0, 0.0, 1.0)
    with pytest.raises(ZeroDivisionError, match="row 1"):
        R.factor(A, 0)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_ilu_factor_plan_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ilu_factor_plan_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "dealii-ns-gls_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "ilu_factor_plan_sanitize.cc"),
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
