"""The host least squares of the device GMRES solvers (csrc/hessenberg.h:
gls::HessenbergLsq, shared by krylov.hip, mg.hip and dist_mg.hip) as a
stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/cpp/hessenberg_sanitize.cc: the estimate against the direct residual,
incremental against re-factorised bitwise, lucky breakdown, the identity
rotation), and its printed matrices and solutions against numpy: the
matrices are well conditioned (cond < 1e4), so the Givens QR's y agrees with
numpy.linalg.lstsq to 1e-10 relative."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _floats(line):
    return np.array([float.fromhex(t) for t in line.split()[1:]])


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_hessenberg_asan_ubsan(tmp_path):
    exe = str(tmp_path / "hessenberg_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "dealii-ns-gls_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "hessenberg_sanitize.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "0 failures" in out and "FAIL" not in out, out[-3000:]
    lines = r.stdout.splitlines()
    cases = [i for i, l in enumerate(lines) if l.startswith("CASE ")]
    # 4 seeds x 5 lengths, 3 breakdowns
    assert len(cases) == 23
    seen = set()
    for i in cases:
        _, name, jd, g0 = lines[i].split()
        jd, g0 = int(jd), float.fromhex(g0)
        seen.add(jd)
        H = _floats(lines[i + 1]).reshape(jd + 1, jd)
        y = _floats(lines[i + 2])
        assert y.shape == (jd,)
        # the generator: sub-diagonal in [0.5, 1.5] (0 at a breakdown), upper
        # Hessenberg
        assert np.all(np.tril(H, -2) == 0)
        sub = np.diag(H, -1)
        assert np.all((sub[:-1] >= 0.5) & (sub[:-1] <= 1.5))
        assert sub[-1] == 0 if name.startswith("breakdown") else 0.5 <= sub[-1] <= 1.5
        cond = np.linalg.cond(H)
        rhs = np.zeros(jd + 1)
        rhs[0] = g0
        ref = np.linalg.lstsq(H, rhs, rcond=None)[0]
        err = np.linalg.norm(y - ref) / np.linalg.norm(ref)
        print(f"{name}: cond {cond:.1f}, y vs lstsq {err:.1e}")
        assert cond < 1e4, (name, cond)
        assert err < 1e-10, (name, err)
    assert {1, 28} <= seen
