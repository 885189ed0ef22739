"""The kernel-instantiation dispatch of the host code (csrc/dispatch.h:
gls::with_real, gls::with_dim_degree, gls::with_int) as a stand-alone program
under AddressSanitizer + UndefinedBehaviorSanitizer (tests/cpp/
dispatch_check.cc): both precisions reach their type, each of the six
supported (dim, degree) pairs its own tags, the degree-capped form refuses
Q3, unsupported values throw a runtime_error naming the caller, and a
visitor's return value is passed through."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_dispatch_asan_ubsan(tmp_path):
    exe = str(tmp_path / "dispatch_check")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "dealii-ns-gls_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "dispatch_check.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert "0 failures" in out and "FAIL" not in out, out[-3000:]
