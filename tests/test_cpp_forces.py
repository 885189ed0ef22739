"""Drag / lift and the probe through the C++ facade (include/gls_operator.hpp)
— tests/cpp/test_forces.cc: p = x on the r0 cylinder's faces gives
F = -A_h e_x to 1e-12 (A_h from tests/forces_ref.py), the probe at (-D/2, 0)
returns p = -D/2, and surface_force before set_force_faces throws."""
import os
import subprocess

import pytest

import forces_ref as fr
import glsmesh as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "test_forces")


def test_cpp_forces_program_built():
    assert os.access(EXE, os.X_OK), "run `make cpptest` (or __graft_entry__.build())"


@pytest.mark.gpu
@pytest.mark.parametrize("dim,k", [(2, 2), (3, 2)])
def test_cpp_facade_forces(dim, k):
    A = fr.hole_measure(gm.cylinder(dim, k, 0))
    r = subprocess.run([EXE, str(dim), str(k), repr(A)], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "error path ok" in r.stdout and "0 failures" in r.stdout
