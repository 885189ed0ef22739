"""Periodic node identification, host side (gls_mesh_periodic_nodes,
Mesh.periodic_nodes, the Deck's "simulation use wall bc periodic") and the
numpy reference tests/periodic_ref.py against a dense C^T A C.

Pair counts on the generator's cylinder meshes: 85 / 169 node pairs on ids
3/4 in 2D Q2 r1 / r2, 1,649 (3/4) and 1,728 (5/6) in 3D Q2 r1."""
import json
import os
import subprocess

import numpy as np
import pytest

import glsmesh as gm
import periodic_ref as pr
from helpers import deck, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _check_map(mesh, master, pairs):
    n = mesh.n_nodes
    assert master.shape == (n,) and master.dtype == np.int64
    assert np.array_equal(master[master], master)  # idempotent
    slaves = np.nonzero(master != np.arange(n))[0]
    elim = np.zeros(n, dtype=bool)
    for _, b, _ in pairs:
        elim |= ((mesh.node_boundary >> b) & 1).astype(bool)
    assert np.array_equal(slaves, np.nonzero(elim)[0])  # exactly the id_b sides
    fixed = [d for d in range(mesh.dim) if d not in [p[2] for p in pairs]]
    ext = np.ptp(mesh.coords, axis=0).max()
    diff = np.abs(mesh.coords[slaves] - mesh.coords[master[slaves]])
    assert diff[:, fixed].max(initial=0.0) <= 1e-9 * ext
    return slaves


@pytest.mark.parametrize("dim,n_ref,pairs,count", [
    (2, 1, [(3, 4, 1)], 85), (2, 2, [(3, 4, 1)], 169),
    (3, 1, [(3, 4, 1)], 1649), (3, 1, [(5, 6, 2)], 1728)])
def test_cylinder_pair_counts(dim, n_ref, pairs, count):
    mesh = gm.cylinder(dim, 2, n_ref)
    master = mesh.periodic_nodes(pairs)
    slaves = _check_map(mesh, master, pairs)
    assert len(slaves) == count
    # the masters lie on id_a
    assert np.all((mesh.node_boundary[master[slaves]] >> pairs[0][0]) & 1)


def test_chains_on_3d_edges():
    mesh = gm.cylinder(3, 2, 1)
    pairs = [(3, 4, 1), (5, 6, 2)]
    master = mesh.periodic_nodes(pairs)
    slaves = _check_map(mesh, master, pairs)
    on = lambda b: ((mesh.node_boundary >> b) & 1).astype(bool)
    assert len(slaves) == 1649 + 1728 - (on(4) & on(6)).sum()
    # a node of the edge y-bottom / z-bottom is the master of four nodes
    edge = np.nonzero(on(3) & on(5))[0]
    assert len(edge) > 0
    size = np.bincount(master, minlength=mesh.n_nodes)
    assert np.all(size[edge] == 4)
    for e in edge[:3]:
        grp = np.nonzero(master == e)[0]
        x = mesh.coords[grp]
        assert np.ptp(x[:, 0]) <= 1e-12
        assert len(np.unique(np.round(x[:, 1:], 9), axis=0)) == 4
    # the order of the pairs does not change the groups
    other = mesh.periodic_nodes(pairs[::-1])
    assert np.array_equal(other, master)


@pytest.mark.parametrize("dims,degree,periodic,n_slaves", [
    ((2, 2), 1, "y", 5), ((2, 1), 2, "y", 9), ((2, 2, 1), 2, "z", 81),
    ((2, 2, 2), 2, "yz", 2 * 81 - 9)])
def test_boxes(dims, degree, periodic, n_slaves):
    mesh = pr.box(dims, degree, 1)
    if dims == (2, 2, 1):
        assert (mesh.n_cells, mesh.n_nodes, mesh.brick()) == (32, 405, (2, 2, 2))
    master = mesh.periodic_nodes(pr.PAIRS[periodic])
    slaves = _check_map(mesh, master, pr.PAIRS[periodic])
    assert len(slaves) == n_slaves
    if periodic == "yz":
        assert np.bincount(master).max() == 4


def test_free_nodes_and_no_pairs():
    mesh = gm.cylinder(2, 1, 0)
    assert np.array_equal(mesh.periodic_nodes([]), np.arange(mesh.n_nodes))


def test_errors():
    mesh = gm.cylinder(2, 2, 1)
    with pytest.raises(RuntimeError, match="direction out of range"):
        mesh.periodic_nodes([(3, 4, 2)])
    with pytest.raises(RuntimeError, match="direction out of range"):
        mesh.periodic_nodes([(3, 4, -1)])
    with pytest.raises(RuntimeError, match=r"boundary id 2 has a curved or oblique face"):
        mesh.periodic_nodes([(2, 4, 1)])
    with pytest.raises(RuntimeError, match=r"\d+ nodes on id 0 but \d+ on id 4"):
        mesh.periodic_nodes([(0, 4, 1)])
    with pytest.raises(RuntimeError, match=r"node \d+ on id 4 has no partner on id 3"):
        mesh.periodic_nodes([(3, 4, 0)])
    with pytest.raises(RuntimeError, match="two different ids"):
        mesh.periodic_nodes([(3, 3, 1)])
    # equal counts, no partner: the inflow against the outflow in y
    assert ((mesh.node_boundary >> 0) & 1).sum() == ((mesh.node_boundary >> 1) & 1).sum()
    with pytest.raises(RuntimeError, match="has no partner"):
        mesh.periodic_nodes([(0, 1, 1)])


def test_deck_flag(tmp_path):
    name = "input_hoffmann_3D_Re3900.json"
    d = deck(name)
    assert not d.wall_bc_periodic and d.periodic_bcs() == []
    mesh = d.mesh(0)
    assert d.node_master(mesh) is None
    before = d.boundary_descriptor()
    raw = dict(d.raw)
    raw["simulation use wall bc periodic"] = True
    path = tmp_path / "periodic.json"
    path.write_text(json.dumps(raw))
    p = gm.read_deck(str(path))
    assert p.wall_bc_periodic
    assert p.periodic_bcs() == [(3, 4, 1), (5, 6, 2)]
    vel, pres, slip = p.boundary_descriptor()
    walls = set(range(3, 3 + 2 * d.dim))  # every id the non-periodic branch lists
    assert not walls & set(vel) and not walls & set(slip)  # simulation.cc:406-422
    assert [i for i in before[0] + before[2] if i not in walls] == vel + slip
    assert pres == before[1]
    master = p.node_master(mesh)
    assert np.array_equal(master, mesh.periodic_nodes([(3, 4, 1), (5, 6, 2)]))
    d2 = deck("input_turek_2D_Re100.json")
    d2.wall_bc_periodic = True
    assert d2.periodic_bcs() == [(3, 4, 1)]
    # rows on slave nodes are dropped: the cylinder touches no wall, so all stay
    d2.no_slip_cylinder = False
    m2 = d2.mesh(0)
    nodes, comp, coef = d2.node_constraints(m2)
    assert len(nodes) == len(m2.node_constraints([2])[0]) > 0 and np.all(d2.node_master(m2)[nodes] == nodes)
    with pytest.raises(NotImplementedError):
        p.node_master(gm.IsoQ1Mesh(mesh))


def test_reference_against_dense():
    """periodic_ref.vmult / diagonal equal the dense C^T A C assembled from the
    oracle's cell matrices (1e-12: summation order only)."""
    case = pr.box_case((2, 2), 1, 1, "y")
    o = pr.oracle(case)
    pm = case.pm
    M = pr.dense_constrained(o, case.mesh, pm)
    x = case.src
    assert rel_err(pr.vmult(o, pm, x), M @ x) < 1e-12
    assert rel_err(pr.diagonal(o, pm), np.diag(M)) < 1e-12
    s = pm.sdofs
    assert np.all(M[s, s] == 1.0) and np.abs(M[s]).sum() == len(s)
    assert np.abs(pr.sparse_constrained(o, case.mesh, pm).toarray() - M).max() <= 1e-12 * np.abs(M).max()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_periodic_nodes_asan_ubsan(tmp_path):
    exe = str(tmp_path / "periodic_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "periodic_sanitize.cc"),
           os.path.join(ROOT, "dealii-ns-gls_amd", "host", "mesh.cc"), "-o", exe]
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
