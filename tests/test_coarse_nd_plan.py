"""The nested-dissection plan of the "nd" direct coarse solver
(csrc/coarse_nd.cc through gls_nd_plan_*, host only): the tree's invariants
on the decks' coarse meshes, the storage it promises, the algebra of the two
sweeps over it (tests/nd_ref.py against numpy.linalg.solve) and the planner
under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import nd_ref
from helpers import deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

DECK_MESHES = {
    "re3900_r0": ("input_hoffmann_3D_Re3900.json", 0),
    "turek3d_r0": ("input_turek_3D_Re100.json", 0),
    "turek2d_re100_r1": ("input_turek_2D_Re100.json", 1),
    "turek2d_re20_r1": ("input_turek_2D_Re20_stat.json", 1),
}


def _deck_mesh(key, shuffled=False):
    name, r = DECK_MESHES[key]
    d = deck(name)
    m = d.mesh(r)
    if shuffled:
        from shuffle import ShuffledMesh
        m = ShuffledMesh(m, seed=11)
    vel, p, slip = d.boundary_descriptor()
    cm = m.constraint_mask(vel, p, slip)
    cn = np.asarray(m.cell_nodes).reshape(m.n_cells, -1)
    return cn, nd_ref.node_dof_counts(m, cm)


def _strip(n, first_node):
    """n Q1 quads in a row on nodes of their own."""
    c = np.arange(n)
    return np.stack([2 * c, 2 * c + 2, 2 * c + 1, 2 * c + 3], axis=1) + first_node


MESHES = list(DECK_MESHES) + ["re3900_r0_shuffled", "one_cell", "single_tree_node",
                              "single_tree_node_more", "two_groups"]


def _mesh_case(name):
    """(cell -> node table, dofs per node, max_leaf_cells)"""
    if name in DECK_MESHES:
        return _deck_mesh(name) + (25 if "3d" in name or "3900" in name else 20,)
    if name == "re3900_r0_shuffled":
        return _deck_mesh("re3900_r0", shuffled=True) + (25,)
    if name == "one_cell":
        return np.array([[0, 1, 2, 3]]), np.full(4, 3, np.int32), 4
    if name.startswith("single_tree_node"):  # max_leaf_cells >= n_cells
        cn, w = _deck_mesh("turek2d_re20_r1")
        return cn, w, cn.shape[0] + (7 if name.endswith("more") else 0)
    assert name == "two_groups"  # two disconnected strips
    return np.concatenate([_strip(9, 0), _strip(14, 20)]), np.full(50, 2, np.int32), 3


def _plan(cn, w, leaf):
    import glsamd
    return glsamd.NdPlan(cn, w, leaf)


@pytest.mark.parametrize("name", MESHES)
def test_plan_invariants(name):
    cn, w, leaf = _mesh_case(name)
    plan = _plan(cn, w, leaf)
    nodes = plan.nodes
    nf = int(np.sum(w))
    assert plan.info["n_dofs"] == nf and plan.info["sum_own"] == nf
    # the tree: root first, levels, two children or none, leaves within the cap
    assert nodes[0]["parent"] == -1 and nodes[0]["level"] == 0
    cell_leaf = -np.ones(cn.shape[0], dtype=np.int64)
    for t, nd in enumerate(nodes):
        c0, c1 = nd["child"]
        assert (c0 < 0) == (c1 < 0)
        if c0 >= 0:
            assert len(nd["cells"]) == 0
            for c in (c0, c1):
                assert nodes[c]["parent"] == t and nodes[c]["level"] == nd["level"] + 1
        else:
            assert 1 <= len(nd["cells"]) <= max(leaf, 1)
            assert np.all(cell_leaf[nd["cells"]] == -1)
            cell_leaf[nd["cells"]] = t
    assert np.all(cell_leaf >= 0)
    assert plan.info["depth"] == 1 + max(nd["level"] for nd in nodes)
    if leaf >= cn.shape[0]:
        assert len(nodes) == 1 and len(nodes[0]["own"]) == nf and len(nodes[0]["boundary"]) == 0
    else:
        assert plan.info["depth"] >= 2
    # every participating dof is owned exactly once
    own = np.concatenate([nd["own"] for nd in nodes])
    assert np.array_equal(np.sort(own), np.arange(nf))
    owner = np.empty(nf, dtype=np.int64)
    for t, nd in enumerate(nodes):
        owner[nd["own"]] = t
        assert np.all(np.diff(nd["own"]) > 0) and np.all(np.diff(nd["boundary"]) > 0)

    def path(t):  # t, its parent, ..., the root
        out = []
        while t >= 0:
            out.append(t)
            t = nodes[t]["parent"]
        return out

    # a cell's dofs are owned on its leaf's path to the root; B_t is exactly
    # the ancestors' dofs in the cells of t's subtree
    cd = nd_ref.plan_cell_dofs(cn, w)
    expect_b = [set() for _ in nodes]
    for c in range(cn.shape[0]):
        pth = path(int(cell_leaf[c]))
        for d in cd[c][cd[c] >= 0]:
            o = int(owner[d])
            assert o in pth, (c, d, o)
            for u in pth[:pth.index(o)]:
                expect_b[u].add(int(d))
    for t, nd in enumerate(nodes):
        assert sorted(expect_b[t]) == nd["boundary"].tolist(), t
    # extend-add maps
    for t, nd in enumerate(nodes):
        if t == 0:
            assert len(nd["boundary"]) == 0
            continue
        p = nodes[nd["parent"]]
        both = np.concatenate([p["own"], p["boundary"]])
        assert np.array_equal(both[nd["map"]], nd["boundary"])
        assert len(set(nd["map"].tolist())) == len(nd["map"])
    # statistics
    st = sum(len(nd["own"]) ** 2 + 2 * len(nd["own"]) * len(nd["boundary"]) for nd in nodes)
    assert plan.info["stored_entries"] == st
    assert plan.info["max_own"] == max(len(nd["own"]) for nd in nodes)
    assert plan.info["max_boundary"] == max(len(nd["boundary"]) for nd in nodes)
    # deterministic
    again = _plan(cn, w, leaf)
    assert again.info == plan.info
    for a, b in zip(again.nodes, nodes):
        assert a["parent"] == b["parent"] and a["child"] == b["child"]
        for k in ("own", "boundary", "map", "cells"):
            assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("key", list(DECK_MESHES))
def test_plan_storage(key):
    """Stored entries (sum of |I|^2 + 2 |I| |B|) at 50 cells per leaf: at
    most a quarter of the dense block (counted 0.16 - 0.18 with the plain
    bisection; a degenerate tree -- everything in the root -- gives 1)."""
    cn, w = _deck_mesh(key)
    plan = _plan(cn, w, 50)
    nf = int(np.sum(w))
    frac = plan.info["stored_entries"] / nf ** 2
    print(f"{key}: nf {nf}, {plan.info['tree_nodes']} tree nodes, depth {plan.info['depth']}, "
          f"stored {plan.info['stored_entries']} = {frac:.3f} nf^2, max |I| "
          f"{plan.info['max_own']}, max |B| {plan.info['max_boundary']}")
    assert frac <= 0.25


@pytest.mark.parametrize("leaf", [6, 20])
def test_sweeps_solve_the_system(leaf):
    """The forward / backward sweeps over the library's plan solve a random
    strictly diagonally dominant matrix with Turek-2D r1's cell sparsity to
    1e-10 of numpy.linalg.solve: the boundary sets capture all the fill."""
    cn, w = _deck_mesh("turek2d_re100_r1")
    plan = _plan(cn, w, leaf)
    assert plan.info["depth"] >= 3
    cd = nd_ref.plan_cell_dofs(cn, w)
    nloc = cd.shape[1]
    rng = np.random.default_rng(3)
    E = rng.uniform(-1.0, 1.0, (cn.shape[0], nloc, nloc))
    E[:, np.arange(nloc), np.arange(nloc)] = nloc + 1.0
    nf = int(np.sum(w))
    A = np.zeros((nf, nf))
    for c in range(cn.shape[0]):
        loc = np.nonzero(cd[c] >= 0)[0]
        A[np.ix_(cd[c][loc], cd[c][loc])] += E[c][np.ix_(loc, loc)]
    b = rng.standard_normal(nf)
    fac = nd_ref.factor(plan, nd_ref.leaf_fronts(plan, cd, E))
    x = nd_ref.solve(plan, fac, b)
    ref = np.linalg.solve(A, b)
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print(f"leaf {leaf}: depth {plan.info['depth']}, sweeps vs numpy.linalg.solve {err:.2e}")
    assert err < 1e-10


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")
def test_plan_asan_ubsan(tmp_path):
    exe = str(tmp_path / "coarse_nd_sanitize")
    cmd = [CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "dealii-ns-gls_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "coarse_nd_sanitize.cc"),
           os.path.join(ROOT, "dealii-ns-gls_amd", "csrc", "coarse_nd.cc"), "-o", exe]
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
