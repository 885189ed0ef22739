#!/usr/bin/env python3
"""The two forms of the direct coarse solver side by side in one process:
  python scripts/time_coarse_direct.py [deck] [n_ref] [leaves] [reps] [iso_q1] [nt]
dense and nested dissection ("nd", one object per leaf size in `leaves`, a
comma-separated list; 0 = the library's default) on the hierarchy r0..n_ref,
FP32 levels.  Per solver: the setup (wall ms of mg.setup() re-run on the
built hierarchy, median of 5, and the library's own split), the coarse solve
alone (a one-level multigrid on the coarse operator, FP32 in / out) and the
whole V-cycle.  Solves and V-cycles are timed between two device events each,
after a warm-up, the solvers alternating call by call; median and p10 / p90
of `reps` calls.  iso_q1 = 1: the coarsest level as FE_Q_iso_Q1 (the sphere
deck), where the dense solver refuses the size and is left out.  nt = 1: beside
every nd solver (non-temporal factor loads, the default) one with cacheable
loads (GLS_COARSE_ND_NT=0, read when the solver is created), named *_cached.
Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-ns-gls_amd", "python"))


def main():
    import numpy as np
    import torch
    import glsamd
    import glsinputs as gi
    import glsmesh as gm
    deck = sys.argv[1] if len(sys.argv) > 1 else "input_hoffmann_3D_Re3900.json"
    nref = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    leaves = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "13,25,50,100").split(",")]
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    iso = len(sys.argv) > 5 and sys.argv[5] == "1"
    nt = len(sys.argv) > 6 and sys.argv[6] == "1"
    d = gm.read_deck(os.path.join(gm.DECK_DIR, deck))
    meshes = [d.mesh(r) for r in range(nref + 1)]
    cm = [m.constraint_mask(*d.boundary_descriptor()) for m in meshes]
    prm, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, prm["order"])

    solvers = ([] if iso else [("dense", {})]) + [
        (f"nd{leaf}", dict(coarse_direct="nd", coarse_leaf_cells=leaf or None)) for leaf in leaves]
    if nt:
        solvers += [(n + "_cached", kw) for n, kw in solvers if n != "dense"]
    built = {}
    for name, kw in solvers:
        os.environ["GLS_COARSE_ND_NT"] = "0" if name.endswith("_cached") else "1"
        mg, ops = glsamd.build_gmg(meshes, cm, prm, u, hist, w, precision="f32",
                                   coarse_iso_q1=iso, coarse_n_iterations=-1, **kw)
        one = glsamd.Multigrid([ops[0]], [], coarse_n_iterations=-1, outer_precision="f32", **kw)
        one.setup()
        built[name] = (mg, ops, one)
    n_fine, n_coarse = meshes[-1].n_dofs, built[solvers[0][0]][1][0].n_dofs
    b = torch.from_numpy(gi.src_vector(n_fine)).cuda()
    x = torch.zeros_like(b)
    bc = torch.from_numpy(gi.src_vector(n_coarse)).cuda().float()
    xc = torch.zeros_like(bc)

    out = {"deck": deck, "n_ref": nref, "iso_q1": iso, "n_dofs": int(n_fine),
           "n_coarse_dofs": int(n_coarse), "reps": reps, "solvers": {}}
    q = lambda a, p: float(np.percentile(a, p))  # noqa: E731
    for name, (mg, ops, one) in built.items():
        wall = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mg.setup()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["solvers"][name] = {"setup_wall_ms_median": q(wall, 50), "info": mg.coarse_direct_info()}
        if name == "dense":
            out["solvers"][name]["dense_setup"] = mg.coarse_setup_times()
    calls = {"coarse_solve_us": lambda m: m[2].vcycle(xc, bc), "vcycle_us": lambda m: m[0].vcycle(x, b)}
    for what, fn in calls.items():
        for m in built.values():
            for _ in range(10):
                fn(m)
        dev = {name: [] for name in built}
        for _ in range(reps):
            for name, m in built.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn(m)
                e1.record()
                torch.cuda.synchronize()
                dev[name].append(e0.elapsed_time(e1) * 1e3)
        for name in built:
            out["solvers"][name][what] = {"median": q(dev[name], 50), "p10": q(dev[name], 10),
                                          "p90": q(dev[name], 90)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
