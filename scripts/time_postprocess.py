#!/usr/bin/env python3
"""Cost of the once-per-time-step calls on one deck / refinement:
  python scripts/time_postprocess.py [deck] [n_ref] [prec] [reps]
surface_force + probe (csrc/forces.hip) beside get_max_u and one vmult.
Every call is timed on its own between two device events on the call's
stream (the calls return synchronised, so the events bracket the kernels and
the copy back) and by the host clock around it; warm-up first, then the
median and the spread of `reps` calls.  Prints one JSON line."""
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
    prec = sys.argv[3] if len(sys.argv) > 3 else "f64"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    d = gm.read_deck(os.path.join(gm.DECK_DIR, deck))
    m = d.mesh(nref)
    cm = m.constraint_mask(*d.boundary_descriptor())
    prm, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(m.n_nodes, m.dim, d.u_max)
    op = glsamd.NavierStokesOperator(m, cm, prec)
    op.set_parameters(**prm)
    op.set_linearization_point(u)
    if prm["order"] > 0:
        op.set_previous_solution(gi.history(u, prm["order"]), w)
    cells, faces = d.cylinder_faces(m)
    op.set_force_faces(cells, faces, 3)
    found = op.set_probe_points(d.pressure_probe_points(m))
    x = op._dev(u)
    dst = op.initialize_dof_vector()

    calls = {"surface_force": lambda: op.surface_force(x),
             "probe": lambda: op.probe(x),
             "surface_force+probe": lambda: (op.surface_force(x), op.probe(x)),
             "get_max_u": lambda: op.get_max_u(x),
             "vmult": lambda: (op.vmult(dst, x), torch.cuda.synchronize())}
    out = {"deck": deck, "n_ref": nref, "precision": prec, "n_dofs": int(m.n_dofs),
           "n_cells": int(m.n_cells), "n_force_faces": int(len(cells)),
           "probe_cells_found": [int(c) for c in found], "reps": reps, "us": {}}
    for name, fn in calls.items():
        for _ in range(10):
            fn()
        dev, host = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
            dev.append(e0.elapsed_time(e1) * 1e3)
        q = lambda a, p: float(np.percentile(a, p))  # noqa: E731
        out["us"][name] = {"device_median": q(dev, 50), "device_p10": q(dev, 10),
                           "device_p90": q(dev, 90), "host_median": q(host, 50)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
