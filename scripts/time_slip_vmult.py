#!/usr/bin/env python3
"""Cost of the node constraints (no-normal-flux rows on the cylinder) on the
Re3900 deck: vmult and compute_inverse_diagonal with the cylinder no-slip
(Dirichlet mask only) against the cylinder on slip (rows: two extra launches
per vmult, dim * n_colours extra applies per diagonal), on one build; then
one V-cycle of the FP32 hierarchy r0..n_ref (10 coarse sweeps) with rows on
every level (unfused smoother) against the same hierarchy without them.

  python scripts/time_slip_vmult.py [n_ref=2] [reps=200] [windows=7]

Device events around `reps` back-to-back calls, after a warm-up; the two
operators alternate window by window and the median window is reported.
The figures are end to end: each call is enqueued from Python, so a window
holds the host's launch cost wherever the queue runs dry.
Prints one line per (precision, operator) and one per hierarchy."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-ns-gls_amd", "python"))


def window(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def main():
    import numpy as np
    import glsamd
    import glsinputs as gi
    import glsmesh as gm
    n_ref = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    name = "input_hoffmann_3D_Re3900.json"
    for prec in ("f64", "f32"):
        ops = {}
        for kind in ("noslip", "slip"):
            d = gm.read_deck(os.path.join(gm.DECK_DIR, name))
            d.no_slip_cylinder = kind == "noslip"
            m = d.mesh(n_ref)
            prm, w = d.operator_parameters(2.5e-4)
            u = gi.linearization_point(m.n_nodes, m.dim, d.u_max)
            op = glsamd.NavierStokesOperator(m, d.mask(m), prec,
                                             node_constraints=d.node_constraints(m))
            op.set_parameters(**prm)
            op.set_linearization_point(u)
            if prm["order"] > 0:
                op.set_previous_solution(gi.history(u, prm["order"]), w)
            src = op._dev(gi.src_vector(m.n_dofs))
            dst, dg = op.initialize_dof_vector(), op.initialize_dof_vector()
            ops[kind] = (op, (lambda op=op, dst=dst, src=src: op.vmult(dst, src)),
                         (lambda op=op, dg=dg: op.compute_inverse_diagonal(dg)))
        t = {(k, what): [] for k in ops for what in ("vmult", "diag")}
        for k in ops:  # warm-up
            window(ops[k][1], 20)
            window(ops[k][2], 2)
        for _ in range(windows):
            for k in ops:  # alternating
                t[(k, "vmult")].append(window(ops[k][1], reps))
                t[(k, "diag")].append(window(ops[k][2], max(1, reps // 20)))
        for k in ops:
            rows, colours = ops[k][0].n_node_constraints
            v, g = np.array(t[(k, "vmult")]), np.array(t[(k, "diag")])
            print(f"re3900 r{n_ref} {prec} {k:6s} rows {rows:5d} colours {colours:3d} "
                  f"vmult {np.median(v):8.2f} us (min {v.min():.2f} max {v.max():.2f}) "
                  f"inverse_diagonal {np.median(g):9.2f} us (min {g.min():.2f} max {g.max():.2f})",
                  flush=True)
    # one V-cycle, FP32 levels r0..n_ref, FP64 in and out
    import torch
    cyc = {}
    for kind in ("noslip", "slip"):
        d = gm.read_deck(os.path.join(gm.DECK_DIR, name))
        d.no_slip_cylinder = kind == "noslip"
        meshes = [d.mesh(r) for r in range(n_ref + 1)]
        prm, w = d.operator_parameters(2.5e-4)
        u = gi.linearization_point(meshes[-1].n_nodes, 3, d.u_max)
        mg, lops = glsamd.build_gmg(meshes, [d.mask(m) for m in meshes], prm, u,
                                    gi.history(u, prm["order"]), w, precision="f32",
                                    node_constraints=[d.node_constraints(m) for m in meshes],
                                    coarse_n_iterations=10)
        b = torch.from_numpy(gi.src_vector(meshes[-1].n_dofs)).cuda()
        x = torch.zeros_like(b)
        cyc[kind] = (mg, lops, (lambda mg=mg, x=x, b=b: mg.vcycle(x, b)))
    tv = {k: [] for k in cyc}
    for k in cyc:
        window(cyc[k][2], 10)
    for _ in range(windows):
        for k in cyc:
            tv[k].append(window(cyc[k][2], max(1, reps // 4)))
    for k in cyc:
        v = np.array(tv[k])
        rows = [op.n_node_constraints[0] for op in cyc[k][1]]
        print(f"re3900 r0..r{n_ref} f32 {k:6s} rows per level {rows} vcycle {np.median(v):8.2f} us "
              f"(min {v.min():.2f} max {v.max():.2f})", flush=True)


if __name__ == "__main__":
    main()
