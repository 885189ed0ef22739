#!/usr/bin/env python3
"""Cost of periodic walls (glsOpDesc.node_master) on the Re3900 deck: vmult
with the deck's slip walls (components of the Dirichlet mask) against the
walls periodic ("simulation use wall bc periodic": the same kernels over a
brick plan with more shared nodes), on one build; then one V-cycle of the FP32
hierarchy r0..n_ref (10 coarse sweeps) with the map on every level against the
same hierarchy without it.

  python scripts/time_periodic_vmult.py [n_ref=2] [reps=200] [windows=7]

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


def deck(kind):
    import glsmesh as gm
    d = gm.read_deck(os.path.join(gm.DECK_DIR, "input_hoffmann_3D_Re3900.json"))
    d.wall_bc_periodic = kind == "periodic"
    return d


def main():
    import numpy as np
    import torch
    import glsamd
    import glsinputs as gi
    n_ref = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    kinds = ("walls", "periodic")
    for prec in ("f64", "f32"):
        ops = {}
        for kind in kinds:
            d = deck(kind)
            m = d.mesh(n_ref)
            prm, w = d.operator_parameters(2.5e-4)
            u = gi.linearization_point(m.n_nodes, m.dim, d.u_max)
            nm = d.node_master(m)
            op = glsamd.NavierStokesOperator(m, d.mask(m), prec, node_master=nm)
            op.set_parameters(**prm)
            op.set_linearization_point(u)
            if prm["order"] > 0:
                op.set_previous_solution(gi.history(u, prm["order"]), w)
            src = op._dev(gi.src_vector(m.n_dofs))
            dst = op.initialize_dof_vector()
            slaves = 0 if nm is None else int((nm != np.arange(len(nm))).sum())
            ops[kind] = (op, (lambda op=op, dst=dst, src=src: op.vmult(dst, src)), slaves)
        t = {k: [] for k in ops}
        for k in ops:  # warm-up
            window(ops[k][1], 20)
        for _ in range(windows):
            for k in ops:  # alternating
                t[k].append(window(ops[k][1], reps))
        for k in ops:
            v = np.array(t[k])
            print(f"re3900 r{n_ref} {prec} {k:8s} slaves {ops[k][2]:6d} brick {ops[k][0].brick_shape} "
                  f"vmult {np.median(v):8.2f} us (min {v.min():.2f} max {v.max():.2f})", flush=True)
    # one V-cycle, FP32 levels r0..n_ref, FP64 in and out
    cyc = {}
    for kind in kinds:
        d = deck(kind)
        meshes = [d.mesh(r) for r in range(n_ref + 1)]
        prm, w = d.operator_parameters(2.5e-4)
        u = gi.linearization_point(meshes[-1].n_nodes, 3, d.u_max)
        mg, lops = glsamd.build_gmg(meshes, [d.mask(m) for m in meshes], prm, u,
                                    gi.history(u, prm["order"]), w, precision="f32",
                                    node_master=[d.node_master(m) for m in meshes],
                                    coarse_n_iterations=10)
        b = torch.from_numpy(gi.src_vector(meshes[-1].n_dofs)).cuda()
        x = torch.zeros_like(b)
        cyc[kind] = (mg, lops, (lambda mg=mg, x=x, b=b: mg.vcycle(x, b)))
    tv = {k: [] for k in cyc}
    for k in cyc:
        window(cyc[k][2], 10)
    base = {k: [op.sweep_stats()[0] for op in cyc[k][1]] for k in cyc}
    for _ in range(windows):
        for k in cyc:
            tv[k].append(window(cyc[k][2], max(1, reps // 4)))
    for k in cyc:
        v = np.array(tv[k])
        n_cycles = windows * max(1, reps // 4)
        res = [(op.sweep_stats()[0] - b0) / n_cycles for op, b0 in zip(cyc[k][1], base[k])]
        print(f"re3900 r0..r{n_ref} f32 {k:8s} resident launches per cycle and level {res} "
              f"vcycle {np.median(v):8.2f} us (min {v.min():.2f} max {v.max():.2f})", flush=True)


if __name__ == "__main__":
    main()
