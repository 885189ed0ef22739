#!/usr/bin/env python3
"""N vmults of the Re3900 operator with the deck's walls or with periodic
walls, for counting kernel launches under a kernel trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- \\
      python scripts/count_vmult_launches.py walls|periodic N [f64|f32] [n_ref=2]

The launches per vmult are the difference of the summed "Calls" column of
OUT/*/t_kernel_stats.csv between two values of N, divided by the difference
of N (the set-up launches cancel)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-ns-gls_amd", "python"))


def main():
    import torch
    import glsamd
    import glsinputs as gi
    import glsmesh as gm
    kind, n = sys.argv[1], int(sys.argv[2])
    prec = sys.argv[3] if len(sys.argv) > 3 else "f64"
    n_ref = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    d = gm.read_deck(os.path.join(gm.DECK_DIR, "input_hoffmann_3D_Re3900.json"))
    d.wall_bc_periodic = kind == "periodic"
    m = d.mesh(n_ref)
    prm, w = d.operator_parameters(2.5e-4)
    u = gi.linearization_point(m.n_nodes, 3, d.u_max)
    op = glsamd.NavierStokesOperator(m, d.mask(m), prec, node_master=d.node_master(m))
    op.set_parameters(**prm)
    op.set_linearization_point(u)
    op.set_previous_solution(gi.history(u, prm["order"]), w)
    src, dst = op._dev(gi.src_vector(m.n_dofs)), op.initialize_dof_vector()
    for _ in range(n):
        op.vmult(dst, src)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
