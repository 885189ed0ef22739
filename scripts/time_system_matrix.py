#!/usr/bin/env python3
"""Cost of the system matrix and of the matrix-based apply on one deck /
refinement:
  python scripts/time_system_matrix.py [deck] [n_ref] [prec] [reps]
  (a) host assembly gls_op_system_matrix (host wall time; it returns
      synchronised)
  (b) device assembly gls_op_system_matrix_device after an invalidation:
      total, and split into the element-matrix kernels and the gather
      (the library's timer sections, GPU time between events on the stream)
  (c) k_csr_vmult per apply (matrix-based gls_op_vmult)
  (d) rocSPARSE SpMV, csr_adaptive, on the same matrix, set up as
      tools/gls_vmult.hip does (FP64 operators only)
  (e) the matrix-free gls_op_vmult
Applies are timed between two device events on the stream, warm, the median
and the 10 / 90 % quantiles of `reps` calls; with the bytes each kernel moves
at least.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-ns-gls_amd", "python"))


class RocsparseSpmv:
    """y = A x with rocsparse_spmv_alg_csr_adaptive on torch tensors (int64
    row_ptr and cols, float64 vals): buffer size, preprocess, then compute"""

    def __init__(self, rp, ci, va, x, y, stream):
        L = self.L = C.CDLL("librocsparse.so")
        vp, i64 = C.c_void_p, C.c_int64
        self.h, self.mat, self.vx, self.vy = vp(), vp(), vp(), vp()
        L.rocsparse_create_csr_descr.argtypes = [C.POINTER(vp), i64, i64, i64, vp, vp, vp, C.c_int,
                                                 C.c_int, C.c_int, C.c_int]
        L.rocsparse_create_dnvec_descr.argtypes = [C.POINTER(vp), i64, vp, C.c_int]
        L.rocsparse_set_stream.argtypes = [vp, vp]
        L.rocsparse_spmv.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_size_t), vp]
        n, nnz = x.numel(), va.numel()
        self._ok(L.rocsparse_create_handle(C.byref(self.h)))
        self._ok(L.rocsparse_set_stream(self.h, stream))
        # indextype i64 = 3, index base zero = 0, datatype f64_r = 152
        self._ok(L.rocsparse_create_csr_descr(C.byref(self.mat), n, n, nnz, rp.data_ptr(),
                                              ci.data_ptr(), va.data_ptr(), 3, 3, 0, 152))
        self._ok(L.rocsparse_create_dnvec_descr(C.byref(self.vx), n, x.data_ptr(), 152))
        self._ok(L.rocsparse_create_dnvec_descr(C.byref(self.vy), n, y.data_ptr(), 152))
        self.one, self.zero = C.c_double(1.0), C.c_double(0.0)
        self.bsz, self.buf, self._keep = C.c_size_t(0), None, (rp, ci, va, x, y)
        self._stage(1)
        import torch
        self.buf = torch.empty(max(8, self.bsz.value), dtype=torch.uint8, device="cuda")
        self._stage(2)

    @staticmethod
    def _ok(rc):
        if rc != 0:
            raise RuntimeError(f"rocsparse status {rc}")

    def _stage(self, stage):
        # operation none = 111, alg csr_adaptive = 2
        self._ok(self.L.rocsparse_spmv(self.h, 111, C.byref(self.one), self.mat, self.vx,
                                       C.byref(self.zero), self.vy, 152, 2, stage,
                                       C.byref(self.bsz),
                                       None if self.buf is None else self.buf.data_ptr()))

    def __call__(self):
        self._stage(3)


def main():
    import numpy as np
    import torch
    import glsamd
    import glsinputs as gi
    import glsmesh as gm
    deck = sys.argv[1] if len(sys.argv) > 1 else "input_hoffmann_3D_Re3900.json"
    nref = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    prec = sys.argv[3] if len(sys.argv) > 3 else "f64"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 50
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
    x = op._dev(gi.src_vector(m.n_dofs))
    dst = op.initialize_dof_vector()
    q = lambda a, p: float(np.percentile(a, p))  # noqa: E731
    ts = 8 if prec == "f64" else 4
    ndof = (m.degree + 1) ** m.dim * (m.dim + 1)

    rp, ci, va = op.system_matrix_device()
    n, nnz = int(m.n_dofs), int(va.numel())
    plan = glsamd.assemble_plan_host(m.cell_nodes, cm, m.dim, m.degree)
    e_bytes = int(m.n_cells) * ndof * ndof * ts
    out = {"deck": deck, "n_ref": nref, "precision": prec, "n_dofs": n, "n_cells": int(m.n_cells),
           "nnz": nnz, "n_pairs": int(plan["n_pairs"]), "reps": reps, "ms": {}, "bytes": {}}
    # least traffic: the element matrices written once and read once; the
    # gather also reads the pair and incidence lists and writes each value
    out["bytes"] = {"element_matrices_write": e_bytes,
                    "gather": e_bytes + nnz * 8 + int(plan["n_pairs"]) * 12
                    + int(plan["n_incidence"]) * 8,
                    "csr_vmult": nnz * 12 + (n + 1) * 8 + 2 * n * ts,
                    "matrix_free_vmult": float(op.vmult_bytes())}

    # (a) host assembly
    host = []
    for _ in range(max(2, min(5, reps))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.system_matrix()
        host.append((time.perf_counter() - t0) * 1e3)
    out["ms"]["host_system_matrix_wall"] = {"median": q(host, 50), "min": min(host)}

    # (b) device assembly, from the timer sections
    names = {"total": "ns::initialize_system_matrix",
             "element_matrices": "ns::initialize_system_matrix::element_matrices",
             "gather": "ns::initialize_system_matrix::gather"}
    for _ in range(3):
        op.invalidate_system()
        op.system_matrix_device_raw()
    torch.cuda.synchronize()
    was = glsamd.timer_enable(True)
    tot = {k: [] for k in names}
    wall = []
    for _ in range(reps):
        glsamd.timer_reset()
        op.invalidate_system()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.system_matrix_device_raw()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        t = glsamd.timer_sections()
        for k, nm in names.items():
            tot[k].append(t[nm]["gpu_ms"])
    glsamd.timer_enable(was)
    glsamd.timer_reset()
    for k in names:
        out["ms"]["device_assembly_" + k] = {"median": q(tot[k], 50), "p10": q(tot[k], 10),
                                             "p90": q(tot[k], 90)}
    out["ms"]["device_assembly_wall"] = {"median": q(wall, 50)}

    # (c), (d), (e) applies
    def mb():
        op.vmult(dst, x)

    calls = {"matrix_free_vmult": mb}
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    if prec == "f64":
        calls["rocsparse_csr_adaptive"] = RocsparseSpmv(rp, ci.to(torch.int64), va, x, y,
                                                        glsamd._stream())
    for name in ("matrix_free_vmult", "csr_vmult", "rocsparse_csr_adaptive"):
        if name == "csr_vmult":
            op.set_matrix_based(True)
            fn = mb
        elif name in calls:
            op.set_matrix_based(False)
            fn = calls[name]
        else:
            continue
        for _ in range(10):
            fn()
        dev = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1))
        out["ms"][name] = {"median": q(dev, 50), "p10": q(dev, 10), "p90": q(dev, 90)}
        if name == "csr_vmult":
            ref = dst.double().clone()
    if prec == "f64":
        out["rocsparse_vs_csr_vmult_rel_l2"] = float(torch.linalg.norm(y - ref)
                                                     / torch.linalg.norm(ref))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
