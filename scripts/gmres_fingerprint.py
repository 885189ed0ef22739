#!/usr/bin/env python3
"""Fingerprints of the three device GMRES solvers (outer gls_gmres_solve /
gls_gmres_solve_prec, the V-cycle's coarse GMRES, the partitioned
gls_dist_gmres_solve): per case one line

    <case> it=<iterations> rst=<restarts> res=<final residual, hex float> sha256=<of x>

Every operator and multigrid runs in deterministic mode, so two builds that
issue the same kernels in the same order with the same host arithmetic print
the same lines (profiles/gmres_core: a change to the solvers' structure is
compared against its parent with this).  A solve that stops at its iteration
limit is a case too: the statistics and the iterate are still written.

    gmres_fingerprint.py [outer] [prec] [coarse] [dist]     (default: all)
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dealii-ns-gls_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import glsamd  # noqa: E402
import glsdist  # noqa: E402
import glsinputs as gi  # noqa: E402
import glsmesh as gm  # noqa: E402

ENV = ("GLS_GMRES_ORTHO", "GLS_GMRES_ZKEEP")


def sha(ts):
    h = hashlib.sha256()
    for t in ts if isinstance(ts, (list, tuple)) else [ts]:
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def line(case, st, xs):
    print(f"{case} it={st['n_iterations']} rst={st['n_restarts']} "
          f"res={float(st['final_residual']).hex()} sha256={sha(xs)}", flush=True)


def with_env(env, fn):
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in ENV:
            os.environ.pop(k, None)


def hierarchy(name, n_ref, dt=2.5e-4):
    d = gm.read_deck(os.path.join(gm.DECK_DIR, name))
    meshes = [d.mesh(r) for r in range(n_ref + 1)]
    vel, p, slip = d.boundary_descriptor()
    cm = [m.constraint_mask(vel, p, slip) for m in meshes]
    params, w = d.operator_parameters(dt)
    u = gi.linearization_point(meshes[-1].n_nodes, meshes[-1].dim, d.u_max)
    hist = gi.history(u, params["order"])
    return meshes, cm, dict(params, deterministic=True), w, u, hist


def fine_operator(meshes, cm, params, w, u, hist):
    A = glsamd.NavierStokesOperator(meshes[-1], cm[-1], "f64")
    A.set_parameters(**params)
    A.set_linearization_point(u)
    if params["order"] > 0:
        A.set_previous_solution(hist, w)
    return A


def solve(case, A, prec, b, env=None, **kw):
    def run():
        s = glsamd.LinearSolverGMRES(A, prec, **kw)
        x = A.initialize_dof_vector()
        try:
            s.solve(x, b)
        except glsamd.GlsError as e:
            if "no convergence" not in str(e):
                raise
        torch.cuda.synchronize()
        line(case, s.last, x)
    with_env(env or {}, run)


def outer():
    """identity preconditioner: Turek 2D Re100 r0 (351 rows, odd: the narrow
    DCGS2 passes) and Re20 r0 (1230 rows, even: the wide ones)"""
    for deck, tag in (("input_turek_2D_Re100.json", "re100"),
                      ("input_turek_2D_Re20_stat.json", "re20")):
        h = hierarchy(deck, 0)
        A = fine_operator(*h)
        n = h[0][-1].n_dofs
        b = A._dev(gi.src_vector(n))
        kw = dict(relative_tolerance=1e-8, absolute_tolerance=1e-12)
        name = f"outer/{tag}-n{n}"
        solve(f"{name}/tmp5", A, None, b, n_max_iterations=60, max_n_tmp_vectors=5, **kw)
        solve(f"{name}/tmp30", A, None, b, n_max_iterations=120, max_n_tmp_vectors=30, **kw)
        # a full cycle of 34: the three-pass tier at 32 columns, rocBLAS beyond
        solve(f"{name}/tmp36", A, None, b, n_max_iterations=80, max_n_tmp_vectors=36, **kw)
        for ortho in ("cgs2", "cgs3", "rocblas", "dcgs-narrow"):
            solve(f"{name}/tmp30-{ortho}", A, None, b, env={"GLS_GMRES_ORTHO": ortho},
                  n_max_iterations=120, max_n_tmp_vectors=30, **kw)
        solve(f"{name}/tmp30-zkeep0", A, None, b, env={"GLS_GMRES_ZKEEP": "0"},
              n_max_iterations=120, max_n_tmp_vectors=30, **kw)
        # full GMRES to convergence (test_gmres_identity_matches_restatement)
        solve(f"{name}/full", A, None, b, n_max_iterations=3000, max_n_tmp_vectors=n + 2, **kw)


def prec():
    """Re3900 r0..r1 (test_gmres_gmg_newton_system): the FP32 V-cycle, the
    same with the coarse GMRES (a non-linear preconditioner: CGS2, M^-1 (V y)),
    and ILU(0) of the device-assembled matrix"""
    h = hierarchy("input_hoffmann_3D_Re3900.json", 1)
    meshes, cm, params, w, u, hist = h
    A = fine_operator(*h)
    b = A._dev(gi.rnd(3, meshes[-1].n_dofs))
    kw = dict(n_max_iterations=400, relative_tolerance=1e-6)
    mg, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                             coarse_n_iterations=10)
    solve("prec/re3900-r1/gmg", A, mg, b, **kw)
    solve("prec/re3900-r1/gmg-tmp8", A, mg, b, max_n_tmp_vectors=8, **kw)
    solve("prec/re3900-r1/gmg-cgs2", A, mg, b, env={"GLS_GMRES_ORTHO": "cgs2"}, **kw)
    solve("prec/re3900-r1/gmg-zkeep0", A, mg, b, env={"GLS_GMRES_ZKEEP": "0"}, **kw)
    del mg
    mgc, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision="f32",
                              coarse_n_iterations=10, coarse_iterate=True, coarse_reltol=1e-4,
                              coarse_maxiter=500)
    solve("prec/re3900-r1/gmg-coarse-gmres", A, mgc, b, **kw)
    solve("prec/re3900-r1/gmg-coarse-gmres-tmp8", A, mgc, b, max_n_tmp_vectors=8, **kw)
    print("prec/re3900-r1/gmg-coarse-gmres coarse_statistics", mgc.coarse_statistics(),
          flush=True)
    del mgc
    ilu = glsamd.ILU.from_operator(A, 0)
    solve("prec/re3900-r1/ilu0", A, ilu, b, n_max_iterations=200, relative_tolerance=1e-6)
    solve("prec/re3900-r1/ilu0-tmp8", A, ilu, b, n_max_iterations=60, relative_tolerance=1e-6,
          max_n_tmp_vectors=8)


def one_cycle(case, mg, b):
    x = torch.zeros_like(b)
    try:
        mg.vcycle(x, b)
    except glsamd.GlsError as e:
        if "no convergence" not in str(e):
            raise
    torch.cuda.synchronize()
    it, conv = mg.coarse_statistics()
    print(f"{case} it={it} conv={int(conv)} sha256={sha(x)}", flush=True)


def coarse():
    """one V-cycle with the coarse GMRES (test_coarse_gmres_vcycle's two
    hierarchies), FP32 and FP64 levels"""
    for deck, n_ref, sweeps in (("input_turek_2D_Re20_stat.json", 2, -1),
                                ("input_sphere_amg.json", 1, 10)):
        meshes, cm, params, w, u, hist = hierarchy(deck, n_ref)
        b = torch.from_numpy(gi.rnd(11, meshes[-1].n_dofs)).cuda()
        for precision in ("f32", "f64"):
            mg, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision=precision,
                                     coarse_n_iterations=sweeps, coarse_iterate=True,
                                     coarse_reltol=1e-4, coarse_maxiter=500)
            one_cycle(f"coarse/{deck[6:-5]}-r{n_ref}/{precision}", mg, b)
            # a tight tolerance: restarts of the 28-column cycle
            mg2, _ = glsamd.build_gmg(meshes, cm, params, u, hist, w, precision=precision,
                                      coarse_n_iterations=sweeps, coarse_iterate=True,
                                      coarse_reltol=1e-9 if precision == "f64" else 1e-5,
                                      coarse_maxiter=500)
            one_cycle(f"coarse/{deck[6:-5]}-r{n_ref}/{precision}-tight", mg2, b)
            del mg, mg2


def dist_solve(ops, mgs, xs, bs, n_max_iterations=10000, relative_tolerance=1e-8,
               max_n_tmp_vectors=30):
    """gls_dist_gmres_solve as glsamd.dist_gmres_solve calls it, the
    statistics also returned when the solve stops at its iteration limit"""
    import ctypes as C
    hs, n = glsamd._handles(ops)
    ms = None if mgs is None else glsamd._handles(mgs)[0]
    desc = glsamd.GMRESDesc(max_n_tmp_vectors, n_max_iterations, 0.0, relative_tolerance)
    res = glsamd.GMRESResult()
    rc = glsamd.lib().gls_dist_gmres_solve(
        C.cast(hs, C.c_void_p), None if ms is None else C.cast(ms, C.c_void_p), n, C.byref(desc),
        C.cast(glsamd._ptrs(xs), C.c_void_p), C.cast(glsamd._ptrs(bs), C.c_void_p), C.byref(res),
        glsamd._stream())
    st = {f: getattr(res, f) for f, _ in glsamd.GMRESResult._fields_}
    if rc != 0 and st["n_iterations"] < n_max_iterations:
        glsamd._check(rc)
    return st


def dist():
    """in-process groups of 2 and 4 on Re3900 r0..r1 (test_native_group_gmres):
    the FP64 multigrid and the identity preconditioner, fused passes and rocBLAS"""
    meshes, cm, params, w, u, hist = hierarchy("input_hoffmann_3D_Re3900.json", 1)
    bg = gi.rnd(12, meshes[-1].n_dofs)
    for world in (2, 4):
        g = glsdist.NativeGroupMultigrid(meshes, cm, world, precision="f64",
                                         coarse_n_iterations=-1)
        g.setup(params, u, hist, w)
        bs = g.scatter(bg)
        for ortho in ("", "rocblas"):
            for tag, mgs, kw in (("gmg", g.mg, dict(relative_tolerance=1e-8)),
                                 ("gmg-tmp6", g.mg, dict(relative_tolerance=1e-8,
                                                         max_n_tmp_vectors=6)),
                                 ("identity", None, dict(relative_tolerance=1e-8,
                                                         n_max_iterations=40)),
                                 ("identity-tmp36", None, dict(relative_tolerance=1e-8,
                                                               n_max_iterations=40,
                                                               max_n_tmp_vectors=36))):
                def run():
                    xs = [torch.zeros_like(x) for x in bs]
                    st = dist_solve(g.fine_native, mgs, xs, bs, **kw)
                    torch.cuda.synchronize()
                    return st, xs
                st, xs = with_env({"GLS_GMRES_ORTHO": ortho} if ortho else {}, run)
                line(f"dist/re3900-r1/world{world}/{tag}{'-' + ortho if ortho else ''}", st, xs)
        del g


if __name__ == "__main__":
    groups = sys.argv[1:] or ["outer", "prec", "coarse", "dist"]
    torch.cuda.set_device(0)
    for name in groups:
        {"outer": outer, "prec": prec, "coarse": coarse, "dist": dist}[name]()
