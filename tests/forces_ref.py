"""numpy restatement of SimulationCylinder::postprocess (simulation.cc:451-511)
and of its point probe (:512-541): the test reference of csrc/forces.hip.

Lagrange basis and derivatives on the Gauss-Lobatto nodes
(glsmesh._gll_nodes), numpy's Gauss-Legendre rule, the Jacobian from the
cell's node coordinates.  Works on anything with dim, degree, cell_nodes and
coords (glsmesh.Mesh, ShuffledMesh, glsdist.LocalMesh)."""
import numpy as np

import glsmesh as gm


def gauss01(n):
    """QGauss(n) on [0, 1]."""
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 + 0.5 * x, 0.5 * w


def lagrange(nodes, x):
    """values [len(x)][n] and derivatives [len(x)][n] of the Lagrange basis
    on `nodes` at the points x."""
    nodes = np.asarray(nodes, dtype=np.float64)
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    n = len(nodes)
    v = np.ones((len(x), n))
    dv = np.zeros((len(x), n))
    for i in range(n):
        for j in range(n):
            if j == i:
                continue
            v[:, i] *= (x - nodes[j]) / (nodes[i] - nodes[j])
            prod = np.full(len(x), 1.0 / (nodes[i] - nodes[j]))
            for m in range(n):
                if m != i and m != j:
                    prod *= (x - nodes[m]) / (nodes[i] - nodes[m])
            dv[:, i] += prod
    return v, dv


def basis_at(degree, dim, xi):
    """phi [npts][nq] and reference gradients [npts][nq][dim] of the tensor
    Q_k basis (lexicographic, x fastest) at reference points xi [npts][dim]."""
    nodes = gm._gll_nodes(degree)
    n = degree + 1
    xi = np.asarray(xi, dtype=np.float64).reshape(-1, dim)
    vd = [lagrange(nodes, xi[:, e]) for e in range(dim)]
    i = np.arange(n ** dim)
    ia = [i % n, (i // n) % n, i // (n * n)]
    phi = np.ones((len(xi), n ** dim))
    for e in range(dim):
        phi *= vd[e][0][:, ia[e]]
    grad = np.ones((len(xi), n ** dim, dim))
    for e in range(dim):
        for e2 in range(dim):
            grad[:, :, e] *= vd[e2][1 if e2 == e else 0][:, ia[e2]]
    return phi, grad


def face_points(dim, face_no, n_q_1d):
    """Reference points [nqf][dim] and weights [nqf] of QGauss<dim-1>(n_q_1d)
    on face 2*axis + side, first tangential axis fastest."""
    ax, side = face_no // 2, face_no % 2
    x, w = gauss01(n_q_1d)
    tang = [e for e in range(dim) if e != ax]
    nqf = n_q_1d ** (dim - 1)
    q = np.arange(nqf)
    qt = [q % n_q_1d, q // n_q_1d]
    xi = np.zeros((nqf, dim))
    wt = np.ones(nqf)
    xi[:, ax] = side
    for t, e in enumerate(tang):
        xi[:, e] = x[qt[t]]
        wt *= w[qt[t]]
    return xi, wt


def surface_force(mesh, cells, face_no, vec, nu, n_q_1d=3):
    """(per_face [n_faces][dim], S_face [n_faces]): the force
    sum_q (-p I + 2 nu eps(u)) . n JxW of every face with n = -(outward unit
    normal) (simulation.cc:487-495) and the sum of the |.| of its per-point
    contributions (the error scale)."""
    dim, k = mesh.dim, mesh.degree
    nc = dim + 1
    cells = np.asarray(cells, dtype=np.int64)
    face_no = np.asarray(face_no, dtype=np.int64)
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    X = np.asarray(mesh.coords, dtype=np.float64)
    V = np.asarray(vec, dtype=np.float64).reshape(-1, nc)
    per_face = np.zeros((len(cells), dim))
    scale = np.zeros(len(cells))
    for fn in np.unique(face_no):
        sel = np.nonzero(face_no == fn)[0]
        ax, side = int(fn) // 2, int(fn) % 2
        xi, wt = face_points(dim, int(fn), n_q_1d)
        phi, grad = basis_at(k, dim, xi)
        nodes = cn[cells[sel]]                                # [f][nq]
        Xc, Vc = X[nodes], V[nodes]                           # [f][nq][dim], [f][nq][nc]
        J = np.einsum("fid,qie->fqde", Xc, grad)              # dx_d / dxi_e
        inv = np.linalg.inv(J)                                # dxi_a / dx_e
        det = np.linalg.det(J)
        m = (2 * side - 1) * inv[:, :, ax, :]                 # J^{-T} n_ref
        mn = np.linalg.norm(m, axis=-1)
        n_out = m / mn[..., None]
        jxw = np.abs(det) * mn * wt[None, :]
        p = np.einsum("qi,fi->fq", phi, Vc[:, :, dim])
        GU = np.einsum("fid,qia->fqda", Vc[:, :, :dim], grad)  # du_d / dxi_a
        G = np.einsum("fqda,fqae->fqde", GU, inv)              # du_d / dx_e
        stress = nu * (G + np.swapaxes(G, -1, -2))
        stress = stress - p[..., None, None] * np.eye(dim)
        f = np.einsum("fqde,fqe->fqd", stress, -n_out) * jxw[..., None]
        per_face[sel] = f.sum(axis=1)
        scale[sel] = np.linalg.norm(f, axis=-1).sum(axis=1)
    return per_face, scale


def total_force(mesh, cells, face_no, vec, nu, n_q_1d=3):
    """(F [dim], S): the summed force and its error scale."""
    pf, s = surface_force(mesh, cells, face_no, vec, nu, n_q_1d)
    return pf.sum(axis=0), float(s.sum())


def cells_measure(mesh, n_q_1d=4):
    """sum over the cells of the integral of |det J| by QGauss(n_q_1d)."""
    dim, k = mesh.dim, mesh.degree
    x, w = gauss01(n_q_1d)
    q = np.arange(n_q_1d ** dim)
    qa = [q % n_q_1d, (q // n_q_1d) % n_q_1d, q // (n_q_1d * n_q_1d)]
    xi = np.stack([x[qa[e]] for e in range(dim)], axis=1)
    wt = np.prod([w[qa[e]] for e in range(dim)], axis=0)
    _, grad = basis_at(k, dim, xi)
    Xc = np.asarray(mesh.coords)[np.asarray(mesh.cell_nodes, dtype=np.int64)]
    J = np.einsum("cid,qie->cqde", Xc, grad)
    return float((np.abs(np.linalg.det(J)) * wt[None, :]).sum())


def hole_measure(mesh):
    """A_h: the bounding box's volume minus the mapped cells' (the discrete
    cylinder's cross-section, times the height in 3D)."""
    X = np.asarray(mesh.coords)
    return float(np.prod(X.max(axis=0) - X.min(axis=0))) - cells_measure(mesh)


def locate(mesh, points, tol=1e-6):
    """Per point the list of (cell, xi) whose Q_k mapping contains it: Newton
    inversion in the cells of the closest node, reference tolerance `tol`,
    clamped to the unit cell."""
    dim, k = mesh.dim, mesh.degree
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    X = np.asarray(mesh.coords, dtype=np.float64)
    used = np.zeros(len(X), dtype=bool)
    used[cn.ravel()] = True
    out = []
    for p in np.asarray(points, dtype=np.float64).reshape(-1, dim):
        d2 = ((X - p) ** 2).sum(axis=1)
        d2[~used] = np.inf
        best = int(np.argmin(d2))
        pairs = []
        for c in np.nonzero((cn == best).any(axis=1))[0]:
            Xc = X[cn[c]]
            xi = np.full(dim, 0.5)
            ok = False
            for _ in range(40):
                phi, grad = basis_at(k, dim, xi[None, :])
                r = p - phi[0] @ Xc
                J = np.einsum("id,ie->de", Xc, grad[0])
                try:
                    dxi = np.linalg.solve(J, r)
                except np.linalg.LinAlgError:
                    break
                xi = xi + dxi
                if not np.all((xi > -2.0) & (xi < 3.0)):
                    break
                if np.abs(dxi).max() < 1e-13:
                    ok = True
                    break
            if ok and np.all((xi >= -tol) & (xi <= 1.0 + tol)):
                pairs.append((int(c), np.clip(xi, 0.0, 1.0)))
        out.append(pairs)
    return out


def probe(mesh, points, vec):
    """(values [n_points][dim+1], counts [n_points]): all components at the
    points, averaged over the cells found (point_values<1>(avg)); a point in
    no cell gives 0."""
    dim, k = mesh.dim, mesh.degree
    nc = dim + 1
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    V = np.asarray(vec, dtype=np.float64).reshape(-1, nc)
    found = locate(mesh, points)
    vals = np.zeros((len(found), nc))
    cnt = np.zeros(len(found), dtype=np.int64)
    for i, pairs in enumerate(found):
        for c, xi in pairs:
            phi, _ = basis_at(k, dim, xi[None, :])
            vals[i] += phi[0] @ V[cn[c]]
        cnt[i] = len(pairs)
        if pairs:
            vals[i] /= len(pairs)
    return vals, cnt
