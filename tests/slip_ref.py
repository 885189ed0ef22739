"""TEST INFRASTRUCTURE — numpy restatement of the node constraints
(no-normal-flux rows on curved boundaries) on top of the oracle.

Rows (nodes, comp, coef): u[node][comp] = sum_e coef[e] u[node][e].  C is the
identity with the row of every eliminated dof replaced by coef; the
constrained operator is C^T A C with identity rows on the eliminated dofs.
Also the mesh side: the averaged face normals restated with numpy."""
import numpy as np

import glsmesh as gm
from helpers import Case, deck


class Rows:
    def __init__(self, dim, nodes, comp, coef):
        self.dim, self.nc = dim, dim + 1
        self.nodes = np.asarray(nodes, dtype=np.int64)
        self.comp = np.asarray(comp, dtype=np.int64)
        self.coef = np.asarray(coef, dtype=np.float64).reshape(-1, dim)
        self.elim = self.nodes * self.nc + self.comp

    def resolve(self, x):
        """C x"""
        y = np.array(x, dtype=np.float64, copy=True)
        acc = np.zeros(len(self.nodes))
        for e in range(self.dim):
            acc += self.coef[:, e] * y[self.nodes * self.nc + e]
        y[self.elim] = acc
        return y

    def transpose(self, y):
        """C^T y (zero on the eliminated dofs)"""
        z = np.array(y, dtype=np.float64, copy=True)
        r = z[self.elim].copy()
        for e in range(self.dim):
            z[self.nodes * self.nc + e] += self.coef[:, e] * r
        z[self.elim] = 0.0
        return z

    def distribute(self, x, cmask, g=None):
        """AffineConstraints::distribute: Dirichlet values, then the rows."""
        y = np.array(x, dtype=np.float64, copy=True)
        con = ((np.asarray(cmask)[:, None] >> np.arange(self.nc)[None, :]) & 1).astype(bool).ravel()
        y[con] = 0.0 if g is None else np.asarray(g)[con]
        return self.resolve(y)

    def dense(self, n_dofs):
        Cm = np.eye(n_dofs)
        Cm[self.elim, self.elim] = 0.0
        for e in range(self.dim):
            Cm[self.elim, self.nodes * self.nc + e] += self.coef[:, e]
        return Cm


def vmult(o, rows, x):
    """C^T A C x with identity rows on the eliminated dofs"""
    y = rows.transpose(o.vmult(rows.resolve(x)))
    y[rows.elim] = np.asarray(x)[rows.elim]
    return y


def residual(o, rows, x, cmask, g=None):
    """evaluate_residual: distribute, residual cell loop, C^T, zero rows"""
    return rows.transpose(o.evaluate_residual(rows.distribute(x, cmask, g)))


def residual_plain(o, rows, x):
    return rows.transpose(o.evaluate_residual(x))


def diagonal(o, rows, mesh):
    """diag(C^T A C) from the cell matrices of the cells touching listed nodes"""
    d = o.diagonal()
    dim, nc = rows.dim, rows.nc
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    row_of = -np.ones(mesh.n_nodes, dtype=np.int64)
    row_of[rows.nodes] = np.arange(len(rows.nodes))
    B = np.zeros((len(rows.nodes), dim, dim))
    for c in np.nonzero((row_of[cn] >= 0).any(axis=1))[0]:
        M = o.cell_matrix(c)
        for p, node in enumerate(cn[c]):
            i = row_of[node]
            if i >= 0:
                B[i] += M[p * nc:p * nc + dim, p * nc:p * nc + dim]
    for i, (node, c) in enumerate(zip(rows.nodes, rows.comp)):
        for e in range(dim):
            k = rows.coef[i, e]
            if e != c and k != 0.0:
                d[node * nc + e] = B[i, e, e] + k * (B[i, e, c] + B[i, c, e]) + k * k * B[i, c, c]
        d[node * nc + c] = 1.0
    return d


def inverse_diagonal(o, rows, mesh):
    d = diagonal(o, rows, mesh)
    return np.where(np.abs(d) > 1e-10, 1.0 / d, 1.0)


def dense_matrix(o, mesh, cmask):
    """A assembled densely from cell_matrix, Dirichlet rows and columns unit"""
    nc = mesh.dim + 1
    n = mesh.n_nodes * nc
    A = np.zeros((n, n))
    for c, cnodes in enumerate(np.asarray(mesh.cell_nodes, dtype=np.int64)):
        dofs = (cnodes[:, None] * nc + np.arange(nc)[None, :]).ravel()
        A[np.ix_(dofs, dofs)] += o.cell_matrix(c)
    con = ((np.asarray(cmask)[:, None] >> np.arange(nc)[None, :]) & 1).astype(bool).ravel()
    A[con, :] = 0.0
    A[:, con] = 0.0
    A[con, con] = 1.0
    return A


def dense_constrained(A, rows):
    Cm = rows.dense(A.shape[0])
    M = Cm.T @ A @ Cm
    M[rows.elim, rows.elim] = 1.0
    return M


# ---------------------------------------------------------------- the normals
def _dlagrange(k):
    if k == 1:
        return np.array([[-1.0, 1.0], [-1.0, 1.0]])
    return np.array([[-3.0, 4.0, -1.0], [-1.0, 0.0, 1.0], [1.0, -4.0, 3.0]])


def normals(mesh, bid, vel_ids=()):
    """(nodes, comp, coef, normals) of boundary id `bid` by the rule of
    gls_mesh_no_normal_flux, restated with numpy."""
    dim, k = mesh.dim, mesh.degree
    n = k + 1
    dl = _dlagrange(k)
    X = np.asarray(mesh.coords)
    cn = np.asarray(mesh.cell_nodes, dtype=np.int64)
    cells, faces = gm.boundary_faces(mesh, bid)
    per_cell = {}
    face_n = []
    for c, f in zip(cells, faces):
        a, side = f // 2, f % 2
        for p in range(n ** dim):
            idx = [p % n, (p // n) % n, p // (n * n)][:dim]
            if idx[a] != side * k:
                continue
            J = np.zeros((dim, dim))
            for b in range(dim):
                for i in range(n):
                    q = list(idx)
                    q[b] = i
                    lin = sum(q[t] * n ** t for t in range(dim))
                    J[:, b] += dl[idx[b], i] * X[cn[c, lin]]
            e = np.zeros(dim)
            e[a] = 1.0 if side else -1.0
            v = np.linalg.solve(J.T, e)
            v /= np.linalg.norm(v)
            v[np.abs(v) < 1e-13] = 0.0
            v /= np.linalg.norm(v)
            node = cn[c, p]
            per_cell.setdefault(node, {}).setdefault(c, []).append(v)
            face_n.append((node, v))
    nodes = sorted(per_cell)
    out_nodes, comp, coef, nrm = [], [], [], []
    min_dot = 1.0
    avg = {}
    for node in nodes:
        s = np.zeros(dim)
        for c in sorted(per_cell[node]):
            t = np.sum(per_cell[node][c], axis=0)
            s += t / np.linalg.norm(t)
        avg[node] = s / np.linalg.norm(s)
    for node, v in face_n:
        min_dot = min(min_dot, float(v @ avg[node]))
    vel_bits = sum(1 << int(i) for i in vel_ids)
    for node in nodes:
        if int(mesh.node_boundary[node]) & vel_bits:
            continue
        s = avg[node]
        c = int(np.nonzero(np.abs(s) >= (1 - 1e-10) * np.abs(s).max())[0][0])
        k_ = -s / s[c]
        k_[c] = 0.0
        k_[np.abs(k_) <= np.finfo(float).eps] = 0.0
        out_nodes.append(node)
        comp.append(c)
        coef.append(k_)
        nrm.append(s)
    return (np.asarray(out_nodes, dtype=np.int64), np.asarray(comp, dtype=np.int32),
            np.asarray(coef).reshape(-1, dim), np.asarray(nrm).reshape(-1, dim), min_dot)


# ------------------------------------------------------------------ the cases
def slip_case(name, n_ref, dt=2.5e-4, outflow=None, **overrides):
    """A deck with the cylinder on slip: (Case with the Dirichlet mask,
    Rows from the library's own node constraints, outflow faces or None)."""
    d = deck(name)
    d.no_slip_cylinder = False
    if outflow is not None:
        d.outflow_bc = outflow
    for k, v in overrides.items():
        setattr(d, k, v)
    m = d.mesh(n_ref)
    cmask = d.mask(m)
    params, w = d.operator_parameters(dt)
    case = Case(m, cmask, params, w, u_inf=d.u_max)
    nodes, comp, coef = d.node_constraints(m)
    case.rows = Rows(m.dim, nodes, comp, coef)
    case.node_constraints = (nodes, comp, coef)
    faces = d.outflow_faces(m)
    case.outflow = None if faces is None else (faces[0], faces[1], d.outflow)
    return case


def gpu(case, precision="f64", brick=None, deterministic=False):
    import glsamd
    op = glsamd.NavierStokesOperator(case.mesh, case.cmask, precision, brick=brick,
                                     outflow=case.outflow,
                                     node_constraints=case.node_constraints)
    op.set_parameters(**dict(case.params, deterministic=deterministic))
    op.set_linearization_point(case.u_star)
    if case.params["order"] > 0:
        op.set_previous_solution(case.hist, case.weights)
    return op


# ------------------------------------------------------------- the multigrid
class _WrappedLevel:
    """A level operator with node constraints: C^T A C, identity rows."""

    def __init__(self, o, rows):
        self.o, self.rows = o, rows

    def vmult(self, x):
        return vmult(self.o, self.rows, x)


class SlipOracleGMG:
    """mg_ref.OracleGMG with node constraints on every level: the wrapped
    level operators and their diagonals; "constrained" for the transfer
    weights of a fine level and for the power iteration's start vector means
    the Dirichlet mask plus the eliminated components; the prolongation reads
    C_c x_c, the restriction ends with C_c^T (zero on the eliminated coarse
    components)."""

    def __new__(cls, meshes, cmasks, rows, params, u_star, hist=None, weights=None, **kw):
        import mg_ref
        import oracle as orc

        class _GMG(mg_ref.OracleGMG):
            def prolongate_add(self, l, dst_f, src_c):
                orc.prolongate_add(self.om_plain[l - 1], self.om[l], self.child[l], dst_f,
                                   self.rows[l - 1].resolve(src_c))

            def restrict_add(self, l, dst_c, src_f):
                t = np.zeros_like(dst_c)
                orc.restrict_add(self.om_plain[l - 1], self.om[l], self.child[l], t, src_f)
                dst_c += self.rows[l - 1].transpose(t)

        g = _GMG(meshes, cmasks, params, u_star, hist, weights, **kw)
        g.rows = rows
        g.om_plain = g.om
        all_masks = []
        for m, cm, r in zip(meshes, cmasks, rows):
            a = np.array(cm, dtype=np.uint8, copy=True)
            a[r.nodes] |= (1 << r.comp).astype(np.uint8)
            all_masks.append(a)
        g.om = [orc.OracleMesh(m, a) for m, a in zip(meshes, all_masks)]
        g.plain_ops = g.ops
        g.invdiag = [inverse_diagonal(o, r, m) for o, r, m in zip(g.ops, rows, meshes)]
        g.ops = [_WrappedLevel(o, r) for o, r in zip(g.ops, rows)]
        return g


def slip_hierarchy(name, n_levels, **overrides):
    """(deck, meshes r0.., Dirichlet masks, Rows per level, node constraints
    per level, params, weights) of a deck with the cylinder on slip."""
    d = deck(name)
    d.no_slip_cylinder = False
    for k, v in overrides.items():
        setattr(d, k, v)
    meshes = [d.mesh(r) for r in range(n_levels)]
    cm = [d.mask(m) for m in meshes]
    ncs = [d.node_constraints(m) for m in meshes]
    rows = [Rows(m.dim, *nc) for m, nc in zip(meshes, ncs)]
    params, w = d.operator_parameters(2.5e-4)
    return d, meshes, cm, rows, ncs, params, w


def gmres_right(A, M, b, rtol, restart=28, maxiter=200):
    """Right-preconditioned restarted GMRES as gls_gmres_solve runs it
    (solver_l.cc:45-74), x0 = 0, keeping z_j = M v_j (x += Z y): with an FP32
    V-cycle as M, M(V y) and Z y differ by the preconditioner's rounding, which
    a restatement through M(V y) cannot get below.  Returns (x, iterations)."""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    tol = rtol * np.linalg.norm(b)
    it = 0
    r = b.copy()
    res = np.linalg.norm(r)
    while res > tol and it < maxiter:
        V, Z = [r / res], []
        H = np.zeros((restart + 1, restart))
        g = np.zeros(restart + 1)
        g[0] = res
        cs, sn = np.zeros(restart), np.zeros(restart)
        jd = 0
        for j in range(restart):
            Z.append(M(V[j]))
            w = A(Z[j])
            h = np.zeros(j + 1)
            for _ in range(2):  # CGS2
                hp = np.array([v @ w for v in V])
                w = w - sum(c * v for c, v in zip(hp, V))
                h += hp
            hn = np.linalg.norm(w)
            H[:j + 1, j], H[j + 1, j] = h, hn
            V.append(w / hn if hn > 0 else w)
            for i in range(j):
                t = cs[i] * H[i, j] + sn[i] * H[i + 1, j]
                H[i + 1, j] = -sn[i] * H[i, j] + cs[i] * H[i + 1, j]
                H[i, j] = t
            rr = np.hypot(H[j, j], H[j + 1, j])
            cs[j], sn[j] = (H[j, j] / rr, H[j + 1, j] / rr) if rr > 0 else (1.0, 0.0)
            H[j, j], H[j + 1, j] = rr, 0.0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            it += 1
            jd += 1
            res = abs(g[j + 1])
            if res <= tol or hn == 0 or it >= maxiter:
                break
        y = np.zeros(jd)
        for i in range(jd - 1, -1, -1):
            y[i] = (g[i] - H[i, i + 1:jd] @ y[i + 1:jd]) / H[i, i]
        x = x + sum(c * z for c, z in zip(y, Z[:jd]))
        if res <= tol:
            break
        r = b - A(x)
        res = np.linalg.norm(r)
    return x, it
