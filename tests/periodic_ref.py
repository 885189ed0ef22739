"""TEST INFRASTRUCTURE — numpy restatement of periodic node identification on
top of the oracle, which keeps running over the *caller's* connectivity.

node_master[slave] = master.  C is the map "slave := master"; the periodic
operator is C^T A C with identity rows on the slaves and on the constrained
dofs of the masters, whose mask is the OR of their group's masks (the oracle is
given that group mask on every member, so it treats a group alike)."""
import numpy as np

import glsmesh as gm
import slip_ref
from helpers import Case, deck


class Map:
    def __init__(self, dim, master, cmask):
        self.dim, self.nc = dim, dim + 1
        nc = self.nc
        self.master = np.asarray(master, dtype=np.int64)
        n = len(self.master)
        assert np.array_equal(self.master[self.master], self.master)
        self.slaves = np.nonzero(self.master != np.arange(n))[0]
        comp = np.arange(nc)[None, :]
        self.sdofs = (self.slaves[:, None] * nc + comp).ravel()
        self.mdofs = (self.master[self.slaves][:, None] * nc + comp).ravel()
        # the group mask: OR over the group, on every member
        grp = np.array(cmask, dtype=np.uint8, copy=True)
        np.bitwise_or.at(grp, self.master[self.slaves], np.asarray(cmask, dtype=np.uint8)[self.slaves])
        self.group_mask = grp[self.master]
        # what the operator holds: the OR on the master, every bit on a slave
        self.op_mask = self.group_mask.copy()
        self.op_mask[self.slaves] = (1 << nc) - 1
        bits = lambda m: ((m[:, None] >> comp) & 1).astype(bool).ravel()
        self.con = bits(self.group_mask)   # Dirichlet dofs, slaves' included
        self.fixed = bits(self.op_mask)    # identity rows: con and every slave dof
        self.is_slave_dof = np.zeros(n * nc, dtype=bool)
        self.is_slave_dof[self.sdofs] = True

    def resolve(self, x):
        """C x: slave := master"""
        y = np.array(x, dtype=np.float64, copy=True)
        y[self.sdofs] = y[self.mdofs]
        return y

    def transpose(self, y):
        """C^T y: add the slave into its master, zero the slave"""
        z = np.array(y, dtype=np.float64, copy=True)
        np.add.at(z, self.mdofs, z[self.sdofs])
        z[self.sdofs] = 0.0
        return z

    def distribute(self, x, g=None):
        """AffineConstraints::distribute: Dirichlet values, then slave := master"""
        y = np.array(x, dtype=np.float64, copy=True)
        y[self.con] = 0.0 if g is None else np.asarray(g)[self.con]
        return self.resolve(y)

    def dense(self, n_dofs):
        Cm = np.eye(n_dofs)
        Cm[self.sdofs, self.sdofs] = 0.0
        Cm[self.sdofs, self.mdofs] = 1.0
        return Cm


def fixed_dofs(pm, rows=None):
    """The identity rows: the slaves, the Dirichlet dofs and, with node
    constraints `rows` (slip_ref.Rows, on masters), their eliminated dofs."""
    f = pm.fixed.copy()
    if rows is not None:
        assert not pm.is_slave_dof[rows.elim].any()
        f[rows.elim] = True
    return f


def vmult(o, pm, x, rows=None):
    """C^T A C x; y = x on the slaves and on the masters' constrained dofs
    (without that the oracle's own identity rows on constrained dofs would be
    added once per group member into the master).  With rows C = C_p C_s: the
    rows sit on masters, so slave := master comes last."""
    x = np.asarray(x, dtype=np.float64)
    y = pm.transpose(o.vmult(pm.resolve(x if rows is None else rows.resolve(x))))
    if rows is not None:
        y = rows.transpose(y)
    f = fixed_dofs(pm, rows)
    y[f] = x[f]
    return y


def distribute(pm, x, g=None, rows=None):
    """Dirichlet values, then the rows, then slave := master"""
    if rows is None:
        return pm.distribute(x, g)
    return pm.resolve(rows.distribute(x, pm.op_mask, g))


def _ct(pm, r, rows):
    r = pm.transpose(r)
    if rows is not None:
        r = rows.transpose(r)
    r[fixed_dofs(pm, rows)] = 0.0
    return r


def residual(o, pm, x, g=None, rows=None):
    return _ct(pm, o.evaluate_residual(distribute(pm, x, g, rows)), rows)


def residual_plain(o, pm, x, rows=None):
    return _ct(pm, o.evaluate_residual(pm.resolve(x)), rows)


def diagonal(o, pm, rows=None, mesh=None):
    """diag(C^T A C): the members' diagonals summed (no cell holds two members
    of a group, so no off-diagonal entry of A joins them), 1 on identity rows.
    With rows, slip_ref's diagonal of C_s^T A C_s first: its rows sit on
    masters without slaves, whose entries the sum leaves alone."""
    d = pm.transpose(o.diagonal() if rows is None else slip_ref.diagonal(o, rows, mesh))
    d[fixed_dofs(pm, rows)] = 1.0
    return d


def inverse_diagonal(o, pm, rows=None, mesh=None):
    d = diagonal(o, pm, rows, mesh)
    return np.where(np.abs(d) > 1e-10, 1.0 / d, 1.0)


def dense_constrained(o, mesh, pm):
    """C^T A C with unit rows and columns on the slaves and the constrained dofs"""
    A = slip_ref.dense_matrix(o, mesh, pm.group_mask)
    Cm = pm.dense(A.shape[0])
    M = Cm.T @ A @ Cm
    f = pm.fixed
    M[f, :] = 0.0
    M[:, f] = 0.0
    M[f, f] = 1.0
    return M


def sparse_constrained(o, mesh, pm):
    """The same matrix as scipy CSR, assembled over the mapped connectivity
    (for meshes too large for a dense product)."""
    import scipy.sparse as sp
    nc = mesh.dim + 1
    n = mesh.n_nodes * nc
    cn = pm.master[np.asarray(mesh.cell_nodes, dtype=np.int64)]
    rows, cols, vals = [], [], []
    for c, cnodes in enumerate(cn):
        dofs = (cnodes[:, None] * nc + np.arange(nc)[None, :]).ravel()
        M = o.cell_matrix(c)
        rows.append(np.repeat(dofs, len(dofs)))
        cols.append(np.tile(dofs, len(dofs)))
        vals.append(M.ravel())
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(n, n))
    keep = sp.diags((~pm.fixed).astype(np.float64))
    return (keep @ A @ keep + sp.diags(pm.fixed.astype(np.float64))).tocsr()


# ------------------------------------------------------------------ the meshes
def box(dims, degree, n_ref, extent=None):
    """A box of dims coarse cells (2 or 3 entries) with tagged sides: x 0/1,
    y 3/4, z 5/6, refined n_ref times.  Uniform cells."""
    dim = len(dims)
    extent = extent or [1.0 * n for n in dims]
    nv = [n + 1 for n in dims]
    grids = np.meshgrid(*[np.linspace(0.0, e, n) for e, n in zip(extent, nv)], indexing="ij")
    vid = np.arange(int(np.prod(nv))).reshape(nv[::-1])  # [z][y][x]: x fastest
    verts = np.zeros((vid.size, dim))
    for idx in np.ndindex(*nv):
        verts[vid[idx[::-1]]] = [g[idx] for g in grids]
    cells, bfaces, bids = [], [], []
    tags = [(0, 1), (3, 4), (5, 6)]
    for c in np.ndindex(*dims):
        vs = []
        for o in range(2 ** dim):
            off = [(o >> a) & 1 for a in range(dim)]  # x fastest
            vs.append(vid[tuple((c[a] + off[a]) for a in range(dim))[::-1]])
        cells.append(vs)
        for a in range(dim):
            for side in range(2):
                if c[a] != (dims[a] - 1 if side else 0):
                    continue
                fv = [vs[o] for o in range(2 ** dim) if ((o >> a) & 1) == side]
                bfaces.append(fv)
                bids.append(tags[a][side])
    coarse = dict(vertices=verts, cells=np.asarray(cells, dtype=np.int32),
                  bfaces=np.asarray(bfaces, dtype=np.int32), bids=np.asarray(bids, dtype=np.int32))
    m = gm.from_coarse(coarse, degree, n_ref, "box")
    m.params["height"] = extent[1]
    return m


PAIRS = {"y": [(3, 4, 1)], "z": [(5, 6, 2)], "yz": [(3, 4, 1), (5, 6, 2)],
         "xy": [(0, 1, 0), (3, 4, 1)], "xyz": [(0, 1, 0), (3, 4, 1), (5, 6, 2)]}


def _params(dim, fixed=False, order=2):
    d = deck("input_turek_2D_Re100.json" if dim == 2 else "input_turek_3D_Re100.json")
    if fixed:
        d.nonlinear_solver = "Picard"
    return d.operator_parameters(2.5e-4)


def box_case(dims, degree, n_ref, periodic, fixed=False):
    """A box with inflow Dirichlet velocity on x = 0 (id 0), pressure on the
    outflow (id 1) -- unless x is periodic --, the pairs `periodic` and
    no-slip on the other walls."""
    m = box(dims, degree, n_ref)
    pairs = PAIRS[periodic]
    used = {i for p in pairs for i in p[:2]}
    vel = [i for i in [0, 3, 4, 5, 6][:1 + 2 * (m.dim - 1)] if i not in used]
    p = [1] if 1 not in used else []
    cmask = m.constraint_mask(vel, p, [])
    params, w = _params(m.dim, fixed)
    case = Case(m, cmask, params, w)
    case.node_master = m.periodic_nodes(pairs)
    case.pm = Map(m.dim, case.node_master, cmask)
    case.outflow = None
    case.node_constraints = None
    case.rows = None
    return case


def cylinder_case(name, n_ref, outflow=None, slip_cylinder=False, fixed=False, **overrides):
    """A cylinder deck with "simulation use wall bc periodic"."""
    d = deck(name)
    d.wall_bc_periodic = True
    if outflow is not None:
        d.outflow_bc = outflow
    if slip_cylinder:
        d.no_slip_cylinder = False
    if fixed:
        d.nonlinear_solver = "Picard"
    for k, v in overrides.items():
        setattr(d, k, v)
    m = d.mesh(n_ref)
    cmask = d.mask(m)
    params, w = d.operator_parameters(2.5e-4)
    case = Case(m, cmask, params, w, u_inf=d.u_max)
    case.deck = d
    case.node_master = d.node_master(m)
    case.pm = Map(m.dim, case.node_master, cmask)
    faces = d.outflow_faces(m)
    case.outflow = None if faces is None else (faces[0], faces[1], d.outflow)
    case.node_constraints = d.node_constraints(m) if slip_cylinder else None
    case.rows = slip_ref.Rows(m.dim, *case.node_constraints) if slip_cylinder else None
    return case


def oracle(case):
    """The oracle over the caller's connectivity with the group mask."""
    import oracle as orc
    om = orc.OracleMesh(case.mesh, case.pm.group_mask)
    o = orc.Oracle(om, **case.params)
    if case.outflow is not None:
        o.set_outflow_faces(*case.outflow)
    o.set_linearization_point(case.pm.resolve(case.u_star))
    if case.params["order"] > 0:
        o.set_previous_solution([case.pm.resolve(h) for h in case.hist], case.weights)
    return o


def gpu(case, precision="f64", brick=None, deterministic=False, u_star=None, hist=None):
    import glsamd
    op = glsamd.NavierStokesOperator(case.mesh, case.cmask, precision, brick=brick,
                                     outflow=case.outflow, node_constraints=case.node_constraints,
                                     node_master=case.node_master)
    op.set_parameters(**dict(case.params, deterministic=deterministic))
    op.set_linearization_point(case.u_star if u_star is None else u_star)
    if case.params["order"] > 0:
        op.set_previous_solution(case.hist if hist is None else hist, case.weights)
    return op


# ------------------------------------------------- shared by the GPU tests
RE100 = "input_turek_2D_Re100.json"
# (a) 2D Q1 2x2 y; (b) 2D Q2 2x1 y: the 2x2 brick spans the period of two
# cells; (c) 3D Q2 2x2x2 y and z: edges with three slaves; (d) 3D Q2 2x2x1 z:
# the 2x2x2 brick spans the period; (e) 2D Q2 cylinder r1 (curved cells; slave
# and master both Dirichlet at the inflow and outflow corners), once with "cut"
# outflow faces, once with slip rows on the cylinder
SHAPES = {
    "a_2d_q1": lambda fixed: box_case((2, 2), 1, 1, "y", fixed),
    "b_2d_q2_brick_period": lambda fixed: box_case((2, 1), 2, 1, "y", fixed),
    "c_3d_q2_yz": lambda fixed: box_case((2, 2, 2), 2, 1, "yz", fixed),
    "d_3d_q2_brick_period": lambda fixed: box_case((2, 2, 1), 2, 1, "z", fixed),
    "e_cylinder": lambda fixed: cylinder_case(RE100, 1, fixed=fixed, fe_degree=2),
    "e_cylinder_cut": lambda fixed: cylinder_case(RE100, 1, outflow="cut", fixed=fixed,
                                                  fe_degree=2),
    "e_cylinder_slip": lambda fixed: cylinder_case(RE100, 1, slip_cylinder=True, fixed=fixed,
                                                   fe_degree=2),
}
_cache = {}


def to_np(t):
    return t.double().cpu().numpy()


def poison(pm, v):
    """v with NaN on every slave entry"""
    v = np.array(v, dtype=np.float64, copy=True)
    v[pm.sdofs] = np.nan
    return v


def ref_case(shape, fixed=False):
    """The case, its oracle and the reference results, computed once."""
    key = (shape, fixed)
    if key not in _cache:
        case = SHAPES[shape](fixed)
        pm, rows = case.pm, case.rows
        assert len(pm.slaves) > 0
        o = oracle(case)
        if hasattr(case, "deck"):
            g = case.deck.constraint_values(case.mesh, 0.02)
        else:
            g = np.cos(np.arange(case.n_dofs) * 0.37) + 0.2
        ref = dict(vmult=vmult(o, pm, case.src, rows),
                   res=residual(o, pm, case.u_star, g, rows),
                   plain=residual_plain(o, pm, case.u_star, rows),
                   rhs=residual(o, pm, np.zeros(case.n_dofs), g, rows),
                   diag=diagonal(o, pm, rows, case.mesh), g=g)
        ref["inv"] = np.where(np.abs(ref["diag"]) > 1e-10, 1.0 / ref["diag"], 1.0)
        _cache[key] = (case, ref)
    return _cache[key]


def gpu_poisoned(case, prec, brick=None, deterministic=False):
    """The operator fed NaN on every slave entry of its state vectors."""
    pm = case.pm
    return gpu(case, prec, brick=brick, deterministic=deterministic,
               u_star=poison(pm, case.u_star), hist=[poison(pm, h) for h in case.hist])


# ------------------------------------------------------------- the multigrid
class _WrappedLevel:
    """A level operator with a periodic map: C^T A C, identity rows."""

    def __init__(self, o, pm):
        self.o, self.pm = o, pm

    def vmult(self, x):
        return vmult(self.o, self.pm, x)


class PeriodicOracleGMG:
    """mg_ref.OracleGMG with a periodic map on every level.  The oracle's
    level operators and transfers keep the caller's connectivity and the group
    masks; with P the oracle's prolongation between the full vectors, S_f the
    restriction to the fine masters and C_c the coarse "slave := master", the
    periodic prolongation is S_f P C_c and the restriction its transpose
    C_c^T P^T S_f^T.  "Constrained", for the power iteration's start vector,
    is what the operator holds: the masters' OR-ed mask and every slave dof."""

    def __new__(cls, meshes, cmasks, masters, params, u_star, hist=None, weights=None, **kw):
        import mg_ref
        import oracle as orc

        pms = [Map(m.dim, nm, cm) for m, nm, cm in zip(meshes, masters, cmasks)]

        class _GMG(mg_ref.OracleGMG):
            def prolongate_add(self, l, dst_f, src_c):
                t = np.zeros_like(dst_f)
                orc.prolongate_add(self.om_plain[l - 1], self.om_plain[l], self.child[l], t,
                                   self.pms[l - 1].resolve(src_c))
                t[self.pms[l].sdofs] = 0.0
                dst_f += t

            def restrict_add(self, l, dst_c, src_f):
                r = np.array(src_f, dtype=np.float64, copy=True)
                r[self.pms[l].sdofs] = 0.0
                t = np.zeros_like(dst_c)
                orc.restrict_add(self.om_plain[l - 1], self.om_plain[l], self.child[l], t, r)
                dst_c += self.pms[l - 1].transpose(t)

            def coarse_direct(self, b):
                """x_c = b_c on the identity rows, sparse LU of the free block"""
                import scipy.sparse.linalg as spl
                if not hasattr(self, "_lu0"):
                    A = sparse_constrained(self.plain_ops[0], self.meshes[0], self.pms[0])
                    free = np.nonzero(~self.pms[0].fixed)[0]
                    self._lu0 = spl.splu(A[free][:, free].tocsc())
                    self._free0 = free
                x = np.asarray(b, dtype=np.float64).copy()
                x[self._free0] = self._lu0.solve(x[self._free0])
                return x

        res = pms[-1].resolve
        g = _GMG(meshes, [pm.group_mask for pm in pms], params, res(u_star),
                 None if hist is None else [res(h) for h in hist], weights, **kw)
        g.pms = pms
        g.om_plain = g.om
        g.om = [orc.OracleMesh(m, pm.op_mask) for m, pm in zip(meshes, pms)]
        g.plain_ops = g.ops
        g.invdiag = [inverse_diagonal(o, pm) for o, pm in zip(g.ops, pms)]
        g.ops = [_WrappedLevel(o, pm) for o, pm in zip(g.ops, pms)]
        return g


def periodic_hierarchy(name, n_levels, **overrides):
    """(deck, meshes r0.., Dirichlet masks, node maps per level, params,
    weights) of a cylinder deck with "simulation use wall bc periodic"."""
    d = deck(name)
    d.wall_bc_periodic = True
    for k, v in overrides.items():
        setattr(d, k, v)
    meshes = [d.mesh(r) for r in range(n_levels)]
    cm = [d.mask(m) for m in meshes]
    masters = [d.node_master(m) for m in meshes]
    params, w = d.operator_parameters(2.5e-4)
    return d, meshes, cm, masters, params, w


gmres_right = slip_ref.gmres_right
