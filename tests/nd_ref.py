"""TEST INFRASTRUCTURE: a numpy restatement of the nested-dissection coarse
solver's algebra over the library's plan (glsamd.NdPlan): fronts from cell
blocks, the bottom-up elimination with explicit pivot-block inverses and the
forward / backward sweeps, all dense numpy per tree node.

Per tree node t with own dofs I and boundary dofs B (front order: I, then B):
  Z = F_II^-1, W = F_BI Z, G = Z F_IB, U = F_BB - W F_IB  (U -> the parent)
  forward:  f = [b_I ; 0] + children's f_B;  f_B -= W f_I
  backward: x_I = Z f_I - G x_B
"""
import numpy as np


def node_dof_counts(mesh, cmask, condense=True):
    """Participating dofs per mesh node as the direct coarse solver counts
    them: the free components, and 0 for the cell-interior nodes of a
    Q_k, k >= 2 mesh when the cells' interiors are condensed."""
    nc = mesh.dim + 1
    cm = np.asarray(cmask, dtype=np.int64)
    w = np.array([nc - bin(int(m) & ((1 << nc) - 1)).count("1") for m in cm], dtype=np.int32)
    k = mesh.degree
    if condense and k >= 2:
        p = np.arange((k + 1) ** mesh.dim)
        co = [p % (k + 1), (p // (k + 1)) % (k + 1)]
        if mesh.dim == 3:
            co.append(p // ((k + 1) ** 2))
        inside = np.all([(c > 0) & (c < k) for c in co], axis=0)
        cn = np.asarray(mesh.cell_nodes).reshape(mesh.n_cells, -1)
        w[np.unique(cn[:, inside])] = 0
    return w


def plan_cell_dofs(cell_nodes, node_dofs):
    """[n_cells][nq * ncmax] plan dofs of each cell (-1: none); plan dofs are
    numbered mesh node by mesh node."""
    cn = np.asarray(cell_nodes, dtype=np.int64)
    w = np.asarray(node_dofs, dtype=np.int64)
    d0 = np.concatenate([[0], np.cumsum(w)])
    ncmax = int(w.max())
    out = -np.ones((cn.shape[0], cn.shape[1] * ncmax), dtype=np.int64)
    for k in range(ncmax):
        has = w[cn] > k
        out[:, k::ncmax][has] = (d0[cn] + k)[has]
    return out


def leaf_fronts(plan, cell_dofs, E):
    """Front of every leaf: the sum of its cells' blocks E[c] (on the cell's
    dofs cell_dofs[c], -1 entries dropped) on I then B."""
    fronts = {}
    for t, nd in enumerate(plan.nodes):
        if nd["child"][0] >= 0:
            continue
        idx = np.concatenate([nd["own"], nd["boundary"]]).astype(np.int64)
        pos = {int(d): i for i, d in enumerate(idx)}
        F = np.zeros((len(idx), len(idx)))
        for c in nd["cells"]:
            loc = [i for i, d in enumerate(cell_dofs[c]) if d >= 0]
            at = [pos[int(cell_dofs[c][i])] for i in loc]  # KeyError: B misses a dof
            F[np.ix_(at, at)] += E[c][np.ix_(loc, loc)]
        fronts[t] = F
    return fronts


def factor(plan, fronts):
    """Bottom-up elimination; returns {t: (Z, W, G)}."""
    nodes = plan.nodes
    F = dict(fronts)
    fac = {}
    for t in sorted(range(len(nodes)), key=lambda t: -nodes[t]["level"]):
        nd = nodes[t]
        ni, nb = len(nd["own"]), len(nd["boundary"])
        if t not in F:
            F[t] = np.zeros((ni + nb, ni + nb))
            for c in nd["child"]:
                m = nodes[c]["map"]
                F[t][np.ix_(m, m)] += fac[c][3]
        Ft = F[t]
        Z = np.linalg.inv(Ft[:ni, :ni]) if ni else np.zeros((0, 0))
        W = Ft[ni:, :ni] @ Z
        G = Z @ Ft[:ni, ni:]
        U = Ft[ni:, ni:] - W @ Ft[:ni, ni:]
        fac[t] = (Z, W, G, U)
    return {t: f[:3] for t, f in fac.items()}


def solve(plan, fac, b):
    nodes = plan.nodes
    order = sorted(range(len(nodes)), key=lambda t: -nodes[t]["level"])
    f = {}
    for t in order:
        nd = nodes[t]
        ni, nb = len(nd["own"]), len(nd["boundary"])
        v = np.zeros(ni + nb)
        v[:ni] = b[nd["own"]]
        for c in nd["child"]:
            if c >= 0:
                v[nodes[c]["map"]] += f[c][len(nodes[c]["own"]):]
        v[ni:] -= fac[t][1] @ v[:ni]
        f[t] = v
    x = np.zeros_like(b, dtype=np.float64)
    for t in reversed(order):
        nd = nodes[t]
        ni = len(nd["own"])
        Z, _, G = fac[t]
        x[nd["own"]] = Z @ f[t][:ni] - G @ x[nd["boundary"]]
    return x
