"""TEST INFRASTRUCTURE: a hyper cube with smoothly displaced nodes, for any
degree the hyper-cube generator builds (1..3).

The cylinder and sphere generators stop at Q2, so this is the only curved
mesh at Q3: the isoparametric Q_k mapping through the displaced nodes makes
every cell truly non-affine while the domain stays the unit cube (the
displacement vanishes on its boundary).  WarpedMesh duck-types glsmesh.Mesh
for orc.OracleMesh and glsamd.NavierStokesOperator the way
glsmesh.ShuffledMesh does (dim, degree, n_cells, n_nodes, n_dofs, cell_nodes,
coords, node_boundary, brick(), cell_measure())."""
import numpy as np


def displacement(X, amp=0.06, flat_axis=None):
    """u_d = amp (1 + d/2) cos(1.3 X_{d+1}) prod_e sin(pi X_e), times
    8 max(0, X_a - 1/2)^2 with flat_axis = a (exactly 0 for X_a <= 1/2)."""
    X = np.asarray(X, dtype=np.float64)
    dim = X.shape[1]
    bubble = np.prod(np.sin(np.pi * X), axis=1)
    if flat_axis is not None:
        bubble = bubble * 8.0 * np.maximum(0.0, X[:, flat_axis] - 0.5) ** 2
    u = np.empty_like(X)
    for d in range(dim):
        u[:, d] = amp * (1.0 + d / 2.0) * np.cos(1.3 * X[:, (d + 1) % dim]) * bubble
    return u


class WarpedMesh:
    """gm.hypercube(dim, k, n_ref) with displaced nodes.

    flat_axis=a: cells with X_a <= 1/2 stay exactly Cartesian, so one mesh
    holds both geometry classes of the operator.
    keep: indices of the cells to retain, node numbering unchanged (nodes no
    kept cell touches stay in the vectors with empty rows); brick() is then
    (0, 0, 0), the per-cell kernel.
    cell_measure(): the base's (measure, hmin) scaled per cell by
    f_c = 1 + 0.3 sin(c) resp. f_c^(1/dim): inputs to both sides, only there
    so that h differs from cell to cell.
    ref_coords: the undisplaced coordinates (constraint masks by position)."""

    def __init__(self, base, amp=0.06, flat_axis=None, keep=None):
        self.base = base
        self.dim, self.degree = base.dim, base.degree
        self.n_nodes = base.n_nodes
        self.ref_coords = np.array(base.coords, dtype=np.float64)
        self.coords = self.ref_coords + displacement(self.ref_coords, amp, flat_axis)
        self.node_boundary = np.asarray(base.node_boundary)
        self.keep = None if keep is None else np.asarray(keep, dtype=np.int64)
        cn = np.asarray(base.cell_nodes)
        self.cell_nodes = np.ascontiguousarray(cn if keep is None else cn[self.keep])
        self.n_cells = self.cell_nodes.shape[0]

    @property
    def n_dofs(self):
        return self.n_nodes * (self.dim + 1)

    def brick(self):
        return self.base.brick() if self.keep is None else (0, 0, 0)

    def cell_measure(self):
        meas, hmin = self.base.cell_measure()
        f = 1.0 + 0.3 * np.sin(np.arange(self.base.n_cells, dtype=np.float64))
        meas, hmin = np.asarray(meas) * f, np.asarray(hmin) * f ** (1.0 / self.dim)
        if self.keep is not None:
            meas, hmin = meas[self.keep], hmin[self.keep]
        return np.ascontiguousarray(meas), np.ascontiguousarray(hmin)

    def touched_nodes(self):
        """Boolean [n_nodes]: the nodes some cell of the mesh lists."""
        t = np.zeros(self.n_nodes, bool)
        t[np.asarray(self.cell_nodes, dtype=np.int64).ravel()] = True
        return t


def position_mask(ref_coords):
    """The constraint mask of the degree tests: all velocity bits on the
    faces X_0 = 0 and X_1 = 0, the pressure bit on X_0 = 1."""
    X = np.asarray(ref_coords)
    dim = X.shape[1]
    m = np.zeros(len(X), np.uint8)
    m[(np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 1]) < 1e-12)] |= (1 << dim) - 1
    m[np.abs(X[:, 0] - 1.0) < 1e-12] |= 1 << dim
    return m


def drop_middle(n_cells, n_keep):
    """n_keep of n_cells cell indices, the dropped ones taken from the middle
    of the list and not adjacent to each other."""
    n_drop = n_cells - n_keep
    drop = n_cells // 2 + 2 * (np.arange(n_drop) - n_drop // 2)
    return np.setdiff1d(np.arange(n_cells), drop)
