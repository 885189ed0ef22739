"""CPU restatement of the ILU(k) preconditioner of csrc/ilu_plan.cc and
csrc/ilu.hip (test infrastructure: the checker of gls_ilu_*, not a product
path).

The library's ILU stands for TrilinosWrappers::PreconditionILU (Ifpack,
preconditioner.cc:5-28, multigrid.cc:403-447); Ifpack is not available here,
so parity with it is unpinned and this file pins the implementation to the
published rules: the level-of-fill pattern in the matrix's own row order, the
diagonal modification a_ii <- rtol a_ii + sign(a_ii) atol (sign(0) = +1)
before a row-wise elimination, unit-diagonal L, and the dependency levels of
the two triangular solves.  Plain numpy / scipy; `dtype` lets the solve and
the factorisation run in np.longdouble for the tests' error floors."""
import numpy as np
import scipy.sparse as sp

from amg_ref import AMGRef


def symbolic(A, k):
    """pattern of ILU(k): (indptr, indices) with sorted columns, the diagonal
    always present"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    rows, levs = [], []  # per finished row: columns, levels of fill (dicts in column order)
    for i in range(n):
        lev = {int(c): 0 for c in A.indices[A.indptr[i]:A.indptr[i + 1]]}
        lev.setdefault(i, 0)
        done = set()
        while True:
            todo = [c for c in lev if c < i and c not in done]
            if not todo:
                break
            p = min(todo)
            done.add(p)
            lp = lev[p]
            for j, lj in zip(rows[p], levs[p]):
                if j <= p:
                    continue
                l = lp + lj + 1
                if l <= k and l < lev.get(j, k + 1):
                    lev[j] = l
        cols = sorted(lev)
        rows.append(cols)
        levs.append([lev[c] for c in cols])
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([c for r in rows for c in r], dtype=np.int64)
    return indptr, indices


def factor(A, k=0, atol=0.0, rtol=1.0, dtype=np.float64):
    """(L, U): L strictly lower (unit diagonal implied), U upper with the
    pivots, as scipy CSR of `dtype` on the ILU(k) pattern.  Raises
    ZeroDivisionError naming the row on a zero or non-finite pivot."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    indptr, indices = symbolic(A, k)
    val = np.zeros(indices.shape[0], dtype=dtype)
    diag = np.zeros(n, dtype=np.int64)
    where = np.full(n, -1, dtype=np.int64)  # column -> position in the current row
    for i in range(n):
        r0, r1 = indptr[i], indptr[i + 1]
        cols = indices[r0:r1]
        where[cols] = np.arange(r0, r1)
        diag[i] = where[i]
        val[where[A.indices[A.indptr[i]:A.indptr[i + 1]]]] = A.data[A.indptr[i]:A.indptr[i + 1]]
        d = val[diag[i]]
        val[diag[i]] = dtype(rtol) * d + (-dtype(atol) if d < 0 else dtype(atol))
        for q in range(r0, diag[i]):
            p = indices[q]
            l = val[q] / val[diag[p]]
            val[q] = l
            t = np.arange(diag[p] + 1, indptr[p + 1])
            w = where[indices[t]]
            val[w[w >= 0]] -= l * val[t[w >= 0]]
        where[cols] = -1
        piv = val[diag[i]]
        if piv == 0 or not np.isfinite(piv):
            raise ZeroDivisionError(f"ilu_ref: zero or non-finite pivot in row {i}")
    row = np.repeat(np.arange(n), np.diff(indptr))
    low = indices < row
    return _csr(val[low], row[low], indices[low], n), _csr(val[~low], row[~low], indices[~low], n)


def _csr(v, r, c, n):
    # by hand: the constructors may drop explicit zeros or change the dtype,
    # the pattern has to stay exactly the symbolic one (entries are row-major)
    out = sp.csr_matrix((n, n), dtype=np.float64)
    out.indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    out.indices, out.data = c.astype(np.int64), np.array(v)
    return out


def solve(L, U, b):
    """U^-1 L^-1 b, row by row in the dtype of the factors"""
    dt = L.data.dtype
    n = L.shape[0]
    x = np.array(b, dtype=dt)
    for i in range(n):
        q = slice(L.indptr[i], L.indptr[i + 1])
        x[i] -= np.dot(L.data[q], x[L.indices[q]])
    for i in range(n - 1, -1, -1):
        q = slice(U.indptr[i] + 1, U.indptr[i + 1])  # the pivot comes first
        x[i] = (x[i] - np.dot(U.data[q], x[U.indices[q]])) / U.data[U.indptr[i]]
    return x


def levels(L, U):
    """(level of each row for the forward solve, for the backward solve):
    level(i) = 1 + max level(j) over the row's off-diagonal columns, 0 without"""
    n = L.shape[0]
    ll = np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = L.indices[L.indptr[i]:L.indptr[i + 1]]
        ll[i] = 1 + ll[c].max() if len(c) else 0
    lu = np.zeros(n, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        c = U.indices[U.indptr[i]:U.indptr[i + 1]]
        c = c[c != i]
        lu[i] = 1 + lu[c].max() if len(c) else 0
    return ll, lu


class ILURef:
    """factor once, vmult = U^-1 L^-1"""

    def __init__(self, A, fill_level=0, atol=1e-12, rtol=1.0, dtype=np.float64):
        self.L, self.U = factor(A, fill_level, atol, rtol, dtype)
        self.n = self.L.shape[0]

    def vmult(self, b):
        return solve(self.L, self.U, b)


class AMGRefILU(AMGRef):
    """AMGRef with `sweeps` ILU steps as the smoother of every smoothed level
    (first step from a zero start x = M^-1 f, otherwise x += M^-1 (f - A x))
    and, with coarse_ilu, the same steps as the coarsest solve."""

    def __init__(self, A, smoother_ilu=True, coarse_ilu=True, ilu_fill=1, ilu_atol=1e-6,
                 ilu_rtol=1.0, **kw):
        super().__init__(A, **kw)
        self.smoother_ilu, self.coarse_ilu = smoother_ilu, coarse_ilu
        last = len(self.levels) - 1
        for l, L in enumerate(self.levels):
            if (smoother_ilu and l < last) or (coarse_ilu and l == last):
                L["ilu"] = ILURef(L["A"], ilu_fill, ilu_atol, ilu_rtol)

    def _ilu_steps(self, L, f, x):
        for _ in range(max(1, self.sweeps)):
            x = L["ilu"].vmult(f) if x is None else x + L["ilu"].vmult(f - L["A"] @ x)
        return x

    def _cheb(self, L, f, x):
        if "ilu" in L and L is not self.levels[-1]:
            return self._ilu_steps(L, f, x)
        return super()._cheb(L, f, x)

    def _vcycle(self, l, f):
        L = self.levels[l]
        if l + 1 == len(self.levels) and self.coarse_ilu:
            return self._ilu_steps(L, f, None)
        return super()._vcycle(l, f)


# ---- test matrices
def poisson(m):
    """m x m 5-point Poisson matrix, natural order"""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    return (sp.kron(I, T) + sp.kron(T, I)).tocsr()


def tridiagonal(n):
    i = np.arange(n)
    return sp.diags([-1.0 - 0.3 * np.sin(i[1:]), 2.5 + 0.1 * np.cos(i), -0.8 + 0.2 * np.sin(2.0 * i[:-1])],
                    [-1, 0, 1]).tocsr()


def stencil_block(shape, b, seed=0):
    """kron-like matrix of a 9-point (2-D) / 27-point (3-D) node stencil with
    a dense b x b block per node pair: the sparsity of a Q1 system matrix with
    b dofs per node, nonsymmetric values, diagonally dominant"""
    rng = np.random.default_rng(seed)
    S = None
    for m in shape:
        T = sp.diags([1.0, 1.0, 1.0], [-1, 0, 1], shape=(m, m))
        S = (T if S is None else sp.kron(S, T)).tocsr()
        S.eliminate_zeros()  # kron of small factors stores dense blocks
    P = sp.kron(S, np.ones((b, b))).tocsr()
    P.sort_indices()
    P.data = rng.uniform(-1.0, 1.0, P.nnz)
    d = np.abs(P).sum(axis=1).A1 + 1.0
    return (P + sp.diags(d)).tocsr()


def block3():
    """kron(P_12, dense 3 x 3): n = 432"""
    A = sp.kron(poisson(12), np.ones((3, 3))).tocsr()
    A.sort_indices()
    rng = np.random.default_rng(5)
    A.data = A.data * rng.uniform(0.5, 1.0, A.nnz)
    return (A + sp.diags(np.full(A.shape[0], 30.0))).tocsr()


def with_dirichlet(A, every=7):
    """identity rows and columns at every `every`-th dof (constrained dofs)"""
    A = sp.lil_matrix(A)
    idx = np.arange(0, A.shape[0], every)
    for i in idx:
        A[i, :] = 0
        A[:, i] = 0
        A[i, i] = 1.0
    A = A.tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def nonsymmetric(n=60, seed=2):
    """random sparse nonsymmetric matrix with diagonal entries of both signs"""
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=0.08, random_state=rng, format="lil")
    s = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    for i in range(n):
        A[i, i] = s[i] * (4.0 + rng.uniform())
    A = A.tocsr()
    A.sort_indices()
    return A
