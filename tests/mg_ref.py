"""numpy restatements behind the p-multigrid tests (a helper, not a test): TensorProductPRefinementTransferOperator
(fem/transfer.cpp:2223-2592) with ElementRestriction::BooleanMask (fem/restriction.cpp:248-283), and Multigrid's
V-cycle (fem/multigrid.cpp:106-232) with the prolongations' essential rows and columns removed as
GeometricMultigrid does (fem/multigrid.cpp:296-309, RectangularConstrainedOperator), over cheb_ref's smoother and
PCG.

Transfer(..., dtype): float64 restates the reference (the 1D table from the oracle's gauss_lobatto / basis_eval,
the sum factorisation x, y, z of Prolongation3D and of Restriction3D); numpy.longdouble is the 80-bit evaluation
the componentwise constant is measured against (the table from the product form on the float64 nodes, as
hp_ref.tables).  bound_*(x) is S = |B| (x) |B| (x) |B| |x| through the same maps.

C_XFER follows hp_ref.py's rule: c_ref = the worst constant of the float64 restatement against the 80-bit one over
tests/test_mg_reference.py's case matrix (both directions, the six (pc, pf), temperature-like inputs
37 + 20 exp(-10 |p|^2)) = 3.50 (Mult, p 3 -> 4; 1.3 .. 3.0 elsewhere); 4 c_ref = 14, rounded up to a power of two.
The chains are short: Dc (or Df) terms per stage, three stages, plus the valence of a coarse dof in the restriction.
"""
import numpy as np

import cheb_ref as CR
import hp_ref as HP
from hp_ref import LD, U  # noqa: F401

C_XFER = 16.0


def basis(pc, pf, dtype=np.float64):
    """B [Df][Dc]: the coarse GLL Lagrange basis at the fine GLL nodes."""
    import oracle as O
    xc, xf = O.gauss_lobatto(pc + 1)[0], O.gauss_lobatto(pf + 1)[0]
    if dtype is LD:
        return HP.tables(pc, pf + 1, pts=xf)[0]
    return np.array([O.basis_eval(pc, xc, y)[0] for y in xf])


def owner_mask(gm_f, nf):
    """BooleanMask: 1 at an L-dof's first occurrence in the fine E-vector (the lowest element holding it)."""
    flat = np.asarray(gm_f).reshape(-1)
    first = np.full(nf, -1, np.int64)
    # (reversed assignment: the lowest E-vector index wins)
    first[flat[::-1]] = np.arange(flat.size - 1, -1, -1)
    return (first[flat] == np.arange(flat.size)).reshape(np.asarray(gm_f).shape)


class Transfer:
    def __init__(self, gm_c, nc, pc, gm_f, nf, pf, dtype=np.float64):
        self.gc, self.gf = np.asarray(gm_c, np.int64), np.asarray(gm_f, np.int64)
        self.nc, self.nf, self.pc, self.pf, self.dtype = nc, nf, pc, pf, dtype
        self.ne = self.gc.shape[0]
        assert self.gf.shape[0] == self.ne
        self.B = basis(pc, pf, dtype)
        self.mask = owner_mask(self.gf, nf)
        assert self.mask.sum() == nf

    def _prolong(self, B, x):
        Dc = self.pc + 1
        xe = np.asarray(x, self.dtype)[self.gc].reshape(self.ne, Dc, Dc, Dc)      # [e][dz][dy][dx]
        t = np.einsum("xa,ecba->ecbx", B, xe)
        t = np.einsum("yb,ecbx->ecyx", B, t)
        ye = np.einsum("zc,ecyx->ezyx", B, t).reshape(self.ne, -1)
        y = np.zeros(self.nf, self.dtype)
        y[self.gf[self.mask]] = ye[self.mask]                                       # every dof once, by its owner
        return y

    def _restrict(self, B, x):
        Df = self.pf + 1
        xe = (np.asarray(x, self.dtype)[self.gf] * self.mask).reshape(self.ne, Df, Df, Df)
        t = np.einsum("xa,ezyx->ezya", B, xe)
        t = np.einsum("yb,ezya->ezba", B, t)
        ye = np.einsum("zc,ezba->ecba", B, t).reshape(-1)
        y = np.zeros(self.nc, self.dtype)
        np.add.at(y, self.gc.reshape(-1), ye)                                       # ascending E-vector order
        return y

    def mult(self, x):
        return self._prolong(self.B, x)

    def mult_transpose(self, x):
        return self._restrict(self.B, x)

    def bound_mult(self, x):
        return self._prolong(np.abs(self.B), np.abs(np.asarray(x, self.dtype)))

    def bound_mult_transpose(self, x):
        return self._restrict(np.abs(self.B), np.abs(np.asarray(x, self.dtype)))

    def dense(self):
        I = np.eye(self.nc)
        return np.stack([self.mult(I[:, j]) for j in range(self.nc)], axis=1)


class Level:
    """One level of the cycle: the unconstrained Mult, the essential dofs, the smoother x -> S x and (for a coarse
    PCG) Jacobi's dinv."""

    def __init__(self, mult, ess, smoother, dinv=None):
        self.mult, self.ess, self.S, self.dinv = mult, np.asarray(ess, np.int64), smoother, dinv
        self.A = CR.constrained(mult, ess)


def vcycle(levels, transfers, pre=1, post=1, coarse_pcg=None, dot="matmul"):
    """MultigridBase::Mult as a callable x -> y: one V-cycle from a zero guess.  coarse_pcg: None (the coarsest
    level's smoother once) or (rel_tol, max_iter) (a constrained Jacobi-PCG there)."""
    def coarse(X):
        l = levels[0]
        if coarse_pcg is None:
            return l.S(X)
        rel_tol, max_iter = coarse_pcg
        return CR.pcg(l.mult, X, l.ess, lambda a: l.dinv * a, rel_tol=rel_tol, max_iter=max_iter, dot=dot).x

    def step(l, X, Y):
        R = X - l.A(Y)
        return Y + l.S(R)

    def cycle(k, X):
        if k == 0:
            return coarse(X)
        l, c, P = levels[k], levels[k - 1], transfers[k - 1]
        Y = np.zeros_like(X)
        for i in range(pre):
            Y = l.S(X) if i == 0 else step(l, X, Y)
        R = X - l.A(Y)
        R[l.ess] = 0.0
        Xc = P.mult_transpose(R)
        Xc[c.ess] = 0.0
        Yc = cycle(k - 1, Xc)
        Yc = Yc.copy()
        Yc[c.ess] = 0.0
        Z = P.mult(Yc)
        Z[l.ess] = 0.0
        Y = Y + Z
        for _ in range(post):
            Y = step(l, X, Y)
        return Y
    return lambda x: cycle(len(levels) - 1, np.asarray(x, np.float64))
