"""numpy restatement behind the h-multigrid tests (a helper, not a test): FiniteElementSpace::RefinementOperator
(fem/fespace.cpp:1833-2120) between an H1 space on a hex mesh and the H1 space of the same order on its uniform
refinement, as the reference writes it: dense D^3 x D^3 local matrices (GetLocalRefinementMatrices, :1786-1807:
the parent's 3D shape values -- products of the 1D ones -- at the child's nodes, entries below 1e-12 set to zero,
fem/fe/fe_base.cpp:884-893), the fine elements visited in ascending order, the `processed` marks of MultTranspose
(:2030-2085) deciding which element's entry of a shared fine dof counts.  Mult uses the same marks (every fine dof
is set once, by the first element that holds it; the reference's Mult lets the last SetSubVector stand, and the
elements that share a dof compute the same value up to rounding, which C_HXFER covers).

HTransfer(..., dtype): float64 restates the reference (1D values from the oracle's gauss_lobatto / basis_eval);
numpy.longdouble is the 80-bit evaluation the componentwise constant is measured against (1D values from the
product form on the float64 nodes, hp_ref.tables).  bound_*(x) is S = |P| |x| and |P|^T |x| through the same maps and
marks.  The cycle and the PCG over it are mg_ref.vcycle and cheb_ref.pcg, which take these transfers as they are.

C_HXFER follows hp_ref.py's rule: c_ref = the worst constant of the float64 restatement against the 80-bit one over
tests/hmg_cases.py's transfer cases (both directions, random and temperature-like inputs) = 8.37 (Mult, moved 3 x 2 x 2, p = 4, random; 5.2 with the temperature there, 1.0 .. 4.1 at p <= 3);
4 c_ref = 33.5, rounded up to a power of two.  The restatement's chain is the dense row: D^3 = 125 terms in one
dot product at p = 4 -- longer than the tensor form's three stages of D terms, which the device is therefore well
inside -- plus, in the restriction, the children and parents that reach a coarse dof.

CYCLE_TOL, the device tolerance of a fixed-work V-cycle and of six PCG iterations relative to max|x|:
tests/test_hmg_reference.py measures the spread of both under three summation orders and asserts that it stays
100 x below 1e-12 (it is 1e-15 or less), as tests/test_mg_reference.py did for the p-cycle.
"""
import numpy as np

import hp_ref as HP
from hp_ref import LD, U  # noqa: F401

C_HXFER = 64.0
CYCLE_TOL = 1e-12
ZERO = 1e-12


def shape1d(p, dtype=np.float64):
    """[o][q][d]: the parent's 1D basis function d at child o's node q, l_d((o + xi_q) / 2), not thresholded."""
    import oracle as O
    xi = O.gauss_lobatto(p + 1)[0]
    out = []
    for o in (0, 1):
        pts = 0.5 * (o + xi)
        if dtype is LD:
            out.append(HP.tables(p, p + 1, pts=0.5 * (LD(o) + xi.astype(LD)))[0])
        else:
            out.append(np.array([O.basis_eval(p, xi, y)[0] for y in pts]))
    return np.stack(out)


def tables1d(p, dtype=np.float64):
    """The thresholded 1D tables B_o [o][q][d] of the tensor form."""
    B = shape1d(p, dtype).copy()
    B[np.abs(B) < ZERO] = 0
    return B


def local_matrix(p, octant, dtype=np.float64):
    """The reference's dense local matrix of an octant, [i][j] lexicographic fine / coarse local dofs: the 3D shape
    values, thresholded."""
    s = shape1d(p, dtype)
    ox, oy, oz = octant & 1, (octant >> 1) & 1, octant >> 2
    n = (p + 1) ** 3
    # shape_x(i) * shape_y(j) * shape_z(k) (H1_HexahedronElement::CalcShape)
    M = ((s[ox][None, None, :, None, None, :] * s[oy][None, :, None, None, :, None])
         * s[oz][:, None, None, :, None, None]).reshape(n, n)
    M = M.copy()
    M[np.abs(M) < ZERO] = 0
    return M


def tensor_matrix(p, octant, dtype=np.float64):
    """B_oz (x) B_oy (x) B_ox from the thresholded 1D tables (what the device applies, never forming it)."""
    B = tables1d(p, dtype)
    ox, oy, oz = octant & 1, (octant >> 1) & 1, octant >> 2
    return np.kron(B[oz], np.kron(B[oy], B[ox]))


def processed_mask(gm_f, nf):
    """1 where the fine element is the first, in ascending order, to hold the dof (not yet `processed`)."""
    flat = np.asarray(gm_f).reshape(-1)
    first = np.full(nf, -1, np.int64)
    first[flat[::-1]] = np.arange(flat.size - 1, -1, -1)
    return (first[flat] == np.arange(flat.size)).reshape(np.asarray(gm_f).shape)


class HTransfer:
    def __init__(self, gm_c, nc, gm_f, nf, p, parent, octant, dtype=np.float64):
        self.gc, self.gf = np.asarray(gm_c, np.int64), np.asarray(gm_f, np.int64)
        self.parent, self.octant = np.asarray(parent, np.int64), np.asarray(octant, np.int64)
        self.nc, self.nf, self.p, self.dtype = nc, nf, p, dtype
        assert self.gf.shape[0] == self.parent.size == self.octant.size
        self.lP = np.stack([local_matrix(p, o, dtype) for o in range(8)])
        self.mask = processed_mask(self.gf, nf)
        assert self.mask.sum() == nf

    def _prolong(self, lP, x):
        xe = np.asarray(x, self.dtype)[self.gc[self.parent]]                       # [f][j]: the parent's dofs
        ye = np.zeros(self.gf.shape, self.dtype)
        for o in range(8):
            sel = self.octant == o
            ye[sel] = xe[sel] @ lP[o].T                                            # lP.Mult(subX, subY)
        y = np.zeros(self.nf, self.dtype)
        y[self.gf[self.mask]] = ye[self.mask]
        return y

    def _restrict(self, lP, x):
        xe = np.asarray(x, self.dtype)[self.gf] * self.mask                        # processed entries zeroed
        ce = np.zeros(self.gf.shape, self.dtype)
        for o in range(8):
            sel = self.octant == o
            ce[sel] = xe[sel] @ lP[o]                                              # lP.MultTranspose(subX, subY)
        y = np.zeros(self.nc, self.dtype)
        np.add.at(y, self.gc[self.parent].reshape(-1), ce.reshape(-1))             # ascending fine elements
        return y

    def mult(self, x):
        return self._prolong(self.lP, x)

    def mult_transpose(self, x):
        return self._restrict(self.lP, x)

    def bound_mult(self, x):
        return self._prolong(np.abs(self.lP), np.abs(np.asarray(x, self.dtype)))

    def bound_mult_transpose(self, x):
        return self._restrict(np.abs(self.lP), np.abs(np.asarray(x, self.dtype)))

    def dense(self):
        I = np.eye(self.nc)
        return np.stack([self.mult(I[:, j]) for j in range(self.nc)], axis=1)
