"""hp_ref.py -- extended-precision (80-bit numpy.longdouble) reference of the PA operator, and the
componentwise criterion measured against it (TEST INFRASTRUCTURE ONLY, numpy only).

    y = R^T (B^T M B + G^T D G) R x,   M = W alpha det J,   D = W beta adj(J) adj(J)^T / det J

on hexahedra with corner (trilinear) geometry, evaluated by plain einsum contractions in longdouble
from float64 inputs that are taken as exact: the corner coordinates, the gather map, the 1D
Gauss-Legendre points / weights and Gauss-Lobatto nodes (oracle.gauss_legendre / gauss_lobatto), the
per-point coefficients and x.  B and G come from the Lagrange product form, not from the oracle's
barycentric evaluation.  The reference's own rounding error is about k * 1.1e-19 * S_i, 10^3 below
what it measures.

The criterion.  bound(x) is S, the same expression with every factor replaced by its magnitude
(|B|, |G|, |x|, |M|, W |beta| |adj J| |adj J|^T / |det J|, entrywise, before the product): the running
bound of the sum-factorised evaluation, so a float64 evaluation's error is k u S_i componentwise with
u = 2^-53 and k a small multiple of the number of roundings per term.  constant(y, y_hp, S) is
max_i |y_i - y_hp,i| / (u S_i) over all dofs.  Unlike the global relerr <= 1e-12 it holds for inputs
whose sums cancel (temperature fields), and it is as tight as the arithmetic: a 1e-12 relative error at
one quadrature point is hundreds of units.

C and C_DIAG are the bounds of the device tests: 4 * c_ref rounded up to a power of two, where c_ref
is the worst constant of the CPU oracle over the case matrix -- of its two independent Mult evaluations
(PA and element-matrix) for C, of its diagonal for C_DIAG (tests/test_hp_reference.py measures both and
checks the constants against them; DESIGN.md "Tolerance" has the tables and the reasoning).  C_CONV and
C_CONV_QD are the same rule for the convection term's products and its qdata, whose reference and bound
live in tests/conv_ref.py (measured by tests/test_conv_reference.py).  C_LF / C_LF_JOULE
(the device linear form: tests/lform_ref.py, tests/test_lform_reference.py) and C_BDR /
C_BDR_DIAG / C_BDR_QD (the Robin face terms: tests/bdr_ref.py, tests/test_bdr_reference.py, section 4b) likewise,
over the case matrix of tests/rhs_cases.py.
"""
import numpy as np

LD = np.longdouble
# 80-bit extended precision (x86-64): a missing type is a hard failure, not a skip
assert np.finfo(LD).eps < 2e-19, "numpy.longdouble is not the 80-bit extended type: %r" % np.finfo(LD).eps

U = 2.0 ** -53          # float64 unit roundoff

# Mult: c_ref = 11.1 (the oracle's PA path, 8 x 8 x 5 non-aligned, p = 2), 4 * c_ref = 44 -> 64.  The sum-factorised
# chains are short: D or Q terms per stage, six stages, plus the dof's valence.
C = 64.0
# Diagonal: c_ref = 41.8 (p = 4, Q = 6), 4 * c_ref = 167 -> 256.  It has a constant of its own because
# the oracle (the reference's AssembleDiagonalPA restated) adds all Q^3 = 27 ... 216 point terms of an
# entry in ONE running sum, each a product of 7 - 9 factors, and the terms are mostly of one sign (S_i
# is close to d_i), so the error grows with that chain: 3 - 10 at p = 1, 7 - 26 at p = 2, 20 - 42 at
# p = 4.  One bound for both would be 256 for the Mult too, above the 190 - 620 units of a 1e-12
# relative error at one quadrature point, which the Mult bound must see.
C_DIAG = 256.0
# The convection term (tests/conv_ref.py: S and Pabs over the edge-form |J|; tests/test_conv_reference.py measures
# both).  Mult and MultTranspose jointly: c_ref = 4.13 (the float64 checker's dense element matrices, perturbed
# 5 x 4 x 3, p = 1, Q = 2), 4 * c_ref = 16.5 -> 32.  The chains are those of the volume Mult with one qdata
# factor per point instead of a 3 x 3 product.
C_CONV = 32.0
# Its qdata alpha W adj(J) v against Pabs: c_ref = 7.14 (perturbed, p = 4, Q = 6), 4 * c_ref = 28.6 -> 32: two
# roundings per Jacobian entry, a difference of two products per cofactor, three terms and two scalings.
C_CONV_QD = 32.0
# The device linear form (tests/lform_ref.py: LFRef.bound; tests/test_lform_reference.py measures it over
# tests/rhs_cases.py).  Point, grid-function and affine sources: c_ref = 9.06 (the float64 checker, perturbed
# 5 x 4 x 4, p = 4, Q = 5, the signed per-point source), 4 * c_ref = 36.2 -> 64.  The chains are the mass Mult's
# second half -- three B^T stages and the dof's valence -- behind det J's 14 operations.
C_LF = 64.0
# The Joule source: c_ref = 3.19 (perturbed, p = 4, Q = 6, the electrode potential, constant sigma), 4 * c_ref =
# 12.8 -> 16.  Smaller than C_LF because its F carries the gradient's own running bound: 2 |g| Sg is several
# times |g|^2 even where nothing cancels.
C_LF_JOULE = 16.0
# The Robin face terms (tests/bdr_ref.py; tests/test_bdr_reference.py).  Mult (both of the checker's
# evaluations) and the face linear form: c_ref = 7.75 (the face linear form, perturbed 5 x 4 x 3, p = 4, the
# default 3-point rule, signed g), 4 * c_ref = 31.0 -> 32.
C_BDR = 32.0
# The face diagonal: c_ref = 8.39 (perturbed, p = 4, Q = 6), 4 * c_ref = 33.5 -> 64: Q^2 = 36 terms of one sign in
# one running sum.
C_BDR_DIAG = 64.0
# The face qdata W c |x_xi x x_eta| against W |c| Dabs: c_ref = 4.87 (perturbed, p = 4, Q = 6), 4 * c_ref = 19.5 -> 32.
C_BDR_QD = 32.0


def _oracle():
    import oracle
    return oracle


def tables(p, q1d, pts=None):
    """B, G [Q][D] in longdouble: the Lagrange basis on the float64 GLL nodes and its derivative at
    the float64 Gauss-Legendre points (or at `pts`), from the product form."""
    O = _oracle()
    nodes = O.gauss_lobatto(p + 1)[0].astype(LD)
    pts = O.gauss_legendre(q1d)[0].astype(LD) if pts is None else np.asarray(pts, LD)
    D = p + 1
    B = np.ones((q1d, D), LD)
    G = np.zeros((q1d, D), LD)
    for j in range(D):
        for i in range(D):
            if i != j:
                B[:, j] *= (pts - nodes[i]) / (nodes[j] - nodes[i])
        for k in range(D):
            if k == j:
                continue
            t = np.full(q1d, LD(1) / (nodes[j] - nodes[k]), LD)
            for i in range(D):
                if i != j and i != k:
                    t *= (pts - nodes[i]) / (nodes[j] - nodes[i])
            G[:, j] += t
    return B, G


def _interp(Tx, Ty, Tz, xe):
    """[e][dz][dy][dx] -> [e][qz][qy][qx] with the 1D tables Tx, Ty, Tz [Q][D]."""
    t = np.einsum("xa,ecba->ecbx", Tx, xe)
    t = np.einsum("yb,ecbx->ecyx", Ty, t)
    return np.einsum("zc,ecyx->ezyx", Tz, t)


def _interp_t(Tx, Ty, Tz, fq):
    """The transpose: [e][qz][qy][qx] -> [e][dz][dy][dx]."""
    t = np.einsum("zc,ezyx->ecyx", Tz, fq)
    t = np.einsum("yb,ecyx->ecbx", Ty, t)
    return np.einsum("xa,ecbx->ecba", Tx, t)


class HPRef:
    """The operator of one (mesh, p, q1d, alpha, beta): enodes [ne][3][8] lexicographic corners, gm
    [ne][(p+1)^3] lexicographic gather map, alpha / beta a scalar, [ne][nq] float64 (or longdouble)
    values in the oracle's point order, or None (integrator absent).  rule: (points, weights) in
    longdouble in place of the float64 Gauss-Legendre tables -- only for pinning this code against
    analytic values, where the float64 tables' own rounding (2e-17 to 2e-16 on the unit cube's entries) would show;
    every comparison with the oracle or the device uses the float64 tables all three share."""

    def __init__(self, enodes, gm, ndofs, p, q1d, alpha=None, beta=None, rule=None):
        O = _oracle()
        self.p, self.q1d, self.ndofs = p, q1d, int(ndofs)
        self.gm = np.asarray(gm, np.int64)
        self.ne = ne = self.gm.shape[0]
        Q = q1d
        pts, w1 = (np.asarray(a).astype(LD) for a in (O.gauss_legendre(q1d) if rule is None else rule))
        self.B, self.G = tables(p, q1d, pts)
        W = (w1[:, None, None] * w1[None, :, None] * w1[None, None, :])   # [qz][qy][qx]
        # trilinear map: N_a = prod over directions of (xi or 1 - xi), a = ax + 2 ay + 4 az
        N1 = np.stack([1 - pts, pts], 1)                                  # [Q][2]
        dN1 = np.stack([-np.ones(Q, LD), np.ones(Q, LD)], 1)
        Xc = np.asarray(enodes, np.float64).astype(LD).reshape(ne, 3, 2, 2, 2)   # [e][i][az][ay][ax]

        def tri(Tx, Ty, Tz):
            return np.einsum("xa,yb,zc,eicba->eizyx", Tx, Ty, Tz, Xc)
        self.X = tri(N1, N1, N1)                                          # [e][i][qz][qy][qx]
        Xo = O.quad_points(np.asarray(enodes, np.float64), q1d)           # [e][nq][3]
        mine = np.transpose(self.X.reshape(ne, 3, Q ** 3), (0, 2, 1))
        assert np.abs(mine - Xo).max() <= 1e-14, "point order / coordinates differ from oracle.quad_points"
        # J[e][i][j] = d x_i / d xi_j; rows of adj(J) are the cross products of J's columns
        c = [tri(dN1, N1, N1), tri(N1, dN1, N1), tri(N1, N1, dN1)]        # columns j: [e][i][z][y][x]

        def cross(a, b):
            return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                             a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                             a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        A = np.stack([cross(c[1], c[2]), cross(c[2], c[0]), cross(c[0], c[1])], 1)   # [e][r][i][z][y][x]
        det = np.einsum("eizyx,eizyx->ezyx", c[0], A[:, 0])
        self.detJ, self.adjJ, self.W = det, A, W

        def coef(v):
            if v is None:
                return None
            if np.ndim(v) == 0:
                return np.full((ne, Q, Q, Q), LD(float(v)), LD)
            v = np.asarray(v)
            assert v.size == ne * Q ** 3
            return v.astype(LD).reshape(ne, Q, Q, Q)
        a, b = coef(alpha), coef(beta)
        self.M = self.Mabs = self.D = self.Dabs = None
        if a is not None:
            self.M = W * a * det
            self.Mabs = W * np.abs(a) * np.abs(det)
        if b is not None:
            self.D = np.einsum("ezyx,erizyx,esizyx->erszyx", W * b / det, A, A)
            Aa = np.abs(A)
            self.Dabs = np.einsum("ezyx,erizyx,esizyx->erszyx", W * np.abs(b) / np.abs(det), Aa, Aa)

    # ---- the operator --------------------------------------------------------------------------
    def _apply(self, B, G, M, D, x):
        D1 = self.p + 1
        xe = x[self.gm].reshape(self.ne, D1, D1, D1)
        ye = np.zeros_like(xe)
        if M is not None:
            ye += _interp_t(B, B, B, M * _interp(B, B, B, xe))
        if D is not None:
            g = np.stack([_interp(G, B, B, xe), _interp(B, G, B, xe), _interp(B, B, G, xe)], 1)   # [e][s]...
            f = np.einsum("erszyx,eszyx->erzyx", D, g)
            ye += _interp_t(G, B, B, f[:, 0]) + _interp_t(B, G, B, f[:, 1]) + _interp_t(B, B, G, f[:, 2])
        y = np.zeros(self.ndofs, LD)
        np.add.at(y, self.gm.ravel(), ye.reshape(-1))
        return y

    def mult(self, x):
        """y_hp = A x in longdouble (x: float64 values taken as exact)."""
        return self._apply(self.B, self.G, self.M, self.D, np.asarray(x).astype(LD))

    def bound(self, x):
        """S: the same sums over the magnitudes of every factor."""
        return self._apply(np.abs(self.B), np.abs(self.G), self.Mabs, self.Dabs, np.abs(np.asarray(x)).astype(LD))

    # ---- the diagonal --------------------------------------------------------------------------
    def _diag(self, B, G, M, D):
        D1 = self.p + 1
        de = np.zeros((self.ne, D1, D1, D1), LD)
        if M is not None:
            de += _interp_t(B * B, B * B, B * B, M)
        if D is not None:
            T = [(G, B, B), (B, G, B), (B, B, G)]     # (x, y, z) tables of the reference derivative r
            for r in range(3):
                for s in range(3):
                    de += _interp_t(T[r][0] * T[s][0], T[r][1] * T[s][1], T[r][2] * T[s][2], D[:, r, s])
        d = np.zeros(self.ndofs, LD)
        np.add.at(d, self.gm.ravel(), de.reshape(-1))
        return d

    def diagonal(self):
        return self._diag(self.B, self.G, self.M, self.D)

    def diagonal_bound(self):
        return self._diag(np.abs(self.B), np.abs(self.G), self.Mabs, self.Dabs)

    # ---- grid-function coefficients ------------------------------------------------------------
    def field_at_points(self, T):
        """The float64 dof values of T interpolated to the points with the longdouble B: [ne][nq]."""
        D1 = self.p + 1
        Te = np.asarray(T).astype(LD)[self.gm].reshape(self.ne, D1, D1, D1)
        return _interp(self.B, self.B, self.B, Te).reshape(self.ne, -1)


def beta_from_field(ref, T, law):
    """A coefficient that is a law of the H1 field T, at the points of `ref` (an HPRef of the same
    mesh, p and q1d), in longdouble -- law: ("gridfunc",) the field itself; ("affine", scale, slope,
    t_ref): scale (1 + slope (T - t_ref)); ("perfusion", rho_c, gdt_cb, w0, a, t0, t_stop): rho_c +
    gdt_cb w0 max(0, 1 + a (T - t0)) below t_stop, rho_c at or above it (oracle/bioheat.py)."""
    Tq = ref.field_at_points(T)
    kind, par = law[0], [LD(float(v)) for v in law[1:]]
    if kind == "gridfunc":
        return Tq
    if kind == "affine":
        scale, slope, tref = par
        return scale * (1 + slope * (Tq - tref))
    assert kind == "perfusion", kind
    rho_c, gdt_cb, w0, a, t0, t_stop = par
    r = 1 + a * (Tq - t0)
    wb = np.where((Tq < t_stop) & (r > 0), w0 * r, LD(0))
    return rho_c + gdt_cb * wb


def constant(y, y_hp, S):
    """max_i |y_i - y_hp,i| / (u S_i) over ALL dofs; where S_i = 0 (no term reaches the dof) y_i must
    be exactly 0.  Non-finite entries of y give inf."""
    y = np.asarray(y)
    assert y.shape == y_hp.shape == S.shape
    if not np.all(np.isfinite(y)):
        return float("inf")
    err = np.abs(y.astype(LD) - y_hp)
    zero = S == 0
    if np.any(zero) and np.any(y[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float((err[~zero] / (LD(U) * S[~zero])).max())


# one reference per (mesh, p, q1d, form): built once, shared by the tests, left unchanged
_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]
