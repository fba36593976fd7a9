"""numpy restatement of the reference's ConvectionIntegrator (a helper, not a test): the checker of the
HIP convection term.

  PAConvectionSetup3D       fem/integ/bilininteg_convection_pa.cpp:100-152
                            (pa_data(q, c, e) = alpha W_q (adj J(q) v(q))_c, layout [e][3][nq])
  PAConvectionApply3D       fem/integ/bilininteg_convection_kernels.hpp:274-451 (y_e += B^T [(pa . grad_ref) x_e])
  PAConvectionApplyT3D      bilininteg_convection_kernels.hpp:897- (y_e += sum_c G_c^T [pa_c (B x_e)])
  AssembleElementMatrix     fem/bilininteg.cpp:1509- (elmat(i, j) = alpha w detJ (v . J^-T grad_ref phi_j) phi_i)
  AddMultWithMarkers        fem/bilinearform_ext.cpp:753-774 (an excluded element's E-vector rows are zero)

Two paths that share only the basis tables (oracle.dof_to_quad / gauss_legendre) and the Jacobians of the
trilinear map: PA (sum-factorised, adj J) and FA (dense element matrices in physical space, J^-1 v and
det J).

dtype=np.longdouble is the extended-precision reference of the componentwise criterion (tests/hp_ref.py's
conventions: float64 inputs are exact, everything else is 80-bit; the tables are hp_ref.tables, the Lagrange
product form).  Beside each quantity it evaluates the running bound over the magnitudes of every factor:
Jabs (the edge form's convex combination of |edge vectors|, or |J| in Jacobian mode), adj_bound (per
cofactor the sum of the magnitudes of its two products), pa_bound = Pabs = |alpha| W sum_d Aabs_cd |v_d|
for the qdata and bound = S, the apply over |B|, |G|, Pabs, |x|, for C x and C^T x.  hp_ref.constant
measures a float64 result against them; tests/test_conv_reference.py pins the float64 instance that way
(c_ref) and derives the device bounds hp_ref.C_CONV / C_CONV_QD from it.

Geometry: from the corners (the trilinear map in edge form, which keeps entries that vanish on an
axis-aligned mesh exactly zero) or from given Jacobians (ConvRef.from_jacobians, MFEM's layout).

E-vectors are [ne][nd], lexicographic (dx fastest); qdata [ne][3][nq], q = qx + Q (qy + Q qz).
"""
import numpy as np

import oracle as O


def reference_velocity(P):
    """The reference test's velocity (tests/unit/fem/test_pa_kernels.cpp:498-578, 3D): (y, -x, x)."""
    return np.stack([P[..., 1], -P[..., 0], P[..., 0]], -1)


def marker_keep(attr, marker):
    """markers[e] = attr[e] > 0 && marker[attr[e] - 1] (all elements without a marker)."""
    attr = np.asarray(attr)
    if marker is None:
        return np.ones(attr.shape[0], bool)
    mk = np.asarray(marker)
    return np.array([a > 0 and mk[a - 1] != 0 for a in attr], bool)


def _tables(p, q1d, dtype):
    """B, G [Q][D], the 1D points and the point weights W [nq]: the oracle's float64 tables, or for
    np.longdouble hp_ref.tables (the Lagrange product form on the float64 nodes and points, taken as
    exact) -- not the float64 dof_to_quad cast up, whose own rounding the reference must not inherit."""
    if dtype is np.longdouble:
        import hp_ref
        B, G = hp_ref.tables(p, q1d)
    else:
        B, G = (a.astype(dtype) for a in O.dof_to_quad(p, q1d))
    t, w = (a.astype(dtype) for a in O.gauss_legendre(q1d))
    W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(-1)   # [qz][qy][qx]
    return B, G, t, W


def _edge_jacobians(X, t):
    """J and its magnitude bound of the trilinear map, edge form: column j at a point is the convex
    combination of the four edge vectors along reference direction j, weights >= 0 the products of xi
    or 1 - xi in the other two directions; Jabs the same combination of the edges' |.|.  An entry all
    four of whose edge differences vanish (an axis-aligned mesh) is exactly 0, with bound 0.
    X [ne][3][8] (corner a = ax + 2 ay + 4 az), t [Q] -> [ne][nq][i][j] twice."""
    ne, Q = X.shape[0], t.shape[0]
    Xc = X.reshape(ne, 3, 2, 2, 2)                                  # [e][i][az][ay][ax]
    N1 = np.stack([1 - t, t], 1)                                    # [Q][2]
    d = [Xc[:, :, :, :, 1] - Xc[:, :, :, :, 0],                     # [e][i][az][ay]
         Xc[:, :, :, 1, :] - Xc[:, :, :, 0, :],                     # [e][i][az][ax]
         Xc[:, :, 1, :, :] - Xc[:, :, 0, :, :]]                     # [e][i][ay][ax]
    out = []
    for f in (lambda a: a, np.abs):
        c0 = np.einsum("zc,yb,eicb->eizy", N1, N1, f(d[0]))[:, :, :, :, None]
        c1 = np.einsum("zc,xa,eica->eizx", N1, N1, f(d[1]))[:, :, :, None, :]
        c2 = np.einsum("yb,xa,eiba->eiyx", N1, N1, f(d[2]))[:, :, None, :, :]
        J = np.stack([np.broadcast_to(c, (ne, 3, Q, Q, Q)) for c in (c0, c1, c2)], 2)   # [e][i][j][z][y][x]
        out.append(np.ascontiguousarray(J.reshape(ne, 3, 3, Q ** 3).transpose(0, 3, 1, 2)))
    return out


class ConvRef:
    def __init__(self, p, q1d, gm, ndofs, enodes, dtype=np.float64):
        self._common(p, q1d, gm, ndofs, dtype)
        t, Q = self.t, q1d
        # the trilinear map at the points: corners a = ax + 2 ay + 4 az, X [ne][3][8]
        X = np.asarray(enodes).astype(dtype)
        one = dtype(1.0)
        xi = np.tile(t, Q * Q)
        et = np.tile(np.repeat(t, Q), Q)
        zt = np.repeat(t, Q * Q)
        N = np.empty((8, Q ** 3), dtype)
        for a in range(8):
            fx = xi if a & 1 else one - xi
            fy = et if a & 2 else one - et
            fz = zt if a & 4 else one - zt
            N[a] = fx * fy * fz
        self.P = np.einsum("eia,aq->eqi", X, N)              # [ne][nq][3]
        self.J, self.Jabs = _edge_jacobians(X, t)            # J[i][j] = dx_i / dxi_j, [ne][nq][3][3]

    def _common(self, p, q1d, gm, ndofs, dtype):
        self.p, self.q1d, self.ndofs, self.dtype = p, q1d, int(ndofs), dtype
        self.gm = np.asarray(gm)
        assert (self.gm >= 0).all()
        self.ne, self.nd = self.gm.shape
        self.B, self.G, self.t, self.W = _tables(p, q1d, dtype)                # B, G [Q][D]

    @classmethod
    def from_jacobians(cls, J, p, q1d, gm, ndofs, dtype=np.float64):
        """The same term on a mesh given by its Jacobians at the points, J [ne][3 (j)][3 (i)][nq]:
        GeometricFactors::JACOBIANS' memory order, what Mesh.jacobians and helpers.curved_fichera
        return.  J is an exact input (its magnitude bound is |J|); there are no point coordinates."""
        self = cls.__new__(cls)
        self._common(p, q1d, gm, ndofs, dtype)
        J = np.asarray(J)
        assert J.shape == (self.ne, 3, 3, q1d ** 3), J.shape
        self.J = np.ascontiguousarray(J.astype(dtype).transpose(0, 3, 2, 1))   # [ne][nq][i][j]
        self.Jabs = np.abs(self.J)
        self.P = None
        return self

    # ---- geometry ----
    @staticmethod
    def _adj(J, s):
        """Cofactor (c, d) = first product + s * second product: s = -1 adj(J), s = +1 on |J| its bound."""
        A = np.empty_like(J)
        A[..., 0, 0] = J[..., 1, 1] * J[..., 2, 2] + s * (J[..., 1, 2] * J[..., 2, 1])
        A[..., 0, 1] = J[..., 2, 1] * J[..., 0, 2] + s * (J[..., 0, 1] * J[..., 2, 2])
        A[..., 0, 2] = J[..., 0, 1] * J[..., 1, 2] + s * (J[..., 1, 1] * J[..., 0, 2])
        A[..., 1, 0] = J[..., 2, 0] * J[..., 1, 2] + s * (J[..., 1, 0] * J[..., 2, 2])
        A[..., 1, 1] = J[..., 0, 0] * J[..., 2, 2] + s * (J[..., 0, 2] * J[..., 2, 0])
        A[..., 1, 2] = J[..., 1, 0] * J[..., 0, 2] + s * (J[..., 0, 0] * J[..., 1, 2])
        A[..., 2, 0] = J[..., 1, 0] * J[..., 2, 1] + s * (J[..., 2, 0] * J[..., 1, 1])
        A[..., 2, 1] = J[..., 2, 0] * J[..., 0, 1] + s * (J[..., 0, 0] * J[..., 2, 1])
        A[..., 2, 2] = J[..., 0, 0] * J[..., 1, 1] + s * (J[..., 0, 1] * J[..., 1, 0])
        return A

    def adj(self):
        return self._adj(self.J, self.dtype(-1.0))

    def adj_bound(self):
        """Aabs: per cofactor the sum of the magnitudes of its two products of Jabs entries."""
        return self._adj(self.Jabs, self.dtype(1.0))

    def det(self):
        J = self.J
        return (J[..., 0, 0] * (J[..., 1, 1] * J[..., 2, 2] - J[..., 2, 1] * J[..., 1, 2])
                - J[..., 1, 0] * (J[..., 0, 1] * J[..., 2, 2] - J[..., 2, 1] * J[..., 0, 2])
                + J[..., 2, 0] * (J[..., 0, 1] * J[..., 1, 2] - J[..., 1, 1] * J[..., 0, 2]))

    def velocity(self, v):
        """A constant 3-vector or per-point values [ne][nq][3] -> [ne][nq][3]."""
        v = np.asarray(v)
        if v.ndim == 1:
            return np.broadcast_to(v.astype(self.dtype), (self.ne, self.q1d ** 3, 3))
        return v.reshape(self.ne, -1, 3).astype(self.dtype)

    # ---- PA path ----
    def pa_data(self, v, alpha=1.0, keep=None):
        """alpha W (adj J v), [ne][3][nq]; zeros on the elements `keep` (bool [ne]) excludes."""
        pa = self.dtype(alpha) * self.W[None, None, :] * np.einsum("eqcd,eqd->ecq", self.adj(), self.velocity(v))
        if keep is not None:
            pa = np.where(np.asarray(keep)[:, None, None], pa, self.dtype(0.0))
        return pa

    def pa_bound(self, v, alpha=1.0, keep=None):
        """Pabs [ne][3][nq] = |alpha| W sum_d Aabs_cd |v_d|: the running bound of pa_data, zero on the
        elements `keep` excludes."""
        pa = abs(self.dtype(alpha)) * self.W[None, None, :] * np.einsum("eqcd,eqd->ecq", self.adj_bound(),
                                                                         np.abs(self.velocity(v)))
        if keep is not None:
            pa = np.where(np.asarray(keep)[:, None, None], pa, self.dtype(0.0))
        return pa

    def _lex(self, xe):
        D = self.p + 1
        return np.asarray(xe).astype(self.dtype).reshape(self.ne, D, D, D)      # [dz][dy][dx]

    def apply(self, pa, xe, tables=None):
        (B, G), Q = tables or (self.B, self.G), self.q1d
        X = self._lex(xe)
        pa = pa.reshape(self.ne, 3, Q, Q, Q)
        gx = np.einsum("xa,yb,zc,ecba->ezyx", G, B, B, X, optimize=True)
        gy = np.einsum("xa,yb,zc,ecba->ezyx", B, G, B, X, optimize=True)
        gz = np.einsum("xa,yb,zc,ecba->ezyx", B, B, G, X, optimize=True)
        u = pa[:, 0] * gx + pa[:, 1] * gy + pa[:, 2] * gz
        return np.einsum("xa,yb,zc,ezyx->ecba", B, B, B, u, optimize=True).reshape(self.ne, -1)

    def apply_t(self, pa, xe, tables=None):
        (B, G), Q = tables or (self.B, self.G), self.q1d
        pa = pa.reshape(self.ne, 3, Q, Q, Q)
        u = np.einsum("xa,yb,zc,ecba->ezyx", B, B, B, self._lex(xe), optimize=True)
        y = np.einsum("xa,yb,zc,ezyx->ecba", G, B, B, pa[:, 0] * u, optimize=True)
        y = y + np.einsum("xa,yb,zc,ezyx->ecba", B, G, B, pa[:, 1] * u, optimize=True)
        y = y + np.einsum("xa,yb,zc,ezyx->ecba", B, B, G, pa[:, 2] * u, optimize=True)
        return y.reshape(self.ne, -1)

    # ---- FA path ----
    def element_matrices(self, v, alpha=1.0):
        """Dense elmat [ne][i][j] = sum_q alpha W detJ (v . J^-T grad_ref phi_j) phi_i, in physical space."""
        B, G, Q, D = self.B, self.G, self.q1d, self.p + 1
        nq, nd = Q ** 3, D ** 3
        phi = np.einsum("xa,yb,zc->zyxcba", B, B, B).reshape(nq, nd)
        dphi = np.stack([np.einsum("xa,yb,zc->zyxcba", G, B, B).reshape(nq, nd),
                         np.einsum("xa,yb,zc->zyxcba", B, G, B).reshape(nq, nd),
                         np.einsum("xa,yb,zc->zyxcba", B, B, G).reshape(nq, nd)], 0)   # [c][q][j]
        det = self.det()
        Jinv = self.adj() / det[..., None, None]
        vr = np.einsum("eqcd,eqd->eqc", Jinv, self.velocity(v))       # J^-1 v: the velocity in reference space
        vg = np.einsum("eqc,cqj->eqj", vr, dphi)                       # v . grad phi_j at the points
        wq = self.dtype(alpha) * self.W[None, :] * det
        return np.matmul(phi.T[None], wq[:, :, None] * vg)             # [e][i][j]

    # ---- restriction and the form-level operations ----
    def gather(self, x):
        return np.asarray(x).astype(self.dtype)[self.gm]

    def scatter_add(self, ye, y=None, keep=None):
        y = np.zeros(self.ndofs, self.dtype) if y is None else np.array(y, self.dtype)
        k = np.ones(self.ne, bool) if keep is None else np.asarray(keep)
        np.add.at(y, self.gm[k].ravel(), ye[k].ravel())
        return y

    def mult(self, v, x, alpha=1.0, keep=None, transpose=False, y=None, pa=None):
        """y += C x (C^T x): the PA path (pa: pa_data(v, alpha, keep), computed before)."""
        pa = self.pa_data(v, alpha, keep) if pa is None else pa
        ye = (self.apply_t if transpose else self.apply)(pa, self.gather(x))
        return self.scatter_add(ye, y, keep)

    def bound(self, v, x, alpha=1.0, keep=None, transpose=False, pabs=None):
        """S: the forward (transposed) apply over the magnitudes of every factor -- |B|, |G|, Pabs, |x| --
        scattered as mult does: the running bound of the sum-factorised evaluation (hp_ref.HPRef.bound's
        construction).  pabs: pa_bound(v, alpha, keep), computed before."""
        tables = (np.abs(self.B), np.abs(self.G))
        pabs = self.pa_bound(v, alpha, keep) if pabs is None else pabs
        ye = (self.apply_t if transpose else self.apply)(pabs, np.abs(self.gather(x)), tables)
        return self.scatter_add(ye, None, keep)

    def fa_mult(self, v, x, alpha=1.0, keep=None, transpose=False, y=None, M=None):
        """y += C x (C^T x): the dense element matrices (M: those of (v, alpha), computed before)."""
        M = self.element_matrices(v, alpha) if M is None else M
        if transpose:
            M = M.transpose(0, 2, 1)
        ye = np.einsum("eij,ej->ei", M, self.gather(x))
        return self.scatter_add(ye, y, keep)

    def unit_load(self):
        """M_1 1: sum_q W detJ phi_i assembled (the linear form of the constant 1)."""
        B, Q = self.B, self.q1d
        w = (self.W[None, :] * self.det()).reshape(self.ne, Q, Q, Q)
        be = np.einsum("xa,yb,zc,ezyx->ecba", B, B, B, w, optimize=True).reshape(self.ne, -1)
        return self.scatter_add(be)
