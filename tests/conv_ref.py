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
det J).  dtype=np.longdouble restates the same formulas in extended precision: the float64 helper's own
error, which keeps the GPU tolerance honest (tests/test_conv_reference.py prints and pins it).

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


class ConvRef:
    def __init__(self, p, q1d, gm, ndofs, enodes, dtype=np.float64):
        self.p, self.q1d, self.ndofs, self.dtype = p, q1d, int(ndofs), dtype
        self.gm = np.asarray(gm)
        assert (self.gm >= 0).all()
        self.ne, self.nd = self.gm.shape
        B, G = O.dof_to_quad(p, q1d)
        self.B, self.G = B.astype(dtype), G.astype(dtype)                  # [Q][D]
        t, w = (a.astype(dtype) for a in O.gauss_legendre(q1d))
        Q = q1d
        self.W = (w[:, None, None] * w[None, :, None] * w[None, None, :]).reshape(-1)   # [qz][qy][qx]
        # the trilinear map at the points: corners a = ax + 2 ay + 4 az, X [ne][3][8]
        X = np.asarray(enodes).astype(dtype)
        one = dtype(1.0)
        xi = np.tile(t, Q * Q)
        et = np.tile(np.repeat(t, Q), Q)
        zt = np.repeat(t, Q * Q)
        N = np.empty((8, Q ** 3), dtype)
        dN = np.empty((8, 3, Q ** 3), dtype)
        for a in range(8):
            fx = xi if a & 1 else one - xi
            fy = et if a & 2 else one - et
            fz = zt if a & 4 else one - zt
            sx, sy, sz = (one if a & 1 else -one), (one if a & 2 else -one), (one if a & 4 else -one)
            N[a] = fx * fy * fz
            dN[a, 0], dN[a, 1], dN[a, 2] = sx * fy * fz, fx * sy * fz, fx * fy * sz
        self.P = np.einsum("eia,aq->eqi", X, N)              # [ne][nq][3]
        self.J = np.einsum("eia,ajq->eqij", X, dN)           # J[i][j] = dx_i / dxi_j

    # ---- geometry ----
    def adj(self):
        J = self.J
        A = np.empty_like(J)
        A[..., 0, 0] = J[..., 1, 1] * J[..., 2, 2] - J[..., 1, 2] * J[..., 2, 1]
        A[..., 0, 1] = J[..., 2, 1] * J[..., 0, 2] - J[..., 0, 1] * J[..., 2, 2]
        A[..., 0, 2] = J[..., 0, 1] * J[..., 1, 2] - J[..., 1, 1] * J[..., 0, 2]
        A[..., 1, 0] = J[..., 2, 0] * J[..., 1, 2] - J[..., 1, 0] * J[..., 2, 2]
        A[..., 1, 1] = J[..., 0, 0] * J[..., 2, 2] - J[..., 0, 2] * J[..., 2, 0]
        A[..., 1, 2] = J[..., 1, 0] * J[..., 0, 2] - J[..., 0, 0] * J[..., 1, 2]
        A[..., 2, 0] = J[..., 1, 0] * J[..., 2, 1] - J[..., 2, 0] * J[..., 1, 1]
        A[..., 2, 1] = J[..., 2, 0] * J[..., 0, 1] - J[..., 0, 0] * J[..., 2, 1]
        A[..., 2, 2] = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        return A

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

    def _lex(self, xe):
        D = self.p + 1
        return np.asarray(xe).astype(self.dtype).reshape(self.ne, D, D, D)      # [dz][dy][dx]

    def apply(self, pa, xe):
        B, G, Q = self.B, self.G, self.q1d
        X = self._lex(xe)
        pa = pa.reshape(self.ne, 3, Q, Q, Q)
        gx = np.einsum("xa,yb,zc,ecba->ezyx", G, B, B, X, optimize=True)
        gy = np.einsum("xa,yb,zc,ecba->ezyx", B, G, B, X, optimize=True)
        gz = np.einsum("xa,yb,zc,ecba->ezyx", B, B, G, X, optimize=True)
        u = pa[:, 0] * gx + pa[:, 1] * gy + pa[:, 2] * gz
        return np.einsum("xa,yb,zc,ezyx->ecba", B, B, B, u, optimize=True).reshape(self.ne, -1)

    def apply_t(self, pa, xe):
        B, G, Q = self.B, self.G, self.q1d
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

    def mult(self, v, x, alpha=1.0, keep=None, transpose=False, y=None):
        """y += C x (C^T x): the PA path."""
        pa = self.pa_data(v, alpha, keep)
        ye = (self.apply_t if transpose else self.apply)(pa, self.gather(x))
        return self.scatter_add(ye, y, keep)

    def fa_mult(self, v, x, alpha=1.0, keep=None, transpose=False, y=None):
        """y += C x (C^T x): the dense element matrices."""
        M = self.element_matrices(v, alpha)
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
