"""numpy restatement of the reference's boundary-face terms (a helper, not a test): the checker of
the HIP boundary MassIntegrator and BoundaryLFIntegrator.

  MassIntegrator::AssemblePABoundary   fem/integ/bilininteg_mass_pa.cpp:81-125
                                       (pa_data(q, f) = W_q c detJ_face(q, f), dim = 2)
  2D mass apply / diagonal             bilininteg_mass_pa.cpp:127-169 (B^T D B; sum_q B^2 B^2 D)
  FaceGeometricFactors DETERMINANTS    mesh/mesh.cpp:15275-15334 (|dx/dxi x dx/deta|)
  PABilinearFormExtension              fem/bilinearform_ext.cpp:625-675 (Mult's boundary block:
                                       AddMultWithMarkers per integrator, then the transposed add),
                                       :441-452 (AssembleDiagonal: one shared face vector, a marked
                                       integrator zeroes the faces it excludes after adding)
  LinearFormExtension::Assemble        fem/linearform_ext.cpp:70-111 (markers[e] = attr > 0 &&
                                       marker[attr - 1]; each integrator transposed and added)
  BLFEvalAssemble3D                    fem/integ/lininteg_boundary.cpp:74-153 (Y += B B (W c detJ))

Built from oracle.dof_to_quad, oracle.gauss_legendre and plain numpy.  Face data are [nbe][Q][Q]
([q2][q1]) and [nbe][D][D] ([i2][i1]), i.e. x fastest when flattened, in the frame of the boundary
map's rows (xi: v0 -> v1, eta: v0 -> v3).  dtype=np.longdouble restates the same formulas in extended
precision: the float64 helper's own error, which keeps the GPU tolerance honest
(tests/test_bdr_reference.py pins it).

The componentwise criterion (tests/hp_ref.py's rule): pa_bound, mult_bound, diagonal_bound and
assemble_bound are the same expressions over |B|, |x| and W |c| Dabs, Dabs = face_detj_bound (the
corners) or |detJ| (a caller's array); hp_ref.C_BDR / C_BDR_DIAG / C_BDR_QD are derived in
tests/test_bdr_reference.py.

Integrators are (c, marker) pairs: c a scalar or per-point values [nbe][Q*Q]; marker None or 0 / 1
per boundary attribute.
"""
import os

import numpy as np

import oracle as O
from helpers import GOLDEN


def face_detj(bnodes, q1d, dtype=np.float64):
    """|x_xi x x_eta| of bilinear quads at the q1d^2 Gauss-Legendre points: bnodes [nbe][3][4]
    lexicographic corners (v0, v1, v3, v2) -> [nbe][q1d^2] (q = q1 + q1d q2)."""
    t = O.gauss_legendre(q1d)[0].astype(dtype)
    X = np.asarray(bnodes).astype(dtype)
    one = dtype(1.0)
    xi = np.tile(t, q1d)[None, None, :]        # q1 fastest
    et = np.repeat(t, q1d)[None, None, :]
    x0, x1, x2, x3 = (X[:, :, a, None] for a in range(4))
    tx = (one - et) * (x1 - x0) + et * (x3 - x2)
    ty = (one - xi) * (x2 - x0) + xi * (x3 - x1)
    n = np.stack([tx[:, 1] * ty[:, 2] - tx[:, 2] * ty[:, 1], tx[:, 2] * ty[:, 0] - tx[:, 0] * ty[:, 2],
                  tx[:, 0] * ty[:, 1] - tx[:, 1] * ty[:, 0]], 1)
    return np.sqrt(np.sum(n * n, axis=1))


def face_detj_bound(bnodes, q1d, dtype=np.float64):
    """Dabs, the running magnitude of face_detj: the tangents over the |edge differences| (their convex
    combinations), every cross-product component the SUM of the magnitudes of its two products, and the
    norm of those three sums -- divided by nothing, so it is >= |x_xi x x_eta| with equality on a
    planar axis-aligned face."""
    t = O.gauss_legendre(q1d)[0].astype(dtype)
    X = np.asarray(bnodes).astype(dtype)
    one = dtype(1.0)
    xi = np.tile(t, q1d)[None, None, :]
    et = np.repeat(t, q1d)[None, None, :]
    x0, x1, x2, x3 = (X[:, :, a, None] for a in range(4))
    tx = (one - et) * np.abs(x1 - x0) + et * np.abs(x3 - x2)
    ty = (one - xi) * np.abs(x2 - x0) + xi * np.abs(x3 - x1)
    n = np.stack([tx[:, 1] * ty[:, 2] + tx[:, 2] * ty[:, 1], tx[:, 2] * ty[:, 0] + tx[:, 0] * ty[:, 2],
                  tx[:, 0] * ty[:, 1] + tx[:, 1] * ty[:, 0]], 1)
    return np.sqrt(np.sum(n * n, axis=1))


def marker_keep(attr, marker):
    """markers[e] = attr[e] > 0 && marker[attr[e] - 1] (all faces without a marker)."""
    attr = np.asarray(attr)
    if marker is None:
        return np.ones(attr.shape[0], bool)
    mk = np.asarray(marker)
    return np.array([a > 0 and mk[a - 1] != 0 for a in attr], bool)


class BdrRef:
    def __init__(self, p, q1d, bmap, battr, ndofs, bnodes=None, detj=None, dtype=np.float64):
        self.p, self.q1d, self.ndofs, self.dtype = p, q1d, int(ndofs), dtype
        self.bmap, self.attr = np.asarray(bmap), np.asarray(battr)
        self.nbe = self.bmap.shape[0]
        self.B = O.dof_to_quad(p, q1d)[0].astype(dtype)               # [Q][D]
        w = O.gauss_legendre(q1d)[1].astype(dtype)
        self.W = (w[None, :] * w[:, None]).reshape(-1)                # [q1 + Q q2]
        self.detJ = (np.asarray(detj).reshape(self.nbe, -1).astype(dtype) if detj is not None
                     else face_detj(bnodes, q1d, dtype))
        # Dabs of the componentwise bounds: |detJ| of a caller's array (an exact input), else the corners'
        self.Dabs = np.abs(self.detJ) if detj is not None else face_detj_bound(bnodes, q1d, dtype)

    # ---- AssemblePABoundary ----
    def pa_data(self, c, marker=None):
        """W c detJ, [nbe][Q*Q]; zeros on the faces the marker excludes (the marker folded in)."""
        if np.ndim(c) == 0:
            cq = np.full(self.detJ.shape, c, self.dtype)
        else:
            cq = np.asarray(c).reshape(self.nbe, -1).astype(self.dtype)
        pa = self.W[None, :] * cq * self.detJ
        return np.where(marker_keep(self.attr, marker)[:, None], pa, self.dtype(0.0))

    def _sheet(self, pa):
        return pa.reshape(self.nbe, self.q1d, self.q1d)

    # ---- the 2D kernels on face vectors ----
    def face_apply(self, pa, xf):
        B = self.B
        u = np.einsum("xa,yb,fba->fyx", B, B, xf) * self._sheet(pa)
        return np.einsum("xa,yb,fyx->fba", B, B, u)

    def face_diag(self, pa):
        B2 = self.B * self.B
        return np.einsum("xa,yb,fyx->fba", B2, B2, self._sheet(pa))

    def face_lform(self, pa):
        return np.einsum("xa,yb,fyx->fba", self.B, self.B, self._sheet(pa))

    def face_matrix(self, pa):
        """The face mass matrices assembled entry by entry: M[f][i][j] = sum_q phi_i phi_j pa."""
        D, Q = self.p + 1, self.q1d
        phi = np.einsum("xa,yb->yxba", self.B, self.B).reshape(Q * Q, D * D)   # [q][i]
        return np.einsum("qi,qj,fq->fij", phi, phi, pa)

    # ---- restriction and its transposed add ----
    def gather(self, x):
        D = self.p + 1
        return np.asarray(x).astype(self.dtype)[self.bmap].reshape(self.nbe, D, D)

    def add_transpose(self, yf, y):
        """y[d] += the face entries that map to d, in ascending face order."""
        np.add.at(y, self.bmap.ravel(), yf.reshape(-1))
        return y

    # ---- the form-level operations ----
    def mult(self, integrators, x, y=None):
        """y += H x: every integrator's AddMultPA masked by its marker, then the transposed add."""
        xf = self.gather(x)
        D = self.p + 1
        yf = np.zeros((self.nbe, D, D), self.dtype)
        for c, marker in integrators:
            yf += np.where(marker_keep(self.attr, marker)[:, None, None], self.face_apply(self.pa_data(c), xf), 0)
        y = np.zeros(self.ndofs, self.dtype) if y is None else np.array(y, self.dtype)
        return self.add_transpose(yf, y)

    def diagonal(self, integrators, d=None):
        """AssembleDiagonal's boundary block: one shared face vector; after an integrator's diagonal
        is added, its marker zeroes the excluded faces of that vector."""
        D = self.p + 1
        df = np.zeros((self.nbe, D, D), self.dtype)
        for c, marker in integrators:
            df += self.face_diag(self.pa_data(c))
            if marker is not None:
                df[~marker_keep(self.attr, marker)] = 0
        d = np.zeros(self.ndofs, self.dtype) if d is None else np.array(d, self.dtype)
        return self.add_transpose(df, d)

    def assemble(self, integrators, b=None):
        """The linear form's boundary loop: b += each integrator, in the order added."""
        b = np.zeros(self.ndofs, self.dtype) if b is None else np.array(b, self.dtype)
        for c, marker in integrators:
            self.add_transpose(self.face_lform(self.pa_data(c, marker)), b)
        return b

    # ---- the running bounds S of the componentwise criterion (tests/hp_ref.py's rule): the same
    # ---- expressions over |B|, |x| and W |c| Dabs
    def pa_bound(self, c, marker=None):
        """W |c| Dabs, [nbe][Q*Q]; zeros on the faces the marker excludes."""
        if np.ndim(c) == 0:
            cq = np.full(self.Dabs.shape, abs(c), self.dtype)
        else:
            cq = np.abs(np.asarray(c).reshape(self.nbe, -1).astype(self.dtype))
        pa = self.W[None, :] * cq * self.Dabs
        return np.where(marker_keep(self.attr, marker)[:, None], pa, self.dtype(0.0))

    def _magnitudes(self):
        """A copy of this reference over |B| (the face kernels then sum magnitudes only)."""
        m = BdrRef.__new__(BdrRef)
        m.__dict__.update(self.__dict__)
        m.B = np.abs(self.B)
        return m

    def mult_bound(self, integrators, x):
        m = self._magnitudes()
        xf = m.gather(np.abs(np.asarray(x)))
        yf = sum(m.face_apply(self.pa_bound(c, marker), xf) for c, marker in integrators)
        return self.add_transpose(yf, np.zeros(self.ndofs, self.dtype))

    def diagonal_bound(self, integrators):
        """The diagonal's shared face vector over the magnitudes, with the same marker rule."""
        D = self.p + 1
        df = np.zeros((self.nbe, D, D), self.dtype)
        for c, marker in integrators:
            df += self.face_diag(self.pa_bound(c))
            if marker is not None:
                df[~marker_keep(self.attr, marker)] = 0
        return self.add_transpose(df, np.zeros(self.ndofs, self.dtype))

    def assemble_bound(self, integrators):
        m = self._magnitudes()
        S = np.zeros(self.ndofs, self.dtype)
        for c, marker in integrators:
            self.add_transpose(m.face_lform(self.pa_bound(c, marker)), S)
        return S


def lf_default_q1d(p):
    """BoundaryLFIntegrator's default rule, order a p + b with a = b = 1: (p + 1) // 2 + 1 points."""
    return (p + 1) // 2 + 1


# ---------------------------------------------------------------------------------------
# The meshes and coefficients shared by the CPU pins and the GPU tests
# ---------------------------------------------------------------------------------------
def mesh_small(E):
    """2 x 1 x 1 Cartesian: 10 boundary faces, fewer than any workgroup."""
    return E.Mesh.MakeCartesian3D(2, 1, 1, 2.0, 1.0, 1.0)


def mesh_perturbed(E):
    """5 x 4 x 3 Cartesian, every vertex (the boundary ones too) moved by up to 0.15 h in every
    direction: 94 non-planar boundary faces -- more than one workgroup of either face kernel (64 or
    8 faces) and a multiple of neither."""
    m = E.Mesh.MakeCartesian3D(5, 4, 3, 1.0, 0.8, 0.6)
    V = m.vertices()
    V += np.random.default_rng(23).uniform(-0.15 * 0.2, 0.15 * 0.2, V.shape)
    m.set_vertices(V)
    return m


def mesh_fichera(E):
    """The reference's fichera fixture refined once: 96 boundary faces with the file's attributes."""
    m = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    m.UniformRefinement()
    return m


MESHES = {"small": mesh_small, "perturbed": mesh_perturbed, "fichera": mesh_fichera}


def face_points(bnodes, q1d):
    """Physical coordinates of the face quadrature points [nbe][q1d^2][3] (the bilinear map)."""
    t = O.gauss_legendre(q1d)[0]
    xi, et = np.tile(t, q1d), np.repeat(t, q1d)
    N = np.stack([(1 - xi) * (1 - et), xi * (1 - et), (1 - xi) * et, xi * et], 0)   # [a][q]
    return np.einsum("fca,aq->fqc", np.asarray(bnodes), N)


def h_points(P):
    """A smooth positive convection coefficient at points P [..., 3]."""
    return 25.0 * (1.0 + 0.3 * np.sin(2.0 * P[..., 0] + 0.5) * np.cos(1.5 * P[..., 1]) + 0.2 * P[..., 2])


def positive_field(X):
    """A positive L-vector (so that the boundary term does not cancel against the volume one)."""
    return 1.0 + 0.5 * np.sin(1.7 * X[:, 0] + 0.3) * np.cos(1.1 * X[:, 1]) + 0.25 * X[:, 2] ** 2
