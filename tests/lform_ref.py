"""numpy restatement of the reference's device linear form (a helper, not a test): the checker of
the HIP LinearForm.

  DLFEvalAssemble3D              fem/integ/lininteg_domain_kernels.hpp:164-300 (map_type == VALUE)
  LinearFormExtension::Assemble  fem/linearform_ext.cpp:20-68 (markers; the first R^T stores, later add)
  GridFunctionCoefficient / GradientGridFunctionCoefficient / JouleHeatingCoefficient::Eval
                                 fem/coefficient.cpp:250-253, coefficient.hpp:872, joule_solver.cpp:898

Built from the oracle's blocks (oracle.dof_to_quad, cube_weights, geom or the given J,
restriction_mult_transpose).  dtype=np.longdouble restates the same formulas in extended precision
(its own trilinear geometry and reduction): the float64 helper's own error, which keeps the GPU
tolerance honest.  tests/test_lform_reference.py pins it.

The componentwise criterion (tests/hp_ref.py's rule; float64 tables and inputs are exact): LFRef.bound is
S = R^T |B|^T |B|^T |B|^T (W F |det J|), the same expression with every factor replaced by its magnitude --
point_bound is F, geometry_bound the running magnitudes of adj J and det J over conv_ref's edge-form |J|
(|J| itself in Jacobian mode).  hp_ref.constant measures a float64 result against the np.longdouble
instance's assemble and bound; hp_ref.C_LF / C_LF_JOULE are derived in tests/test_lform_reference.py.
edge_form=True evaluates the trilinear map from its edge differences in any dtype (what the 80-bit
reference uses, and the float64 checker where the coordinates are large against the edges).

Sources are dicts: {"kind": "constant", "value"}, {"kind": "quad", "values" [ne][nq]},
{"kind": "gridfunc", "field"}, {"kind": "affine", "field", "scale", "slope", "t_ref"},
{"kind": "joule", "phi", "sigma", "slope", "t_ref", "T" (or None)}.
"""
import os

import numpy as np

import conv_ref
import helpers
import oracle as O
from helpers import GOLDEN
from hp_ref import U


def _adj(Jm):
    """adj(J) of Jm[..., i, j] (PADiffusionSetup3D's adjugate): A J = det J I."""
    A = np.empty_like(Jm)
    J = Jm
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


def _trilinear_jacobians(enodes, q1d, dtype):
    """GeometricFactors::JACOBIANS of trilinear hexes (mesh.cpp:15220-15273) in `dtype`:
    Jm[e][q][i][j] = sum_c X[e][i][c] dN_c / dxi_j at the Gauss-Legendre points (q lexicographic)."""
    t = O.gauss_legendre(q1d)[0].astype(dtype)
    X = np.asarray(enodes).astype(dtype)
    nq = q1d ** 3
    dN = np.zeros((nq, 8, 3), dtype)
    one = dtype(1.0)
    for q in range(nq):
        xi = (t[q % q1d], t[(q // q1d) % q1d], t[q // (q1d * q1d)])
        for c in range(8):
            ck = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            f = [xi[k] if ck[k] else one - xi[k] for k in range(3)]
            for j in range(3):
                v = one if ck[j] else -one
                for k in range(3):
                    if k != j:
                        v = v * f[k]
                dN[q, c, j] = v
    return np.einsum("eic,qcj->eqij", X, dN)


class LFRef:
    """The linear form's reference on one space: p, q1d, gather map, and the geometry from the
    lexicographic corners (enodes [ne][3][8]) or from MFEM-layout Jacobians J [ne][3 (j)][3 (i)][nq]."""

    def __init__(self, p, q1d, gm, ndofs, enodes=None, J=None, dtype=np.float64, edge_form=False):
        self.p, self.q1d, self.ndofs, self.dtype = p, q1d, int(ndofs), dtype
        self.enodes = None if J is not None else np.asarray(enodes)
        self.gm = np.asarray(gm)
        self.ne = self.gm.shape[0]
        B, G = O.dof_to_quad(p, q1d)                      # [Q][D]
        self.B, self.G = B.astype(dtype), G.astype(dtype)
        self.W = O.cube_weights(q1d).astype(dtype)
        if J is not None:
            self.Jm = np.transpose(np.asarray(J), (0, 3, 2, 1)).astype(dtype)   # [e][q][i][j]
            self.detJ = None
        elif edge_form:
            # the trilinear map from its edge differences (conv_ref._edge_jacobians), in `dtype`: a float64
            # evaluation that stays accurate when the coordinates are large against the edges
            self.Jm = conv_ref._edge_jacobians(self.enodes.astype(dtype), O.gauss_legendre(q1d)[0].astype(dtype))[0]
            self.detJ = None
        elif dtype == np.float64:
            _, Jo, detJ = O.geom(enodes, q1d)             # J [e][j][i][q]
            self.Jm = np.ascontiguousarray(np.transpose(Jo, (0, 3, 2, 1)))
            self.detJ = detJ
        else:
            self.Jm = _trilinear_jacobians(enodes, q1d, dtype)
            self.detJ = None
        self.A = _adj(self.Jm)
        if self.detJ is None:
            self.detJ = (self.Jm[..., 0, 0] * self.A[..., 0, 0] + self.Jm[..., 0, 1] * self.A[..., 1, 0]
                         + self.Jm[..., 0, 2] * self.A[..., 2, 0])
        if dtype == np.float64:
            self.off, self.idx = O.build_csr(self.gm, self.ndofs)

    # ---- fields at the points ----
    def _evec(self, x):
        x = np.asarray(x).astype(self.dtype)
        g = self.gm
        xe = np.where(g >= 0, x[np.where(g >= 0, g, -1 - g)], -x[np.where(g >= 0, g, -1 - g)])
        D = self.p + 1
        return xe.reshape(self.ne, D, D, D)               # [e][dz][dy][dx]

    def interp(self, x):
        """The field at the points [ne][nq] (qfunction.cpp:73-98)."""
        B = self.B
        return np.einsum("xa,yb,zc,ecba->ezyx", B, B, B, self._evec(x)).reshape(self.ne, -1)

    def ref_grad(self, x, magnitudes=False):
        """The reference gradient at the points [ne][nq][3]; magnitudes: its running bound, the same sums
        over |B|, |G| and |x|."""
        xe, B, G = self._evec(x), self.B, self.G
        if magnitudes:
            xe, B, G = np.abs(xe), np.abs(B), np.abs(G)
        return np.stack([np.einsum("xa,yb,zc,ecba->ezyx", G, B, B, xe).reshape(self.ne, -1),
                         np.einsum("xa,yb,zc,ecba->ezyx", B, G, B, xe).reshape(self.ne, -1),
                         np.einsum("xa,yb,zc,ecba->ezyx", B, B, G, xe).reshape(self.ne, -1)], -1)

    def grad(self, x):
        """The physical gradient at the points [ne][nq][3]: J^-T grad_ref = adj(J)^T grad_ref / det J."""
        return np.einsum("eqji,eqj->eqi", self.A, self.ref_grad(x)) / self.detJ[..., None]

    def point_values(self, src):
        """f at the quadrature points, [ne][nq]."""
        k = src["kind"]
        dt = self.dtype
        if k == "constant":
            return np.full((self.ne, self.q1d ** 3), src["value"], dt)
        if k == "quad":
            return np.asarray(src["values"]).reshape(self.ne, -1).astype(dt)
        if k == "gridfunc":
            return self.interp(src["field"])
        if k == "affine":
            return dt(src["scale"]) * (dt(1.0) + dt(src["slope"]) * (self.interp(src["field"]) - dt(src["t_ref"])))
        assert k == "joule", k
        gp = self.grad(src["phi"])
        sigma = dt(src["sigma"])
        if src.get("T") is not None:
            sigma = sigma * (dt(1.0) + dt(src["slope"]) * (self.interp(src["T"]) - dt(src["t_ref"])))
        return sigma * np.sum(gp * gp, axis=-1)

    # ---- DLFEvalAssemble3D ----
    def element_vectors(self, f, keep=None, B=None, detJ=None):
        """be[e][nd] = B^T B^T B^T (W f det J), lexicographic; keep (bool [ne]): markers[e] != 0.
        (B, detJ: other tables in their place, for the bound.)"""
        Q, B = self.q1d, self.B if B is None else B
        w = (self.W[None, :] * f * (self.detJ if detJ is None else detJ)).reshape(self.ne, Q, Q, Q)   # [e][qz][qy][qx]
        u = np.einsum("zc,ezyx->ecyx", B, w)
        u = np.einsum("yb,ecyx->ecbx", B, u)
        be = np.einsum("xa,ecbx->ecba", B, u).reshape(self.ne, -1)
        if keep is not None:
            be = np.where(np.asarray(keep, bool)[:, None], be, 0.0).astype(self.dtype)
        return be

    def reduce(self, be):
        """ElementRestriction::MultTranspose."""
        if self.dtype == np.float64:
            return O.restriction_mult_transpose(self.off, self.idx, np.ascontiguousarray(be))
        g = self.gm
        y = np.zeros(self.ndofs, self.dtype)
        np.add.at(y, np.where(g >= 0, g, -1 - g).ravel(), np.where(g >= 0, be, -be).ravel())
        return y

    def assemble(self, integrators):
        """LinearFormExtension::Assemble: integrators = [(src, keep or None), ...] in order."""
        b = None
        for src, keep in integrators:
            y = self.reduce(self.element_vectors(self.point_values(src), keep))
            b = y if b is None else b + y
        return b if b is not None else np.zeros(self.ndofs, self.dtype)

    # ---- the running bound S of the componentwise criterion (tests/hp_ref.py's rule) ----
    def geometry_bound(self):
        """(Aabs [ne][nq][3][3], detabs [ne][nq]): the running magnitudes of adj(J) and det J over Jabs --
        conv_ref's edge-form bound of the trilinear map (the convex combination of the |edge vectors|), or
        |J| in Jacobian mode; per cofactor the sum of the magnitudes of its two products
        (conv_ref.ConvRef._adj), and the first-row expansion of det J over them."""
        if not hasattr(self, "_gb"):
            if self.enodes is None:
                Jabs = np.abs(self.Jm)
            else:
                Jabs = conv_ref._edge_jacobians(self.enodes.astype(self.dtype),
                                                O.gauss_legendre(self.q1d)[0].astype(self.dtype))[1]
            Aabs = conv_ref.ConvRef._adj(Jabs, self.dtype(1.0))
            detabs = Jabs[..., 0, 0] * Aabs[..., 0, 0] + Jabs[..., 0, 1] * Aabs[..., 1, 0] + Jabs[..., 0, 2] * Aabs[..., 2, 0]
            self._gb = (Aabs, detabs)
        return self._gb

    def _interp_bound(self, x):
        """sum |B| |x| at the points."""
        B = np.abs(self.B)
        xe = np.abs(self._evec(x))
        return np.einsum("xa,yb,zc,ecba->ezyx", B, B, B, xe).reshape(self.ne, -1)

    def _affine_bound(self, scale, slope, t_ref, T):
        dt = self.dtype
        return abs(dt(scale)) * (dt(1.0) + abs(dt(slope)) * (self._interp_bound(T) + abs(dt(t_ref))))

    def point_bound(self, src):
        """F: the per-point running bound of f, [ne][nq] -- the same expression over the magnitudes of
        every factor.  JOULE: with g_hat = G phi the reference gradient, Sg_hat = sum |G| |phi| its bound,
        g = adj^T g_hat / det and Sg_i = sum_r Aabs_ri Sg_hat_r / |det| the bound of the mapped gradient,
        F = |sigma| sum_i (2 |g_i| Sg_i + u Sg_i^2) + Ssigma |g|^2: the first-order error of a square is
        twice the value times the error of its argument; the second-order term keeps F positive where
        the gradient vanishes."""
        k = src["kind"]
        dt = self.dtype
        if k in ("constant", "quad"):
            return np.abs(self.point_values(src))
        if k == "gridfunc":
            return self._interp_bound(src["field"])
        if k == "affine":
            return self._affine_bound(src["scale"], src["slope"], src["t_ref"], src["field"])
        assert k == "joule", k
        Aabs, _ = self.geometry_bound()
        Sgh = self.ref_grad(src["phi"], magnitudes=True)
        Sg = np.einsum("eqji,eqj->eqi", Aabs, Sgh) / np.abs(self.detJ)[..., None]
        g = np.abs(self.grad(src["phi"]))
        sigma = np.full(self.detJ.shape, abs(dt(src["sigma"])), dt)
        Ssigma = sigma
        if src.get("T") is not None:
            sigma = np.abs(dt(src["sigma"]) * (dt(1.0) + dt(src["slope"]) * (self.interp(src["T"]) - dt(src["t_ref"]))))
            Ssigma = self._affine_bound(src["sigma"], src["slope"], src["t_ref"], src["T"])
        return sigma * np.sum(2 * g * Sg + dt(U) * Sg * Sg, axis=-1) + Ssigma * np.sum(g * g, axis=-1)

    def bound(self, integrators):
        """S = R^T |B|^T |B|^T |B|^T (W F |det J|) summed over the integrators, |det J| the running
        magnitude; an excluded element contributes 0 (a dof no kept element touches has S = 0 and must
        be exactly 0)."""
        S = np.zeros(self.ndofs, self.dtype)
        _, detabs = self.geometry_bound()
        g = self.gm
        for src, keep in integrators:
            be = self.element_vectors(self.point_bound(src), keep, B=np.abs(self.B), detJ=detabs)
            np.add.at(S, np.where(g >= 0, g, -1 - g).ravel(), be.ravel())
        return S


def marker_keep(attr, marker):
    """markers[e] of linearform_ext.cpp:57-60."""
    mk = np.asarray(marker)
    return np.array([a > 0 and mk[a - 1] != 0 for a in attr])


# ---------------------------------------------------------------------------------------
# The meshes, fields and sources shared by the CPU pins and the GPU tests
# ---------------------------------------------------------------------------------------
def mesh_small(E):
    """2 x 1 x 1 Cartesian: fewer elements than one workgroup or wave."""
    return E.Mesh.MakeCartesian3D(2, 1, 1, 2.0, 1.0, 1.0)


def mesh_perturbed(E):
    """5 x 4 x 4 Cartesian, every vertex moved by up to 0.15 h (seeded): 80 non-affine elements."""
    m = E.Mesh.MakeCartesian3D(5, 4, 4, 1.0, 0.8, 0.8)
    V = m.vertices()
    V += np.random.default_rng(11).uniform(-0.15 * 0.2, 0.15 * 0.2, V.shape)
    m.set_vertices(V)
    a = np.ones(m.GetNE(), np.int32)
    a[1::3] = 2
    m.SetAttributes(a)
    return m


def mesh_fichera(E):
    """The reference's fichera fixture refined once: 56 elements, unstructured sharing."""
    m = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    m.UniformRefinement()
    return m


MESHES = {"small": mesh_small, "perturbed": mesh_perturbed, "fichera": mesh_fichera}
# (mesh, p, Q1D - p): the small mesh at p = 1; the others at p = 1..4, both rules
CASES = [("small", 1, 1), ("small", 1, 2)] + [(n, p, dq) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4)
                                              for dq in (1, 2)]


def phi_field(X):
    """A smooth potential (no symmetry: all three gradient components matter)."""
    return np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1]) + 0.7 * X[:, 2] * X[:, 0] + 0.2 * X[:, 1]


def temp_field(X):
    return helpers.temperature(X - 0.3)


SIGMA0, SIGMA_SLOPE, T_REF = 0.6, 0.015, 37.0
KINDS = ["constant", "quad", "gridfunc", "affine", "joule", "joule_T"]


def make_source(kind, X, P):
    """The source `kind` on dof coordinates X [ndofs][3] and quadrature points P [ne][nq][3]; all
    non-negative (nothing cancels in the sums)."""
    if kind == "constant":
        return {"kind": "constant", "value": 2.5}
    if kind == "quad":
        return {"kind": "quad", "values": helpers.coeff_function(P)}
    if kind == "gridfunc":
        return {"kind": "gridfunc", "field": temp_field(X)}
    if kind == "affine":
        return {"kind": "affine", "field": temp_field(X), "scale": 0.8, "slope": 0.02, "t_ref": T_REF}
    if kind == "joule":
        return {"kind": "joule", "phi": phi_field(X), "sigma": SIGMA0, "slope": 0.0, "t_ref": 0.0, "T": None}
    assert kind == "joule_T", kind
    return {"kind": "joule", "phi": phi_field(X), "sigma": SIGMA0, "slope": SIGMA_SLOPE, "t_ref": T_REF,
            "T": temp_field(X)}
