"""The advection-diffusion cases of the BiCGSTAB tests (a helper, not a test), shared by the CPU pin of the
numpy reference (tests/test_bicgstab_reference.py) and the GPU parity tests (tests/test_gpu_bicgstab.py).

Mesh: a Cartesian lattice with the vertices moved by (x + 0.05 sin(3y) z, y + 0.04 cos(2x), z + 0.03 x y);
"p2": 5 x 4 x 3 elements, p = 2 (693 dofs, odd: the 16-byte passes' tail lane; the thread-per-element
convection kernel); "p3": 4 x 3 x 3, p = 3 (the sheet kernel).
Operator: T = Mass(2 + sin x cos y) + c dt [Diffusion(1 + z / 2) + Convection((y, -x, x), 20)], c dt =
0.4359 * 0.05; the boundary dofs essential; Jacobi from the symmetric part M + c dt K; b ~ U[0, 1) seeded.
Marked: the convection on the attributes [0, 1, 1] of 1 + e mod 3.
"""
import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import conv_ref as CR
import bicgstab_ref as BR

CDT = 0.4359 * 0.05
CONV_SCALE = 20.0
MARKER = [0, 1, 1]
MESHES = {"p2": (5, 4, 3, 2), "p3": (4, 3, 3, 3)}
CASES = [("p2", False), ("p2", True), ("p3", False), ("p3", True)]
_CACHE = {}


def move(V):
    V = np.array(V, dtype=np.float64, copy=True)
    x, y, z = V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()
    V[:, 0] = x + 0.05 * np.sin(3.0 * y) * z
    V[:, 1] = y + 0.04 * np.cos(2.0 * x)
    V[:, 2] = z + 0.03 * x * y
    return V


def alpha_fn(P):
    return 2.0 + np.sin(P[..., 0]) * np.cos(P[..., 1])


def beta_fn(P):
    return 1.0 + 0.5 * P[..., 2]


class Case:
    """The host side of one case: mesh, space, the CPU checkers of T and of its symmetric part."""

    def __init__(self, name, marked, conv_scale=CONV_SCALE):
        nx, ny, nz, p = MESHES[name]
        self.name, self.marked, self.order, self.conv_scale = name, marked, p, conv_scale
        m = E.Mesh.MakeCartesian3D(nx, ny, nz)
        m.set_vertices(move(m.vertices()))
        m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32))
        self.mesh, self.fes = m, E.H1Space(m, p)
        fes = self.fes
        self.n = fes.ndofs
        q1d = O.default_q1d(p)
        self.P = O.quad_points(m.element_nodes(), q1d)
        self.sym = O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=alpha_fn(self.P),
                                    beta=CDT * beta_fn(self.P))
        self.conv = CR.ConvRef(p, q1d, fes.gather_map(), fes.ndofs, m.element_nodes())
        self.v = CR.reference_velocity(self.conv.P)
        self.keep = CR.marker_keep(m.GetAttributes(), MARKER) if marked else None
        self.pa = self.conv.pa_data(self.v, CDT * conv_scale, self.keep)
        self.ess = np.asarray(fes.boundary_dofs(), dtype=np.int32)
        self.dinv = BR.jacobi_vector(self.sym.diagonal(), self.ess)
        self.b = np.random.default_rng(11).uniform(0.0, 1.0, self.n)

    def conv_mult(self, x):
        return self.conv.mult(self.v, x, CDT * self.conv_scale, self.keep, pa=self.pa)

    def mult(self, x):
        """T x (unconstrained)."""
        return self.sym.mult(x) + self.conv_mult(x)

    def solve(self, dot="matmul", jacobi=True, **kw):
        return BR.bicgstab(self.mult, self.b, self.ess, self.dinv if jacobi else None, dot=dot, **kw)

    def true_residual(self, x):
        """||b - A x|| / ||b|| of the constrained system, by the CPU checkers."""
        A = BR.constrained(self.mult, self.ess)
        return float(np.linalg.norm(self.b - A(np.asarray(x, dtype=np.float64))) / np.linalg.norm(self.b))

    def convective_share(self, x):
        return float(np.abs(self.conv_mult(x)).max() / np.abs(self.sym.mult(x)).max())

    # ---- the device forms (GPU tests) ----
    def device_forms(self):
        """(T, its symmetric part) as assembled BilinearForms."""
        import torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        ne = self.fes.ne
        forms = []
        for with_conv in (True, False):
            f = E.BilinearForm(self.fes)
            f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(dev(alpha_fn(self.P).reshape(ne, -1)))))
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(dev(CDT * beta_fn(self.P).reshape(ne, -1)))))
            if with_conv:
                ci = E.ConvectionIntegrator(E.VectorCoefficient(dev(self.v)), CDT * self.conv_scale)
                if self.marked:
                    f.AddDomainIntegrator(ci, MARKER)
                else:
                    f.AddDomainIntegrator(ci)
            f.Assemble()
            forms.append(f)
        return forms


def case(name, marked):
    key = (name, marked)
    if key not in _CACHE:
        _CACHE[key] = Case(name, marked)
    return _CACHE[key]


_REF = {}


def reference(name, marked, max_iter):
    """The numpy reference's solve of a case (matmul dots, rel_tol 1e-12), computed once and left unchanged."""
    key = (name, marked, max_iter)
    if key not in _REF:
        _REF[key] = case(name, marked).solve(rel_tol=1e-12, max_iter=max_iter)
    return _REF[key]
