"""The cases of the Chebyshev smoother's tests (a helper, not a test), shared by the CPU pin of the numpy
reference (tests/test_cheb_reference.py) and the GPU parity tests (tests/test_gpu_chebyshev.py).

Mesh: the moved-vertex lattice of bicgstab_cases.move; the boundary dofs essential unless said otherwise.
    k2        5 x 4 x 3, p 2   693 dofs (odd: the 16-byte passes' tail lane)   Diffusion(1 + z / 2) alone
    k3        4 x 3 x 3, p 3   1300 dofs (the line kernel)                     the same
    k1        5 x 4 x 3, p 1   120 dofs (fewer entries than one workgroup)     the same
    mk2       as k2            Mass(2 + sin x cos y) + 0.4359 * 0.05 Diffusion(1 + z / 2): a heat stage
    mk2_free  as mk2, no essential dofs (the essential kernels are not launched)
    sym2, sym3, sym4   the unit 4 x 4 x 4 lattice, p 2, 3, 4, DiffusionIntegrator's default coefficient: the mesh
              of the reference's own test (tests/unit/linalg/test_chebyshev.cpp)
b ~ U[0, 1) seeded; the power method's start vector ~ U(0, 1) seeded (the same one on the device).
"""
import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import bicgstab_cases as BC
import cheb_ref as CR

#        mesh, p, moved, mass, diffusion scale, essential boundary
SPECS = {
    "k2": ((5, 4, 3), 2, True, False, 1.0, True),
    "k3": ((4, 3, 3), 3, True, False, 1.0, True),
    "k1": ((5, 4, 3), 1, True, False, 1.0, True),
    "mk2": ((5, 4, 3), 2, True, True, BC.CDT, True),
    "mk2_free": ((5, 4, 3), 2, True, True, BC.CDT, False),
    "sym2": ((4, 4, 4), 2, False, False, None, True),
    "sym3": ((4, 4, 4), 3, False, False, None, True),
    "sym4": ((4, 4, 4), 4, False, False, None, True),
}
CASES = ["k2", "k3", "k1", "mk2", "mk2_free"]     # the solver's cases
SYM = ["sym2", "sym3", "sym4"]
ALL = CASES + SYM
ORDERS = CR.ORDERS_ALL
_CACHE, _REF = {}, {}


class Case:
    """The host side of one case: mesh, space, the CPU checker of the operator, Jacobi's dinv, b, v0."""

    def __init__(self, name):
        (nx, ny, nz), p, moved, mass, dscale, ess_bdr = SPECS[name]
        self.name, self.order = name, p
        m = E.Mesh.MakeCartesian3D(nx, ny, nz)
        if moved:
            m.set_vertices(BC.move(m.vertices()))
        self.mesh, self.fes = m, E.H1Space(m, p)
        fes = self.fes
        self.n = fes.ndofs
        self.P = O.quad_points(m.element_nodes(), O.default_q1d(p))
        self.alpha = BC.alpha_fn(self.P) if mass else None
        self.beta = 1.0 if dscale is None else dscale * BC.beta_fn(self.P)
        self.op = O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=self.alpha, beta=self.beta)
        self.ess = np.asarray(fes.boundary_dofs() if ess_bdr else [], dtype=np.int32)
        self.dinv = CR.jacobi_vector(self.op.diagonal(), self.ess)
        self.b = np.random.default_rng(11).uniform(0.0, 1.0, self.n)
        self.v0 = np.random.default_rng(12345).uniform(0.0, 1.0, self.n)
        self._power = {}

    def mult(self, x):
        """A x (unconstrained)."""
        return self.op.mult(x)

    def constrained(self):
        return CR.constrained(self.mult, self.ess)

    def power(self, num_steps=10, tol=1e-8, dot="matmul"):
        key = (num_steps, tol, dot)
        if key not in self._power:
            self._power[key] = CR.power_method(self.mult, self.dinv, self.ess, self.v0, num_steps, tol, dot)
        return self._power[key]

    @property
    def max_eig(self):
        """The power method's estimate with the reference's defaults (10 steps, 1e-8)."""
        return self.power().eig

    def smoother(self, order, max_eig=None):
        return CR.smoother(self.mult, self.dinv, self.ess, CR.coefficients(order, max_eig or self.max_eig))

    def solve(self, order, dot="matmul", max_eig=None, b=None, **kw):
        """Chebyshev-PCG of `order`; order 0: Jacobi-PCG."""
        prec = self.smoother(order, max_eig) if order else (lambda a: self.dinv * a)
        return CR.pcg(self.mult, self.b if b is None else b, self.ess, prec, dot=dot, **kw)

    def true_residual(self, x, b=None):
        """||b - A~ x|| / ||b|| by the CPU checker."""
        b = self.b if b is None else b
        return float(np.linalg.norm(b - self.constrained()(np.asarray(x, dtype=np.float64))) / np.linalg.norm(b))

    def dense(self):
        """The constrained operator as a dense matrix (small cases only)."""
        A = self.constrained()
        I = np.eye(self.n)
        return np.stack([A(I[:, j]) for j in range(self.n)], axis=1)

    # ---- the device form (GPU tests) ----
    def device_form(self):
        import torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        ne = self.fes.ne
        f = E.BilinearForm(self.fes)
        if self.alpha is not None:
            f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(dev(self.alpha.reshape(ne, -1)))))
        if isinstance(self.beta, float):
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(self.beta)))
        else:
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(dev(self.beta.reshape(ne, -1)))))
        f.Assemble()
        return f


def case(name):
    if name not in _CACHE:
        _CACHE[name] = Case(name)
    return _CACHE[name]


def reference(name, order, max_iter):
    """The numpy reference's solve of a case (matmul dots, rel_tol 1e-12), computed once and left unchanged."""
    key = (name, order, max_iter)
    if key not in _REF:
        _REF[key] = case(name).solve(order, rel_tol=1e-12, max_iter=max_iter)
    return _REF[key]
