"""The cases of the p-multigrid tests (a helper, not a test), shared by the CPU pin of the numpy reference
(tests/test_mg_reference.py) and the GPU tests (tests/test_gpu_transfer.py, tests/test_gpu_multigrid.py).

Solver cases: a p-hierarchy on one mesh, DiffusionIntegrator alone (the RF potential's operator, no mass term), the
boundary dofs essential on every level, order-2 Chebyshev smoothers with the power method's estimate (10 steps,
start vector ~ U(0, 1) seeded) on every level, b ~ U[0, 1) from seed 11.
    flat4     4 x 4 x 4 flat,   p 1 -> 2        729 dofs   coefficient 1
    moved543  5 x 4 x 3 moved,  p 1 -> 2        693 dofs (odd: the tail lane)   coefficient 1 + z / 2
    moved433  4 x 3 x 3 moved,  p 1 -> 2 -> 4   2873 dofs (three levels; the line kernel at p 4)   the same
    flat8     8 x 8 x 8 flat,   p 1 -> 2        4913 dofs   coefficient 1
The moved lattice is bicgstab_cases.move's.
"""
import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import bicgstab_cases as BC
import cheb_ref as CR
import mg_ref as MR

#          mesh, moved, orders
SPECS = {
    "flat4": ((4, 4, 4), False, (1, 2)),
    "moved543": ((5, 4, 3), True, (1, 2)),
    "moved433": ((4, 3, 3), True, (1, 2, 4)),
    "flat8": ((8, 8, 8), False, (1, 2)),
}
CASES = ["flat4", "moved543", "moved433", "flat8"]
CYCLE_CASES = CASES[:3]
EX26_COARSE = (1e-2, 200)   # examples/ex26.cpp: CGSolver rel_tol sqrt(1e-4), 200 iterations, Jacobi
SMOOTHER_ORDER = 2
# iterations to rel_tol 1e-12 the reference takes (tests/test_mg_reference.py asserts them): Jacobi, Chebyshev-2,
# V-cycle with the smoother as the coarse solve, V-cycle with ex26's coarse PCG
COUNTS = {"flat4": (27, 15, 7, 7), "moved543": (40, 24, 10, 10), "moved433": (88, 52, 11, 11), "flat8": (57, 33, 10, 8)}
_CACHE, _REF = {}, {}


def lattice(dims, moved, sfc=False):
    m = E.Mesh.MakeCartesian3D(*dims, sfc_ordering=sfc)
    if moved:
        m.set_vertices(BC.move(m.vertices()))
    return m


class LevelCase:
    def __init__(self, mesh, p, moved, eig_scale=1.0):
        self.p, self.fes = p, E.H1Space(mesh, p)
        fes = self.fes
        self.n = fes.ndofs
        self.P = O.quad_points(mesh.element_nodes(), O.default_q1d(p))
        self.beta = BC.beta_fn(self.P) if moved else 1.0
        self.op = O.OracleOperator(mesh.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=None, beta=self.beta)
        self.ess = np.asarray(fes.boundary_dofs(), dtype=np.int32)
        self.dinv = CR.jacobi_vector(self.op.diagonal(), self.ess)
        self.v0 = np.random.default_rng(12345).uniform(0.0, 1.0, self.n)
        # (eig_scale < 1: an estimate far too small, which makes the smoother -- and the cycle -- indefinite)
        self.max_eig = eig_scale * CR.power_method(self.op.mult, self.dinv, self.ess, self.v0).eig
        self.coeffs = CR.coefficients(SMOOTHER_ORDER, self.max_eig)
        self.S = CR.smoother(self.op.mult, self.dinv, self.ess, self.coeffs)

    def ref_level(self):
        return MR.Level(self.op.mult, self.ess, self.S, self.dinv)

    def device_form(self):
        import torch
        f = E.BilinearForm(self.fes)
        if isinstance(self.beta, float):
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(self.beta)))
        else:
            q = torch.as_tensor(np.ascontiguousarray(self.beta.reshape(self.fes.ne, -1))).cuda()
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(q)))
        f.Assemble()
        return f


class Case:
    def __init__(self, name, eig_scale=1.0):
        dims, moved, orders = SPECS[name]
        self.name, self.orders = name, orders
        self.mesh = lattice(dims, moved)
        self.levels = [LevelCase(self.mesh, p, moved, eig_scale) for p in orders]
        self.transfers = [MR.Transfer(a.fes.gather_map(), a.n, a.p, b.fes.gather_map(), b.n, b.p)
                          for a, b in zip(self.levels[:-1], self.levels[1:])]
        self.fine = self.levels[-1]
        self.n = self.fine.n
        self.b = np.random.default_rng(11).uniform(0.0, 1.0, self.n)

    def cycle(self, coarse_pcg=None, dot="matmul"):
        return MR.vcycle([l.ref_level() for l in self.levels], self.transfers, 1, 1, coarse_pcg, dot)

    def solve(self, kind, coarse_pcg=None, dot="matmul", b=None, **kw):
        """kind: "jacobi", "cheb" (the finest level's smoother) or "mg" (the V-cycle)."""
        f = self.fine
        prec = {"jacobi": lambda a: f.dinv * a, "cheb": f.S}.get(kind) or self.cycle(coarse_pcg, dot)
        return CR.pcg(f.op.mult, self.b if b is None else b, f.ess, prec, dot=dot, **kw)


def case(name, eig_scale=1.0):
    if (name, eig_scale) not in _CACHE:
        _CACHE[name, eig_scale] = Case(name, eig_scale)
    return _CACHE[name, eig_scale]


def reference(name, kind, coarse_pcg, max_iter):
    """The numpy reference's solve (matmul dots, rel_tol 1e-12), computed once and left unchanged."""
    key = (name, kind, coarse_pcg, max_iter)
    if key not in _REF:
        _REF[key] = case(name).solve(kind, coarse_pcg, rel_tol=1e-12, max_iter=max_iter)
    return _REF[key]
