"""The cases of the h-multigrid tests (a helper, not a test), shared by the CPU pin of the numpy reference
(tests/test_hmg_reference.py), the host replay (tests/test_htransfer_host.py) and the GPU tests
(tests/test_gpu_htransfer.py, tests/test_gpu_hmultigrid.py).

Transfer cases, a coarse mesh and its uniform refinement at one order:
    moved322   moved 3 x 2 x 2 -> 6 x 4 x 4, p 1..4   12 parents: no multiple of any workgroup's parent count
    moved543   moved 5 x 4 x 3 -> 10 x 8 x 6, p 1, 2   more than one workgroup, an odd dof count
    fichera    fichera.mesh -> refined once, p 1, 2    shared faces with differing local orientations
    fichera1   refined once -> refined twice, p 1, 2
    sfc4       an SFC-ordered 4 x 4 x 4, p 1, 2
    struct433  4 x 3 x 3 with the coarse space in the structured numbering, p 1, 2
Hierarchy cases (h0 1, h1 1, h1 2), set up as mg_cases' (DiffusionIntegrator alone, the boundary essential on every
level, order-2 Chebyshev smoothers, b ~ U[0, 1) from seed 11): hmoved433 (moved 4 x 3 x 3 -> 8 x 6 x 6) and hflat4
(flat 4^3 -> 8^3).
"""
import os

import numpy as np

import helpers  # noqa: F401
import ecm2_amd as E
import cheb_ref as CR
import hmg_ref as HR
import mg_cases as MC
import mg_ref as MR
from helpers import GOLDEN, temperature

TRANSFER_CASES = [("moved322", p) for p in (1, 2, 3, 4)] + [(n, p) for n in ("moved543", "fichera", "fichera1", "sfc4",
                                                                              "struct433") for p in (1, 2)]
# iterations to rel_tol 1e-12 the reference takes (tests/test_hmg_reference.py asserts them): Jacobi on the finest
# level, the p-only cycle (h1 1, h1 2), the three-level cycle (h0 1, h1 1, h1 2)
COUNTS = {"hmoved433": (66, 12, 9), "hflat4": (57, 10, 8)}
H_SPECS = {"hmoved433": ((4, 3, 3), True), "hflat4": ((4, 4, 4), False)}
H_CASES = ["hmoved433", "hflat4"]
_PAIRS, _CASES, _REF = {}, {}, {}


def refined(mesh):
    fine = mesh.Copy()
    fine.UniformRefinement()
    return fine


def coarse_mesh(name):
    if name == "moved322":
        return MC.lattice((3, 2, 2), True)
    if name == "moved543":
        return MC.lattice((5, 4, 3), True)
    if name == "fichera":
        return E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    if name == "fichera1":
        return refined(E.Mesh(os.path.join(GOLDEN, "fichera.mesh")))
    if name == "sfc4":
        return MC.lattice((4, 4, 4), True, sfc=True)
    assert name == "struct433", name
    return MC.lattice((4, 3, 3), True)


class Pair:
    """A coarse space, the space of the same order on the refined mesh, and the embedding."""

    def __init__(self, name, p):
        self.name, self.p = name, p
        self.coarse = coarse_mesh(name)
        self.fine = refined(self.coarse)
        numbering = E.NUMBERING_STRUCTURED if name == "struct433" else E.NUMBERING_ENTITY
        self.lf, self.hf = E.H1Space(self.coarse, p, numbering), E.H1Space(self.fine, p)
        self.parent, self.octant = self.coarse.refinement_embedding()
        rng = np.random.default_rng(9)
        # (x_c, x_f) of both kinds of input
        self.inputs = {"temperature": (temperature(self.lf.dof_coords()), temperature(self.hf.dof_coords())),
                       "random": (rng.uniform(-1, 1, self.lf.ndofs), rng.uniform(-1, 1, self.hf.ndofs))}
        self._ref = {}

    def ref(self, dtype=np.float64, gf=None, parent=None, octant=None):
        key = (dtype is HR.LD, gf is None)
        if gf is not None:
            return HR.HTransfer(self.lf.gather_map(), self.lf.ndofs, gf, self.hf.ndofs, self.p, parent, octant, dtype)
        if key not in self._ref:
            self._ref[key] = HR.HTransfer(self.lf.gather_map(), self.lf.ndofs, self.hf.gather_map(), self.hf.ndofs, self.p,
                                          self.parent, self.octant, dtype)
        return self._ref[key]


def pair(name, p):
    """Built once, shared by the tests, left unchanged."""
    if (name, p) not in _PAIRS:
        _PAIRS[name, p] = Pair(name, p)
    return _PAIRS[name, p]


class HCase:
    """(h0, 1) -> (h1, 1) -> (h1, 2) with mg_cases' level setup; p_only: the two levels on h1 alone."""

    def __init__(self, name):
        dims, moved = H_SPECS[name]
        self.name = name
        self.coarse = MC.lattice(dims, moved)
        self.finemesh = refined(self.coarse)
        self.levels = [MC.LevelCase(self.coarse, 1, moved), MC.LevelCase(self.finemesh, 1, moved),
                       MC.LevelCase(self.finemesh, 2, moved)]
        l0, l1, l2 = self.levels
        self.parent, self.octant = self.coarse.refinement_embedding()
        self.transfers = [HR.HTransfer(l0.fes.gather_map(), l0.n, l1.fes.gather_map(), l1.n, 1, self.parent, self.octant),
                          MR.Transfer(l1.fes.gather_map(), l1.n, 1, l2.fes.gather_map(), l2.n, 2)]
        self.fine = l2
        self.n = l2.n
        self.b = np.random.default_rng(11).uniform(0.0, 1.0, self.n)

    def cycle(self, p_only=False, coarse_pcg=None, dot="matmul"):
        lv = [l.ref_level() for l in self.levels]
        if p_only:
            return MR.vcycle(lv[1:], self.transfers[1:], 1, 1, coarse_pcg, dot)
        return MR.vcycle(lv, self.transfers, 1, 1, coarse_pcg, dot)

    def solve(self, kind, p_only=False, coarse_pcg=None, dot="matmul", **kw):
        f = self.fine
        prec = (lambda a: f.dinv * a) if kind == "jacobi" else self.cycle(p_only, coarse_pcg, dot)
        return CR.pcg(f.op.mult, self.b, f.ess, prec, dot=dot, **kw)


def hcase(name):
    if name not in _CASES:
        _CASES[name] = HCase(name)
    return _CASES[name]


def reference(name, max_iter):
    """The numpy reference's solve with the three-level cycle (matmul dots, rel_tol 1e-12), computed once."""
    if (name, max_iter) not in _REF:
        _REF[name, max_iter] = hcase(name).solve("mg", rel_tol=1e-12, max_iter=max_iter)
    return _REF[name, max_iter]
