"""The case matrix of the convection term's componentwise criterion (tests/conv_ref.py with the bound of
tests/hp_ref.py), shared by the CPU pins of the float64 checker (test_conv_reference.py: c_ref) and the
device tests (test_gpu_convection_componentwise.py).

Meshes, those of test_gpu_convection.py, the smallest at which each kernel can go wrong: `perturbed`
(5 x 4 x 3, every vertex moved: 60 non-affine elements, one partial wave and a partial sheet group for
Q = 4, 6), `fichera` refined once (56 elements, unstructured valence, partial for Q = 5) and `cube8`
(8 x 8 x 8 axis-aligned, 1 x 0.7 x 1.3, whose ragged marker keeps 347 elements: several workgroups, a
multiple of none of 64 / 16 / 10 / 7, and Jacobian entries that are exactly zero).  In Jacobian mode:
`perturbed` through Mesh.jacobians and the reference's curved fichera-q2 / fichera-q3 meshes.

A *geometry* is (mesh, p, q1d): on it live the four states of cw_cases (from the dof coordinates), the
float64 checker `lo`, its extended-precision instance `hi`, and per (velocity, marked, transpose) the
reference products y_hp and bounds S of every state -- computed once, cached, left unchanged."""
import tempfile

import numpy as np

import ecm2_amd as E
import oracle as O
import bdr_ref as BR
import conv_ref as R
import hp_ref as HP
import helpers
from cw_cases import STATES
from helpers import temperature

LD = np.longdouble
CALPHA = 1.7                    # ConvectionIntegrator's alpha
VCONST = np.array([0.8, -0.3, 0.5])
MARKER = (0, 1, 1)              # on attributes 1 + e mod 3 (cube8: the 320 + 27 elements)
NUMBERING = {"cube8": E.NUMBERING_STRUCTURED}


def cube8_attributes():
    """8 x 8 x 8, lexicographic elements: attribute 2 on the z layers 1, 2, 3, 5, 6 (320 elements), 3 on
    the first 27 elements of layer 7, 1 elsewhere."""
    e = np.arange(512)
    iz, r = e // 64, e % 64
    attr = np.ones(512, np.int32)
    attr[np.isin(iz, [1, 2, 3, 5, 6])] = 2
    attr[(iz == 7) & (r < 27)] = 3
    return attr


def _mesh(name):
    if name == "cube8":
        m = E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3)
        m.SetAttributes(cube8_attributes())
    else:
        m = BR.MESHES[name](E)
        m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32))
    return m


def states(X, p):
    """The four states exactly as cw_cases.Space builds them, from the dof coordinates."""
    T = temperature(X)
    return {"random": np.random.default_rng(1000 + p).uniform(-1, 1, X.shape[0]),
            "celsius": T,
            "kelvin": T + 273.15,
            "linear": 310.15 + X @ np.array([0.3, -1.1, 0.7])}


# ---- the cases: (geometry kind, mesh, p, q1d) -----------------------------------------------------
CORNER_CASES = ([("corners", n, p, p + dq) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4) for dq in (1, 2)]
                + [("corners", "cube8", 2, 4), ("corners", "cube8", 4, 6)])
# (every curved case lies within has_conv_apply: p + 1 or p + 2 points, orders >= the map's)
JACOBIAN_CASES = ([("jacobians", "perturbed", p, p + dq) for p in (2, 4) for dq in (1, 2)]
                  + [("jacobians", "fichera-q2", 2, 4), ("jacobians", "fichera-q2", 3, 5),
                     ("jacobians", "fichera-q3", 3, 5), ("jacobians", "fichera-q3", 4, 6)])
CASES = CORNER_CASES + JACOBIAN_CASES
CURVED = ("fichera-q2", "fichera-q3")


def case_id(c):
    return "%s-%s-p%d-q%d" % c


class Geometry:
    """One (kind, mesh, p, q1d): the space, the states, both checkers and the cached references."""

    def __init__(self, kind, name, p, q1d):
        self.kind, self.name, self.p, self.q1d = kind, name, p, q1d
        self.J = None
        if name in CURVED:
            assert kind == "jacobians"
            with tempfile.TemporaryDirectory() as tmp:
                self.mesh, self.fes, self.J, self.X = helpers.curved_fichera(tmp, p, q1d, name + ".mesh")
            self.mesh.SetAttributes(1 + (np.arange(self.mesh.GetNE()) % 3).astype(np.int32))
        else:
            self.mesh = HP.cached(("conv-mesh", name), lambda: _mesh(name))
            self.fes = HP.cached(("conv-fes", name, p),
                                 lambda: E.H1Space(self.mesh, p, NUMBERING.get(name, E.NUMBERING_ENTITY)))
            self.X = self.fes.dof_coords()
            if kind == "jacobians":
                self.J = self.mesh.jacobians(q1d, device="cpu").numpy()
        self.en, self.gm, self.ndofs = self.mesh.element_nodes(), self.fes.gather_map(), self.fes.ndofs
        self.ne = self.gm.shape[0]
        self.attr = self.mesh.GetAttributes()
        self.keep = R.marker_keep(self.attr, MARKER)
        assert 0 < self.keep.sum() < self.ne
        self.x = states(self.X, p)
        if kind == "corners":
            self.lo = R.ConvRef(p, q1d, self.gm, self.ndofs, self.en)
            self.hi = R.ConvRef(p, q1d, self.gm, self.ndofs, self.en, dtype=LD)
        else:
            self.lo = R.ConvRef.from_jacobians(self.J, p, q1d, self.gm, self.ndofs)
            self.hi = R.ConvRef.from_jacobians(self.J, p, q1d, self.gm, self.ndofs, dtype=LD)
        # the per-point velocity (y, -x, x) at the trilinear map's points: float64 values every side takes
        # as exact (on a curved mesh the corner map's points: any smooth per-point values)
        self.vpts = R.reference_velocity(O.quad_points(self.en, q1d))
        self._refs = {}

    def velocity(self, vname):
        return VCONST if vname == "const" else self.vpts

    def keep_of(self, marked):
        return self.keep if marked else None

    def n_active(self, marked):
        return int(self.keep.sum()) if marked else self.ne

    def mult_ref(self, vname, marked, transpose):
        """{state: (y_hp, S)} of C x (C^T x) in extended precision."""
        key = ("mult", vname, marked, transpose)
        if key not in self._refs:
            v, keep = self.velocity(vname), self.keep_of(marked)
            pa, pabs = self.qdata_ref(vname, marked)
            self._refs[key] = {s: (self.hi.mult(v, self.x[s], CALPHA, keep, transpose, pa=pa),
                                   self.hi.bound(v, self.x[s], CALPHA, keep, transpose, pabs=pabs)) for s in STATES}
        return self._refs[key]

    def qdata_ref(self, vname, marked):
        """(pa_hp, Pabs) [ne][3][nq]."""
        key = ("qdata", vname, marked)
        if key not in self._refs:
            v, keep = self.velocity(vname), self.keep_of(marked)
            self._refs[key] = (self.hi.pa_data(v, CALPHA, keep), self.hi.pa_bound(v, CALPHA, keep))
        return self._refs[key]


def geometry(kind, name, p, q1d):
    return HP.cached(("conv-geometry", kind, name, p, q1d), lambda: Geometry(kind, name, p, q1d))


VARIANTS = [(vname, marked, tr) for vname in ("const", "points") for marked in (False, True) for tr in (False, True)]
