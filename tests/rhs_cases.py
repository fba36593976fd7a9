"""The case matrix of the componentwise criterion for the right-hand side and the Robin face terms
(tests/lform_ref.py and tests/bdr_ref.py in numpy.longdouble with their running bounds, measured by
hp_ref.constant), shared by the CPU pins (test_lform_reference.py, test_bdr_reference.py: c_ref) and
the device tests (test_gpu_lform_componentwise.py, test_gpu_boundary_componentwise.py), so that the
reference and the device see identical float64 inputs.

Linear form.  A *space* is (mesh, p, q1d) on the existing smallest meshes of lform_ref (`small`,
`perturbed`, `fichera`), on `translated` -- `perturbed` moved by (10, -7, 3): coordinates large against
the edges -- and on `curved`, the fichera-q2 fixture in Jacobian mode.  On it live the source states:
point sources (constant, positive, signed), the field in celsius / kelvin / uniform(-1, 1), the affine
law of either temperature scale, and the Joule heat of four potentials (the suite's phi_field, the same
with an offset, an electrode-like 30 exp(-40 |x|^2) whose heat spans 50 decades, and a linear one), each
with a constant sigma and with sigma(T), T in kelvin.  The fields are functions of the coordinates
relative to the mesh's own origin, so that every mesh sees the same physics; the linear potential alone
takes the coordinates as they are.

Face terms.  A space is (mesh, p): bdr_ref's `small`, `perturbed`, `fichera`, `translated` and the
structured 8 x 8 x 8 `cube8`; a *rule* adds the face q1d.  The bilinear form is s (M_alpha + K_beta) + H
with the volume half scaled by a power of two s (exact on every side) chosen so that S_vol,i <=
S_bdr,i on every dof of a marked face, for every state and for the diagonal: a face error cannot hide
behind the volume term ("balanced", as in cw_cases).

Everything is computed once, cached in hp_ref.cached and left unchanged.
"""
import math
import tempfile

import numpy as np

import ecm2_amd as E
import oracle as O
import bdr_ref as BR
import hp_ref as HP
import helpers
import lform_ref as LR
from conv_cases import states
from cw_cases import STATES

LD = np.longdouble
SHIFT = np.array([10.0, -7.0, 3.0])
A_LIN = np.array([1.5, -0.7, 0.4])        # the linear potential a . x + 30
KELVIN = 273.15


# ======================================================================================
# The linear form
# ======================================================================================
LF_SPACES = ([("perturbed", p, p + dq) for p in (1, 2, 3, 4) for dq in (1, 2)]
             + [("fichera", 2, 3), ("fichera", 4, 5), ("small", 1, 2), ("translated", 2, 3),
                ("curved", 2, 3), ("curved", 2, 4)])
POINT_KINDS = ("constant", "quad_pos", "quad_signed")
FIELD_KINDS = ("gf_celsius", "gf_kelvin", "gf_random", "aff_celsius", "aff_kelvin")
POTENTIALS = ("phi", "offset", "electrode", "linear")
JOULE_KINDS = tuple("joule_" + n for n in POTENTIALS) + tuple("joule_%s_T" % n for n in POTENTIALS)
LF_KINDS = POINT_KINDS + FIELD_KINDS + JOULE_KINDS
LF_MARKER = [0, 1]


def lf_id(c):
    return "%s-p%d-q%d" % c


def _translated(make, shift=SHIFT):
    m = make(E)
    m.set_vertices(m.vertices() + shift)
    return m


class LFSpace:
    def __init__(self, name, p, q1d):
        self.name, self.p, self.q1d = name, p, q1d
        self.J = self.P = None
        origin = np.zeros(3)
        if name == "curved":
            with tempfile.TemporaryDirectory() as tmp:
                self.mesh, self.fes, self.J, self.X = helpers.curved_fichera(tmp, p, q1d)
        else:
            if name == "translated":
                self.mesh, origin = _translated(LR.mesh_perturbed), SHIFT
            else:
                self.mesh = LR.MESHES[name](E)
            self.fes = E.H1Space(self.mesh, p, E.NUMBERING_ENTITY)
            self.X = self.fes.dof_coords()
            self.P = O.quad_points(self.mesh.element_nodes(), q1d)
        self.gm, self.ndofs = self.fes.gather_map(), self.fes.ndofs
        self.ne = self.gm.shape[0]
        self.attr = self.mesh.GetAttributes()
        self.X0 = self.X - origin                     # coordinates relative to the mesh's own origin
        kw = dict(J=self.J) if self.J is not None else dict(enodes=self.mesh.element_nodes())
        # the float64 checker: the oracle's geometry (or the given J); on `translated` the edge form,
        # because the oracle's sum_c X_c dN_c loses |X| / h digits there that no bound over |edges| covers
        self.lo = LR.LFRef(p, q1d, self.gm, self.ndofs, edge_form=(name == "translated"), **kw)
        self.lo_oracle_geom = LR.LFRef(p, q1d, self.gm, self.ndofs, **kw) if name == "translated" else None
        self.hi = LR.LFRef(p, q1d, self.gm, self.ndofs, dtype=LD, edge_form=self.J is None, **kw)
        self._src, self._refs = None, {}

    def sources(self):
        if self._src is None:
            X0, nq = self.X0, self.q1d ** 3
            rng = np.random.default_rng(50 + self.p)
            if self.P is not None:
                P0 = self.P - (self.X - X0)[0]
                pos = helpers.coeff_function(P0)
            else:
                pos = rng.uniform(0.5, 2.0, (self.ne, nq)) + 1.0
            T = LR.temp_field(X0)
            s = {"constant": {"kind": "constant", "value": 2.5},
                 "quad_pos": {"kind": "quad", "values": pos},
                 "quad_signed": {"kind": "quad", "values": pos - 2.0},          # source minus sink
                 "gf_celsius": {"kind": "gridfunc", "field": T},
                 "gf_kelvin": {"kind": "gridfunc", "field": T + KELVIN},
                 "gf_random": {"kind": "gridfunc", "field": rng.uniform(-1.0, 1.0, self.ndofs)},
                 "aff_celsius": {"kind": "affine", "field": T, "scale": 0.8, "slope": 0.02, "t_ref": LR.T_REF},
                 "aff_kelvin": {"kind": "affine", "field": T + KELVIN, "scale": 0.8, "slope": 0.02,
                                "t_ref": LR.T_REF + KELVIN}}
            phi = {"phi": LR.phi_field(X0),
                   "offset": 30.0 + 1e-3 * LR.phi_field(X0),
                   "electrode": 30.0 * np.exp(-40.0 * np.sum(X0 * X0, axis=1)),
                   "linear": self.X @ A_LIN + 30.0}
            for n in POTENTIALS:
                s["joule_" + n] = {"kind": "joule", "phi": phi[n], "sigma": LR.SIGMA0, "slope": 0.0, "t_ref": 0.0,
                                   "T": None}
                s["joule_%s_T" % n] = {"kind": "joule", "phi": phi[n], "sigma": LR.SIGMA0, "slope": LR.SIGMA_SLOPE,
                                       "t_ref": LR.T_REF + KELVIN, "T": T + KELVIN}
            assert sorted(s) == sorted(LF_KINDS)
            self._src = s
        return self._src

    def keep(self):
        return LR.marker_keep(self.attr, LF_MARKER)

    def integrators(self, cname):
        """cname: a source kind (one unmarked integrator), "marked" (sigma(T) Joule heat on attribute 2)
        or "two" (the affine law everywhere, then the marked offset-potential Joule heat: order kept)."""
        s = self.sources()
        if cname == "marked":
            return [(s["joule_phi_T"], self.keep())]
        if cname == "two":
            return [(s["aff_kelvin"], None), (s["joule_offset_T"], self.keep())]
        return [(s[cname], None)]

    def ref(self, cname):
        """(b_hp, S) in extended precision."""
        if cname not in self._refs:
            integ = self.integrators(cname)
            self._refs[cname] = (self.hi.assemble(integ), self.hi.bound(integ))
        return self._refs[cname]

    def mass_one(self):
        """(M 1)_hp and its bound: the unit source's linear form."""
        return self.ref_of("unit", [({"kind": "constant", "value": 1.0}, None)])

    def ref_of(self, key, integ):
        if key not in self._refs:
            self._refs[key] = (self.hi.assemble(integ), self.hi.bound(integ))
        return self._refs[key]

    def family(self, cname):
        return "joule" if "joule" in cname or cname == "marked" else "point"

    def limit(self, cname):
        """(b_hp, L): the case's reference and its whole entrywise allowance in units of u, L = C S with
        the family's constant -- for "two" the bounds added, C_LF S_affine + C_LF_JOULE S_joule.
        hp_ref.constant(b, b_hp, L) <= 1 passes."""
        if cname == "two":
            a, j = self.integrators("two")
            key = ("limit", cname)
            if key not in self._refs:
                self._refs[key] = (self.hi.assemble([a, j]),
                                   LD(HP.C_LF) * self.hi.bound([a]) + LD(HP.C_LF_JOULE) * self.hi.bound([j]))
            return self._refs[key]
        b_hp, S = self.ref(cname)
        return b_hp, LD(HP.C_LF_JOULE if self.family(cname) == "joule" else HP.C_LF) * S

    def linear_potential_rhs(self):
        """sigma |a|^2 (M 1)_hp: what the Joule heat of phi = a . x + 30 is in exact arithmetic (the
        isoparametric map reproduces a linear function, so grad phi = a at every point)."""
        a = A_LIN.astype(LD)
        return LD(LR.SIGMA0) * np.sum(a * a) * self.mass_one()[0]


def lf_space(name, p, q1d):
    return HP.cached(("rhs-lf", name, p, q1d), lambda: LFSpace(name, p, q1d))


def lf_cases(name):
    """The integrator cases of a space: every kind; the marked and two-integrator cases where the mesh
    has two attributes (`perturbed`)."""
    return LF_KINDS + (("marked", "two") if name == "perturbed" else ())


# ======================================================================================
# The face terms
# ======================================================================================
ALPHA, BETA = 2.0, 0.7                     # the volume form s (M_alpha + K_beta)
BDR_SPACES = ([("small", 1), ("small", 2)] + [(n, p) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4)]
              + [("translated", 2)])
BDR_RULES = [(n, p, p + dq) for n, p in BDR_SPACES for dq in (1, 2)]
NUMBERING = {"cube8": E.NUMBERING_STRUCTURED}
T_B = 310.15                                # the blood temperature of g = h T_b


def bdr_id(c):
    return "%s-p%d-q%d" % c


def lf_rules(name, p):
    return sorted({BR.lf_default_q1d(p), p + 1, p + 2})


class BdrSpace:
    def __init__(self, name, p):
        self.name, self.p = name, p
        if name == "cube8":
            self.mesh = E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3)
        elif name == "translated":
            self.mesh = _translated(BR.mesh_perturbed)
        else:
            self.mesh = BR.MESHES[name](E)
        self.fes = E.H1Space(self.mesh, p, NUMBERING.get(name, E.NUMBERING_ENTITY))
        self.X = self.fes.dof_coords()
        self.gm, self.ndofs = self.fes.gather_map(), self.fes.ndofs
        origin = SHIFT if name == "translated" else np.zeros(3)
        self.x = states(self.X - origin, p)       # random, celsius, kelvin, 310.15 + a . x
        self.bmap, self.battr, self.bnodes = self.fes.boundary_map(), self.mesh.GetBdrAttributes(), self.mesh.boundary_nodes()
        self.origin = origin
        self._vol = None

    def volume(self):
        """The unit-scale volume reference M_alpha + K_beta (default rule): y_hp and S per state, the
        diagonal and its bound."""
        if self._vol is None:
            hp = HP.HPRef(self.mesh.element_nodes(), self.gm, self.ndofs, self.p, O.default_q1d(self.p),
                          alpha=ALPHA, beta=BETA)
            self._vol = dict(hp=hp, y={s: hp.mult(self.x[s]) for s in STATES}, S={s: hp.bound(self.x[s]) for s in STATES},
                             d=hp.diagonal(), dS=hp.diagonal_bound())
        return self._vol


def bdr_space(name, p):
    return HP.cached(("rhs-bdr", name, p), lambda: BdrSpace(name, p))


class BdrRule:
    """(space, face q1d): both checkers, the marker cases and the references of every case."""

    def __init__(self, name, p, q1d):
        self.space = s = bdr_space(name, p)
        self.name, self.p, self.q1d = name, p, q1d
        args = (p, q1d, s.bmap, s.battr, s.ndofs)
        self.lo = BR.BdrRef(*args, bnodes=s.bnodes)
        self.hi = BR.BdrRef(*args, bnodes=s.bnodes, dtype=LD)
        self.Pf = BR.face_points(s.bnodes, q1d) - s.origin            # face points, mesh-relative
        self.hq = BR.h_points(self.Pf)
        self._refs = {}

    def cases(self):
        """name -> [(h, marker)]: test_gpu_boundary's marker cases (unmarked constant; one attribute,
        per-point h; two integrators whose masks overlap)."""
        n = int(self.space.battr.max())
        one = [1 if a + 1 == 3 else 0 for a in range(n)]
        odd3 = [1 if (a + 1) % 2 == 1 or a + 1 == 3 else 0 for a in range(n)]
        hi = [1 if a + 1 >= 3 else 0 for a in range(n)]
        return {"unmarked": [(12.5, None)], "one": [(self.hq, one)], "two": [(12.5, odd3), (self.hq, hi)]}

    def lf_cases(self):
        """The face linear form's sources: g = h T_b per point (T_b in kelvin) on the overlapping
        markers, and a signed g (the flux h (T_b - T) changes sign over the surface)."""
        c = self.cases()
        signed = self.hq * np.sin(3.0 * self.Pf[..., 0] + 1.0)
        return {"hTb": [(12.5 * T_B, c["two"][0][1]), (self.hq * T_B, c["two"][1][1])],
                "signed": [(signed, None)], "signed_marked": [(signed, c["one"][0][1])]}

    def marked(self, integ):
        keep = np.zeros(self.lo.nbe, bool)
        for _, mk in integ:
            keep |= BR.marker_keep(self.lo.attr, mk)
        return keep

    def form_ref(self, cname):
        """The bilinear case: dict(integ, keep, scale s, y_hp / S_vol / S_bdr per state, d_hp, dS_vol,
        dS_bdr); S_vol already scaled by s."""
        key = ("form", cname)
        if key not in self._refs:
            integ = self.cases()[cname]
            vol, sp, hi = self.space.volume(), self.space, self.hi
            yb = {s: hi.mult(integ, sp.x[s]) for s in STATES}
            Sb = {s: hi.mult_bound(integ, sp.x[s]) for s in STATES}
            db, dSb = hi.diagonal(integ), hi.diagonal_bound(integ)
            keep = self.marked(integ)
            dofs = np.unique(sp.bmap[keep])
            # the diagonal's marker rule can zero a face the Mult keeps: balance where its bound is positive
            ratios = [float((Sb[s][dofs] / vol["S"][s][dofs]).min()) for s in STATES]
            dd = dofs[dSb[dofs] > 0]
            ratios.append(float((dSb[dd] / vol["dS"][dd]).min()))
            scale = 2.0 ** math.floor(math.log2(min(ratios)))
            sc = LD(scale)
            self._refs[key] = dict(integ=integ, keep=keep, dofs=dofs, ddofs=dd, scale=scale,
                                   y_hp={s: sc * vol["y"][s] + yb[s] for s in STATES},
                                   S_vol={s: sc * vol["S"][s] for s in STATES}, S_bdr=Sb,
                                   y_bdr=yb, d_hp=sc * vol["d"] + db, dS_vol=sc * vol["dS"], dS_bdr=dSb, d_bdr=db)
        return self._refs[key]

    def lform_ref(self, cname):
        key = ("lform", cname)
        if key not in self._refs:
            integ = self.lf_cases()[cname]
            self._refs[key] = (integ, self.hi.assemble(integ), self.hi.assemble_bound(integ))
        return self._refs[key]


def bdr_rule(name, p, q1d):
    return HP.cached(("rhs-bdr-rule", name, p, q1d), lambda: BdrRule(name, p, q1d))


def two_term_constant(y, y_hp, S_vol, S_bdr, c_vol):
    """max_i |y_i - y_hp,i| / (u (c_vol S_vol,i + C_BDR S_bdr,i)) as a fraction of 1: the bilinear form's
    criterion (<= 1 passes)."""
    return HP.constant(y, y_hp, LD(c_vol) * S_vol + LD(HP.C_BDR) * S_bdr)
