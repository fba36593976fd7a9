"""CPU pins of tests/lform_ref.py (the numpy restatement of DLFEvalAssemble3D + the source
coefficients that the GPU linear form is compared with), so that comparison means something:
identities against the oracle's mass operator, the exactness of a linear potential's gradient on a
non-affine mesh, the total source, and the helper's own float64 error against an extended-precision
restatement of the same formulas.

The componentwise criterion (second half; run with -s for the tables): the float64 checker's constants
against the extended-precision instance over the device case matrix (tests/rhs_cases.py) -- c_ref per
source family --, the rule hp_ref.C_LF / C_LF_JOULE = 4 c_ref rounded up to a power of two, and what the
criterion sees: a 1e-12 error at one point of the last workgroup, the electrode source's small entries
(which relerr < 1e-12 passes), an untransposed adjugate on one element, and the linear potential's heat
against sigma |a|^2 M 1."""
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import hp_ref as HP
import lform_ref as R
import rhs_cases as RC
from helpers import RTOL, relerr


def _space(name, p):
    m = R.MESHES[name](E)
    fes = E.H1Space(m, p, E.NUMBERING_ENTITY)
    return m, fes


def _ref(m, fes, p, q1d, dtype=np.float64):
    return R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, enodes=m.element_nodes(), dtype=dtype)


def _mass(m, fes, p, q1d):
    return O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=1.0, beta=None, q1d=q1d)


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dq", [1, 2])
def test_unit_source_is_mass_times_one(name, p, dq):
    """f = 1: b = M 1 of the oracle's mass operator at the same rule."""
    m, fes = _space(name, p)
    ref = _ref(m, fes, p, p + dq)
    b = ref.assemble([({"kind": "constant", "value": 1.0}, None)])
    assert relerr(b, _mass(m, fes, p, p + dq).mult(np.ones(fes.ndofs))) < RTOL


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_field_source_is_mass_times_field(name, p):
    """f = g in V_h (GridFunctionCoefficient) at Q1D = p + 2: b = M g."""
    m, fes = _space(name, p)
    g = np.random.default_rng(2).uniform(0.5, 1.5, fes.ndofs)
    ref = _ref(m, fes, p, p + 2)
    b = ref.assemble([({"kind": "gridfunc", "field": g}, None)])
    assert relerr(b, _mass(m, fes, p, p + 2).mult(g)) < RTOL


@pytest.mark.parametrize("p", [1, 2, 3, 4])
@pytest.mark.parametrize("dq", [1, 2])
def test_linear_potential_on_nonaffine_mesh(p, dq):
    """phi = a . x on the perturbed mesh: the trilinear isoparametric map reproduces linear functions,
    so grad phi = a at every point and b = sigma |a|^2 (M 1): pins J^-T."""
    m, fes = _space("perturbed", p)
    a = np.array([1.5, -0.7, 0.4])
    phi = fes.dof_coords() @ a
    ref = _ref(m, fes, p, p + dq)
    b = ref.assemble([({"kind": "joule", "phi": phi, "sigma": 0.6, "slope": 0.0, "t_ref": 0.0, "T": None}, None)])
    want = 0.6 * (a @ a) * _mass(m, fes, p, p + dq).mult(np.ones(fes.ndofs))
    assert relerr(b, want) < RTOL


@pytest.mark.parametrize("kind", R.KINDS)
def test_total_source(kind):
    """1^T b = sum_q W det J f (partition of unity)."""
    p, q1d = 2, 3
    m, fes = _space("perturbed", p)
    ref = _ref(m, fes, p, q1d)
    src = R.make_source(kind, fes.dof_coords(), O.quad_points(m.element_nodes(), q1d))
    b = ref.assemble([(src, None)])
    total = float(np.sum(ref.W[None, :] * ref.detJ * ref.point_values(src)))
    assert abs(b.sum() - total) < RTOL * abs(total)


def test_markers_and_order():
    """An excluded element contributes nothing; integrators add in order."""
    p, q1d = 2, 3
    m, fes = _space("perturbed", p)
    ref = _ref(m, fes, p, q1d)
    X, P = fes.dof_coords(), O.quad_points(m.element_nodes(), q1d)
    keep = R.marker_keep(m.GetAttributes(), [0, 1])
    assert 0 < keep.sum() < fes.ne
    s1, s2 = R.make_source("joule_T", X, P), R.make_source("affine", X, P)
    b = ref.assemble([(s1, keep), (s2, None)])
    f1 = ref.point_values(s1) * keep[:, None]
    want = ref.reduce(ref.element_vectors(f1)) + ref.reduce(ref.element_vectors(ref.point_values(s2)))
    assert relerr(b, want) < 1e-15


@pytest.mark.parametrize("name,p,dq", R.CASES)
def test_float64_helper_against_extended_precision(name, p, dq):
    """The float64 helper agrees with the np.longdouble restatement of the same formulas to better
    than 1e-13 on the meshes and sources of the GPU tests (the GPU bar is 1e-12)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is float64 on this platform")
    m, fes = _space(name, p)
    q1d = p + dq
    r64, rld = _ref(m, fes, p, q1d), _ref(m, fes, p, q1d, dtype=np.longdouble)
    X, P = fes.dof_coords(), O.quad_points(m.element_nodes(), q1d)
    for kind in R.KINDS:
        src = R.make_source(kind, X, P)
        be64 = r64.element_vectors(r64.point_values(src))
        beld = rld.element_vectors(rld.point_values(src))
        err = float(np.abs(be64 - beld).max() / np.abs(beld).max())
        b_err = relerr(r64.assemble([(src, None)]), rld.assemble([(src, None)]).astype(np.float64))
        print(f"{name} p={p} q1d={q1d} {kind}: element vectors {err:.2e}, b {b_err:.2e}")
        assert err < 1e-13 and b_err < 1e-13


def test_curved_jacobian_mode_helper(tmp_path):
    """The Jacobian-mode helper on the curved fichera mesh: f = 1 gives the oracle's M 1 from the same
    Jacobians, and float64 agrees with the extended-precision restatement."""
    p, q1d = 2, 3
    mesh, fes, J, X = helpers.curved_fichera(tmp_path, p, q1d)
    ref = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, J=J)
    b = ref.assemble([({"kind": "constant", "value": 1.0}, None)])
    op = O.OracleOperator.from_jacobians(J, fes.gather_map(), fes.ndofs, p, alpha=1.0, beta=None, q1d=q1d)
    assert relerr(b, op.mult(np.ones(fes.ndofs))) < RTOL
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        rld = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, J=J, dtype=np.longdouble)
        src = R.make_source("joule_T", X, None)
        assert relerr(ref.assemble([(src, None)]), rld.assemble([(src, None)]).astype(np.float64)) < 1e-13


# ---- the componentwise criterion: c_ref, the device bounds and what they see --------------------------
_ROWS = {}


def _oracle_mass(sp):
    if sp.J is not None:
        return O.OracleOperator.from_jacobians(sp.J, sp.gm, sp.ndofs, sp.p, alpha=1.0, beta=None, q1d=sp.q1d)
    return O.OracleOperator(sp.mesh.element_nodes(), sp.gm, sp.ndofs, sp.p, alpha=1.0, beta=None, q1d=sp.q1d)


def _checker_constants(case):
    """{case name: constant of the float64 checker}, plus "mass:<kind>": the oracle's mass Mult of the
    same field against the grid-function references (not on `translated`: the oracle's geometry sums
    X_c dN_c over coordinates 50 times the edges, which no bound over the edges covers)."""
    if case not in _ROWS:
        sp = RC.lf_space(*case)
        row = {}
        for cname in RC.lf_cases(sp.name):
            b_hp, S = sp.ref(cname)
            row[cname] = HP.constant(sp.lo.assemble(sp.integrators(cname)), b_hp, S)
        if sp.name != "translated":
            op = _oracle_mass(sp)
            for kind in ("gf_celsius", "gf_kelvin", "gf_random"):
                row["mass:" + kind] = HP.constant(op.mult(sp.sources()[kind]["field"]), *sp.ref(kind))
        _ROWS[case] = row
    return _ROWS[case]


def _worst(case):
    sp, row = RC.lf_space(*case), _checker_constants(case)
    fam = {"point": 0.0, "joule": 0.0}
    for k, v in row.items():
        if k != "two":                                  # (two families in one vector: held to the added bounds)
            f = sp.family(k.split(":")[-1])
            fam[f] = max(fam[f], v)
    return fam


@pytest.mark.parametrize("case", RC.LF_SPACES, ids=[RC.lf_id(c) for c in RC.LF_SPACES])
def test_checker_componentwise_constants(case):
    """The float64 checker (and, for the grid-function sources, the oracle's mass Mult) sits within
    C_LF / 4 (the Joule sources, the marked and the two-integrator case: C_LF_JOULE / 4) of the
    extended-precision reference on every source state.  Run with -s for the row."""
    row = _checker_constants(case)
    print("\n%-18s %s" % (RC.lf_id(case), " ".join("%s %.2f" % kv for kv in row.items())))
    w = _worst(case)
    assert 4.0 * w["point"] <= HP.C_LF and 4.0 * w["joule"] <= HP.C_LF_JOULE, w
    sp = RC.lf_space(*case)
    if "two" in row:
        two = HP.constant(sp.lo.assemble(sp.integrators("two")), *sp.limit("two"))
        print("   two integrators against C_LF S_affine + C_LF_JOULE S_joule: %.3f" % two)
        assert 4.0 * two <= 1.0
    if sp.lo_oracle_geom is not None:
        og = max(HP.constant(sp.lo_oracle_geom.assemble(sp.integrators(k)), *sp.ref(k)) for k in RC.POINT_KINDS)
        print("   the same checker on the oracle's geometry (sum_c X_c dN_c, not part of c_ref): %.1f" % og)


def test_lform_device_bounds_are_four_c_ref():
    """hp_ref.C_LF and C_LF_JOULE = 4 c_ref rounded up to a power of two over the whole case matrix."""
    worst = [_worst(c) for c in RC.LF_SPACES]
    for name, fam, have in (("C_LF", "point", HP.C_LF), ("C_LF_JOULE", "joule", HP.C_LF_JOULE)):
        c_ref = max(w[fam] for w in worst)
        want = 2.0 ** math.ceil(math.log2(4.0 * c_ref))
        print(f"\n{name}: c_ref = {c_ref:.2f}, 4 c_ref = {4 * c_ref:.1f} -> {want:g} (hp_ref.{name} = {have:g})")
        assert have == want


def test_marked_case_leaves_untouched_dofs_exactly_zero():
    """With the marker [0, 1] a dof no kept element touches has S = 0, and hp_ref.constant then demands
    an exact 0: a value of 1e-300 there is an infinite constant."""
    sp = RC.lf_space("perturbed", 2, 3)
    b_hp, S = sp.ref("marked")
    b = sp.lo.assemble(sp.integrators("marked"))
    zero = np.flatnonzero(S == 0)
    assert zero.size and np.all(b[zero] == 0.0)
    assert HP.constant(b, b_hp, S) <= HP.C_LF_JOULE / 4
    b[zero[0]] = 1e-300
    assert HP.constant(b, b_hp, S) == float("inf")


@pytest.mark.parametrize("p,q1d", [(1, 2), (2, 3), (2, 4), (3, 5), (4, 6)])
def test_one_point_error_in_the_last_workgroup_is_seen(p, q1d):
    """W f det J at one quadrature point off by 1e-12 relative, in the last element of `perturbed` (80
    elements: the device's workgroups hold 64 / 28 / 16 / 10 / 7 at Q1D = 2..6, so that element sits in
    the last group -- a partial one but at Q1D = 4, where 80 = 5 x 16): above C_LF on the positive, the
    signed and the kelvin grid-function source."""
    sp = RC.lf_space("perturbed", p, q1d)
    lo = sp.lo
    for kind in ("quad_pos", "quad_signed", "gf_kelvin"):
        f = lo.point_values(sp.sources()[kind])
        bad = f.copy()
        bad[sp.ne - 1, (q1d ** 3) // 2] *= 1.0 + 1e-12
        b_hp, S = sp.ref(kind)
        good, hurt = (HP.constant(lo.reduce(lo.element_vectors(v)), b_hp, S) for v in (f, bad))
        print(f"\np={p} q1d={q1d} {kind}: {good:.2f} -> {hurt:.1f} (C_LF = {HP.C_LF:g})")
        assert good <= HP.C_LF / 4 and hurt > HP.C_LF


def test_small_entries_of_the_electrode_source_are_seen():
    """The electrode potential's Joule heat spans 50 decades here.  Every entry below 1e-12 max |b| multiplied by
    1 + 1e-6: the global relerr < 1e-12 passes (those entries are invisible to it), the componentwise
    constant is 1e-6 / u |b_i| / S_i, far above C_LF_JOULE."""
    sp = RC.lf_space("perturbed", 2, 3)
    b_hp, S = sp.ref("joule_electrode")
    b = sp.lo.assemble(sp.integrators("joule_electrode"))
    small = np.abs(b) < 1e-12 * np.abs(b).max()
    assert small.sum() > 100 and np.abs(b).min() < 1e-45 * np.abs(b).max()
    bad = np.where(small, b * (1.0 + 1e-6), b)
    good, hurt = HP.constant(b, b_hp, S), HP.constant(bad, b_hp, S)
    old = relerr(bad, b_hp.astype(np.float64))
    print(f"\nelectrode: {int(small.sum())} of {b.size} entries below 1e-12 max|b|; relerr {old:.2e}; constant {good:.2f} -> {hurt:.3g}")
    assert old < RTOL
    assert good <= HP.C_LF_JOULE / 4 and hurt > HP.C_LF_JOULE


@pytest.mark.parametrize("pot", ["phi", "offset", "electrode"])
def test_untransposed_adjugate_on_one_element_is_seen(pot):
    """The gradient mapped by adj J instead of adj J^T on one non-affine element (the last one)."""
    sp = RC.lf_space("perturbed", 2, 3)
    lo, src = sp.lo, sp.sources()["joule_" + pot]
    f = lo.point_values(src)
    e = sp.ne - 1
    g = np.einsum("qij,qj->qi", lo.A[e], lo.ref_grad(src["phi"])[e]) / lo.detJ[e][:, None]
    bad = f.copy()
    bad[e] = src["sigma"] * np.sum(g * g, axis=-1)
    b_hp, S = sp.ref("joule_" + pot)
    good, hurt = (HP.constant(lo.reduce(lo.element_vectors(v)), b_hp, S) for v in (f, bad))
    print(f"\njoule_{pot}: {good:.2f} -> {hurt:.3g} (C_LF_JOULE = {HP.C_LF_JOULE:g})")
    assert good <= HP.C_LF_JOULE / 4 and hurt > HP.C_LF_JOULE


@pytest.mark.parametrize("case", [c for c in RC.LF_SPACES if c[0] != "small"], ids=RC.lf_id)
def test_linear_potential_componentwise(case):
    """phi = a . x + 30 (the isoparametric map reproduces it, so grad phi = a at every point): the
    checker's b against sigma |a|^2 (M 1)_hp within the Joule bound of that very case -- the offset 30 and,
    on `translated`, the coordinates cancel in the gradient, and S accounts for it."""
    sp = RC.lf_space(*case)
    want = sp.linear_potential_rhs()
    S = sp.ref("joule_linear")[1]
    c = HP.constant(sp.lo.assemble(sp.integrators("joule_linear")), want, S)
    ch = HP.constant(sp.ref("joule_linear")[0].astype(np.float64), want, S)
    print(f"\n{RC.lf_id(case)}: checker against sigma |a|^2 M 1: {c:.2f}; the reference itself {ch:.2f}")
    assert c <= HP.C_LF_JOULE / 4 and ch <= HP.C_LF_JOULE / 4

