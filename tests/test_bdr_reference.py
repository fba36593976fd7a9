"""CPU pins of tests/bdr_ref.py, the numpy checker of the boundary-face kernels: exact integrals
(1^T H 1 = h area, sum b = g area over the marked faces), the sum-factorised face mass against the
face mass matrix assembled entry by entry, the marker rules, and the helper's own float64 error
against its np.longdouble restatement (it has to stay far below the GPU tests' 1e-12 bar).

The componentwise criterion (second half; run with -s for the tables): the float64 checker's constants
against the extended-precision instance over the device case matrix (tests/rhs_cases.py), the rule
hp_ref.C_BDR / C_BDR_DIAG / C_BDR_QD = 4 c_ref rounded up to a power of two, the balance condition of
the two-term criterion for the bilinear form, and what the criterion sees."""
import math
import os

import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import bdr_ref as R
import hp_ref as HP
import rhs_cases as RC
from cw_cases import STATES
from helpers import GOLDEN, RTOL, relerr


def _ref(mesh, p, q1d, dtype=np.float64, numbering=None):
    fes = E.H1Space(mesh, p, E.NUMBERING_ENTITY if numbering is None else numbering)
    return fes, R.BdrRef(p, q1d, fes.boundary_map(), mesh.GetBdrAttributes(), fes.ndofs,
                         bnodes=mesh.boundary_nodes(), dtype=dtype)


def _quad_areas(mesh):
    """Areas of planar boundary quads from the vertices alone: |(v1 - v0) x (v3 - v0)| (rectangles)."""
    V, Q = mesh.vertices(), mesh.boundary()
    return np.linalg.norm(np.cross(V[Q[:, 1]] - V[Q[:, 0]], V[Q[:, 3]] - V[Q[:, 0]]), axis=1)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_unit_cube_sides_have_area_one(p):
    """Attribute by attribute on the unit cube: 1^T H 1 = h and sum b = g (each side has area 1),
    with MassIntegrator's rule (p + 1) and BoundaryLFIntegrator's default."""
    mesh = E.Mesh.MakeCartesian3D(3, 2, 2)
    h, g = 7.5, 2.25
    fes, ref = _ref(mesh, p, p + 1)
    _, lref = _ref(mesh, p, R.lf_default_q1d(p))
    one = np.ones(fes.ndofs)
    for a in range(1, 7):
        mk = [1 if k + 1 == a else 0 for k in range(6)]
        assert abs(one @ ref.mult([(h, mk)], one) - h) < 1e-13 * h
        assert abs(lref.assemble([(g, mk)]).sum() - g) < 1e-13 * g
    assert abs(one @ ref.mult([(h, None)], one) - 6 * h) < 1e-12


@pytest.mark.parametrize("p", [1, 2, 3])
def test_fichera_file_attributes(p):
    """fichera.mesh (planar rectangular faces): per file attribute, 1^T H 1 = h area and sum b = g
    area, the area taken from the vertices alone."""
    mesh = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    attr, area = mesh.GetBdrAttributes(), _quad_areas(mesh)
    fes, ref = _ref(mesh, p, p + 1)
    _, lref = _ref(mesh, p, R.lf_default_q1d(p))
    one = np.ones(fes.ndofs)
    h, g = 3.0, 0.5
    for a in sorted(set(attr.tolist())):
        mk = np.zeros(attr.max(), np.int32)
        mk[a - 1] = 1
        A = area[attr == a].sum()
        assert abs(one @ ref.mult([(h, mk)], one) - h * A) < 1e-13 * h * A
        assert abs(lref.assemble([(g, mk)]).sum() - g * A) < 1e-13 * g * A


@pytest.mark.parametrize("name,p,dq", [("perturbed", 1, 1), ("perturbed", 2, 2), ("fichera", 3, 1), ("perturbed", 4, 2)])
def test_sum_factorised_mass_equals_entrywise_matrix(name, p, dq):
    """B^T D B on every face equals the face mass matrix assembled entry by entry; its diagonal is
    the PA diagonal; non-planar faces, a per-point h."""
    mesh = R.MESHES[name](E)
    q1d = p + dq
    fes, ref = _ref(mesh, p, q1d)
    pa = ref.pa_data(R.h_points(R.face_points(mesh.boundary_nodes(), q1d)))
    M = ref.face_matrix(pa)
    xf = ref.gather(R.positive_field(fes.dof_coords()))
    D = p + 1
    y_mat = np.einsum("fij,fj->fi", M, xf.reshape(-1, D * D))
    assert relerr(ref.face_apply(pa, xf).reshape(-1, D * D), y_mat) < 1e-14
    assert relerr(ref.face_diag(pa).reshape(-1, D * D), np.einsum("fii->fi", M)) < 1e-14


def test_marker_rules():
    """Mult masks each integrator by its own marker; the diagonal's shared face vector is zeroed by a
    later marked integrator on the faces that one excludes (bilinearform_ext.cpp:441-452)."""
    mesh = R.mesh_perturbed(E)
    p, q1d = 2, 3
    fes, ref = _ref(mesh, p, q1d)
    x = R.positive_field(fes.dof_coords())
    m13, m36 = [1, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 1]
    y = ref.mult([(2.0, m13), (5.0, m36)], x)
    assert relerr(y, ref.mult([(2.0, m13)], x) + ref.mult([(5.0, m36)], x)) < 1e-14
    d = ref.diagonal([(2.0, m13), (5.0, m36)])
    # integrator 1 survives only where integrator 2 acts too: attribute 3
    only3 = [0, 0, 1, 0, 0, 0]
    assert relerr(d, ref.diagonal([(2.0, only3)]) + ref.diagonal([(5.0, m36)])) < 1e-14
    # an unmarked later integrator masks nothing
    d2 = ref.diagonal([(2.0, m13), (5.0, None)])
    assert relerr(d2, ref.diagonal([(2.0, m13)]) + ref.diagonal([(5.0, None)])) < 1e-14
    # pa_data holds zeros on excluded faces
    keep = R.marker_keep(ref.attr, m13)
    assert np.all(ref.pa_data(2.0, m13)[~keep] == 0.0) and np.all(ref.pa_data(2.0, m13)[keep] > 0.0)


@pytest.mark.parametrize("name", ["perturbed", "fichera"])
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_float64_helper_error_is_far_below_the_gpu_bar(name, p):
    """The float64 checker against its np.longdouble restatement: Mult, diagonal and linear form."""
    mesh = R.MESHES[name](E)
    q1d = p + 1
    fes, r64 = _ref(mesh, p, q1d)
    _, rld = _ref(mesh, p, q1d, dtype=np.longdouble)
    x = R.positive_field(fes.dof_coords())
    hq = R.h_points(R.face_points(mesh.boundary_nodes(), q1d))
    nattr = int(mesh.GetBdrAttributes().max())
    mk = [1 if a % 2 == 0 else 0 for a in range(nattr)]
    integ = [(hq, None), (4.0, mk)]
    gaps = (relerr(r64.mult(integ, x), rld.mult(integ, x).astype(np.float64)),
            relerr(r64.diagonal(integ), rld.diagonal(integ).astype(np.float64)),
            relerr(r64.assemble(integ), rld.assemble(integ).astype(np.float64)))
    print(f"{name} p={p}: float64 vs longdouble gaps mult {gaps[0]:.2e} diag {gaps[1]:.2e} lform {gaps[2]:.2e}")
    assert max(gaps) < 1e-13


# ---- the componentwise criterion: c_ref, the device bounds and what they see --------------------------
_ROWS = {}
RULES = RC.BDR_RULES + [("cube8", 2, 3)]


def _matrix_mult(lo, integ, x):
    """The checker's second, independent Mult: the face mass matrices assembled entry by entry."""
    xf = lo.gather(x).reshape(lo.nbe, -1)
    yf = np.zeros_like(xf)
    for h, mk in integ:
        yf += np.einsum("fij,fj->fi", lo.face_matrix(lo.pa_data(h, mk)), xf)
    return lo.add_transpose(yf, np.zeros(lo.ndofs))


def _checker_constants(case):
    if case not in _ROWS:
        r = RC.bdr_rule(*case)
        sp, lo, hi = r.space, r.lo, r.hi
        row = dict(mult=0.0, matrix=0.0, diag=0.0, qd=0.0, lf=0.0, scales=[])
        for cname, integ in r.cases().items():
            f = r.form_ref(cname)
            row["scales"].append(f["scale"])
            for s in STATES:
                ref = (f["y_bdr"][s], f["S_bdr"][s])
                row["mult"] = max(row["mult"], HP.constant(lo.mult(integ, sp.x[s]), *ref))
                row["matrix"] = max(row["matrix"], HP.constant(_matrix_mult(lo, integ, sp.x[s]), *ref))
            row["diag"] = max(row["diag"], HP.constant(lo.diagonal(integ), f["d_bdr"], f["dS_bdr"]))
            for h, mk in integ:
                row["qd"] = max(row["qd"], HP.constant(lo.pa_data(h, mk).ravel(), hi.pa_data(h, mk).ravel(),
                                                       hi.pa_bound(h, mk).ravel()))
        # the face linear form: this rule, and with the p + 1 rule the default one too
        rules = {case[2]} | ({R.lf_default_q1d(case[1])} if case[2] == case[1] + 1 else set())
        for q in sorted(rules):
            rr = RC.bdr_rule(case[0], case[1], q)
            for cname in rr.lf_cases():
                integ, b_hp, S = rr.lform_ref(cname)
                row["lf"] = max(row["lf"], HP.constant(rr.lo.assemble(integ), b_hp, S))
        _ROWS[case] = row
    return _ROWS[case]


@pytest.mark.parametrize("case", RULES, ids=[RC.bdr_id(c) for c in RULES])
def test_checker_componentwise_constants(case):
    """The float64 checker against its extended-precision instance on every marker case and state: Mult
    (sum-factorised and entrywise matrices) and the face linear form within C_BDR / 4, the diagonal within
    C_BDR_DIAG / 4, the qdata within C_BDR_QD / 4.  And the balance condition of the two-term criterion,
    which is a condition, not a measurement: S_vol,i <= S_bdr,i on every dof of a marked face, for every
    state and for the diagonal."""
    row = _checker_constants(case)
    print("\n%-18s Mult %.2f | matrices %.2f | diagonal %.2f | qdata %.2f | linear form %.2f | volume scale %s" % (
        RC.bdr_id(case), row["mult"], row["matrix"], row["diag"], row["qd"], row["lf"], row["scales"]))
    assert 4.0 * max(row["mult"], row["matrix"], row["lf"]) <= HP.C_BDR
    assert 4.0 * row["diag"] <= HP.C_BDR_DIAG and 4.0 * row["qd"] <= HP.C_BDR_QD
    r = RC.bdr_rule(*case)
    for cname in r.cases():
        f = r.form_ref(cname)
        assert f["dofs"].size and f["ddofs"].size
        for s in STATES:
            assert np.all(f["S_vol"][s][f["dofs"]] <= f["S_bdr"][s][f["dofs"]]), (cname, s)
            assert np.all(f["S_bdr"][s][f["dofs"]] > 0)
        assert np.all(f["dS_vol"][f["ddofs"]] <= f["dS_bdr"][f["ddofs"]]), cname


def test_bdr_device_bounds_are_four_c_ref():
    rows = [_checker_constants(c) for c in RULES]
    for name, c_ref, have in (("C_BDR", max(max(r["mult"], r["matrix"], r["lf"]) for r in rows), HP.C_BDR),
                              ("C_BDR_DIAG", max(r["diag"] for r in rows), HP.C_BDR_DIAG),
                              ("C_BDR_QD", max(r["qd"] for r in rows), HP.C_BDR_QD)):
        want = 2.0 ** math.ceil(math.log2(4.0 * c_ref))
        print(f"\n{name}: c_ref = {c_ref:.2f}, 4 c_ref = {4 * c_ref:.1f} -> {want:g} (hp_ref.{name} = {have:g})")
        assert have == want


@pytest.mark.parametrize("p", [2, 3, 4])
def test_one_point_qdata_error_in_the_last_face_group_is_seen(p):
    """qd at one point of the last face of `perturbed` (94 faces: the last, partial group of the 8-face
    workgroups of k_bdr_apply_grp, and of the 64-face ones of k_bdr_apply_tpf) off by 1e-12 relative:
    above C_BDR_QD in the qdata and above C_BDR in H x on every state."""
    r = RC.bdr_rule("perturbed", p, p + 1)
    sp, lo, hi = r.space, r.lo, r.hi
    integ = r.cases()["unmarked"]
    f = r.form_ref("unmarked")
    pa = lo.pa_data(*integ[0])
    bad = pa.copy()
    bad[lo.nbe - 1, (p + 1) ** 2 // 2] *= 1.0 + 1e-12
    ref = (hi.pa_data(*integ[0]).ravel(), hi.pa_bound(*integ[0]).ravel())
    assert HP.constant(pa.ravel(), *ref) <= HP.C_BDR_QD / 4 and HP.constant(bad.ravel(), *ref) > HP.C_BDR_QD
    for s in STATES:
        y = [lo.add_transpose(lo.face_apply(v, lo.gather(sp.x[s])), np.zeros(lo.ndofs)) for v in (pa, bad)]
        good, hurt = (HP.constant(v, f["y_bdr"][s], f["S_bdr"][s]) for v in y)
        print(f"\np={p} {s}: {good:.2f} -> {hurt:.1f} (C_BDR = {HP.C_BDR:g})")
        assert good <= HP.C_BDR / 4 and hurt > HP.C_BDR


@pytest.mark.parametrize("name,p", [("perturbed", 2), ("perturbed", 4), ("fichera", 3)])
def test_face_error_behind_the_volume_term(name, p):
    """One face's contribution to H x scaled by 1 + 1e-10 and added to the volume term.  The two-term
    criterion |y - y_hp|_i <= u (C S_vol,i + C_BDR S_bdr,i) on the balanced form sees it on every state,
    8900 - 17900 times the bound.

    The old bar -- relerr < 1e-12 over all dofs of M_2 + K_0.7 + H on positive_field, the form of
    test_gpu_boundary.py.  On that form the face term is NOT small against the volume term (h = 12.5 on
    faces of 0.2 x 0.2 against alpha h^3 + beta h), so the old bar does see 1e-10: recorded 7.6e-11
    (perturbed p = 2, 4) and 5.9e-11 (fichera p = 3).  Its blind spot starts a hundred times lower: the
    same face scaled by 1 + 1e-12 gives 7.6e-13 / 5.9e-13, which the old bar passes, and is still 90 - 120
    times the two-term bound.  Both halves of that gap are asserted."""
    r = RC.bdr_rule(name, p, p + 1)
    sp, lo = r.space, r.lo
    integ = r.cases()["unmarked"]
    f = r.form_ref("unmarked")
    face = lo.nbe - 1

    def face_part(x, factor):
        yf = lo.face_apply(lo.pa_data(*integ[0]), lo.gather(x))
        yf[face] *= factor
        return lo.add_transpose(yf, np.zeros(lo.ndofs))

    for s in STATES:
        yv = (HP.LD(f["scale"]) * sp.volume()["y"][s]).astype(np.float64)
        good, hurt = (RC.two_term_constant(yv + face_part(sp.x[s], k), f["y_hp"][s], f["S_vol"][s], f["S_bdr"][s], HP.C)
                      for k in (1.0, 1.0 + 1e-10))
        print(f"\n{name} p={p} {s}: {good:.3f} -> {hurt:.1f} of the two-term bound")
        assert good <= 0.25 and hurt > 1.0
    # the suite's form and input under the old bar
    x = R.positive_field(sp.X)
    op = O.OracleOperator(sp.mesh.element_nodes(), sp.gm, sp.ndofs, p, alpha=RC.ALPHA, beta=RC.BETA)
    y_ref = lo.mult(integ, x, op.mult(x))
    old = {k: relerr(op.mult(x) + face_part(x, 1.0 + k), y_ref) for k in (1e-10, 1e-12)}
    s = "kelvin"
    yv = (HP.LD(f["scale"]) * sp.volume()["y"][s]).astype(np.float64)
    new12 = RC.two_term_constant(yv + face_part(sp.x[s], 1.0 + 1e-12), f["y_hp"][s], f["S_vol"][s], f["S_bdr"][s], HP.C)
    print(f"the old bar on the suite's form: relerr {old[1e-10]:.2e} at 1 + 1e-10, {old[1e-12]:.2e} at 1 + 1e-12 "
          f"(RTOL {RTOL:g}); the two-term criterion at 1 + 1e-12: {new12:.1f}")
    assert old[1e-12] < RTOL and new12 > 1.0
