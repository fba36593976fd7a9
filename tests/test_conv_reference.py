"""CPU pins of tests/conv_ref.py, the numpy checker of the convection kernels, on the 5 x 4 x 3 mesh with
every vertex moved (non-affine hexes) and on fichera refined once: the sum-factorised PA path against the
independent dense element matrices (Mult and MultTranspose), C 1 = 0, the duality <w, C x> = <C^T w, x>,
the linear-field identity C (g . p) = alpha (v . g) M_1 1 against the oracle's unit mass, and the helper's
own float64 error against its np.longdouble restatement (it has to stay far below the GPU tests' 1e-12 bar).

The componentwise criterion (second half; run with -s for the tables): the float64 checker's constants
against the extended-precision instance over the device case matrix (tests/conv_cases.py) -- c_ref for
Mult / MultTranspose jointly and for the qdata --, the rule hp_ref.C_CONV / C_CONV_QD = 4 c_ref rounded up to
a power of two, what a 1e-12 qdata error at one point does to each criterion, and the Jacobian-mode
reference against the corner path and on the curved meshes' identities.

Bounds: each quantity is a sum of at most (Q^3 + D^3 + 8) products per entry and per stage, rounded at
2^-53 = 1.1e-16; two different summation orders of the same sums differ by a few hundred units of that
against the largest entry, so 1e-13 relative (inf-norm) separates rounding from any wrong formula, whose
error is O(1)."""
import math

import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import bdr_ref as BR
import conv_ref as R
import conv_cases as CC
import hp_ref as HP
from cw_cases import STATES
from helpers import RTOL, relerr

TOL = 1e-13
ALPHA = 1.7
VCONST = np.array([0.8, -0.3, 0.5])
G = np.array([0.4, -1.1, 0.7])

_CACHE = {}


def setup(name, p, q1d, dtype=np.float64):
    key = (name, p, q1d, dtype)
    if key not in _CACHE:
        mesh = BR.MESHES[name](E)
        fes = E.H1Space(mesh, p, E.NUMBERING_ENTITY)
        ref = R.ConvRef(p, q1d, fes.gather_map(), fes.ndofs, mesh.element_nodes(), dtype=dtype)
        rng = np.random.default_rng(5)
        _CACHE[key] = dict(mesh=mesh, fes=fes, ref=ref, x=rng.uniform(0.0, 1.0, fes.ndofs),
                           w=rng.uniform(0.0, 1.0, fes.ndofs), X=fes.dof_coords())
    return _CACHE[key]


def velocities(ref):
    return {"const": VCONST, "points": R.reference_velocity(ref.P.astype(np.float64))}


CASES = [(n, p, dq) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4) for dq in (1, 2)]


@pytest.mark.parametrize("name,p,dq", CASES)
def test_pa_equals_full_assembly(name, p, dq):
    """The reference's own PA-vs-FA test (test_pa_kernels.cpp:498-578): Mult and MultTranspose."""
    s = setup(name, p, p + dq)
    ref = s["ref"]
    for vname, v in velocities(ref).items():
        for tr in (False, True):
            y_pa = ref.mult(v, s["x"], ALPHA, transpose=tr)
            y_fa = ref.fa_mult(v, s["x"], ALPHA, transpose=tr)
            err = relerr(y_pa, y_fa)
            print(f"{name} p={p} q1d={p + dq} {vname} transpose={tr}: PA vs FA {err:.2e}")
            assert np.abs(y_fa).max() > 1e-3 and err < TOL


@pytest.mark.parametrize("name,p,dq", CASES)
def test_constants_duality_and_linear_fields(name, p, dq):
    s = setup(name, p, p + dq)
    ref, x, w = s["ref"], s["x"], s["w"]
    one = np.ones(ref.ndofs)
    for vname, v in velocities(ref).items():
        y = ref.mult(v, x, ALPHA)
        scale = np.abs(y).max()
        # C 1 = 0: the gradient of a constant vanishes at every point
        assert np.abs(ref.mult(v, one, ALPHA)).max() < TOL * scale
        # <w, C x> = <C^T w, x>, against the sum of the magnitudes the first product adds up
        yt = ref.mult(v, w, ALPHA, transpose=True)
        assert abs(w @ y - yt @ x) < TOL * (np.abs(w) @ np.abs(y))
    # C (g . p) = alpha (v . g) M_1 1 for a constant v: the quadrature sums agree term by term
    # (adj(J) v . J^T g = det J (v . g)); M_1 1 from the oracle's unit mass
    op = O.OracleOperator(s["mesh"].element_nodes(), s["fes"].gather_map(), ref.ndofs, p, alpha=1.0, beta=None,
                          q1d=p + dq)
    m1 = op.mult(one)
    lhs = ref.mult(VCONST, s["X"] @ G, ALPHA)
    rhs = ALPHA * (VCONST @ G) * m1
    assert relerr(lhs, rhs) < TOL
    assert relerr(ref.unit_load(), m1) < TOL


def test_markers_zero_the_excluded_elements():
    s = setup("perturbed", 2, 4)
    ref = s["ref"]
    attr = 1 + (np.arange(ref.ne) % 3)
    keep = R.marker_keep(attr, [0, 1, 0])
    assert 0 < keep.sum() < ref.ne
    pa = ref.pa_data(VCONST, ALPHA, keep)
    assert np.all(pa[~keep] == 0.0) and np.all(np.abs(pa[keep]).max(axis=(1, 2)) > 0)
    y = ref.mult(VCONST, s["x"], ALPHA, keep)
    ye = ref.apply(ref.pa_data(VCONST, ALPHA), ref.gather(s["x"]))
    ye[~keep] = 0.0                                   # AddMultWithMarkers: the rows of excluded elements
    assert relerr(y, ref.scatter_add(ye)) < 1e-15
    assert R.marker_keep(attr, None).all()


@pytest.mark.parametrize("name,p,dq", [("perturbed", 1, 2), ("perturbed", 2, 2), ("fichera", 3, 1), ("perturbed", 4, 2)])
def test_float64_helper_against_longdouble(name, p, dq):
    """The float64 checker's own distance from the extended-precision restatement (80-bit on x86): the
    GPU tests' 1e-12 bar has to sit well above it.  Where longdouble is no wider than double the figure
    is 0 and says nothing; it is printed either way."""
    s = setup(name, p, p + dq)
    hi = setup(name, p, p + dq, np.longdouble)["ref"]
    worst = 0.0
    for vname, v in velocities(s["ref"]).items():
        for tr in (False, True):
            e = relerr(s["ref"].mult(v, s["x"], ALPHA, transpose=tr), hi.mult(v, s["x"], ALPHA, transpose=tr))
            worst = max(worst, e)
        worst = max(worst, relerr(s["ref"].pa_data(v, ALPHA), hi.pa_data(v, ALPHA)))
    print(f"{name} p={p} q1d={p + dq}: float64 checker vs longdouble {worst:.2e} "
          f"(longdouble eps {np.finfo(np.longdouble).eps:.1e}); the GPU bar is 1e-12")
    assert worst < 1e-14


# ---- the componentwise criterion: c_ref, the device bounds and what they see --------------------------
_ROWS = {}


def _checker_constants(case):
    """{"pa", "fa": {state: worst over velocity x marker x direction}, "qd": worst} of the float64
    checker against its extended-precision instance (cached)."""
    if case not in _ROWS:
        g = CC.geometry(*case)
        pa, fa, qd = {s: 0.0 for s in STATES}, {s: 0.0 for s in STATES}, 0.0
        for vname in ("const", "points"):
            v = g.velocity(vname)
            M = g.lo.element_matrices(v, CC.CALPHA)
            for marked in (False, True):
                keep = g.keep_of(marked)
                p_hp, Pabs = g.qdata_ref(vname, marked)
                qd = max(qd, HP.constant(g.lo.pa_data(v, CC.CALPHA, keep).ravel(), p_hp.ravel(), Pabs.ravel()))
                for tr in (False, True):
                    ref = g.mult_ref(vname, marked, tr)
                    for s in STATES:
                        y_hp, S = ref[s]
                        pa[s] = max(pa[s], HP.constant(g.lo.mult(v, g.x[s], CC.CALPHA, keep, tr), y_hp, S))
                        fa[s] = max(fa[s], HP.constant(g.lo.fa_mult(v, g.x[s], CC.CALPHA, keep, tr, M=M), y_hp, S))
        _ROWS[case] = {"pa": pa, "fa": fa, "qd": qd}
    return _ROWS[case]


def _worst(row):
    return max(max(row["pa"].values()), max(row["fa"].values())), row["qd"]


@pytest.mark.parametrize("case", CC.CASES, ids=[CC.case_id(c) for c in CC.CASES])
def test_checker_componentwise_constants(case):
    """The float64 checker's two independent paths (sum-factorised, dense element matrices), Mult and
    MultTranspose, both velocities, marked and unmarked, and its qdata sit within C_CONV / 4 (C_CONV_QD /
    4) of the extended-precision reference on every state (columns: random celsius kelvin linear)."""
    row = _checker_constants(case)
    print("%-28s PA %s | FA %s | qdata %.2f" % (CC.case_id(case), " ".join("%5.2f" % row["pa"][s] for s in STATES),
                                               " ".join("%5.2f" % row["fa"][s] for s in STATES), row["qd"]))
    c_mult, c_qd = _worst(row)
    assert 4.0 * c_mult <= HP.C_CONV
    assert 4.0 * c_qd <= HP.C_CONV_QD


def test_device_bounds_are_four_c_ref():
    """hp_ref.C_CONV and hp_ref.C_CONV_QD = 4 c_ref rounded up to a power of two, c_ref the checker's worst
    constant over the whole device case matrix (of its two Mult paths, both directions; of its qdata)."""
    worst = [_worst(_checker_constants(c)) for c in CC.CASES]
    for name, c_ref, have in (("C_CONV", max(w[0] for w in worst), HP.C_CONV),
                              ("C_CONV_QD", max(w[1] for w in worst), HP.C_CONV_QD)):
        want = 2.0 ** math.ceil(math.log2(4.0 * c_ref))
        print(f"{name}: c_ref = {c_ref:.2f}, 4 c_ref = {4 * c_ref:.1f} -> {want:g} (hp_ref.{name} = {have:g})")
        assert have == want


def test_one_point_qdata_error_passes_rtol_and_fails_the_componentwise_bound():
    """What each criterion can and cannot see.  The float64 checker on `perturbed`, p = 2, Q = 4, per-point
    velocity, with its qdata at one quadrature point of every element scaled by 1 + 1e-12.

    * The global relerr on x ~ U[0, 1), the bar of test_gpu_convection.py, stays below RTOL in both
      directions: that suite would stay green.
    * The qdata criterion sees it outright: 1e-12 / u = 9007 units of the entry itself.
    * MultTranspose sees it on every state (recorded: random 405, celsius 339, kelvin 339, linear 338
      units against 1.4 - 2.0 clean): B x at the point is of the size of |B| |x|, so the qdata error
      reaches y undamped.
    * The forward Mult sees it on the random state only (385 units against 2.4 clean).  On the temperature
      states it does NOT: celsius 5.0, kelvin 0.8, linear 0.2 units (0.2 clean), all inside C_CONV = 32,
      because there the qdata error is multiplied by a gradient that is small against the bound's
      |G| |x|.  So the forward product on the fields the solver applies it to cannot vouch for the qdata,
      which is why the qdata has a componentwise check of its own.  Those three figures are recorded
      (run with -s), and asserted only to stay finite and inside the bound they cannot break."""
    s = setup("perturbed", 2, 4)
    g = CC.geometry("corners", "perturbed", 2, 4)
    lo, v = g.lo, g.velocity("points")
    pa = lo.pa_data(v, CC.CALPHA)
    bad = pa.copy()
    q0 = 21
    bad[:, :, q0] *= 1.0 + 1e-12
    p_hp, Pabs = g.qdata_ref("points", False)
    c_qd = [HP.constant(a.ravel(), p_hp.ravel(), Pabs.ravel()) for a in (pa, bad)]
    print(f"qdata x (1 + 1e-12) at point {q0}: qdata constant {c_qd[0]:.2f} -> {c_qd[1]:.1f} (C_CONV_QD = {HP.C_CONV_QD:g})")
    assert c_qd[0] <= HP.C_CONV_QD / 4 and c_qd[1] > HP.C_CONV_QD
    for tr in (False, True):
        app = lo.apply_t if tr else lo.apply
        # today's bar: global relerr on the non-cancelling input
        x01 = s["x"]
        r = relerr(lo.scatter_add(app(bad, lo.gather(x01))), g.hi.mult(v, x01, CC.CALPHA, None, tr).astype(np.float64))
        assert r < RTOL
        ref = g.mult_ref("points", False, tr)
        good = {st: HP.constant(lo.scatter_add(app(pa, lo.gather(g.x[st]))), *ref[st]) for st in STATES}
        hurt = {st: HP.constant(lo.scatter_add(app(bad, lo.gather(g.x[st]))), *ref[st]) for st in STATES}
        print("transpose=%s: relerr on U[0,1) %.2e (RTOL %g); constants %s (C_CONV = %g)" % (
            tr, r, RTOL, "  ".join("%s %.2f -> %.1f" % (st, good[st], hurt[st]) for st in STATES), HP.C_CONV))
        assert max(good.values()) <= HP.C_CONV / 4
        if tr:
            assert min(hurt.values()) > HP.C_CONV
        else:
            assert hurt["random"] > HP.C_CONV
            assert max(hurt[st] for st in ("celsius", "kelvin", "linear")) <= HP.C_CONV   # blind there


# ---- the Jacobian-mode reference ---------------------------------------------------------------------
@pytest.mark.parametrize("p,q1d", [(2, 3), (2, 4), (4, 5), (4, 6)])
def test_from_jacobians_agrees_with_the_corner_path(p, q1d):
    """ConvRef.from_jacobians on Mesh.jacobians of the trilinear `perturbed` mesh against the corner path:
    qdata, Mult and MultTranspose to 1e-13 (J itself agrees to a few units of 2^-53), in both precisions'
    instances -- the [ne][3 (j)][3 (i)][nq] layout is read the right way round."""
    gc, gj = CC.geometry("corners", "perturbed", p, q1d), CC.geometry("jacobians", "perturbed", p, q1d)
    assert relerr(gj.lo.J, gc.lo.J) < 1e-14
    x = gc.x["random"]
    for a, b in ((gj.lo, gc.lo), (gj.hi, gc.hi)):
        for vname in ("const", "points"):
            v = gc.velocity(vname)
            assert relerr(a.pa_data(v, CC.CALPHA, gc.keep), b.pa_data(v, CC.CALPHA, gc.keep)) < TOL
            for tr in (False, True):
                assert relerr(a.mult(v, x, CC.CALPHA, gc.keep, tr), b.mult(v, x, CC.CALPHA, gc.keep, tr)) < TOL


@pytest.mark.parametrize("name,p,q1d", [c[1:] for c in CC.JACOBIAN_CASES if c[1] in CC.CURVED])
def test_curved_mesh_identities(name, p, q1d):
    """On the reference's curved fichera meshes (orders >= the map's, so that a linear function of the
    physical coordinates is in the space): C 1 = 0 within the componentwise bound, and for a constant v
    C (g . X) = alpha (v . g) M_1 1 against the oracle's unit mass on the same Jacobians."""
    g = CC.geometry("jacobians", name, p, q1d)
    one = np.ones(g.ndofs)
    for vname in ("const", "points"):
        v = g.velocity(vname)
        for ref in (g.lo, g.hi):
            c1 = HP.constant(ref.mult(v, one, CC.CALPHA), np.zeros(g.ndofs, HP.LD), g.hi.bound(v, one, CC.CALPHA))
            print(f"{name} p={p} q1d={q1d} {vname} {ref.dtype.__name__}: |C 1|_i / (u S_i) <= {c1:.2e}")
            assert c1 <= HP.C_CONV / 4
    op = O.OracleOperator.from_jacobians(g.J, g.gm, g.ndofs, p, alpha=1.0, q1d=q1d)
    lhs = g.lo.mult(VCONST, g.X @ G, ALPHA)
    rhs = ALPHA * (VCONST @ G) * op.mult(one)
    assert np.abs(rhs).max() > 1e-3 and relerr(lhs, rhs) < TOL
    assert relerr(g.lo.unit_load(), op.mult(one)) < TOL
