"""CPU tests of the extended-precision reference (tests/hp_ref.py) and of the componentwise criterion.

1. The reference against closed forms, independent of the oracle: the unit cube's p = 1 stiffness and
   mass matrices against their exact rational entries, and on non-aligned and trilinear meshes the
   identities sum_i (K x)_i = 0, K 1 = 0, 1^T M 1 = sum W alpha det J and x^T K x = |g|^2 beta vol.
2. The oracle pinned componentwise: constant() of OracleOperator.mult (PA), .fa_mult (element
   matrices) and .diagonal over the case matrix (tests/cw_cases.py); the maximum is c_ref, and the
   device bound hp_ref.C must be 4 c_ref rounded up to a power of two.  Run with -s for the table.
3. The criterion's power: a 1e-12 relative error of the qdata at one quadrature point passes the
   global relerr <= RTOL and fails the componentwise bound."""
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle as O
import hp_ref as HP
import cw_cases as CW
from helpers import RTOL, nonaligned, relerr

LD = np.longdouble


# ---- 1. closed forms ------------------------------------------------------------------------------
def _unit_cube(p=1):
    en, gm, nd, X = O.cartesian_mesh(1, 1, 1, order=p)
    return en, gm, nd, X


def _gauss_legendre_ld(n):
    """The n-point Gauss-Legendre rule on [0, 1] in longdouble: Newton on P_n from the float64 points."""
    x0, _ = O.gauss_legendre(n)
    t = 2 * x0.astype(LD) - 1
    for _ in range(4):
        p0, p1 = np.ones_like(t), t.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * t * p1 - (k - 1) * p0) / k
        dp = n * (t * p1 - p0) / (t * t - 1)
        t = t - p1 / dp
    p0, p1 = np.ones_like(t), t.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((2 * k - 1) * t * p1 - (k - 1) * p0) / k
    dp = n * (t * p1 - p0) / (t * t - 1)
    return (t + 1) / 2, 1 / ((1 - t * t) * dp * dp)


@pytest.mark.parametrize("q1d", [3, 4])
def test_unit_cube_p1_matrices_are_the_exact_rationals(q1d):
    """K = K1 x M1 x M1 + M1 x K1 x M1 + M1 x M1 x K1 and M = M1 x M1 x M1 with the 1D linear element's
    M1 = [[1/3, 1/6], [1/6, 1/3]], K1 = [[1, -1], [-1, 1]] (dof a = ax + 2 ay + 4 az), to 1e-17.

    The analytic entries are those of the exact rule, so the rule is refined to longdouble here (the
    p = 1 nodes 0, 1 are exact).  With the float64 points and weights every other test uses -- inputs
    the oracle, the device and the reference share and take as exact -- the entries sit 2.1e-17 (q1d 3)
    and 2.1e-16 (q1d 4: those four weights sum to 1 - 2.2e-16) from the rationals: the tables' own
    rounding, not the reference's arithmetic.  That distance is printed and held to what the tables'
    distance from the exact rule allows: an entry is a sum of three products of 1D sums
    sum_q w_q f(x_q) with |f| <= 1, |f'| <= 2, so 3 (sum |dw| + 2 max |dx|)."""
    en, gm, nd, _ = _unit_cube()
    M1 = [[Fraction(1, 3), Fraction(1, 6)], [Fraction(1, 6), Fraction(1, 3)]]
    K1 = [[Fraction(1), Fraction(-1)], [Fraction(-1), Fraction(1)]]
    bits = [(a & 1, (a >> 1) & 1, a >> 2) for a in range(8)]
    Kx = np.empty((8, 8), LD)
    Mx = np.empty((8, 8), LD)
    for a, (ax, ay, az) in enumerate(bits):
        for b, (bx, by, bz) in enumerate(bits):
            k = (K1[ax][bx] * M1[ay][by] * M1[az][bz] + M1[ax][bx] * K1[ay][by] * M1[az][bz]
                 + M1[ax][bx] * M1[ay][by] * K1[az][bz])
            m = M1[ax][bx] * M1[ay][by] * M1[az][bz]
            Kx[a, b] = LD(k.numerator) / LD(k.denominator)
            Mx[a, b] = LD(m.numerator) / LD(m.denominator)
    assert np.array_equal(gm[0], np.arange(8))    # global dof = lexicographic corner
    rule = _gauss_legendre_ld(q1d)
    assert np.abs(rule[0] - O.gauss_legendre(q1d)[0]).max() < 2e-16 and abs(float(rule[1].sum() - 1)) < 1e-18
    x64, w64 = O.gauss_legendre(q1d)
    tol64 = 1e-17 + 3.0 * float(np.abs(w64 - rule[1]).sum() + 2 * np.abs(x64 - rule[0]).max())
    for tag, rl, tol in (("exact rule", rule, 1e-17), ("float64 tables", None, tol64)):
        hk = HP.HPRef(en, gm, nd, 1, q1d, beta=1.0, rule=rl)
        hm = HP.HPRef(en, gm, nd, 1, q1d, alpha=1.0, rule=rl)
        Kh = np.stack([hk.mult(np.eye(8)[:, j]) for j in range(8)], 1)
        Mh = np.stack([hm.mult(np.eye(8)[:, j]) for j in range(8)], 1)
        ek, em = float(np.abs(Kh - Kx).max()), float(np.abs(Mh - Mx).max())
        dk = float(np.abs(hk.diagonal() - np.diag(Kx)).max())
        dm = float(np.abs(hm.diagonal() - np.diag(Mx)).max())
        print(f"unit cube p=1 q1d={q1d}, {tag}: |K - exact| = {ek:.2e}, |M - exact| = {em:.2e}, "
              f"diagonals {dk:.2e} {dm:.2e}")
        assert max(ek, em, dk, dm) <= tol


def _identity_meshes():
    out = []
    for p in (1, 2, 3, 4):
        out.append(("nonaligned-p%d" % p, O.cartesian_mesh(5, 4, 3, order=p, transform=nonaligned), p))

    def bump(V):                                   # every hex genuinely trilinear
        return V + 0.04 * np.sin(5.0 * V[:, [1, 2, 0]] + 1.0)
    for p in (1, 2, 3):
        out.append(("trilinear-p%d" % p, O.cartesian_mesh(4, 3, 3, order=p, transform=bump), p))
    return out


@pytest.mark.parametrize("name,mesh,p", _identity_meshes(), ids=[m[0] for m in _identity_meshes()])
def test_reference_identities(name, mesh, p):
    en, gm, nd, X = mesh
    q1d = O.default_q1d(p)
    P = O.quad_points(en, q1d)
    beta = 0.5 * (1.0 + 0.3 * np.sin(4.0 * P[..., 1]))
    alpha = 2.0 + np.cos(3.0 * P[..., 0])
    hk = HP.HPRef(en, gm, nd, p, q1d, beta=beta)
    hm = HP.HPRef(en, gm, nd, p, q1d, alpha=alpha)
    x = np.random.default_rng(3).uniform(-1, 1, nd)
    # sum_i (K x)_i = 1^T K x = 0, relative to the same sum of magnitudes
    y, S = hk.mult(x), hk.bound(x)
    r_sum = float(abs(y.sum()) / S.sum())
    # K 1 = 0 entrywise
    one = np.ones(nd)
    y1, S1 = hk.mult(one), hk.bound(one)
    r_one = float((np.abs(y1) / (LD(HP.U) * S1)).max())
    # 1^T M 1 = sum_q W alpha det J
    tot = hm.M.sum()
    r_mass = float(abs(hm.mult(one).sum() - tot) / tot)
    print(f"{name}: |sum Kx|/sum S = {r_sum:.2e}   max |K 1|_i/(u S_i) = {r_one:.2e}   1^T M 1: {r_mass:.2e}")
    assert r_sum <= 1e-17
    assert r_one <= 1e-3
    assert r_mass <= 1e-17


@pytest.mark.parametrize("p", [1, 2])
def test_reference_linear_field_energy(p):
    """x^T K x = |g|^2 beta vol for x = g . X, constant beta, on an affine mesh: the 4^3 cube sheared by
    y += x / 4, z += 3 x / 8 -- every vertex, every p <= 2 node (GLL nodes 0, 1/2, 1) and g are dyadic,
    so x is the linear field exactly and the elements are exact parallelepipeds; vol = sum W det J."""
    def shear(V):
        V = V.copy()
        V[:, 1] += 0.25 * V[:, 0]
        V[:, 2] += 0.375 * V[:, 0]
        return V
    en, gm, nd, X = O.cartesian_mesh(4, 4, 4, order=p, transform=shear)
    g = np.array([0.25, -1.125, 0.75])
    x = X @ g
    assert np.array_equal(x.astype(LD), X.astype(LD) @ g.astype(LD))      # exact in float64
    beta = 0.5
    h = HP.HPRef(en, gm, nd, p, O.default_q1d(p), beta=beta)
    vol = (h.W * h.detJ).sum()
    energy = (x.astype(LD) * h.mult(x)).sum()
    want = LD(float(g @ g)) * LD(beta) * vol
    r = float(abs(energy - want) / want)
    print(f"p={p}: x^T K x = {float(energy):.17g}, |g|^2 beta vol = {float(want):.17g}, rel {r:.2e}, "
          f"vol - 1 = {float(vol - 1):.2e}")
    assert r <= 1e-17
    assert abs(float(vol - 1)) < 1e-15            # (the float64 weights sum to 1 within their rounding)


# ---- 2. the oracle pinned componentwise -------------------------------------------------------------
_ROWS = {}


def _oracle_constants(sp, forms):
    """name -> {form: {"pa": max over states, "fa": ..., "diag": ...}} (cached)."""
    key = (sp.name, sp.p, sp.numbering)
    if key in _ROWS:
        return _ROWS[key]
    rows = {}
    for fname in forms:
        f, op = sp.form(fname), sp.oracle(fname)
        pa = {s: HP.constant(op.mult(sp.x[s]), f["y_hp"][s], f["S"][s]) for s in CW.STATES}
        fa = {s: HP.constant(op.fa_mult(sp.x[s]), f["y_hp"][s], f["S"][s]) for s in CW.STATES}
        dg = HP.constant(op.diagonal(), f["d_hp"], f["dS"])
        rows[fname] = {"pa": pa, "fa": fa, "diag": dg}
    _ROWS[key] = rows
    return rows


def _print_rows(sp, rows):
    for fname, r in rows.items():
        print("%-10s p=%d %-7s PA %s | FA %s | diag %.2f" % (
            sp.name, sp.p, fname, " ".join("%5.2f" % r["pa"][s] for s in CW.STATES),
            " ".join("%5.2f" % r["fa"][s] for s in CW.STATES), r["diag"]))


def _worst(rows):
    """(Mult: PA and element-matrix, every state; diagonal)."""
    return (max(max(max(r["pa"].values()), max(r["fa"].values())) for r in rows.values()),
            max(r["diag"] for r in rows.values()))


_REF_SPACES = None


def _ref_spaces():
    global _REF_SPACES
    if _REF_SPACES is None:
        _REF_SPACES = CW.reference_spaces()
    return _REF_SPACES


def _ref_ids():
    seen = {}
    for c in CW.CASES:
        seen.setdefault((c.mesh, c.p, c.numbering), None)
    ids = ["%s-p%d-%s" % (m, p, "structured" if n == CW.STRUCTURED else "entity") for m, p, n in seen]
    return ids + ["oracle-na444-p%d" % p for p in (1, 2, 4)] + ["oracle-cart888-p2"]


@pytest.mark.parametrize("i", range(len(_ref_ids())), ids=_ref_ids())
def test_oracle_componentwise_constants(i):
    """The CPU oracle's PA Mult, element-matrix Mult and diagonal sit within C / 4 (C_DIAG / 4) of the
    extended-precision answer on every state (columns: random celsius kelvin linear)."""
    sp, forms = _ref_spaces()[i]
    rows = _oracle_constants(sp, forms)
    _print_rows(sp, rows)
    c_mult, c_diag = _worst(rows)
    assert 4.0 * c_mult <= HP.C
    assert 4.0 * c_diag <= HP.C_DIAG


def test_device_bounds_are_four_c_ref():
    """hp_ref.C and hp_ref.C_DIAG = 4 c_ref rounded up to a power of two, c_ref the worst constant of the
    whole matrix (of the two Mult evaluations; of the diagonal)."""
    worst = [_worst(_oracle_constants(sp, forms)) for sp, forms in _ref_spaces()]
    for name, c_ref, have in (("C", max(w[0] for w in worst), HP.C), ("C_DIAG", max(w[1] for w in worst), HP.C_DIAG)):
        want = 2.0 ** math.ceil(math.log2(4.0 * c_ref))
        print(f"{name}: c_ref = {c_ref:.2f}, 4 c_ref = {4 * c_ref:.1f} -> {want:g} (hp_ref.{name} = {have:g})")
        assert have == want


# ---- 3. what the criterion sees that relerr <= RTOL does not ----------------------------------------
@pytest.mark.parametrize("which", ["M", "D"])
def test_one_point_qdata_error_passes_rtol_and_fails_the_componentwise_bound(which):
    """The oracle with its qdata at one quadrature point (of every element) scaled by 1 + 1e-12, on the
    5 x 4 x 3 non-aligned mesh, p = 2, random x: the global relerr stays below RTOL = 1e-12 -- the
    existing suite is green -- while the componentwise constant is far above C."""
    sp = CW.space("na543", 2)
    fname = "M" if which == "M" else "K"
    f, op = sp.form(fname), sp.oracle(fname)
    x = sp.x["random"]
    good = op.mult(x)
    q0 = 21
    if which == "M":
        op.M[:, q0] *= 1.0 + 1e-12
    else:
        op.D[:, :, q0] *= 1.0 + 1e-12
    bad = op.mult(x)
    c_good = HP.constant(good, f["y_hp"]["random"], f["S"]["random"])
    c_bad = HP.constant(bad, f["y_hp"]["random"], f["S"]["random"])
    r = relerr(bad, np.asarray(f["y_hp"]["random"], np.float64))
    print(f"{which} x (1 + 1e-12) at point {q0}: relerr {r:.2e} (RTOL {RTOL:g}); constant {c_good:.2f} -> {c_bad:.1f} "
          f"(C = {HP.C:g})")
    assert r <= RTOL
    assert c_good <= HP.C / 4
    assert c_bad > HP.C
