"""Pins of the cell-death tests' 80-bit reference (tests/celldeath_ref.py) without the product, and the bounds the
other cell-death tests import.

The reference against mpmath.expm of the 3 x 3 generator at 50 digits (near a double eigenvalue too), against the
b = 0 closed form N = exp(-a t), the semigroup property (a step of dt = two of dt / 2 = nsub substeps at a frozen
field), and the hazards of the formulation (overflow at 95 C and dt = 300 s; degenerate rates; monotone death).

Bounds (4 c_ref rounded up to a power of two, c_ref the float64 numpy restatement's own worst figure
over tests/celldeath_cases.py's measured_cases -- the grid and the near-double-eigenvalue cases -- against the
80-bit run, never a device figure; the factor 4 covers the device's exp / expm1 and FMA contraction), per entry
with the entry's own x_max = max_i dE_i / (R T_K), one constant per model:
  three-state  |X - X_hp| <= C_CD u (1 + x_max); measured c_ref = 3.021 (a = c, b / a = 1e-14, four substeps;
               the grid alone 0.629) -> C_CD = 16
  Arrhenius    the same with Omega relative to max(1, Omega); measured 2.242 -> C_CD_ARRHENIUS = 16
  sum          |N + U + D - 1| grows by at most C_SUM u per substep; measured 5 u -> C_SUM = 32
test_bounds_follow_the_rule re-measures all three and fails if the constants no longer follow from the figures."""
import math

import numpy as np
import pytest

import celldeath_cases as CC
import celldeath_ref as CR

C_CD = 16.0
C_CD_ARRHENIUS = 16.0
C_SUM = 32.0


def c_cd(model):
    return C_CD_ARRHENIUS if model == CR.ARRHENIUS else C_CD
LD = np.longdouble
U80 = float(np.finfo(LD).eps) / 2


def _pow2_above(x):
    return 2.0 ** math.ceil(math.log2(x))


def _run(c, dtype):
    return CR.step(c["model"], c["A"], c["dE"], c["t_offset"], c["T0"], c["T1"], c["dt"], c["nsub"], c["N"], c["U"],
                   c["D"], dtype=dtype)


def test_bounds_follow_the_rule():
    assert U80 < 1e-19, "numpy.longdouble is not the 80-bit format here"
    c_ref, c_sum, worst = {CR.THREE_STATE: 0.0, CR.ARRHENIUS: 0.0}, 0.0, {}
    for c in CC.measured_cases():
        hp, lo = _run(c, LD), _run(c, np.float64)
        assert not hp[3].any() and not lo[3].any()
        tol1 = CC.tolerance(c, 1.0)
        for X, h, l in zip("NUD", hp, lo):
            assert np.isfinite(l).all(), (c["name"], X)
            scale = np.maximum(1.0, np.abs(h)) if (c["model"] == CR.ARRHENIUS and X == "U") else 1.0
            e = float((np.abs(l.astype(LD) - h) / scale / tol1).max())
            key = c["name"].split()[0]
            worst[key] = max(worst.get(key, 0.0), e)
            c_ref[c["model"]] = max(c_ref[c["model"]], e)
        if c["model"] == CR.THREE_STATE:
            s0, s1 = c["N"] + c["U"] + c["D"], lo[0] + lo[1] + lo[2]
            grow = np.abs(s1 - 1.0) - np.abs(s0 - 1.0)
            c_sum = max(c_sum, float(grow.max()) / CR.U_ROUND / c["nsub"])
            # the exact conditions hold for the restatement too
            assert (lo[2] >= c["D"]).all() and (lo[0] >= 0).all() and (lo[1] >= 0).all(), c["name"]
    for k, v in sorted(worst.items()):
        print(f"c_ref[{k}] = {v:.3f}")
    print(f"c_ref = {c_ref}, sum growth = {c_sum:.1f} u per substep")
    assert _pow2_above(4.0 * c_ref[CR.THREE_STATE]) == C_CD, c_ref
    assert _pow2_above(4.0 * c_ref[CR.ARRHENIUS]) == C_CD_ARRHENIUS, c_ref
    assert _pow2_above(4.0 * c_sum) == C_SUM, c_sum


def test_reference_near_double_eigenvalue_against_mpmath():
    """The reference itself near a double eigenvalue, where a divided difference over 2 delta would lose
    u80 / (2 delta dt): a = 1, b = 0, c = 1 + eps and a = c, b = 1e-14, state (1, 0, 0), dt = 1."""
    mp = pytest.importorskip("mpmath")
    for A in [(1.0, 0.0, 1.0 + e) for e in (1e-3, 1e-6, 1e-9, 1e-12, -1e-9)] + [(1.0, 1e-14, 1.0), (1.0, 0.0, 1.0)]:
        got = CR.step(CR.THREE_STATE, A, (0.0, 0.0, 0.0), 0.0, [300.0], None, 1.0, 1, [1.0], [0.0], [0.0])
        want = CR.closed_form_mp(A, (0.0, 0.0, 0.0), 300.0, 1.0, (1.0, 0.0, 0.0))
        with mp.workdps(50):
            for g, w in zip(got[:3], want):
                err = abs(mp.mpf(float(g[0])) + mp.mpf(float(g[0] - LD(float(g[0])))) - w)
                assert float(err) <= C_CD * CR.U_ROUND / 256.0, (A, float(err))


MP_CASES = [("mild", T, t, s) for T in (37.0, 60.0, 80.0, 95.0) for t in (1e-3, 1.0, 300.0)
            for s in ((1.0, 0.0, 0.0), (0.25, 0.5, 0.25))] + \
           [("tissue", T, t, (1.0, 0.0, 0.0)) for T, t in ((37.0, 300.0), (50.0, 30.0), (60.0, 1.0), (70.0, 1e-3))]


def test_reference_against_mpmath_expm():
    mp = pytest.importorskip("mpmath")
    worst = 0.0
    for name, T, t, s in MP_CASES:
        A, dE = CC.PARAMS[name]
        TK = T + 273.15     # (a kelvin field, t_offset = 0: both sides see the same float64 T_K)
        got = CR.step(CR.THREE_STATE, A, dE, 0.0, [TK], None, t, 1, [s[0]], [s[1]], [s[2]])
        want = CR.closed_form_mp(A, dE, TK, t, s)
        x = CR.x_max(dE, TK)
        with mp.workdps(50):     # (the difference too: at the default precision it would round to 53 bits)
            for g, w in zip(got[:3], want):
                err = abs(mp.mpf(float(g[0])) + mp.mpf(float(g[0] - LD(float(g[0])))) - w)
                worst = max(worst, float(err) / (U80 * (1.0 + x)))
    print(f"80-bit reference against mpmath.expm: worst {worst:.2f} u80 (1 + x_max)")
    # the reference judges float64 results against C_CD u (1 + x_max): its own error must be negligible there,
    # at most 2^-8 of that bound (80-bit rounding is 2^-11 of u)
    assert worst * U80 <= C_CD * CR.U_ROUND / 256.0, worst


def test_reference_against_b0_closed_form():
    """b = 0, state (1, 0, 0): N = exp(-a t), and with c = 0 too U = 1 - N."""
    mp = pytest.importorskip("mpmath")
    A, dE = CC.PARAMS["mild"]
    for T in (37.0, 70.0, 95.0, 120.0):
        for t in (1e-3, 1.0, 300.0):
            for A3 in (A[2], 0.0):
                got = CR.step(CR.THREE_STATE, (A[0], 0.0, A3), dE, 0.0, [T + 273.15], None, t, 1, [1.0], [0.0], [0.0])
                with mp.workdps(50):
                    a = mp.mpf(A[0]) * mp.exp(-mp.mpf(dE[0]) / (mp.mpf(CR.R_GAS) * mp.mpf(T + 273.15)))
                    Nw = mp.exp(-a * t)
                    bound = C_CD * CR.U_ROUND / 256.0 * (1.0 + CR.x_max(dE, T + 273.15))
                    assert abs(mp.mpf(float(got[0][0])) + mp.mpf(float(got[0][0] - LD(float(got[0][0])))) - Nw) <= bound
                    if A3 == 0.0:
                        assert float(got[2][0]) == 0.0
                        assert abs(float(got[1][0]) - float(1 - Nw)) <= C_CD * CR.U_ROUND * (1.0 + CR.x_max(dE, T + 273.15))


def test_reference_semigroup():
    """A step of dt equals two steps of dt / 2 and one step in two substeps (frozen field)."""
    n = 54
    for name in ("mild", "tissue"):
        A, dE = CC.PARAMS[name]
        T0, _ = CC.temperatures(n, 3, False)
        N, U, D = CC.states(n, 4)
        for dt in (1e-3, 1.0, 300.0):
            one = CR.step(CR.THREE_STATE, A, dE, 273.15, T0, None, dt, 1, N, U, D)
            half = CR.step(CR.THREE_STATE, A, dE, 273.15, T0, None, dt / 2, 1, N, U, D)
            # (the second half step from the 80-bit state: propagate takes the arrays as they are)
            k = CR.rates(A, dE, T0.astype(LD) + LD(273.15), LD)
            two = CR.propagate(k[0], k[1], k[2], LD(dt / 2), half[0], half[1], half[2])
            sub = CR.step(CR.THREE_STATE, A, dE, 273.15, T0, None, dt, 2, N, U, D)
            tol = C_CD * CR.U_ROUND / 256.0 * (1.0 + CR.x_max(dE, 310.15)) * 2
            for a, b, c in zip(one[:3], two, sub[:3]):
                assert float(np.abs(a - b).max()) <= tol, (name, dt)
                assert float(np.abs(a - c).max()) <= tol, (name, dt)


def test_reference_hazards():
    A, dE = CC.PARAMS["tissue"]
    n = 54
    N, U, D = CC.states(n, 9)
    # overflow: 95 C, dt = 300 s (sinh(delta dt) overflows; this form does not)
    out = CR.step(CR.THREE_STATE, A, dE, 273.15, np.full(n, 95.0), None, 300.0, 1, N, U, D)
    assert all(np.isfinite(v.astype(np.float64)).all() for v in out[:3]) and (out[2] > 0.999999).all()
    # degenerate rates: all zero (A = 0, and T_K = 1 K) -> bitwise unchanged; each A_i = 0 in turn is finite
    for args in ((CC.zeroed(A, (0, 1, 2)), dE, 273.15, np.full(n, 60.0)), (A, dE, 0.0, np.full(n, 1.0))):
        out = CR.step(CR.THREE_STATE, args[0], args[1], args[2], args[3], None, 300.0, 1, N, U, D)
        for got, old in zip(out[:3], (N, U, D)):
            assert (got == old.astype(LD)).all()
    for which in ((0,), (1,), (2,), (0, 2), (0, 1), (1, 2)):
        out = CR.step(CR.THREE_STATE, CC.zeroed(A, which), dE, 273.15, np.linspace(37, 120, n), None, 30.0, 1, N, U, D)
        assert all(np.isfinite(v.astype(np.float64)).all() for v in out[:3]), which
        if 2 in which:
            assert (out[2] == D.astype(LD)).all()       # k3 = 0: nothing dies
    # monotone death and non-negative fractions over the whole grid, in both precisions
    for c in CC.grid_cases():
        for dtype in (LD, np.float64):
            out = _run(c, dtype)
            assert (out[2] >= c["D"].astype(dtype)).all() and (out[0] >= 0).all() and (out[1] >= 0).all(), c["name"]
    # invalid entries are reported and untouched
    T = np.linspace(37, 120, n)
    T[5], T[6] = np.nan, -300.0
    out = CR.step(CR.THREE_STATE, A, dE, 273.15, T, None, 1.0, 1, N, U, D)
    assert list(np.flatnonzero(out[3])) == [5, 6] and out[0][5] == N[5] and out[2][6] == D[6]
