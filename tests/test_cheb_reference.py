"""CPU pin of the Chebyshev tests' numpy checker (tests/cheb_ref.py on tests/cheb_cases.py), without the device:
the coefficients against the Chebyshev polynomial they come from, the smoother's symmetry (the reference's own
test), the power method against the dense spectrum, the preconditioned CG against a dense solve, and the
checker's self-gap under three summation orders -- the condition under which tests/test_gpu_chebyshev.py
applies the project's 1e-12 bar to x after a fixed number of iterations."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as C

import helpers  # noqa: F401
import cheb_cases as CC
import cheb_ref as CR


@pytest.mark.parametrize("lam", [0.02, 1.3, 57.0])
@pytest.mark.parametrize("order", CC.ORDERS)
def test_coefficients_are_the_chebyshev_residual_polynomial(lam, order):
    """1 - x p(x) = T_k((theta - x) / delta) / T_k(theta / delta), p(x) = sum_j c_j x^j, at 41 points of
    [0, 1.5 lam].  Measured <= 7.3e-14 (the largest at order 5)."""
    c = CR.coefficients(order, lam)
    assert c.shape == (order,)
    theta, delta = CR.theta_delta(lam)
    x = np.linspace(0.0, 1.5 * lam, 41)
    Tk = [0.0] * order + [1.0]
    lhs = 1.0 - x * np.polynomial.polynomial.polyval(x, c)
    rhs = C.chebval((theta - x) / delta, Tk) / C.chebval(theta / delta, Tk)
    err = float(np.abs(lhs - rhs).max())
    print(f"lam {lam} order {order}: {err:.2e}")
    assert err <= 2e-13


def test_orders_outside_1_to_5_are_refused():
    for order in (0, 6, -1):
        with pytest.raises(ValueError):
            CR.coefficients(order, 1.0)


@pytest.mark.parametrize("name", CC.SYM)
def test_smoother_is_symmetric(name):
    """tests/unit/linalg/test_chebyshev.cpp: |l^T S r - r^T S l| / |l^T S r| < 1e-13, cheb order 2 with the
    power method's estimate.  Measured <= 2e-16."""
    c = CC.case(name)
    S = c.smoother(2)
    rng = np.random.default_rng(3)
    left, right = rng.uniform(0, 1, c.n), rng.uniform(0, 1, c.n)
    fwd, tr = float(left @ S(right)), float(right @ S(left))
    err = abs(fwd - tr) / abs(fwd)
    print(f"{name}: {err:.2e}")
    assert err < 1e-13


def test_power_method_finds_the_dense_spectrum():
    c = CC.case("k1")
    M = c.dinv[:, None] * c.dense()
    want = float(np.abs(np.linalg.eigvals(M)).max())
    pr = CR.power_method(c.mult, c.dinv, c.ess, c.v0, 500, 1e-10)
    print(f"k1: power {pr.eig:.10f} in {pr.steps} steps, dense {want:.10f}")
    assert abs(pr.eig - want) <= 1e-6 * want


def test_default_power_method_runs_all_ten_steps_on_k2():
    """No step's diff is below 1e-2 (measured >= 1.8e-2), far from the default tolerance 1e-8."""
    pr = CC.case("k2").power()
    print(pr.diffs)
    assert pr.steps == 10 and min(pr.diffs) >= 1e-2


def test_pcg_against_a_dense_solve():
    c = CC.case("k1")
    A = c.dense()
    want = np.linalg.solve(A, c.b)
    res = c.solve(2, rel_tol=1e-12, max_iter=1000)
    cond = float(np.linalg.cond(A))
    err = helpers.relerr(res.x, want)
    print(f"k1: {res.final_iter} iterations, stop {res.stop}, residual {c.true_residual(res.x):.2e}, error {err:.2e}, "
          f"cond {cond:.1f}")
    assert res.converged and res.stop == "converged"
    assert c.true_residual(res.x) <= 1e-10
    assert err <= cond * 1e-10


@pytest.mark.parametrize("name", CC.ALL)
def test_self_gap_under_three_dot_orders(name):
    """Equal iteration counts to 1e-12, and after 6 iterations x within 1e-14 of max|x|.  Measured <= 6.1e-15
    (sym4 at order 2; <= 2.2e-15 on the solver's cases)."""
    c = CC.case(name)
    for order in CC.ORDERS:
        full = [c.solve(order, dot=d, rel_tol=1e-12, max_iter=1000) for d in CR.DOTS]
        assert all(r.converged for r in full)
        assert len({r.final_iter for r in full}) == 1, [r.final_iter for r in full]
        six = [c.solve(order, dot=d, rel_tol=1e-12, max_iter=6) for d in CR.DOTS]
        # (k1 at order 5 converges within the six; every other solve stops at max_iter)
        assert len({(r.final_iter, r.stop) for r in six}) == 1 and six[0].final_iter <= 6
        assert six[0].stop == "max_iter" or (name, order) == ("k1", 5)
        gap = max(helpers.relerr(r.x, six[0].x) for r in six[1:])
        print(f"{name} order {order}: {full[0].final_iter} iterations, gap {gap:.2e}")
        assert gap <= 1e-14


@pytest.mark.parametrize("name", CC.ALL)
def test_order_1_and_2_against_jacobi(name):
    """Order 1 is Jacobi scaled by 1 / theta: the same iterations.  Order 2 needs <= 0.65 of Jacobi's
    (measured 0.55 to 0.59)."""
    jac = CC.reference(name, 0, 1000)
    one = CC.reference(name, 1, 1000)
    two = CC.reference(name, 2, 1000)
    print(f"{name}: Jacobi {jac.final_iter}, order 1 {one.final_iter}, order 2 {two.final_iter}")
    assert jac.converged and one.converged and two.converged
    assert one.final_iter == jac.final_iter
    assert two.final_iter <= 0.65 * jac.final_iter


@pytest.mark.parametrize("order", [2, 4])
def test_too_small_estimate_makes_the_preconditioner_negative(order):
    """max_eig = the power method's / 8: (B b, b) < 0 on k2, the solve stops before the loop.  Measured
    nom0 = -4662 against sum |b_i (B b)_i| = 6039 at order 2 (-231752 against 321502 at order 4): the sign is
    not marginal."""
    c = CC.case("k2")
    small = c.max_eig / 8.0
    res = c.solve(order, max_eig=small, rel_tol=1e-12)
    Bb = c.smoother(order, small)(c.b)
    mass = float(np.abs(c.b * Bb).sum())
    print(f"order {order}: nom0 {res.final_norm:.1f} against {mass:.1f}")
    assert res.stop == "neg0" and res.final_iter == 0 and not res.converged
    assert res.final_norm < 0 and res.final_norm == float(c.b @ Bb)
    assert abs(res.final_norm) > 0.05 * mass
