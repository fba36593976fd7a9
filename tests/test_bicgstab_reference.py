"""CPU pins of the numpy restatement of BiCGSTABSolver::Mult (tests/bicgstab_ref.py), the checker of the
device BiCGSTAB: against numpy.linalg.solve on the dense matrix of a small advection-diffusion operator;
every stop on small dense matrices built for it (rho_1 == 0 and omega == 0 included); its self-gap under
three dot summation orders on the cases the GPU tests use; and the closed-form distance of the discrete
steady state of examples/implicit_convect_heat.cpp.

Self-gap (the condition under which the project's RTOL = 1e-12 bar may be applied to x): with the
convection scale 20 the three orders give the same iteration counts and x within 1e-14 of max|x| --
measured <= 1.5e-15 on the four cases (19 / 17 / 27 / 28 iterations, convective share 0.57-0.62, true
residual 4.8e-13-8.9e-13); with a scale of 60 the gap rises to 1e-12 and the counts split (52 / 53 / 54), which is
why the parity cases use 20.
"""
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import oracle as O
import conv_ref as CR
import bicgstab_ref as BR
import bicgstab_cases as BC
from helpers import relerr


def _dense(A, n):
    return np.stack([A(np.eye(n)[:, j]) for j in range(n)], axis=1)


def test_against_dense_solve():
    """A 3 x 2 x 2, p = 2 advection-diffusion operator (175 dofs), constrained: x against numpy.linalg.solve.
    Bound: a converged solve's recursive residual is < 1e-12 ||b||; the true residual is allowed 100 x that
    for the recursion's drift, and the error of x is at most cond(A) x the true residual."""
    enodes, gm, n, X = O.cartesian_mesh(3, 2, 2, order=2, transform=BC.move)
    P = O.quad_points(enodes, O.default_q1d(2))
    sym = O.OracleOperator(enodes, gm, n, 2, alpha=BC.alpha_fn(P), beta=BC.CDT * BC.beta_fn(P))
    conv = CR.ConvRef(2, O.default_q1d(2), gm, n, enodes)
    v = CR.reference_velocity(conv.P)
    pa = conv.pa_data(v, BC.CDT * BC.CONV_SCALE)
    mult = lambda x: sym.mult(x) + conv.mult(v, x, pa=pa)
    onb = np.isclose(X[:, 0], X[:, 0].min()) | np.isclose(X[:, 0], X[:, 0].max())
    ess = np.nonzero(onb)[0]
    A = _dense(BR.constrained(mult, ess), n)
    assert np.abs(A - A.T).max() > 1e-3 * np.abs(A).max()   # nonsymmetric
    b = np.random.default_rng(5).uniform(0, 1, n)
    xs = np.linalg.solve(A, b)
    for dinv in (None, BR.jacobi_vector(sym.diagonal(), ess)):
        res = BR.bicgstab(mult, b, ess, dinv, rel_tol=1e-12, max_iter=500)
        assert res.converged and res.stop in ("r", "s") and res.final_norm < res.tol_goal
        assert res.tol_goal == math.sqrt(float(b @ b)) * 1e-12   # a norm, not its square
        true_res = np.linalg.norm(b - A @ res.x) / np.linalg.norm(b)
        print(f"dense: iters {res.final_iter} true residual {true_res:.2e} err {relerr(res.x, xs):.2e}")
        assert true_res <= 1e-10
        assert relerr(res.x, xs) <= np.linalg.cond(A) * 1e-10


# ---- every stop, on matrices built for it ----
def test_stop_r0():
    res = BR.bicgstab(lambda x: 2.0 * x, np.zeros(4))
    assert (res.final_iter, res.converged, res.stop, res.final_norm) == (0, True, "r0", 0.0)
    assert not res.x.any()
    # abs_tol above ||b||: converged at once
    res = BR.bicgstab(lambda x: 2.0 * x, np.ones(4), abs_tol=3.0)
    assert (res.final_iter, res.converged, res.stop) == (0, True, "r0") and not res.x.any()


def test_stop_s():
    """A = I: alpha = 1, s = 0 in iteration 1; x = alpha phat = b bitwise."""
    b = np.array([0.3, -1.7, 2.9])
    res = BR.bicgstab(lambda x: x.copy(), b)
    assert (res.final_iter, res.converged, res.stop, res.final_norm) == (1, True, "s", 0.0)
    assert np.array_equal(res.x, b)
    # all dofs essential: the constrained operator is the identity
    res = BR.bicgstab(lambda x: 0.0 * x, b, ess=[0, 1, 2], dinv=BR.jacobi_vector(np.zeros(3), [0, 1, 2]))
    assert (res.final_iter, res.converged, res.stop) == (1, True, "s") and np.array_equal(res.x, b)


def test_stop_r_and_max_iter():
    A = np.array([[4.0, 1.0, 0.0], [-1.0, 3.0, 1.0], [0.0, -1.0, 5.0]])
    b = np.array([1.0, 2.0, 3.0])
    res = BR.bicgstab(lambda x: A @ x, b, rel_tol=1e-12, max_iter=50)
    assert res.converged and res.stop in ("r", "s") and res.final_iter <= 4
    assert relerr(res.x, np.linalg.solve(A, b)) < 1e-12
    one = BR.bicgstab(lambda x: A @ x, b, rel_tol=1e-12, max_iter=1)
    assert (one.final_iter, one.converged, one.stop) == (1, False, "max_iter") and one.final_norm >= one.tol_goal
    zero = BR.bicgstab(lambda x: A @ x, b, max_iter=0)
    assert (zero.final_iter, zero.converged, zero.stop) == (0, False, "max_iter")
    assert zero.final_norm == zero.initial_norm and not zero.x.any()


def test_stop_omega_zero():
    """(t, s) == 0 exactly in iteration 1 (every value dyadic): stopped, not converged, after the x update."""
    A = np.array([[-2.0, -2.0], [-2.0, 0.0]])
    res = BR.bicgstab(lambda x: A @ x, np.array([1.0, 0.0]), max_iter=10)
    assert (res.final_iter, res.converged, res.stop, res.final_norm) == (1, False, "omega", 1.0)
    assert np.array_equal(res.x, [-0.5, 0.0])   # x = alpha phat, alpha = 1 / (r~, v) = -1/2


def test_stop_rho_zero():
    """(r~, r) == 0 exactly at the start of iteration 2 (every value dyadic): final_iter = 2, final_norm =
    iteration 1's ||r||, x = iteration 1's."""
    A = np.array([[-2.0, -2.0, -2.0], [-2.0, -2.0, -1.0], [2.0, -2.0, -2.0]])
    res = BR.bicgstab(lambda x: A @ x, np.array([1.0, 0.0, 0.0]), max_iter=10)
    assert (res.final_iter, res.converged, res.stop, res.final_norm) == (2, False, "rho", 1.0)
    assert np.array_equal(res.x, [-0.5, 1.0, -1.0])


def test_nonfinite_aborts():
    with pytest.raises(FloatingPointError):
        BR.bicgstab(lambda x: x.copy(), np.array([1.0, np.nan]))
    # alpha = rho_1 / 0: a zero operator
    with pytest.raises(FloatingPointError):
        BR.bicgstab(lambda x: 0.0 * x, np.ones(3))
    # (r~, v) == 0 with a skew operator
    with pytest.raises(FloatingPointError):
        BR.bicgstab(lambda x: np.array([x[1], -x[0]]), np.array([1.0, 0.0]))


# ---- self-gap on the GPU tests' cases ----
@pytest.mark.parametrize("name,marked", BC.CASES)
def test_self_gap(name, marked):
    c = BC.case(name, marked)
    for max_iter in (6, 1000):
        runs = [c.solve(dot=d, rel_tol=1e-12, max_iter=max_iter) for d in ("matmul", "fsum", "reversed")]
        iters = [r.final_iter for r in runs]
        scale = np.abs(runs[0].x).max()
        gap = max(np.abs(runs[i].x - runs[j].x).max() for i in range(3) for j in range(i)) / scale
        share = c.convective_share(runs[0].x)
        print(f"{name} marked={marked} max_iter={max_iter}: iters {iters} self-gap {gap:.2e} share {share:.2f} "
              f"true residual {c.true_residual(runs[0].x):.2e}")
        assert iters[0] == iters[1] == iters[2]
        assert gap <= 1e-14
        if max_iter == 6:
            assert iters[0] == 6 and not any(r.converged for r in runs)
        else:
            assert all(r.converged for r in runs)
            assert share > 0.1   # the term is not a bystander
            # (the solve the GPU tests share is this one)
            assert np.array_equal(runs[0].x, BC.reference(name, marked, 1000).x)


# ---- the example's discrete steady state ----
def slab_steady_state(pe=10.0):
    """The slab of examples/implicit_convect_heat.cpp: 8 x 2 x 2 elements on 1 x 0.25 x 0.25, p = 2, mass 1,
    diffusion 1, v = (Pe, 0, 0), u = 0 / 1 on the two x faces: (the dofs' coordinates, the discrete steady state
    (K + C) u = 0 by a dense solve)."""
    enodes, gm, n, X = O.cartesian_mesh(8, 2, 2, 1.0, 0.25, 0.25, order=2)
    sym_k = O.OracleOperator(enodes, gm, n, 2, beta=1.0)
    conv = CR.ConvRef(2, O.default_q1d(2), gm, n, enodes)
    v = np.array([pe, 0.0, 0.0])
    pa = conv.pa_data(v)
    kc = lambda x: sym_k.mult(x) + conv.mult(v, x, pa=pa)
    ess = np.nonzero(np.isclose(X[:, 0], 0.0) | np.isclose(X[:, 0], 1.0))[0]
    A = _dense(kc, n)
    g = np.where(np.isclose(X[:, 0], 1.0), 1.0, 0.0)
    free = np.setdiff1d(np.arange(n), ess)
    u = g.copy()
    u[free] = np.linalg.solve(A[np.ix_(free, free)], -(A @ g)[free])
    return X, u


def test_example_steady_state_distance():
    """The discrete steady state's own distance from (e^{Pe x} - 1) / (e^{Pe} - 1) at Pe = 10 is 2.62e-3; the
    example's bound is twice that, 5.3e-3."""
    X, u = slab_steady_state(10.0)
    exact = np.expm1(10.0 * X[:, 0]) / np.expm1(10.0)
    dist = float(np.abs(u - exact).max())
    print(f"discrete steady state: max|u - closed form| = {dist:.3e}")
    assert abs(dist - 2.62e-3) <= 5e-6
    assert 2.0 * dist <= 5.3e-3 < 2.0 * dist * 1.02
