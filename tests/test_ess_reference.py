"""CPU pin of the numpy reference behind the essential-condition tests (tests/ess_ref.py) and of the conditions the
GPU tests (tests/test_gpu_essential.py) rely on:

  * with x0 = 0 the iterative-mode restatements reproduce cheb_ref.pcg / bicgstab_ref.bicgstab bitwise;
  * the eliminated system's converged solution is the dense solve with the essential values imposed (1e-10);
  * with x0[ess] = b[ess] = x_D the essential entries of x are bitwise x_D after any number of iterations (r_ess = 0
    exactly);
  * the fixed-work condition of DESIGN.md section 4e's method: after 6 iterations from the "lift" and "far" starts
    the reference's x under its three summation orders agrees to <= 1e-14 of max|x|, so the device may be held to
    1e-12.  Measured: Jacobi-PCG on k2, k3, k1, mk2 <= 1.45e-15 in all eight; BiCGSTAB p2 2.0e-15 / 4.0e-16,
    p2 marked 2.7e-16 / 2.7e-16, p3 7.1e-16 / 2.9e-16, p3 marked 4.8e-14 (lift) / 4.2e-16: p3 marked misses and is
    left out of the GPU's fixed-work comparison (ADMITTED_BICGSTAB);
  * the warm-start claims: from a start near the solution and an absolute tolerance the count is below the cold
    one; at the converged solution the solve ends before the loop, with a margin (FIXED_POINT_* cases end their cold
    solve at <= 0.6 of the goal, where the true residual and the recurrence's differ by about a hundredth of it);
  * the two discretisation values of examples/rf_electrode.cpp, from the CPU oracle.
"""
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import oracle as O
import bicgstab_cases as BC
import bicgstab_ref as BR
import cheb_cases as CC
import cheb_ref as CR
import ess_ref as ER
from helpers import relerr

CG_CASES = ["k2", "k3", "k1", "mk2"]
DOT_ORDERS = ("matmul", "fsum", "reversed")
SELF_GAP = 1e-14
# the BiCGSTAB cases whose self-gap holds from both starts (test_fixed_work_self_gap_bicgstab)
ADMITTED_BICGSTAB = [("p2", False), ("p2", True), ("p3", False)]
# the cases of the GPU's fixed-point and near-start tests
FIXED_POINT_CG = ["k1", "mk2"]
FIXED_POINT_BICGSTAB = [("p3", False)]


def _cold_goal(P, kind):
    """The goal of the cold solve to rel_tol 1e-12, as an absolute tolerance: PCG's r0 = (rel_tol sqrt(nom_0))^2,
    BiCGSTAB's tol_goal = rel_tol ||r_0||."""
    cold = P.reference(kind, None, 1000)
    assert cold.converged
    return cold, 1e-12 * cold.initial_norm


def test_x0_zero_reproduces_the_cold_references_bitwise():
    c = CC.case("k2")
    prec = lambda a: c.dinv * a
    for max_iter in (3, 1000):
        a = CR.pcg(c.mult, c.b, c.ess, prec, rel_tol=1e-12, max_iter=max_iter)
        b = ER.pcg(c.mult, c.b, c.ess, prec, rel_tol=1e-12, max_iter=max_iter, x0=np.zeros(c.n))
        assert np.array_equal(a.x, b.x) and tuple(a)[1:] == tuple(b)[1:] and a.initial_norm == b.initial_norm
    c = BC.case("p2", False)
    for max_iter in (3, 1000):
        a = BR.bicgstab(c.mult, c.b, c.ess, c.dinv, rel_tol=1e-12, max_iter=max_iter)
        b = ER.bicgstab(c.mult, c.b, c.ess, c.dinv, rel_tol=1e-12, max_iter=max_iter, x0=np.zeros(c.n))
        assert np.array_equal(a.x, b.x) and tuple(a)[1:] == tuple(b)[1:] and a.tol_goal == b.tol_goal


def test_form_linear_system_restates_the_reference():
    c = CC.case("k1")
    P = ER.problem("cg", "k1")
    x = np.random.default_rng(3).uniform(-1, 1, c.n)
    X0, B0 = ER.form_linear_system(c.mult, P.ess, x, c.b, copy_interior=False)
    X1, B1 = ER.form_linear_system(c.mult, P.ess, x, c.b, copy_interior=True)
    free = np.setdiff1d(np.arange(c.n), P.ess)
    assert np.array_equal(X0[P.ess], x[P.ess]) and not X0[free].any() and np.array_equal(X1, x)
    # the elimination reads x on the list only
    assert np.array_equal(B0, B1) and np.array_equal(B0[P.ess], x[P.ess])
    assert np.array_equal(B0, ER.eliminate_rhs(c.mult, P.ess, x, c.b))
    # no essential dof: b keeps its bits
    assert np.array_equal(ER.eliminate_rhs(c.mult, [], x, c.b), c.b)


@pytest.mark.parametrize("name", ["k1", "k2"])
def test_eliminated_solution_is_the_dense_solve_with_the_values_imposed(name):
    c = CC.case(name)
    P = ER.problem("cg", name)
    I = np.eye(c.n)
    A = np.stack([c.mult(I[:, j]) for j in range(c.n)], axis=1)
    free = np.setdiff1d(np.arange(c.n), P.ess)
    xd = P.xd[P.ess]
    dense = P.xd.copy()
    dense[free] = np.linalg.solve(A[np.ix_(free, free)], c.b[free] - A[np.ix_(free, P.ess)] @ xd)
    for start in ER.STARTS + [None]:
        r = P.reference("jacobi", start, 1000)
        assert r.converged
        assert relerr(r.x, dense) <= 1e-10, (start, relerr(r.x, dense))


@pytest.mark.parametrize("start", ER.STARTS)
def test_essential_entries_keep_their_bits(start):
    for kind, key, solver in [("cg", "k2", "jacobi"), ("cg", "mk2", "jacobi"), ("bicgstab", ("p2", False), "bicgstab"),
                              ("bicgstab", ("p3", True), "bicgstab")]:
        P = ER.problem(kind, key)
        for max_iter in (1, 3, 6, 1000):
            r = P.solve(solver, P.starts[start], rel_tol=1e-12, max_iter=max_iter)
            assert np.array_equal(r.x[P.ess], P.xd[P.ess]), (key, max_iter)


def _self_gap(P, kind, start):
    xs = [P.solve(kind, P.starts[start], dot=d, rel_tol=1e-12, max_iter=6) for d in DOT_ORDERS]
    assert all(r.final_iter == 6 and not r.converged for r in xs)
    return max(np.abs(r.x - xs[0].x).max() for r in xs) / np.abs(xs[0].x).max()


@pytest.mark.parametrize("start", ER.STARTS)
@pytest.mark.parametrize("name", CG_CASES)
def test_fixed_work_self_gap_cg(name, start):
    gap = _self_gap(ER.problem("cg", name), "jacobi", start)
    print(f"{name} {start}: self-gap {gap:.2e}")
    assert gap <= SELF_GAP


@pytest.mark.parametrize("start", ER.STARTS)
@pytest.mark.parametrize("key", BC.CASES)
def test_fixed_work_self_gap_bicgstab(key, start):
    """The four cases are measured; the admitted ones must hold, and unmarked p2 is among them."""
    gap = _self_gap(ER.problem("bicgstab", key), "bicgstab", start)
    print(f"{key} {start}: self-gap {gap:.2e}")
    assert ("p2", False) in ADMITTED_BICGSTAB and len(ADMITTED_BICGSTAB) >= len(BC.CASES) - 1
    if key in ADMITTED_BICGSTAB:
        assert gap <= SELF_GAP


@pytest.mark.parametrize("start", ER.STARTS)
@pytest.mark.parametrize("form", ["cheb2", "mg"])
def test_fixed_work_self_gap_preconditioned(form, start):
    """The other two forms of the GPU's fixed-work test: Chebyshev-PCG order 2 on k2, the multigrid PCG on the
    smallest p-cycle.  Measured <= 5.6e-16."""
    import mg_cases as MC
    if form == "cheb2":
        P = ER.problem("cg", "k2")
        prec = lambda d: P.c.smoother(2)
    else:
        P = ER.problem("mg", MC.CASES[0])
        prec = lambda d: P.c.mc.cycle(None, d)
    xs = [P.solve(prec(d), P.starts[start], dot=d, rel_tol=1e-12, max_iter=6) for d in DOT_ORDERS]
    assert all(r.final_iter == 6 and not r.converged for r in xs)
    gap = max(np.abs(r.x - xs[0].x).max() for r in xs) / np.abs(xs[0].x).max()
    print(f"{form} {start}: self-gap {gap:.2e}")
    assert gap <= SELF_GAP


@pytest.mark.parametrize("kind,key,solver", [("cg", k, "jacobi") for k in FIXED_POINT_CG]
                         + [("bicgstab", k, "bicgstab") for k in FIXED_POINT_BICGSTAB])
def test_fixed_point_and_near_start(kind, key, solver):
    P = ER.problem(kind, key)
    cold, goal = _cold_goal(P, solver)
    # the margin the GPU's fixed-point test relies on
    assert cold.final_norm <= 0.6 * goal
    fp = P.solve(solver, cold.x, rel_tol=0.0, abs_tol=goal)
    assert fp.final_iter == 0 and fp.converged and np.array_equal(fp.x, cold.x)
    assert fp.initial_norm <= 0.6 * goal
    near = P.reference(solver, ("near", P.near(cold.x)), 1000, rel_tol=0.0, abs_tol=goal)
    print(f"{key}: cold {cold.final_iter}, near {near.final_iter} iterations")
    assert near.converged and 0 < near.final_iter < cold.final_iter


@pytest.mark.parametrize("n,err_ref,excess_ref", [(8, 1.497e-6, 4.539e-7), (4, 1.964e-5, 7.05e-6)])
def test_rf_electrode_discretisation_values(n, err_ref, excess_ref):
    """examples/rf_electrode.cpp's problem by the CPU oracle: unit cube n^3, p = 2, sigma = 1 + x, phi = 30 on x = 0
    and 0 on x = 1.  The example's bounds are the n = 8 values plus 25 %: 1.9e-6 and 5.7e-7."""
    en, gm, nd, X = O.cartesian_mesh(n, n, n, order=2)
    Pq = O.quad_points(en, O.default_q1d(2))
    V0 = 30.0
    ess = np.nonzero((X[:, 0] == 0.0) | (X[:, 0] == 1.0))[0]
    x0 = np.zeros(nd)
    x0[ess] = np.where(X[ess, 0] < 0.5, V0, 0.0)
    out = {}
    for sigma in ("1 + x", "1"):
        op = O.OracleOperator(en, gm, nd, 2, alpha=None, beta=1.0 + Pq[..., 0] if sigma == "1 + x" else 1.0)
        Xs, B = ER.form_linear_system(op.mult, ess, x0, np.zeros(nd))
        dinv = CR.jacobi_vector(op.diagonal(), ess)
        r = ER.pcg(op.mult, B, ess, lambda a: dinv * a, rel_tol=1e-13, max_iter=2000, x0=Xs)
        assert r.converged and np.array_equal(r.x[ess], x0[ess])
        exact = V0 * (1.0 - np.log1p(X[:, 0]) / math.log(2.0)) if sigma == "1 + x" else V0 * (1.0 - X[:, 0])
        power = V0 * V0 / math.log(2.0) if sigma == "1 + x" else V0 * V0
        out[sigma] = (np.abs(r.x - exact).max() / V0, (float(r.x @ op.mult(r.x)) - power) / power)
    err, excess = out["1 + x"]
    print(f"n = {n}: max|phi_h - phi| / V0 = {err:.4e}, energy excess {excess:+.4e}; sigma = 1: {out['1'][0]:.2e}")
    assert abs(err - err_ref) <= 2e-3 * err_ref and abs(excess - excess_ref) <= 2e-3 * excess_ref
    assert out["1"][0] <= 1e-12 and abs(out["1"][1]) <= 1e-13
    if n == 8:
        assert 1.25 * err <= 1.9e-6 < 1.3 * err and 1.25 * excess <= 5.7e-7 < 1.3 * excess
