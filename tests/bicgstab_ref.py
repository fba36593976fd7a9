"""numpy restatement of the reference's BiCGSTABSolver::Mult (linalg/solvers.cpp:1579-1805; a helper, not
a test): the checker of the device BiCGSTAB, over a callable Mult, around ConstrainedOperator DIAG_ONE
(operator.cpp:586-646) with iterative_mode = false and OperatorJacobiSmoother as a vector dinv.

The operations per entry and their order are the reference's:
    p = r + beta (p - omega v), s = r - alpha v, x = (x + alpha phat) + omega shat, r = s - omega t,
    beta = (rho_1 / rho_2) (alpha / omega);
the stops work on ||.||_2 (tol_goal = max(||r_0|| rel_tol, abs_tol)) and are decided by stop_decision, the
restatement of csrc/bicgstab_stop.hpp's bcg_stop that tests/cpp/bicgstab_stop_check.cpp is compared with.

dot: the summation order of every inner product -- "matmul" (a @ b), "fsum" (math.fsum of the products,
correctly rounded) or "reversed" (a running sum from the last entry to the first): the three orders of the
solver's self-gap (tests/test_bicgstab_reference.py).
"""
import math

import numpy as np

# csrc/bicgstab_stop.hpp
TEST_R0, TEST_RHO, TEST_S, TEST_R, TEST_OMEGA = 0, 1, 2, 3, 4
RUNNING, CONVERGED, CONVERGED_S, MAX_ITER, RHO_ZERO, OMEGA_ZERO, NONFINITE = 0, 1, 2, 3, 4, 5, 6
STOP_NAMES = {CONVERGED: "r", CONVERGED_S: "s", MAX_ITER: "max_iter", RHO_ZERO: "rho", OMEGA_ZERO: "omega",
              NONFINITE: "nonfinite"}


def stop_decision(test, value, tol_goal, it, max_iter):
    """bcg_stop: the status after `test` on `value` in iteration `it`."""
    if test == TEST_R0:
        return NONFINITE if not math.isfinite(value) else (CONVERGED if value <= tol_goal else RUNNING)
    if test == TEST_RHO:
        return RHO_ZERO if value == 0.0 else RUNNING
    if test == TEST_S:
        return NONFINITE if not math.isfinite(value) else (CONVERGED_S if value < tol_goal else RUNNING)
    if test == TEST_R:
        return NONFINITE if not math.isfinite(value) else (CONVERGED if value < tol_goal else RUNNING)
    if test == TEST_OMEGA:
        return OMEGA_ZERO if value == 0.0 else (MAX_ITER if it >= max_iter else RUNNING)
    raise ValueError(test)


def _dot_matmul(a, b):
    return float(a @ b)


def _dot_fsum(a, b):
    return math.fsum((a * b).tolist())


def _dot_reversed(a, b):
    s = 0.0
    for v in (a * b)[::-1].tolist():
        s += v
    return s


DOTS = {"matmul": _dot_matmul, "fsum": _dot_fsum, "reversed": _dot_reversed}


class Result:
    def __init__(self, x, final_iter, final_norm, converged, stop, initial_norm, tol_goal):
        self.x, self.final_iter, self.final_norm, self.converged = x, final_iter, final_norm, converged
        self.stop, self.initial_norm, self.tol_goal = stop, initial_norm, tol_goal

    def __iter__(self):  # (x, final_iter, final_norm, converged, stop)
        return iter((self.x, self.final_iter, self.final_norm, self.converged, self.stop))


def constrained(mult, ess):
    """ConstrainedOperator::ConstrainedMult, DIAG_ONE: w = x with the ess entries zeroed; y = A w; y[ess] = x[ess]."""
    ess = np.asarray(ess, dtype=np.int64)

    def cm(x):
        if ess.size == 0:
            return np.array(mult(x), dtype=np.float64)
        w = np.array(x, dtype=np.float64)
        w[ess] = 0.0
        y = np.array(mult(w), dtype=np.float64)
        y[ess] = x[ess]
        return y
    return cm


def jacobi_vector(diag, ess):
    """OperatorJacobiSmoother on the constrained operator: 1 / diag with the essential rows' diag 1."""
    d = np.array(diag, dtype=np.float64)
    d[np.asarray(ess, dtype=np.int64)] = 1.0
    return 1.0 / d


def bicgstab(mult, b, ess=(), dinv=None, rel_tol=1e-12, abs_tol=0.0, max_iter=1000, dot="matmul"):
    """BiCGSTABSolver::Mult.  Returns Result (x, final_iter, final_norm, converged, stop); stop is one of
    "r0", "r", "s", "max_iter", "rho", "omega"; a non-finite norm (MFEM_VERIFY's abort) raises
    FloatingPointError."""
    dt = DOTS[dot]
    A = constrained(mult, ess)
    b = np.asarray(b, dtype=np.float64)
    norm = lambda a: math.sqrt(dt(a, a))
    prec = (lambda a: dinv * a) if dinv is not None else (lambda a: a.copy())
    x = np.zeros_like(b)
    r = b.copy()
    rtilde = r.copy()
    resid = initial = norm(r)
    tol_goal = max(resid * rel_tol, abs_tol) if math.isfinite(resid) else float("nan")
    st = stop_decision(TEST_R0, resid, tol_goal, 0, max_iter)
    if st == NONFINITE:
        raise FloatingPointError(f"resid = {resid}")
    if st == CONVERGED:
        return Result(x, 0, resid, True, "r0", initial, tol_goal)
    rho_2 = alpha = omega = 1.0
    p = v = None
    with np.errstate(all="ignore"):
        for i in range(1, max_iter + 1):
            rho_1 = dt(rtilde, r)
            if stop_decision(TEST_RHO, rho_1, tol_goal, i, max_iter) == RHO_ZERO:
                return Result(x, i, resid, False, "rho", initial, tol_goal)
            if i == 1:
                p = r.copy()
            else:
                beta = (rho_1 / rho_2) * (alpha / omega)
                p = p + (-omega) * v
                p = r + beta * p
            phat = prec(p)
            v = A(phat)
            alpha = _div(rho_1, dt(rtilde, v))
            s = r + (-alpha) * v
            resid = norm(s)
            st = stop_decision(TEST_S, resid, tol_goal, i, max_iter)
            if st == NONFINITE:
                raise FloatingPointError(f"resid = {resid}")
            if st == CONVERGED_S:
                x = x + alpha * phat
                return Result(x, i, resid, True, "s", initial, tol_goal)
            shat = prec(s)
            t = A(shat)
            omega = _div(dt(t, s), dt(t, t))
            x = x + alpha * phat
            x = x + omega * shat
            r = s + (-omega) * t
            rho_2 = rho_1
            resid = norm(r)
            st = stop_decision(TEST_R, resid, tol_goal, i, max_iter)
            if st == NONFINITE:
                raise FloatingPointError(f"resid = {resid}")
            if st == CONVERGED:
                return Result(x, i, resid, True, "r", initial, tol_goal)
            st = stop_decision(TEST_OMEGA, omega, tol_goal, i, max_iter)
            if st == OMEGA_ZERO:
                return Result(x, i, resid, False, "omega", initial, tol_goal)
            if st == MAX_ITER:
                break
    return Result(x, max(max_iter, 0), resid, False, "max_iter", initial, tol_goal)


def _div(a, b):
    """IEEE division (a / 0 = +-inf or nan, as the C++ double division)."""
    return float(np.float64(a) / np.float64(b))
