"""numpy restatements behind the Chebyshev tests (a helper, not a test): the coefficients of
OperatorChebyshevSmoother::Setup (linalg/solvers.cpp:538-617), its Mult (:619-658), PowerMethod::
EstimateLargestEigenvalue (linalg/operator.cpp:871-928) and CGSolver::Mult (linalg/solvers.cpp:869-1004) with a
callable preconditioner, over a callable Mult around ConstrainedOperator DIAG_ONE (bicgstab_ref.constrained)
with iterative_mode = false.

The operations per entry and their order are the reference's: the smoother's t *= dinv, y += c_k t; the power
method's v0 *= 1 / sqrt((v0, v0)) (Vector::operator/=), v1 = dinv .* (A~ v0), eig_new = (v0, v1); the CG's
x += alpha d, r -= alpha (A d), d = z + beta d.

dot: the summation order of every inner product -- "matmul", "fsum" or "reversed", as in bicgstab_ref.py.
"""
import math

import numpy as np

from bicgstab_ref import DOTS, constrained, jacobi_vector  # noqa: F401  (shared with the cases)

ORDERS_ALL = [1, 2, 3, 4, 5]  # the orders Setup has closed forms for


def coefficients(order, max_eig):
    """Setup's closed forms (** where the reference calls pow); ValueError outside 1..5, where it aborts."""
    hi, lo = 1.2 * max_eig, 0.3 * max_eig
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    d2, t2 = delta ** 2, theta ** 2
    if order == 1:
        c = [1.0 / theta]
    elif order == 2:
        w = 1.0 / (d2 - 2 * t2)
        c = [-4 * theta * w, 2 * w]
    elif order == 3:
        d3 = 3 * d2
        w = 1.0 / (-4 * theta ** 3 + theta * d3)
        c = [w * (d3 - 12 * t2), 12 / (d3 - 4 * t2), -4 * w]
    elif order == 4:
        d8 = 8 * d2
        w = 1.0 / (delta ** 4 + 8 * theta ** 4 - t2 * d8)
        c = [w * (32 * theta ** 3 - 16 * theta * d2), w * (-48 * t2 + d8), 32 * theta * w, -8 * w]
    elif order == 5:
        d45, t4 = 5 * delta ** 4, theta ** 4
        d60, d20, t160 = 60 * d2, 20 * d2, 160 * t2
        wo = 1.0 / (16 * theta ** 5 - theta ** 3 * d20 + theta * d45)
        we = 1.0 / (d45 + 16 * t4 - t2 * d20)
        c = [wo * (d45 + 80 * t4 - t2 * d60), we * (d60 - t160), wo * (-d20 + t160), -80 * we, 16 * wo]
    else:
        raise ValueError(f"Chebyshev smoother not implemented for order = {order}")
    return np.array(c, dtype=np.float64)


def theta_delta(max_eig):
    hi, lo = 1.2 * max_eig, 0.3 * max_eig
    return 0.5 * (hi + lo), 0.5 * (hi - lo)


def smoother(mult, dinv, ess, coeffs):
    """OperatorChebyshevSmoother::Mult as a callable x -> y."""
    A = constrained(mult, ess)
    dinv = np.asarray(dinv, dtype=np.float64)
    coeffs = np.asarray(coeffs, dtype=np.float64)

    def S(x):
        t = np.array(x, dtype=np.float64)
        y = np.zeros_like(t)
        for k, ck in enumerate(coeffs):
            if k > 0:
                t = A(t)
            t = t * dinv
            y = y + ck * t
        return y
    return S


class PowerResult:
    def __init__(self, eig, steps, diffs, v):
        self.eig, self.steps, self.diffs, self.v = eig, steps, diffs, v

    def __iter__(self):  # (eig, steps)
        return iter((self.eig, self.steps))


def power_method(mult, dinv, ess, v0, num_steps=10, tol=1e-8, dot="matmul"):
    """EstimateLargestEigenvalue on D^-1 A~ with seed = 0 (v0 given).  Returns PowerResult: eig, the steps run,
    every step's diff and the last iterate."""
    dt = DOTS[dot]
    A = constrained(mult, ess)
    v0 = np.array(v0, dtype=np.float64)
    eig, diffs = 1.0, []
    for _ in range(num_steps):
        m = 1.0 / math.sqrt(dt(v0, v0))
        v0 = v0 * m
        v1 = A(v0) * dinv
        new = dt(v0, v1)
        diff = abs((new - eig) / eig)
        diffs.append(diff)
        eig = new
        v0 = v1
        if diff < tol:
            break
    return PowerResult(eig, len(diffs), diffs, v0)


class Result:
    def __init__(self, x, final_iter, final_norm, converged, stop, initial_norm):
        self.x, self.final_iter, self.final_norm, self.converged = x, final_iter, final_norm, converged
        self.stop, self.initial_norm = stop, initial_norm

    def __iter__(self):  # (x, final_iter, final_norm, converged, stop)
        return iter((self.x, self.final_iter, self.final_norm, self.converged, self.stop))


def _div(a, b):
    return float(np.float64(a) / np.float64(b))


def pcg(mult, b, ess=(), prec=None, rel_tol=1e-12, abs_tol=0.0, max_iter=1000, dot="matmul"):
    """CGSolver::Mult with prec a callable r -> B r (None: no preconditioner).  Returns Result; stop is one of
    "neg0" ((B r, r) < 0 before the loop), "r0" (converged before it), "den0" ((A d, d) == 0 before it),
    "converged", "neg" ((B r, r) < 0 inside it), "max_iter", "den" ((A d, d) == 0 inside it); final_norm =
    sqrt((B r, r)), or the raw value when it is negative; a non-finite (B r, r) or (A d, d) (MFEM_VERIFY's
    abort) raises FloatingPointError."""
    dt = DOTS[dot]
    A = constrained(mult, ess)
    b = np.asarray(b, dtype=np.float64)
    B = prec if prec is not None else (lambda a: a.copy())
    x = np.zeros_like(b)
    r = b.copy()
    z = B(r)
    d = z.copy()
    nom0 = nom = dt(d, r)
    if not math.isfinite(nom):
        raise FloatingPointError(f"nom = {nom}")
    if nom < 0.0:
        return Result(x, 0, nom, False, "neg0", nom)
    initial = math.sqrt(nom)
    r0 = max(nom * rel_tol * rel_tol, abs_tol * abs_tol)
    if nom <= r0:
        return Result(x, 0, initial, True, "r0", initial)
    z = A(d)
    den = dt(z, d)
    if not math.isfinite(den):
        raise FloatingPointError(f"den = {den}")
    if den == 0.0:
        return Result(x, 0, initial, False, "den0", initial)
    fin = lambda v: math.sqrt(v) if v >= 0 else v
    i = 1
    with np.errstate(all="ignore"):
        while True:
            alpha = _div(nom, den)
            x = x + alpha * d
            r = r + (-alpha) * z
            z = B(r)
            betanom = dt(r, z)
            if not math.isfinite(betanom):
                raise FloatingPointError(f"betanom = {betanom}")
            if betanom < 0.0:
                return Result(x, i, betanom, False, "neg", initial)
            if betanom <= r0:
                return Result(x, i, fin(betanom), True, "converged", initial)
            i += 1
            if i > max_iter:
                return Result(x, max_iter, fin(betanom), False, "max_iter", initial)
            beta = _div(betanom, nom)
            d = z + beta * d
            z = A(d)
            den = dt(d, z)
            if not math.isfinite(den):
                raise FloatingPointError(f"den = {den}")
            if den == 0.0:
                return Result(x, i, fin(betanom), False, "den", initial)
            nom = betanom
    return Result(x, i, fin(nom0), False, "max_iter", initial)
