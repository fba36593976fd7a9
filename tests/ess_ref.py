"""numpy restatements behind the essential-condition tests (a helper, not a test): ConstrainedOperator::EliminateRHS
(linalg/operator.cpp:559-584), Operator::FormLinearSystem for the identity prolongation (:114-129), and CGSolver::Mult
/ BiCGSTABSolver::Mult with iterative_mode = true (linalg/solvers.cpp:875-884, 1618-1627) over the constrained Mult
of bicgstab_ref.constrained, with the three dot orders of bicgstab_ref.DOTS.

The operations per entry and their order are the reference's: w = 0, w[ess] = x[ess], z = A w, b -= z, b[ess] =
x[ess]; the solvers start from r = b - A~ x and go on exactly as cheb_ref.pcg / bicgstab_ref.bicgstab do (x0 = None
calls those).

Also the data the CPU pin (tests/test_ess_reference.py) and the GPU tests (tests/test_gpu_essential.py) share: the
Dirichlet values x_D = 37 + 20 exp(-10 |p - 1/2|^2) at the essential dofs' coordinates, the eliminated right-hand
side, and the two starts "lift" (x_D on the list, 0 elsewhere) and "far" (free entries 37 + 20 U[0, 1), seeded).
"""
import math

import numpy as np

import bicgstab_ref as BR
import cheb_ref as CR
from bicgstab_ref import DOTS, constrained

STARTS = ["lift", "far"]


def eliminate_rhs(mult, ess, x, b):
    """EliminateRHS: returns the new b (x, b unchanged)."""
    ess = np.asarray(ess, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    w = np.zeros_like(x)
    w[ess] = x[ess]
    z = np.array(mult(w), dtype=np.float64)
    out = np.asarray(b, dtype=np.float64) - z
    out[ess] = x[ess]
    return out


def form_linear_system(mult, ess, x, b, copy_interior=False):
    """FormLinearSystem with the identity prolongation: returns (X, B)."""
    ess = np.asarray(ess, dtype=np.int64)
    X = np.array(x, dtype=np.float64)
    if not copy_interior:
        keep = X[ess].copy()
        X[:] = 0.0
        X[ess] = keep
    return X, eliminate_rhs(mult, ess, X, b)


def pcg(mult, b, ess=(), prec=None, rel_tol=1e-12, abs_tol=0.0, max_iter=1000, dot="matmul", x0=None):
    """cheb_ref.pcg with iterative_mode = true when x0 is given: r = b - A~ x0, x is not cleared."""
    if x0 is None:
        return CR.pcg(mult, b, ess, prec, rel_tol, abs_tol, max_iter, dot)
    dt = DOTS[dot]
    A = constrained(mult, ess)
    b = np.asarray(b, dtype=np.float64)
    B = prec if prec is not None else (lambda a: a.copy())
    x = np.array(x0, dtype=np.float64)
    r = b - A(x)
    z = B(r)
    d = z.copy()
    nom0 = nom = dt(d, r)
    if not math.isfinite(nom):
        raise FloatingPointError(f"nom = {nom}")
    if nom < 0.0:
        return CR.Result(x, 0, nom, False, "neg0", nom)
    initial = math.sqrt(nom)
    r0 = max(nom * rel_tol * rel_tol, abs_tol * abs_tol)
    if nom <= r0:
        return CR.Result(x, 0, initial, True, "r0", initial)
    z = A(d)
    den = dt(z, d)
    if not math.isfinite(den):
        raise FloatingPointError(f"den = {den}")
    if den == 0.0:
        return CR.Result(x, 0, initial, False, "den0", initial)
    fin = lambda v: math.sqrt(v) if v >= 0 else v
    i = 1
    with np.errstate(all="ignore"):
        while True:
            alpha = CR._div(nom, den)
            x = x + alpha * d
            r = r + (-alpha) * z
            z = B(r)
            betanom = dt(r, z)
            if not math.isfinite(betanom):
                raise FloatingPointError(f"betanom = {betanom}")
            if betanom < 0.0:
                return CR.Result(x, i, betanom, False, "neg", initial)
            if betanom <= r0:
                return CR.Result(x, i, fin(betanom), True, "converged", initial)
            i += 1
            if i > max_iter:
                return CR.Result(x, max_iter, fin(betanom), False, "max_iter", initial)
            beta = CR._div(betanom, nom)
            d = z + beta * d
            z = A(d)
            den = dt(d, z)
            if not math.isfinite(den):
                raise FloatingPointError(f"den = {den}")
            if den == 0.0:
                return CR.Result(x, i, fin(betanom), False, "den", initial)
            nom = betanom
    return CR.Result(x, i, fin(nom0), False, "max_iter", initial)


def bicgstab(mult, b, ess=(), dinv=None, rel_tol=1e-12, abs_tol=0.0, max_iter=1000, dot="matmul", x0=None):
    """bicgstab_ref.bicgstab with iterative_mode = true when x0 is given: r = b - A~ x0, r~ = r."""
    if x0 is None:
        return BR.bicgstab(mult, b, ess, dinv, rel_tol, abs_tol, max_iter, dot)
    dt = DOTS[dot]
    A = constrained(mult, ess)
    b = np.asarray(b, dtype=np.float64)
    norm = lambda a: math.sqrt(dt(a, a))
    prec = (lambda a: dinv * a) if dinv is not None else (lambda a: a.copy())
    x = np.array(x0, dtype=np.float64)
    r = b - A(x)
    rtilde = r.copy()
    resid = initial = norm(r)
    tol_goal = max(resid * rel_tol, abs_tol) if math.isfinite(resid) else float("nan")
    st = BR.stop_decision(BR.TEST_R0, resid, tol_goal, 0, max_iter)
    if st == BR.NONFINITE:
        raise FloatingPointError(f"resid = {resid}")
    if st == BR.CONVERGED:
        return BR.Result(x, 0, resid, True, "r0", initial, tol_goal)
    rho_2 = alpha = omega = 1.0
    p = v = None
    with np.errstate(all="ignore"):
        for i in range(1, max_iter + 1):
            rho_1 = dt(rtilde, r)
            if BR.stop_decision(BR.TEST_RHO, rho_1, tol_goal, i, max_iter) == BR.RHO_ZERO:
                return BR.Result(x, i, resid, False, "rho", initial, tol_goal)
            if i == 1:
                p = r.copy()
            else:
                beta = (rho_1 / rho_2) * (alpha / omega)
                p = p + (-omega) * v
                p = r + beta * p
            phat = prec(p)
            v = A(phat)
            alpha = BR._div(rho_1, dt(rtilde, v))
            s = r + (-alpha) * v
            resid = norm(s)
            st = BR.stop_decision(BR.TEST_S, resid, tol_goal, i, max_iter)
            if st == BR.NONFINITE:
                raise FloatingPointError(f"resid = {resid}")
            if st == BR.CONVERGED_S:
                x = x + alpha * phat
                return BR.Result(x, i, resid, True, "s", initial, tol_goal)
            shat = prec(s)
            t = A(shat)
            omega = BR._div(dt(t, s), dt(t, t))
            x = x + alpha * phat
            x = x + omega * shat
            r = s + (-omega) * t
            rho_2 = rho_1
            resid = norm(r)
            st = BR.stop_decision(BR.TEST_R, resid, tol_goal, i, max_iter)
            if st == BR.NONFINITE:
                raise FloatingPointError(f"resid = {resid}")
            if st == BR.CONVERGED:
                return BR.Result(x, i, resid, True, "r", initial, tol_goal)
            st = BR.stop_decision(BR.TEST_OMEGA, omega, tol_goal, i, max_iter)
            if st == BR.OMEGA_ZERO:
                return BR.Result(x, i, resid, False, "omega", initial, tol_goal)
            if st == BR.MAX_ITER:
                break
    return BR.Result(x, max(max_iter, 0), resid, False, "max_iter", initial, tol_goal)


# ---- the shared data: a case is a cheb_cases.Case or a bicgstab_cases.Case (mult, ess, dinv, b, fes, n) ----
class Problem:
    """The inhomogeneous problem posed on one case: x_D on its essential dofs, the eliminated b, the two starts."""

    def __init__(self, c):
        self.c = c
        self.ess = np.asarray(c.ess, dtype=np.int64)
        X = c.fes.dof_coords()
        self.xd = np.zeros(c.n)   # x_D on the list, 0 elsewhere: the lift
        d = X[self.ess] - 0.5
        self.xd[self.ess] = 37.0 + 20.0 * np.exp(-10.0 * (d * d).sum(-1))
        self.b = eliminate_rhs(c.mult, self.ess, self.xd, c.b)
        far = 37.0 + 20.0 * np.random.default_rng(2024).uniform(0.0, 1.0, c.n)
        far[self.ess] = self.xd[self.ess]
        self.starts = {"lift": self.xd.copy(), "far": far}
        self._ref = {}

    def near(self, x):
        """x (1 + 1e-3 sin i) on the free entries, x_D on the list."""
        y = np.asarray(x, dtype=np.float64) * (1.0 + 1e-3 * np.sin(np.arange(self.c.n, dtype=np.float64)))
        y[self.ess] = self.xd[self.ess]
        return y

    def solve(self, kind, x0=None, dot="matmul", **kw):
        """kind: "jacobi" (Jacobi-PCG), "bicgstab" (with Jacobi from the case's dinv), or a callable r -> B r
        (the PCG with it)."""
        c = self.c
        if kind == "bicgstab":
            return bicgstab(c.mult, self.b, self.ess, c.dinv, dot=dot, x0=x0, **kw)
        prec = (lambda a: c.dinv * a) if kind == "jacobi" else kind
        return pcg(c.mult, self.b, self.ess, prec, dot=dot, x0=x0, **kw)

    def reference(self, kind, start, max_iter, rel_tol=1e-12, abs_tol=0.0, tag=None):
        """A solve with matmul dots from a named start ("lift", "far", None: cold) or (tag, x0), computed once and
        left unchanged.  A callable `kind` needs a tag of its own."""
        name, x0 = start if isinstance(start, tuple) else (start, self.starts.get(start))
        key = (tag or kind, name, max_iter, rel_tol, abs_tol)
        if key not in self._ref:
            self._ref[key] = self.solve(kind, x0, rel_tol=rel_tol, abs_tol=abs_tol, max_iter=max_iter)
        return self._ref[key]

    def true_residual(self, x):
        """||b - A~ x|| / ||b|| of the eliminated system."""
        A = constrained(self.c.mult, self.ess)
        return float(np.linalg.norm(self.b - A(np.asarray(x, dtype=np.float64))) / np.linalg.norm(self.b))


_PROBLEMS = {}


class _FinestLevel:
    """A multigrid case's finest level with the attributes of a solver case."""

    def __init__(self, mc):
        f = mc.fine
        self.mc, self.mult, self.ess, self.dinv, self.b, self.fes, self.n = mc, f.op.mult, f.ess, f.dinv, mc.b, f.fes, f.n


def problem(kind, key):
    """kind "cg": cheb_cases.case(key); "mg": the finest level of mg_cases.case(key) (P.c.mc: the hierarchy);
    "bicgstab": bicgstab_cases.case(*key).  Built once."""
    if (kind, key) not in _PROBLEMS:
        if kind == "cg":
            import cheb_cases as CC
            c = CC.case(key)
        elif kind == "mg":
            import mg_cases as MC
            c = _FinestLevel(MC.case(key))
        else:
            import bicgstab_cases as BC
            c = BC.case(*key)
        _PROBLEMS[kind, key] = Problem(c)
    return _PROBLEMS[kind, key]
