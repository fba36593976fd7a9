"""The cell-death update of include/ecm2_pa.h ("Cell death") restated in numpy, vectorised over entries, for any
float type: `step(..., dtype=numpy.longdouble)` is the 80-bit reference the device and the C++ header are
compared with; `dtype=numpy.float64` is the restatement whose own error against the 80-bit run measures c_ref
(tests/test_celldeath_reference.py), never a device figure.  The algebra and the substep schedule are those of
csrc/celldeath_math.hpp, term for term; the model is the application's (three-state kinetics N <-> U -> D with
Arrhenius rates), so nothing here cites the reference library.

closed_form_mp() is an independent statement for the pins: mpmath.expm of the 3 x 3 generator."""
import numpy as np

THREE_STATE, ARRHENIUS = 0, 1
R_GAS = 8.31446261815324
U_ROUND = 2.0 ** -53


def rates(A, dE, TK, dtype):
    """k_i = A_i exp(-dE_i / (R T_K)): a list of three arrays."""
    irt = dtype(1) / (dtype(R_GAS) * TK)
    return [dtype(A[i]) * np.exp(-(dtype(dE[i]) * irt)) for i in range(3)]


def propagate(a, b, c, dt, N, U, D):
    """exp(M dt) applied to (N, U, D) at frozen rates, in the arrays' dtype (celldeath_propagate)."""
    dtype = N.dtype.type
    half, one, zero = dtype(0.5), dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        amc = a - c
        two_delta = np.sqrt(amc * amc + b * b + dtype(2) * b * (a + c))
        delta, h = half * two_delta, half * ((b + c) - a)
        lm = -(half * ((a + b) + c) + delta)
        lp = np.where(lm != 0, (a * c) / np.where(lm != 0, lm, one), zero)
        xm = lm * dt
        em, em1m, em1p = np.exp(xm), np.expm1(xm), np.expm1(lp * dt)
        ep = one + em1p
        psim = np.where(lm != 0, em1m / np.where(lm != 0, lm, one), dt)
        psip = np.where(lp != 0, em1p / np.where(lp != 0, lp, one), dt)
        nz = two_delta != 0
        safe2d = np.where(nz, two_delta, one)
        g = np.where(nz, ep * (-np.expm1(-(two_delta * dt))) / safe2d, ep * dt)
        G = np.where(-lp >= two_delta, np.where(lp != 0, (g - psim) / np.where(lp != 0, lp, one), zero),
                     (psip - psim) / safe2d)
        big, prod = np.abs(h) + delta, a * b
        little = np.where(big != 0, prod / np.where(big != 0, big, one), zero)
        p, q = np.where(h >= 0, big, little), np.where(h >= 0, little, big)
        fu = a * N + q * U
        Nn = em * N + g * (p * N + b * U)
        Un = em * U + g * fu
        dD = np.maximum(c * (psim * U + G * fu), zero)
    return np.minimum(Nn, one), np.minimum(Un, one), np.minimum(D + dD, one)


def step(model, A, dE, t_offset, T0, T1, dt, nsub, N, U, D, dtype=np.longdouble):
    """One ecm2_celldeath_step: returns (N, U, D, invalid) -- new arrays of `dtype` and the mask of the entries
    left untouched because T_K was non-finite or <= 0 at some substep."""
    T0 = np.asarray(T0, np.float64).astype(dtype)
    dT = (np.asarray(T1, np.float64).astype(dtype) - T0) if T1 is not None else np.zeros_like(T0)
    N0, U0, D0 = (np.asarray(v, np.float64).astype(dtype) for v in (N, U, D))
    n, u, d = N0.copy(), U0.copy(), D0.copy()
    h = dtype(dt) / dtype(nsub)
    bad = np.zeros(T0.shape, bool)
    with np.errstate(all="ignore"):
        for m in range(nsub):
            w = dtype(m + 0.5) / dtype(nsub)
            TK = (T0 + w * dT) + dtype(t_offset)
            bad |= ~(TK > 0) | ~np.isfinite(TK)
            k = rates(A, dE, np.where(bad, dtype(300), TK), dtype)
            if model == THREE_STATE:
                n, u, d = propagate(k[0], k[1], k[2], h, n, u, d)
            else:
                u = u + h * k[0]
        if model != THREE_STATE:
            moved = u != U0
            dn = np.maximum(D0, -np.expm1(-u))
            d = np.where(moved, dn, D0)
            n = np.where(moved, dtype(1) - dn, N0)
    return np.where(bad, N0, n), np.where(bad, U0, u), np.where(bad, D0, d), bad


def x_max(dE, TK_min):
    """max_i dE_i / (R T_K): the condition number of the rates in their argument."""
    return max(dE) / (R_GAS * TK_min)


def closed_form_mp(A, dE, TK, t, state, digits=50):
    """exp(M t) state by mpmath.expm of the 3 x 3 generator at `digits` digits: a list of three mpf."""
    import mpmath as mp
    with mp.workdps(digits):
        k = [mp.mpf(A[i]) * mp.exp(-mp.mpf(dE[i]) / (mp.mpf(R_GAS) * mp.mpf(TK))) for i in range(3)]
        a, b, c = k
        M = mp.matrix([[-a, b, 0], [a, -(b + c), 0], [0, c, 0]])
        y = mp.expm(M * mp.mpf(t)) * mp.matrix([mp.mpf(float(s)) for s in state])
        return [y[0], y[1], y[2]]
