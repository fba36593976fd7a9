"""The case matrix of the cell-death tests: parameter sets, temperatures, time steps, initial states and the
degenerate inputs, shared by tests/test_celldeath_reference.py (which measures c_ref on it), the C++ header's
check (tests/test_celldeath_host.py) and the device tests (tests/test_gpu_celldeath.py).

Parameter sets (A [1/s], dE [J/mol]; published Arrhenius fits serve as magnitudes, the three-state assignment is
this file's): "tissue" pairs the liver fit A = 7.39e39, dE = 2.577e5 (unfolding) and the Henriques-Moritz skin fit
A = 3.1e98, dE = 6.28e5 (death) with a refolding rate between them -- stiff: k3 runs from 5e-8 1/s at 37 C to 1e15
at 120 C; "mild" has three rates of comparable size, so U is populated."""
import numpy as np

import celldeath_ref as CR

PARAMS = {
    "tissue": ((7.39e39, 1.0e25, 3.1e98), (2.577e5, 1.6e5, 6.28e5)),
    "mild": ((2.0e22, 5.0e19, 1.0e24), (1.5e5, 1.4e5, 1.6e5)),
}
TEMPS_C = np.array([37.0, 43.0, 50.0, 60.0, 70.0, 80.0, 95.0, 105.0, 120.0])
DTS = (1e-3, 0.1, 1.0, 30.0, 300.0)
GPU_DTS = (1e-3, 1.0, 300.0)
SCHEDULES = ((False, 1), (False, 4), (True, 1), (True, 4))   # (T1 present, nsub)
SIZES = (1, 2, 3, 511, 2047, 2048, 2049, 100003)
T1_RISE = 7.25  # the end-of-step field of the cases with T1: T0 + T1_RISE (1 + sin) / 2


def zeroed(A, which):
    return tuple(0.0 if i in which else a for i, a in enumerate(A))


def parameter_sets():
    """(name, model, A, dE): the two sets in both models, and "mild" with every A_i = 0 in turn and all zero."""
    out = []
    for name, (A, dE) in PARAMS.items():
        out.append((name, CR.THREE_STATE, A, dE))
        out.append((name + "-arrhenius", CR.ARRHENIUS, A, dE))
    A, dE = PARAMS["mild"]
    for which in ((0,), (1,), (2,), (0, 1, 2)):
        out.append(("mild-A%s=0" % "".join(str(i + 1) for i in which), CR.THREE_STATE, zeroed(A, which), dE))
    return out


def states(n, seed, model=CR.THREE_STATE):
    """n states: every third (1, 0, 0), the others random and normalised (ARRHENIUS: U = Omega >= 0 with the
    consistent D = 1 - exp(-Omega), N = 1 - D)."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 1.0, (3, n))
    s[2] *= rng.uniform(0.0, 1.0, n) ** 4   # small and large dead fractions
    s /= s.sum(0)
    N, U, D = s
    fresh = np.arange(n) % 3 == 0
    N[fresh], U[fresh], D[fresh] = 1.0, 0.0, 0.0
    if model == CR.ARRHENIUS:
        U = np.where(fresh, 0.0, rng.uniform(0.0, 3.0, n))
        D = -np.expm1(-U)
        N = 1.0 - D
    return np.ascontiguousarray(N), np.ascontiguousarray(U), np.ascontiguousarray(D)


def temperatures(n, seed, kelvin):
    """n temperatures covering 37-120 C (the grid's nine values first, then uniform), and the end-of-step field."""
    rng = np.random.default_rng(seed + 1)
    T0 = np.concatenate([np.repeat(TEMPS_C, 6), rng.uniform(37.0, 120.0, max(0, n - 54))])[:n]
    if n < 54:
        T0 = rng.permutation(np.repeat(TEMPS_C, 6))[:n]
    T1 = T0 + T1_RISE * 0.5 * (1.0 + np.sin(np.arange(n) * 0.7))
    off = 273.15 if kelvin else 0.0
    return T0 + off, T1 + off


def grid_cases():
    """The c_ref grid: 9 temperatures x 6 states per case, every parameter set x dt x schedule x unit."""
    n = 54
    for name, model, A, dE in parameter_sets():
        for dt in DTS:
            for with_T1, nsub in SCHEDULES:
                for kelvin in (False, True):
                    T0, T1 = temperatures(n, 11, kelvin)
                    N, U, D = states(n, 5, model)
                    yield dict(name=f"{name} dt={dt} T1={int(with_T1)} nsub={nsub} {'K' if kelvin else 'C'}",
                               model=model, A=A, dE=dE, t_offset=0.0 if kelvin else 273.15, dt=dt, nsub=nsub,
                               T0=T0, T1=T1 if with_T1 else None, N=N, U=U, D=D)


def near_double_cases():
    """Near a double eigenvalue of the (N, U) block (dE = 0: the rates are the A_i themselves): b = 0 with
    |a - c| / a in {1e-3, 1e-6, 1e-9, 1e-12} on either side, and a = c with b / a = 1e-14, at |lambda dt| about
    0.3, 1 and 3 and at rates of 1 and 1e3 1/s.  The divided difference (psi(lp) - psi(lm)) / (2 delta) loses
    u / (2 delta dt) there."""
    n = 54
    N, U, D = states(n, 23)
    T0 = np.linspace(37.0, 120.0, n)
    for scale, dts in ((1.0, (0.3, 1.0, 3.0)), (1e3, (1e-3,))):
        sets = [(1.0, 0.0, 1.0 + s * e) for e in (1e-3, 1e-6, 1e-9, 1e-12) for s in (1.0, -1.0)]
        sets += [(1.0, 1e-14, 1.0), (1.0, 1e-9, 1.0 + 1e-9)]
        for a, b, c in sets:
            for dt in dts:
                for nsub in (1, 4):
                    yield dict(name=f"near-double a={a * scale} b={b * scale} c-a={(c - a) * scale:.1e} dt={dt} nsub={nsub}",
                               model=CR.THREE_STATE, A=(a * scale, b * scale, c * scale), dE=(0.0, 0.0, 0.0),
                               t_offset=273.15, dt=dt, nsub=nsub, T0=T0, T1=None, N=N, U=U, D=D)


def hazard_cases():
    """The hazards and the degenerate inputs beyond the grid: overflow, underflow, the exact double eigenvalue,
    dt = 0, a step whose rate * dt overflows, invalid entries (at the start, and at a later substep only)."""
    A, dE = PARAMS["tissue"]
    Am, dEm = PARAMS["mild"]
    n = 54
    N, U, D = states(n, 9)
    base = dict(model=CR.THREE_STATE, t_offset=273.15, nsub=1, T1=None, N=N, U=U, D=D)
    out = [dict(base, name="overflow: 95 C, dt = 300", A=A, dE=dE, dt=300.0, T0=np.full(n, 95.0)),
           dict(base, name="overflow: 120 C, dt = 1e6", A=A, dE=dE, dt=1e6, T0=np.full(n, 120.0)),
           dict(base, name="overflow: rate dt = inf", A=(3.0, 0.0, 3.0), dE=(0.0, 0.0, 0.0), dt=1e308,
                T0=np.full(n, 50.0)),
           dict(base, name="underflow: T_K = 1", A=A, dE=dE, dt=300.0, T0=np.full(n, 1.0), t_offset=0.0),
           dict(base, name="double eigenvalue: a = c, b = 0", A=(3.0, 0.0, 3.0), dE=(0.0, 0.0, 0.0), dt=0.5,
                T0=np.full(n, 50.0)),
           dict(base, name="double eigenvalue, tiny step", A=(3.0, 0.0, 3.0), dE=(0.0, 0.0, 0.0), dt=1e-7,
                T0=np.full(n, 50.0)),
           dict(base, name="dt = 0", A=Am, dE=dEm, dt=0.0, T0=np.linspace(37.0, 120.0, n))]
    bad = np.linspace(37.0, 120.0, n)
    bad[3], bad[7], bad[11], bad[20] = np.nan, -300.0, np.inf, -273.15
    out.append(dict(base, name="invalid entries", A=Am, dE=dEm, dt=1.0, T0=bad))
    T0 = np.linspace(37.0, 120.0, n)
    T1 = T0 + 5.0
    T1[3], T1[7], T1[30] = np.inf, -1000.0, np.nan   # (entry 7: T_K > 0 at the first of 4 substeps, < 0 from the second)
    out.append(dict(base, name="invalid at a substep", A=Am, dE=dEm, dt=1.0, T0=T0, T1=T1, nsub=4))
    return out


def measured_cases():
    """What c_ref and the conservation figure are measured on: the grid and the near-double-eigenvalue cases."""
    yield from grid_cases()
    yield from near_double_cases()


def tolerance(case, C):
    """Per entry: C u (1 + x_max), x_max = max_i dE_i / (R T_K) at the entry's own coldest T_K over the step (an
    invalid entry, compared bitwise elsewhere, takes T_K = 1)."""
    T0 = np.asarray(case["T0"], np.float64)
    with np.errstate(invalid="ignore"):
        TK = np.minimum(T0, case["T1"] if case["T1"] is not None else T0) + case["t_offset"]
        TK = np.where(np.isfinite(TK) & (TK > 0), TK, 1.0)
    dE = case["dE"][:1] if case["model"] == CR.ARRHENIUS else case["dE"]   # (ARRHENIUS reads dE_1 alone)
    return C * CR.U_ROUND * (1.0 + max(dE) / (CR.R_GAS * TK))
