"""GPU tests of the cell-death state (CellDeath.Step / .Measure, csrc/k_celldeath.hip) against the 80-bit
restatement tests/celldeath_ref.py, on tests/celldeath_cases.py's matrix.

Sizes: 1, 2, 3 (the odd tail), 511 (less than a workgroup's chunk), 2047 / 2048 / 2049 (either side of a
chunk of 1,024 pairs) and 100003 (many chunks and a tail).  Every size runs the twelve (dt, schedule) pairs --
dt in {1e-3, 1, 300}, T1 absent / present, nsub in {1, 4} -- with the parameter set and the unit (Celsius /
kelvin) alternating, shifted by the size's index, so that the sizes together cover every combination.
Bounds: test_celldeath_reference.py's C_CD / C_CD_ARRHENIUS (state, per entry at its own T_K) and C_SUM
(conservation), derived there from the float64 numpy restatement, never from the device; the exact conditions (D never decreases, fractions >= 0, zero-rate and invalid
entries bitwise untouched) are asserted as such.  Measure: |s - s_hp| <= (d + 1) u sum |terms| with d the depth
of the kernel's summation tree, read from its design (measure_depth below)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers  # noqa: F401
import ecm2_amd as E
import celldeath_cases as CC
import celldeath_ref as CR
from test_celldeath_reference import C_SUM, c_cd

pytestmark = pytest.mark.gpu
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.int64)


@functools.lru_cache(maxsize=None)
def inputs(n, kelvin, model=CR.THREE_STATE):
    T0, T1 = CC.temperatures(n, 21, kelvin)
    return (T0, T1) + CC.states(n, 17, model)


def combos(n):
    shift = CC.SIZES.index(n) if n in CC.SIZES else 0
    sets = ("tissue", "mild")
    for i, (dt, (with_T1, nsub)) in enumerate(itertools.product(CC.GPU_DTS, CC.SCHEDULES)):
        yield sets[(i + shift) % 2], bool(((i + shift) // 2) % 2), dt, with_T1, nsub


def run_step(model, A, dE, kelvin, T0, T1, dt, nsub, N, U, D, check=True):
    cd = E.CellDeath(model, A, dE, T0.size, t_offset=0.0 if kelvin else 273.15)
    n_, u_, d_ = dev(N), dev(U), dev(D)
    bad = cd.Step(dev(T0), dt, n_, u_, d_, T1=dev(T1) if T1 is not None else None, nsub=nsub, check=check)
    torch.cuda.synchronize()
    return n_.cpu().numpy(), u_.cpu().numpy(), d_.cpu().numpy(), bad


def compare(case, got, hp, name):
    C = c_cd(case["model"])
    tol = CC.tolerance(case, C)      # per entry, at the entry's own T_K
    worst = 0.0
    for X, g, h in zip("NUD", got, hp):
        assert np.isfinite(g).all(), (name, X)
        scale = np.maximum(1.0, np.abs(h)) if (case["model"] == CR.ARRHENIUS and X == "U") else 1.0
        e = float((np.abs(g.astype(LD) - h) / scale / tol).max())
        worst = max(worst, e * C)
        assert e <= 1.0, (name, X, e * C, C)
    return worst


@pytest.mark.parametrize("n", CC.SIZES)
def test_step_against_reference(n):
    worst = 0.0
    for name, kelvin, dt, with_T1, nsub in combos(n):
        A, dE = CC.PARAMS[name]
        T0, T1, N, U, D = inputs(n, kelvin)
        T1 = T1 if with_T1 else None
        case = dict(model=CR.THREE_STATE, A=A, dE=dE, t_offset=0.0 if kelvin else 273.15, T0=T0, T1=T1)
        tag = f"n={n} {name} dt={dt} T1={int(with_T1)} nsub={nsub} {'K' if kelvin else 'C'}"
        gn, gu, gd, bad = run_step(CR.THREE_STATE, A, dE, kelvin, T0, T1, dt, nsub, N, U, D)
        assert bad == 0, tag
        hp = CR.step(CR.THREE_STATE, A, dE, case["t_offset"], T0, T1, dt, nsub, N, U, D)
        worst = max(worst, compare(case, (gn, gu, gd), hp, tag))
        assert (gd >= D).all(), tag                                         # monotone death, exactly
        assert (gn >= 0).all() and (gu >= 0).all() and (gn <= 1).all() and (gu <= 1).all() and (gd <= 1).all(), tag
        grow = np.abs(gn + gu + gd - 1.0) - np.abs(N + U + D - 1.0)
        assert (grow <= C_SUM * CR.U_ROUND * nsub).all(), (tag, float(grow.max()) / CR.U_ROUND)
    print(f"n={n}: worst state error {worst:.3f} u (1 + x_max), bound {c_cd(CR.THREE_STATE)}")


@pytest.mark.parametrize("n", (3, 2049))
def test_arrhenius_against_reference(n):
    for name, kelvin, dt, with_T1, nsub in combos(n):
        A, dE = CC.PARAMS[name]
        T0, T1, N, U, D = inputs(n, kelvin, CR.ARRHENIUS)
        T1 = T1 if with_T1 else None
        case = dict(model=CR.ARRHENIUS, A=A, dE=dE, t_offset=0.0 if kelvin else 273.15, T0=T0, T1=T1)
        got = run_step(CR.ARRHENIUS, A, dE, kelvin, T0, T1, dt, nsub, N, U, D)
        assert got[3] == 0
        hp = CR.step(CR.ARRHENIUS, A, dE, case["t_offset"], T0, T1, dt, nsub, N, U, D)
        compare(case, got[:3], hp, f"arrhenius n={n} {name} dt={dt}")
        assert (got[2] >= D).all() and (got[1] >= U).all()


def test_near_double_eigenvalue():
    """b = 0 with |a - c| / a down to 1e-12 and a = c with b / a = 1e-14 at |lambda dt| about 1: the divided
    difference over 2 delta would lose u / (2 delta dt) in D and in N + U + D here."""
    worst = 0.0
    for c in CC.near_double_cases():
        got = run_step(c["model"], c["A"], c["dE"], False, c["T0"], None, c["dt"], c["nsub"], c["N"], c["U"], c["D"])
        assert got[3] == 0
        hp = CR.step(c["model"], c["A"], c["dE"], 273.15, c["T0"], None, c["dt"], c["nsub"], c["N"], c["U"], c["D"])
        worst = max(worst, compare(c, got[:3], hp, c["name"]))
        assert (got[2] >= c["D"]).all(), c["name"]
        grow = np.abs(got[0] + got[1] + got[2] - 1.0) - np.abs(c["N"] + c["U"] + c["D"] - 1.0)
        assert (grow <= C_SUM * CR.U_ROUND * c["nsub"]).all(), (c["name"], float(grow.max()) / CR.U_ROUND)
    print(f"near a double eigenvalue: worst state error {worst:.3f} u, bound {c_cd(CR.THREE_STATE)}")


def test_degenerate_rates():
    n = 2049
    A, dE = CC.PARAMS["mild"]
    T0, T1, N, U, D = inputs(n, False)
    # all rates zero (A = 0; T_K = 1 K: the exponentials underflow): bitwise unchanged
    for args in ((CC.zeroed(A, (0, 1, 2)), dE, False, T0), (CC.PARAMS["tissue"][0], CC.PARAMS["tissue"][1], True,
                                                            np.full(n, 1.0))):
        gn, gu, gd, bad = run_step(CR.THREE_STATE, args[0], args[1], args[2], args[3], None, 300.0, 4, N, U, D)
        assert bad == 0
        for g, old in ((gn, N), (gu, U), (gd, D)):
            assert (g.view(np.int64) == old.view(np.int64)).all()
    # every A_i = 0 in turn
    for which in ((0,), (1,), (2,)):
        Az = CC.zeroed(A, which)
        case = dict(model=CR.THREE_STATE, A=Az, dE=dE, t_offset=273.15, T0=T0, T1=T1)
        got = run_step(CR.THREE_STATE, Az, dE, False, T0, T1, 30.0, 4, N, U, D)
        assert got[3] == 0
        compare(case, got[:3], CR.step(CR.THREE_STATE, Az, dE, 273.15, T0, T1, 30.0, 4, N, U, D), f"A{which}=0")
        if which == (2,):
            assert (got[2].view(np.int64) == D.view(np.int64)).all()      # k3 = 0: nothing dies
    # 95 C, dt = 300 s: the textbook sinh form overflows here
    A, dE = CC.PARAMS["tissue"]
    hot = np.full(n, 95.0)
    got = run_step(CR.THREE_STATE, A, dE, False, hot, None, 300.0, 1, N, U, D)
    case = dict(model=CR.THREE_STATE, A=A, dE=dE, t_offset=273.15, T0=hot, T1=None)
    compare(case, got[:3], CR.step(CR.THREE_STATE, A, dE, 273.15, hot, None, 300.0, 1, N, U, D), "95 C, 300 s")
    assert got[3] == 0 and (got[2] > 0.999999).all()
    # a step whose rate * dt overflows: everything dies, nothing turns NaN
    got = run_step(CR.THREE_STATE, (3.0, 0.0, 3.0), (0.0, 0.0, 0.0), False, hot, None, 1e308, 1, N, U, D)
    assert got[3] == 0 and (got[2] > 0.999999).all() and (got[0] == 0).all() and (got[1] == 0).all()


@pytest.mark.parametrize("n", (3, 2049, 100003))
def test_invalid_entries_are_counted_and_left_untouched(n):
    A, dE = CC.PARAMS["mild"]
    T0, T1, N, U, D = inputs(n, False)
    T0, T1 = T0.copy(), T1.copy()
    where = sorted({0, n // 2, n - 1})
    T0[where[0]] = np.nan
    T0[where[-1]] = T1[where[-1]] = -300.0          # (the tail entry of an odd n)
    if len(where) == 3:
        T1[where[1]] = np.inf       # invalid through T1 alone
    for with_T1, nsub in ((False, 1), (True, 4)):
        t1 = T1 if with_T1 else None
        gn, gu, gd, bad = run_step(CR.THREE_STATE, A, dE, False, T0, t1, 1.0, nsub, N, U, D)
        hp = CR.step(CR.THREE_STATE, A, dE, 273.15, T0, t1, 1.0, nsub, N, U, D)
        mask = hp[3]
        assert bad == int(mask.sum()) and bad == (len(where) if with_T1 else 2)
        for g, old in ((gn, N), (gu, U), (gd, D)):
            assert (g[mask].view(np.int64) == old[mask].view(np.int64)).all()
        ok = ~mask
        if not ok.any():
            continue
        case = dict(model=CR.THREE_STATE, A=A, dE=dE, t_offset=273.15, T0=T0[ok], T1=t1[ok] if with_T1 else None)
        compare(case, (gn[ok], gu[ok], gd[ok]), [h[ok] for h in hp[:3]], f"neighbours n={n}")
        if n > 3:
            assert (gd[ok] > D[ok]).any()       # the neighbours were updated
    # check=False: no count, no read-back
    cd = E.CellDeath(E.CELLDEATH_THREE_STATE, A, dE, n)
    assert cd.Step(dev(T0), 1.0, dev(N), dev(U), dev(D)) is None
    torch.cuda.synchronize()


def test_two_runs_are_bitwise_equal():
    n = 100003
    A, dE = CC.PARAMS["tissue"]
    T0, T1, N, U, D = inputs(n, False)
    a = run_step(CR.THREE_STATE, A, dE, False, T0, T1, 1.0, 4, N, U, D)
    b = run_step(CR.THREE_STATE, A, dE, False, T0, T1, 1.0, 4, N, U, D)
    for x, y in zip(a[:3], b[:3]):
        assert (x.view(np.int64) == y.view(np.int64)).all()
    cd = E.CellDeath(E.CELLDEATH_THREE_STATE, A, dE, n)
    w, d = dev(np.random.default_rng(2).uniform(0.0, 1e-3, n)), dev(a[2])
    assert cd.Measure(d, w, 0.8) == cd.Measure(d, w, 0.8)


def measure_depth(n):
    """The depth of Measure's summation tree for n entries, from k_celldeath.hip and dev_common.hpp: a thread's
    chain (4 pairs = 8 terms, + the tail entry: 9), the wave's shuffle tree (6) and the workgroup's four waves (2)
    in park_partial; in the final pass a thread's chain over its share of the partials (at most
    ceil(parts / 1024) + 7: the unrolled loop's running sums, then the remainder onto the first), their pairwise
    sum (3), the shuffle tree (6), the sixteen waves in pairs (1 + 8)."""
    parts = max(1, (n // 2 + 1023) // 1024)
    return 9 + 6 + 2 + (-(-parts // 1024) + 7) + 3 + 6 + 9


@pytest.mark.parametrize("n", CC.SIZES)
def test_measure(n):
    rng = np.random.default_rng(100 + n)
    D = rng.uniform(0.0, 1.0, n)
    D[rng.uniform(size=n) < 0.2] = 0.8          # entries exactly at the threshold count
    w = rng.uniform(0.0, 2e-3, n)
    cd = E.CellDeath(E.CELLDEATH_THREE_STATE, *CC.PARAMS["mild"], n)
    got = cd.Measure(dev(D), dev(w), 0.8)
    wl, dl = w.astype(LD), D.astype(LD)
    want = ((wl * dl).sum(), wl[D >= 0.8].sum(), wl.sum())
    terms = (float((wl * dl).sum()), float(wl[D >= 0.8].sum()), float(wl.sum()))   # (all terms >= 0)
    bound = (measure_depth(n) + 1) * CR.U_ROUND
    for g, h, t in zip(got, want, terms):
        assert abs(LD(g) - h) <= bound * t, (n, g, float(h))
    assert cd.Measure(dev(D), dev(w), 2.0)[1] == 0.0 and cd.Measure(dev(D), dev(w), -1.0)[1] == got[2]


def test_argument_checks_and_identity():
    n = 2048
    A, dE = CC.PARAMS["mild"]
    T0, T1, N, U, D = inputs(n, False)
    cd = E.CellDeath(E.CELLDEATH_THREE_STATE, A, dE, n)
    assert cd.info() == {"model": 0, "n": n, "A": tuple(A), "dE": tuple(dE), "t_offset": 273.15}
    t0, t1, n_, u_, d_ = dev(T0), dev(T1), dev(N), dev(U), dev(D)
    before = [bits(v).copy() for v in (n_, u_, d_)]

    def refused(*args, **kw):
        with pytest.raises(E.ECM2Error) as ei:
            cd.Step(*args, **kw)
        assert ei.value.code == 1, ei.value           # ECM2_ERR_ARG

    refused(t0, 1.0, n_, u_, d_, nsub=0)
    refused(t0, -1.0, n_, u_, d_)
    refused(t0, float("nan"), n_, u_, d_)
    refused(t0, float("inf"), n_, u_, d_)
    refused(n_, 1.0, n_, u_, d_)                       # T0 aliases a state vector
    refused(t0, 1.0, n_, u_, d_, T1=d_)                # T1 aliases a state vector
    refused(t0, 1.0, n_, n_, d_)                       # the state vectors overlap
    # a misaligned view is refused, whichever vector it is
    cd1 = E.CellDeath(E.CELLDEATH_THREE_STATE, A, dE, n - 1)
    bufs = [dev(np.zeros(n)) for _ in range(5)]
    for k in range(5):
        v = [b[1:] if j == k else b[:n - 1] for j, b in enumerate(bufs)]
        with pytest.raises(E.ECM2Error) as ei:
            cd1.Step(v[0], 1.0, v[2], v[3], v[4], T1=v[1])
        assert ei.value.code == 1
    with pytest.raises(E.ECM2Error) as ei:
        cd1.Measure(bufs[0][1:], bufs[1][:n - 1], 0.5)
    assert ei.value.code == 1
    torch.cuda.synchronize()
    assert all((bits(v) == b).all() for v, b in zip((n_, u_, d_), before))   # nothing was enqueued
    # dt = 0 is the identity
    assert cd.Step(t0, 0.0, n_, u_, d_, T1=t1, nsub=4, check=True) == 0
    assert all((bits(v) == b).all() for v, b in zip((n_, u_, d_), before))
