"""CPU pin of the numpy reference behind the p-multigrid tests (tests/mg_ref.py on the cases of tests/mg_cases.py):
no GPU.  What the GPU tests hold the device to is measured here on the reference itself: the transfer's
componentwise constant against the 80-bit evaluation (C_XFER), and the spread of the fixed-work results under three
summation orders (the condition for the 1e-12 bar of tests/test_gpu_multigrid.py)."""
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import hp_ref as HP
import mg_cases as MC
import mg_ref as MR
from helpers import temperature

PAIRS = [(pc, pf) for pc in (1, 2, 3) for pf in range(pc + 1, 5)]
# the largest spread of x after six iterations (relative to max|x|) under the three summation orders, over the
# cases and both coarse solves, as measured: 4.95e-16
SPREAD_MEASURED = 4.95e-16


def _pair(mesh, pc, pf, dtype=np.float64):
    lf, hf = E.H1Space(mesh, pc), E.H1Space(mesh, pf)
    return lf, hf, MR.Transfer(lf.gather_map(), lf.ndofs, pc, hf.gather_map(), hf.ndofs, pf, dtype)


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_prolongation_reproduces_coarse_polynomials(pc, pf):
    """A polynomial of degree <= pc per variable lies in the coarse space: P of its coarse samples is its fine
    samples, up to the rounding of a few terms of size max|f|."""
    m = MC.lattice((3, 2, 2), False)
    lf, hf, T = _pair(m, pc, pf)
    f = lambda X: (1.0 + X[:, 0] ** pc) * (2.0 - X[:, 1] ** pc) * (0.5 + X[:, 2] ** pc)
    want = f(hf.dof_coords())
    err = np.abs(T.mult(f(lf.dof_coords())) - want).max()
    print(f"p {pc} -> {pf}: max error {err:.2e}")
    assert err <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_restriction_is_the_transpose(pc, pf):
    m = MC.lattice((3, 2, 2), True)
    lf, hf, T = _pair(m, pc, pf)
    rng = np.random.default_rng(2)
    x, y = rng.uniform(0, 1, lf.ndofs), rng.uniform(0, 1, hf.ndofs)
    a, b = float(T.mult(x) @ y), float(x @ T.mult_transpose(y))
    assert abs(a - b) <= 1e-14 * abs(a)
    # the mask: every fine dof is owned once, by the lowest element that holds it
    gf = hf.gather_map()
    assert T.mask.sum() == hf.ndofs
    low = np.full(hf.ndofs, gf.shape[0])
    np.minimum.at(low, gf.reshape(-1), np.repeat(np.arange(gf.shape[0]), gf.shape[1]))
    e, i = np.nonzero(T.mask)
    assert np.array_equal(low[gf[e, i]], e)


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
@pytest.mark.parametrize("term", ["diffusion", "mass"])
def test_galerkin_identity_on_a_flat_lattice(pc, pf, term):
    """Constant coefficient, flat lattice: both default rules are exact, so P^T A_f P = A_c."""
    m = MC.lattice((4, 4, 4), False)
    lf, hf, T = _pair(m, pc, pf)
    kw = {"alpha": None, "beta": 1.0} if term == "diffusion" else {"alpha": 1.0, "beta": None}
    Ac = O.OracleOperator(m.element_nodes(), lf.gather_map(), lf.ndofs, pc, **kw)
    Af = O.OracleOperator(m.element_nodes(), hf.gather_map(), hf.ndofs, pf, **kw)
    x = np.random.default_rng(4).uniform(0, 1, lf.ndofs)
    want = Ac.mult(x)
    err = np.abs(T.mult_transpose(Af.mult(T.mult(x))) - want).max()
    print(f"{term} p {pc} -> {pf}: {err:.2e} against max|A_c x| {np.abs(want).max():.3f}")
    assert err <= 1e-13 * np.abs(want).max()


def test_transfer_constant_follows_the_rule():
    """C_XFER = 4 c_ref rounded up to a power of two, c_ref the float64 restatement against the 80-bit one."""
    m = MC.lattice((3, 2, 2), True)
    worst = 0.0
    for pc, pf in PAIRS:
        lf, hf, T = _pair(m, pc, pf)
        TL = _pair(m, pc, pf, MR.LD)[2]
        xc, xf = temperature(lf.dof_coords()), temperature(hf.dof_coords())
        c1 = HP.constant(T.mult(xc), TL.mult(xc), TL.bound_mult(xc))
        c2 = HP.constant(T.mult_transpose(xf), TL.mult_transpose(xf), TL.bound_mult_transpose(xf))
        print(f"p {pc} -> {pf}: c_ref Mult {c1:.2f}, MultTranspose {c2:.2f}")
        worst = max(worst, c1, c2)
    assert MR.C_XFER == 2.0 ** math.ceil(math.log2(4.0 * worst)), worst


@pytest.mark.parametrize("name", MC.CASES)
def test_cycle_is_symmetric_with_the_smoother_as_coarse_solve(name):
    """(With an inner PCG the cycle is not a symmetric operator -- 1e-5 to 2e-2 -- which is expected and not
    asserted.)"""
    c = MC.case(name)
    rng = np.random.default_rng(3)
    u, v = rng.uniform(0, 1, c.n), rng.uniform(0, 1, c.n)
    B = c.cycle()
    fwd, tr = float(v @ B(u)), float(u @ B(v))
    print(f"{name}: {abs(fwd - tr) / abs(fwd):.2e}")
    assert abs(fwd - tr) <= 1e-13 * abs(fwd)


@pytest.mark.parametrize("name", MC.CASES)
def test_iteration_counts(name):
    c = MC.case(name)
    got = (c.solve("jacobi", rel_tol=1e-12).final_iter, c.solve("cheb", rel_tol=1e-12).final_iter,
           MC.reference(name, "mg", None, 1000).final_iter, MC.reference(name, "mg", MC.EX26_COARSE, 1000).final_iter)
    print(name, got)
    assert got[2] < got[1] < got[0] and got[3] < got[1]
    assert got == MC.COUNTS[name]


@pytest.mark.parametrize("name", MC.CASES)
def test_fixed_work_spread(name):
    """x after six iterations and one cycle's y under the three summation orders: within 1e-13 of max|x|, the
    condition for holding the device to 1e-12 (DESIGN.md section 4e's method)."""
    c = MC.case(name)
    for cp in (None, (0.0, 8)):
        xs = [c.solve("mg", cp, dot=d, rel_tol=1e-12, max_iter=6).x for d in ("matmul", "fsum", "reversed")]
        ys = [c.cycle(cp, d)(c.b) for d in ("matmul", "fsum", "reversed")]
        sx = max(np.abs(xs[0] - a).max() for a in xs[1:]) / np.abs(xs[0]).max()
        sy = max(np.abs(ys[0] - a).max() for a in ys[1:]) / np.abs(ys[0]).max()
        print(f"{name} coarse {cp}: spread of x {sx:.2e}, of the cycle's y {sy:.2e}")
        assert sx <= 1e-13 and sy <= 1e-13   # (measured: SPREAD_MEASURED)
