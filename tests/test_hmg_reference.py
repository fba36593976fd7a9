"""CPU pin of the numpy reference behind the h-multigrid tests (tests/hmg_ref.py on the cases of tests/hmg_cases.py):
no GPU.  What the GPU tests hold the device to is measured here on the reference itself: the transfer's
componentwise constant against the 80-bit evaluation (C_HXFER), and the spread of the fixed-work results under three
summation orders (the condition for the 1e-12 bar of tests/test_gpu_hmultigrid.py)."""
import math

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import hmg_cases as HC
import hmg_ref as HR
import hp_ref as HP
import mg_cases as MC

ORDERS = (1, 2, 3, 4)
# the smallest nonzero magnitude in the 1D tables (transfer.hpp's argument for thresholding them)
MIN_NONZERO = {1: 0.5, 2: 0.125, 3: 0.0559, 4: 0.0319}
# the largest spread of x after six iterations and of one cycle's y (relative to the max) under the three summation
# orders, as measured
SPREAD_MEASURED = 3.58e-16


@pytest.mark.parametrize("p", ORDERS)
def test_dense_local_matrices_equal_the_tensor_form(p):
    """The reference's thresholded D^3 x D^3 matrices against B_oz (x) B_oy (x) B_ox of the thresholded 1D tables: the
    same zeros, 1 ulp elsewhere (the product's association), rows summing to 1; and the figures behind it."""
    s = np.abs(HR.shape1d(p))
    small, big = s[s < HR.ZERO], s[s >= HR.ZERO]
    print(f"p {p}: largest residue {small.max() if small.size else 0.0:.1e}, smallest nonzero {big.min():.4f}")
    assert (small.max() if small.size else 0.0) <= 1e-15 and big.max() <= 1.0
    assert MIN_NONZERO[p] <= big.min() < MIN_NONZERO[p] * 1.01 and big.min() ** 3 > HR.ZERO
    for o in range(8):
        A, B = HR.local_matrix(p, o), HR.tensor_matrix(p, o)
        assert np.array_equal(A == 0, B == 0)
        nz = A != 0
        assert np.all(np.abs(A - B)[nz] <= np.spacing(np.abs(A[nz])))
        assert np.abs(A.sum(1) - 1.0).max() <= 1e-14
        # the 80-bit matrices have the same zeros
        assert np.array_equal(HR.local_matrix(p, o, HR.LD) == 0, A == 0)


@pytest.mark.parametrize("p", ORDERS)
def test_prolongation_reproduces_coarse_polynomials(p):
    """x^a y^b z^c with a, b, c <= p lies in the coarse space of a flat Cartesian mesh: P of its coarse nodal values
    is its fine nodal values."""
    m = MC.lattice((3, 2, 2), False)
    f = HC.refined(m)
    lf, hf = E.H1Space(m, p), E.H1Space(f, p)
    parent, octant = m.refinement_embedding()
    T = HR.HTransfer(lf.gather_map(), lf.ndofs, hf.gather_map(), hf.ndofs, p, parent, octant)
    Xc, Xf = lf.dof_coords(), hf.dof_coords()
    worst = 0.0
    for a in range(p + 1):
        for b in range(p + 1):
            for c in range(p + 1):
                fn = lambda X: X[:, 0] ** a * X[:, 1] ** b * X[:, 2] ** c
                worst = max(worst, np.abs(T.mult(fn(Xc)) - fn(Xf)).max())
    print(f"p {p}: max error {worst:.2e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("name,p", [("moved322", 1), ("moved322", 3), ("fichera", 2), ("struct433", 2)])
def test_restriction_is_the_transpose(name, p):
    P = HC.pair(name, p)
    T = P.ref()
    rng = np.random.default_rng(2)
    x, y = rng.uniform(0, 1, P.lf.ndofs), rng.uniform(0, 1, P.hf.ndofs)
    a, b = float(T.mult(x) @ y), float(x @ T.mult_transpose(y))
    assert abs(a - b) <= 1e-14 * abs(a)


@pytest.mark.parametrize("p", (1, 2))
def test_galerkin_identity_on_a_flat_lattice(p):
    """Constant coefficient, flat lattice: the default rules are exact, so P^T A_f P = A_c."""
    m = MC.lattice((3, 3, 2), False)
    f = HC.refined(m)
    lf, hf = E.H1Space(m, p), E.H1Space(f, p)
    parent, octant = m.refinement_embedding()
    T = HR.HTransfer(lf.gather_map(), lf.ndofs, hf.gather_map(), hf.ndofs, p, parent, octant)
    Ac = O.OracleOperator(m.element_nodes(), lf.gather_map(), lf.ndofs, p, alpha=1.0, beta=1.0)
    Af = O.OracleOperator(f.element_nodes(), hf.gather_map(), hf.ndofs, p, alpha=1.0, beta=1.0)
    x = np.random.default_rng(4).uniform(0, 1, lf.ndofs)
    want = Ac.mult(x)
    err = np.abs(T.mult_transpose(Af.mult(T.mult(x))) - want).max()
    print(f"p {p}: {err:.2e} against max|A_c x| {np.abs(want).max():.3f}")
    assert err <= 1e-13 * np.abs(want).max()


def test_transfer_constant_follows_the_rule():
    """C_HXFER = 4 c_ref rounded up to a power of two, c_ref the float64 restatement against the 80-bit one over the
    transfer cases."""
    worst = 0.0
    for name, p in HC.TRANSFER_CASES:
        P = HC.pair(name, p)
        T, TL = P.ref(), P.ref(HR.LD)
        for kind, (xc, xf) in P.inputs.items():
            c1 = HP.constant(T.mult(xc), TL.mult(xc), TL.bound_mult(xc))
            c2 = HP.constant(T.mult_transpose(xf), TL.mult_transpose(xf), TL.bound_mult_transpose(xf))
            print(f"{name} p {p} {kind}: c_ref Mult {c1:.2f}, MultTranspose {c2:.2f}")
            worst = max(worst, c1, c2)
    assert HR.C_HXFER == 2.0 ** math.ceil(math.log2(4.0 * worst)), worst


@pytest.mark.parametrize("name", HC.H_CASES)
def test_cycle_is_symmetric(name):
    c = HC.hcase(name)
    rng = np.random.default_rng(3)
    u, v = rng.uniform(0, 1, c.n), rng.uniform(0, 1, c.n)
    B = c.cycle()
    fwd, tr = float(v @ B(u)), float(u @ B(v))
    print(f"{name}: {abs(fwd - tr) / abs(fwd):.2e}")
    assert abs(fwd - tr) <= 1e-13 * abs(fwd)


@pytest.mark.parametrize("name", HC.H_CASES)
def test_iteration_counts(name):
    c = HC.hcase(name)
    got = (c.solve("jacobi", rel_tol=1e-12).final_iter, c.solve("mg", p_only=True, rel_tol=1e-12).final_iter,
           HC.reference(name, 1000).final_iter)
    print(name, got)
    assert got[2] <= got[1] < got[0]
    assert got == HC.COUNTS[name]


@pytest.mark.parametrize("name", HC.H_CASES)
def test_fixed_work_spread(name):
    """x after six iterations and one cycle's y under the three summation orders: within 1e-14 of the max, 100 x
    below the 1e-12 the device is held to (hmg_ref.CYCLE_TOL)."""
    c = HC.hcase(name)
    for cp in (None, (0.0, 8)):
        xs = [c.solve("mg", coarse_pcg=cp, dot=d, rel_tol=1e-12, max_iter=6).x for d in ("matmul", "fsum", "reversed")]
        ys = [c.cycle(False, cp, d)(c.b) for d in ("matmul", "fsum", "reversed")]
        sx = max(np.abs(xs[0] - a).max() for a in xs[1:]) / np.abs(xs[0]).max()
        sy = max(np.abs(ys[0] - a).max() for a in ys[1:]) / np.abs(ys[0]).max()
        print(f"{name} coarse {cp}: spread of x {sx:.2e}, of the cycle's y {sy:.2e}")
        assert max(sx, sy) * 100.0 <= HR.CYCLE_TOL   # (measured: SPREAD_MEASURED)
