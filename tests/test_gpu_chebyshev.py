"""GPU tests of the device Chebyshev smoother (ChebyshevSmoother / ecm2_chebyshev_*: OperatorChebyshevSmoother,
linalg/solvers.cpp:455-658), of its power method (power_method / ecm2_power_method: PowerMethod::
EstimateLargestEigenvalue, linalg/operator.cpp:871-928) and of the PCG it preconditions (Operator.PCG(prec=) /
ecm2_operator_pcg_prec: CGSolver::Mult, linalg/solvers.cpp:869-1004, in the fused passes of csrc/k_cheb.hip)
against the numpy restatement tests/cheb_ref.py on the cases of tests/cheb_cases.py -- whose self-gap under
three summation orders (tests/test_cheb_reference.py: <= 1e-14 of max|x|, equal iteration counts) is the
condition under which the project's 1e-12 bar may be applied to x after a fixed number of iterations.
Every output is preset to NaN."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import bicgstab_cases as BC
import cheb_cases as CC
import cheb_ref as CR
from helpers import coeff_function, nonaligned, relerr

pytestmark = pytest.mark.gpu

_DEV, _SM = {}, {}
ERR_ARG, ERR_UNSUPPORTED, ERR_NUMERIC = 1, 5, 8


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _device(name):
    """(case, Operator, b, ess) on the device, built once per case; ess None without essential dofs."""
    import torch
    if name not in _DEV:
        c = CC.case(name)
        ess = torch.as_tensor(c.ess).cuda() if c.ess.size else None
        _DEV[name] = (c, E.Operator(c.device_form()), torch.as_tensor(c.b).cuda(), ess)
    return _DEV[name]


def _smoother(name, order):
    """The device smoother with max_eig passed in from the reference's power method, built once."""
    if (name, order) not in _SM:
        c, A, b, ess = _device(name)
        _SM[name, order] = E.ChebyshevSmoother(A, ess=ess, order=order, max_eig_estimate=c.max_eig)
    return _SM[name, order]


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


@pytest.mark.parametrize("name", CC.ALL)
def test_smoother_mult_matches_reference(name):
    """Random x (non-cancelling: U[0, 1)), orders 1..5: y to the project's RTOL; two calls bitwise equal."""
    import torch
    c, A, b, ess = _device(name)
    xh = np.random.default_rng(5).uniform(0.0, 1.0, c.n)
    x = torch.as_tensor(xh).cuda()
    for order in CC.ORDERS:
        S = _smoother(name, order)
        assert S.order == order and S.power_steps == 0 and S.max_eig == c.max_eig
        want_c = CR.coefficients(order, c.max_eig)
        assert S.coeffs.shape == (order,) and np.abs(S.coeffs / want_c - 1.0).max() <= 1e-15
        y, y2 = _nan(c.n), _nan(c.n)
        S.Mult(x, y)
        S.Mult(x, y2)
        err = relerr(y.cpu().numpy(), c.smoother(order)(xh))
        print(f"{name} order {order}: relerr(y) {err:.2e}")
        assert err <= helpers.RTOL
        assert torch.equal(y, y2)
        assert torch.equal(x.cpu(), torch.as_tensor(xh))  # (the constrained Mult restores its input)


@pytest.mark.parametrize("name", CC.SYM)
def test_smoother_is_symmetric(name):
    """tests/unit/linalg/test_chebyshev.cpp: cheb order 2 with the power method's estimate,
    |l^T S r - r^T S l| / |l^T S r| < 1e-13."""
    import torch
    c, A, b, ess = _device(name)
    S = E.ChebyshevSmoother(A, ess=ess, order=2)
    assert S.power_steps > 0
    rng = np.random.default_rng(3)
    left, right = torch.as_tensor(rng.uniform(0, 1, c.n)).cuda(), torch.as_tensor(rng.uniform(0, 1, c.n)).cuda()
    y = _nan(c.n)
    S.Mult(right, y)
    fwd = float(left @ y)
    S.Mult(left, y)
    tr = float(right @ y)
    err = abs(fwd - tr) / abs(fwd)
    print(f"{name}: max_eig {S.max_eig:.6f} ({S.power_steps} steps), symmetry {err:.2e}")
    assert err < 1e-13


@pytest.mark.parametrize("name", ["k2", "k3", "mk2_free"])
def test_power_method_matches_reference(name):
    """The reference's start vector, its default 10 steps and tolerance: eig to 1e-12, all 10 steps."""
    import torch
    c, A, b, ess = _device(name)
    ref = c.power()
    assert ref.steps == 10
    v0 = torch.as_tensor(c.v0).cuda()
    eig, steps = E.power_method(A, v0, ess=ess)
    err_v = relerr(v0.cpu().numpy(), ref.v)
    print(f"{name}: eig {eig:.15f} (reference {ref.eig:.15f}), steps {steps}, last iterate {err_v:.2e}")
    assert steps == 10
    assert abs(eig - ref.eig) <= 1e-12 * abs(ref.eig)
    assert err_v <= 1e-12
    # the smoother's constructor runs the same estimate
    S = E.ChebyshevSmoother(A, ess=ess, order=3, v0=torch.as_tensor(c.v0).cuda())
    assert S.power_steps == 10 and S.max_eig == eig


def test_power_method_breaks_early():
    """sym2 with tol = 0.1: the reference breaks at step 3 (diffs 0.28, 0.39, 0.023), none of them within a
    factor 2 of the tolerance, so the device breaks at the same step."""
    import torch
    c, A, b, ess = _device("sym2")
    tol = 0.1
    ref = CR.power_method(c.mult, c.dinv, c.ess, c.v0, 10, tol)
    print(ref.diffs)
    assert all(d < tol / 2 or d > 2 * tol for d in ref.diffs) and ref.steps < 10
    eig, steps = E.power_method(A, torch.as_tensor(c.v0).cuda(), ess=ess, tol=tol)
    assert steps == ref.steps
    assert abs(eig - ref.eig) <= 1e-12 * abs(ref.eig)


def test_power_method_default_start_vector():
    c, A, b, ess = _device("k2")
    S1 = E.ChebyshevSmoother(A, ess=ess, order=2)
    S2 = E.ChebyshevSmoother(A, ess=ess, order=2)
    eig, steps = E.power_method(A, None, ess=ess)
    print(f"k2: max_eig {S1.max_eig:.15f} from the library's start vector ({S1.power_steps} steps)")
    assert S1.max_eig == S2.max_eig == eig and S1.power_steps == S2.power_steps == steps
    assert 0.5 < S1.max_eig < 4.0


@pytest.mark.parametrize("name", CC.ALL)
def test_pcg_fixed_work_matches_reference(name):
    """Six iterations (max_iter = 6: not converged), the same work as the reference's: x to 1e-12."""
    c, A, b, ess = _device(name)
    for order in (1, 2, 4):
        ref = CC.reference(name, order, 6)
        assert ref.final_iter == 6 and not ref.converged
        x = _nan(c.n)
        it, nrm = A.PCG(b, x, ess=ess, rel_tol=1e-12, max_iter=6, prec=_smoother(name, order))
        err = relerr(x.cpu().numpy(), ref.x)
        print(f"{name} order {order}: iterations {it}, final_norm {nrm:.3e} (reference {ref.final_norm:.3e}), "
              f"relerr(x) {err:.2e}")
        assert it == 6 and not E.pcg_last_converged()
        assert err <= 1e-12


@pytest.mark.parametrize("name", CC.ALL)
def test_pcg_converged_matches_reference(name):
    c, A, b, ess = _device(name)
    for order in (1, 2, 4):
        ref = CC.reference(name, order, 1000)
        assert ref.converged
        x = _nan(c.n)
        it, nrm = A.PCG(b, x, ess=ess, rel_tol=1e-12, max_iter=1000, prec=_smoother(name, order))
        xh = x.cpu().numpy()
        res_dev, res_ref = c.true_residual(xh), c.true_residual(ref.x)
        err = relerr(xh, ref.x)
        print(f"{name} order {order}: iterations {it} (reference {ref.final_iter}), final_norm {nrm:.3e}, true residual "
              f"{res_dev:.2e} (reference {res_ref:.2e}), relerr(x) {err:.2e}")
        assert E.pcg_last_converged()
        assert abs(it - ref.final_iter) <= 1
        assert res_dev <= 4.0 * res_ref
        assert err <= 1e-10


@pytest.mark.parametrize("name", CC.ALL)
def test_order_1_and_2_against_jacobi_pcg(name):
    """Order 1 is Jacobi scaled by 1 / theta: iteration counts within 1 and the same x; order 2 needs <= 0.65
    of Jacobi's iterations."""
    c, A, b, ess = _device(name)
    xj, x1, x2 = _nan(c.n), _nan(c.n), _nan(c.n)
    itj, _ = A.PCG(b, xj, ess=ess, rel_tol=1e-12, max_iter=1000, jacobi=True)
    assert E.pcg_last_converged()
    it1, _ = A.PCG(b, x1, ess=ess, rel_tol=1e-12, max_iter=1000, prec=_smoother(name, 1))
    assert E.pcg_last_converged()
    it2, _ = A.PCG(b, x2, ess=ess, rel_tol=1e-12, max_iter=1000, prec=_smoother(name, 2))
    assert E.pcg_last_converged()
    err = relerr(x1.cpu().numpy(), xj.cpu().numpy())
    print(f"{name}: Jacobi {itj}, order 1 {it1} (relerr(x) {err:.2e}), order 2 {it2}")
    assert abs(it1 - itj) <= 1 and err <= 1e-10
    assert it2 <= 0.65 * itj


def test_stops():
    import torch
    c, A, b, ess = _device("k2")
    n = c.n
    S = _smoother("k2", 2)
    # b = 0: nom = 0 <= r0, 0 iterations, converged, x = 0
    x = _nan(n)
    it, nrm = A.PCG(torch.zeros_like(b), x, ess=ess, prec=S)
    assert (it, nrm) == (0, 0.0) and E.pcg_last_converged() and not x.any()
    # every dof essential: the constrained operator is the identity, the smoother a multiple of it -- x = b after
    # one iteration (up to the rounding of alpha (s b) with alpha = 1 / s)
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    Se = E.ChebyshevSmoother(A, ess=every, order=2)
    assert abs(Se.max_eig - 1.0) <= 1e-14 and Se.power_steps == 1
    x = _nan(n)
    it, nrm = A.PCG(b, x, ess=every, prec=Se)
    assert it == 1 and E.pcg_last_converged()
    assert relerr(x.cpu().numpy(), c.b) <= 1e-14
    # an estimate far too small: (B b, b) < 0, the solve stops before the loop
    small = c.max_eig / 8.0
    for order in (2, 4):
        ref = c.solve(order, max_eig=small, rel_tol=1e-12)
        assert ref.stop == "neg0" and ref.final_norm < 0
        Sn = E.ChebyshevSmoother(A, ess=ess, order=order, max_eig_estimate=small)
        x = _nan(n)
        it, nrm = A.PCG(b, x, ess=ess, rel_tol=1e-12, prec=Sn)
        print(f"order {order}: nom {nrm:.6f} (reference {ref.final_norm:.6f})")
        assert it == 0 and not E.pcg_last_converged()
        assert nrm < 0 and abs(nrm - ref.final_norm) <= 1e-12 * abs(ref.final_norm)
    # max_iter = 1
    x = _nan(n)
    it, nrm = A.PCG(b, x, ess=ess, max_iter=1, prec=S)
    ref = c.solve(2, rel_tol=1e-12, max_iter=1)
    assert it == 1 and not E.pcg_last_converged()
    assert relerr(x.cpu().numpy(), ref.x) <= 1e-12 and abs(nrm - ref.final_norm) <= 1e-10 * ref.final_norm


def test_nonfinite_is_numeric_error_and_the_next_solve_works():
    c, A, b, ess = _device("k2")
    S = _smoother("k2", 2)
    ref = CC.reference("k2", 2, 1000)
    x = _nan(c.n)
    bad = b.clone()
    bad[c.n // 2] = float("nan")
    assert _code(lambda: A.PCG(bad, x, ess=ess, prec=S)) == ERR_NUMERIC
    assert not E.pcg_last_converged()
    it, _ = A.PCG(b, x, ess=ess, rel_tol=1e-12, prec=S)
    assert E.pcg_last_converged() and abs(it - ref.final_iter) <= 1
    assert relerr(x.cpu().numpy(), ref.x) <= 1e-10


def test_refusals():
    import torch
    c, A, b, ess = _device("k2")
    n = c.n
    S = _smoother("k2", 2)
    # a misaligned x (a view at an odd element offset), before anything is enqueued
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    assert _code(lambda: A.PCG(b, buf[1:], ess=ess, prec=S)) == ERR_ARG
    assert not buf.any()
    assert _code(lambda: S.Mult(b, buf[1:])) == ERR_ARG
    assert not buf.any()
    # a smoother of another size
    S3 = _smoother("k3", 2)
    assert S3.size != n
    assert _code(lambda: A.PCG(b, _nan(n), ess=ess, prec=S3)) == ERR_ARG
    # a diagonal's operator of another size; orders outside 1..5
    assert _code(lambda: E.ChebyshevSmoother(A, ess=ess, order=2, max_eig_estimate=1.5, diag_of=_device("k3")[1])) == ERR_ARG
    for order in (0, 6):
        assert _code(lambda: E.ChebyshevSmoother(A, ess=ess, order=order, max_eig_estimate=1.5)) == ERR_ARG
        assert _code(lambda: E.ChebyshevSmoother(A, ess=ess, order=order)) == ERR_ARG
    # prec and the BiCGSTAB stage solver exclude each other
    with pytest.raises(E.ECM2Error):
        E.ode_step(E.ODE_SDIRK33, A, A, 0.05, _nan(n), ess=ess, solver="bicgstab", prec=S)
    # operators whose dots need communication: a member of a loopback group (contiguous sends: z slabs of the
    # lattice numbering)
    m = E.Mesh.MakeCartesian3D(4, 4, 8)
    fes_s = E.H1Space(m, 2, E.NUMBERING_STRUCTURED)
    er = E.partition_slabs_z(m, 2)
    forms = []
    for r in range(2):
        f = E.ParBilinearForm(E.Partition(fes_s, er, r, 2, decomposition="overlap"))
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.Assemble()
        forms.append(f)
    member = E.Operator(E.ParGroup(forms), member=0)
    assert _code(lambda: E.ChebyshevSmoother(member, order=2)) == ERR_UNSUPPORTED
    assert _code(lambda: E.ChebyshevSmoother(member, order=2, max_eig_estimate=1.5)) == ERR_UNSUPPORTED
    assert _code(lambda: E.power_method(member, None)) == ERR_UNSUPPORTED
    # ... and the PCG's own refusal, with a serial smoother of the member's size (a p = 1 lattice of as many dofs)
    dims = next((i, j, k) for i in range(1, 33) for j in range(1, 33) for k in range(1, 33)
                if (i + 1) * (j + 1) * (k + 1) == member.size)
    sf = E.BilinearForm(E.H1Space(E.Mesh.MakeCartesian3D(*dims), 1))
    sf.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    sf.Assemble()
    Sm = E.ChebyshevSmoother(E.Operator(sf), order=2, max_eig_estimate=1.5)
    assert Sm.size == member.size
    bm = torch.ones(member.size, dtype=torch.float64, device="cuda")
    xm = _nan(member.size)
    assert _code(lambda: member.PCG(bm, xm, prec=Sm)) == ERR_UNSUPPORTED
    assert bool(torch.isnan(xm).all())
    # a misaligned start vector of the power method, before anything is enqueued
    vbuf = torch.ones(n + 1, dtype=torch.float64, device="cuda")
    assert _code(lambda: E.power_method(A, vbuf[1:], ess=ess)) == ERR_ARG
    assert _code(lambda: E.ChebyshevSmoother(A, ess=ess, order=2, v0=vbuf[1:])) == ERR_ARG
    assert bool((vbuf == 1.0).all())
    # an estimate that is zero or not finite
    for bad in (0.0, float("inf"), float("nan")):
        assert _code(lambda: E.ChebyshevSmoother(A, ess=ess, order=2, max_eig_estimate=bad)) == ERR_ARG


def test_two_solves_are_bitwise_equal():
    import torch
    c, A, b, ess = _device("k3")
    S = _smoother("k3", 3)
    outs = []
    for _ in range(2):
        x = _nan(c.n)
        outs.append((A.PCG(b, x, ess=ess, rel_tol=1e-12, prec=S), x))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])


def test_loopback_group_agrees_with_serial():
    """Two z-slabs, 4 x 4 x 8, p = 2: Chebyshev-PCG through Operator(group), whose dots over the concatenated
    true vectors are already global, against the serial solve to 1e-10."""
    import torch
    m = E.Mesh.MakeCartesian3D(4, 4, 8)
    m.set_vertices(nonaligned(m.vertices()))
    fes = E.H1Space(m, 2)
    q1d = O.default_q1d(2)

    def add(form, ne, P):
        form.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(torch.as_tensor(BC.alpha_fn(P).reshape(ne, -1)).cuda())))
        form.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(
            torch.as_tensor(0.05 * coeff_function(P).reshape(ne, -1)).cuda())))
        form.Assemble()
        return form
    serial = add(E.BilinearForm(fes), fes.ne, O.quad_points(m.element_nodes(), q1d))
    er = E.partition_slabs_z(m, 2)
    forms, parts = [], []
    for r in range(2):
        part = E.Partition(fes, er, r, 2)
        forms.append(add(E.ParBilinearForm(part), part.ne_local, E.quadrature_points_subset(m, q1d, part.elems)))
        parts.append(part)
    n = fes.ndofs
    ess = np.asarray(fes.boundary_dofs())
    b = np.random.default_rng(4).uniform(0, 1, n)
    ops = E.Operator(serial)
    essd = torch.as_tensor(ess).cuda()
    xs = _nan(n)
    Ss = E.ChebyshevSmoother(ops, ess=essd, order=2)
    its, _ = ops.PCG(torch.as_tensor(b).cuda(), xs, ess=essd, rel_tol=1e-13, max_iter=2000, prec=Ss)
    assert E.pcg_last_converged()
    opg = E.Operator(E.ParGroup(forms))
    assert opg.size == n
    perm = np.concatenate([p.owned_global for p in parts])
    idx, o = [], 0
    for p in parts:
        idx.append(np.nonzero(np.isin(p.owned_global, ess))[0] + o)
        o += p.n_owned
    essg = torch.as_tensor(np.concatenate(idx).astype(np.int32)).cuda()
    xg = _nan(n)
    # (the library's start vector is a hash of the index, and the group numbers the dofs differently: the same
    # estimate for both, so that the two solves do the same work; the group's own estimate is checked beside it)
    Sg = E.ChebyshevSmoother(opg, ess=essg, order=2, max_eig_estimate=Ss.max_eig)
    eig_g, steps_g = E.power_method(opg, None, ess=essg)
    assert 0.5 < eig_g < 4.0 and 0.5 < Ss.max_eig < 4.0
    itg, _ = opg.PCG(torch.as_tensor(b[perm]).cuda(), xg, ess=essg, rel_tol=1e-13, max_iter=2000, prec=Sg)
    assert E.pcg_last_converged()
    err = relerr(xg.cpu().numpy(), xs.cpu().numpy()[perm])
    print(f"serial {its} iterations (max_eig {Ss.max_eig:.6f}), group {itg} (max_eig {Sg.max_eig:.6f}), relerr(x) {err:.2e}")
    assert 0 < itg < 200 and abs(itg - its) <= 1
    assert err <= 1e-10


def test_ode_step_with_the_smoother():
    """One SDIRK33 step on mk2's mesh and coefficients, rel_tol 1e-12, with prec against the same step with
    jacobi=True: both converge the same three systems (condition number x tolerance stays below 1e-9), and the
    smoother needs fewer iterations in total."""
    import torch
    c = CC.case("mk2")
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    ne, dt = c.fes.ne, 0.05
    cdt = E.ode_implicit_coeff(E.ODE_SDIRK33) * dt
    T, K = E.BilinearForm(c.fes), E.BilinearForm(c.fes)
    T.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(dev(c.alpha.reshape(ne, -1)))))
    T.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(dev(cdt * BC.beta_fn(c.P).reshape(ne, -1)))))
    K.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(dev(BC.beta_fn(c.P).reshape(ne, -1)))))
    T.Assemble()
    K.Assemble()
    Top, Kop = E.Operator(T), E.Operator(K)
    ess = dev(c.ess)
    u0 = np.random.default_rng(8).uniform(0.0, 1.0, c.n)
    uj, uc = dev(u0), dev(u0)
    sj, itj, cj = E.ode_step(E.ODE_SDIRK33, Top, Kop, dt, uj, ess=ess, rel_tol=1e-12, max_iter=1000, jacobi=True)
    S = E.ChebyshevSmoother(Top, ess=ess, order=2)
    sc, itc, cc = E.ode_step(E.ODE_SDIRK33, Top, Kop, dt, uc, ess=ess, rel_tol=1e-12, max_iter=1000, prec=S)
    err = relerr(uc.cpu().numpy(), uj.cpu().numpy())
    print(f"SDIRK33: Jacobi {itj} iterations, Chebyshev order 2 {itc}, relerr(u) {err:.2e}")
    assert (sj, cj) == (3, True) and (sc, cc) == (3, True)
    assert itc < itj
    assert err <= 1e-9
    assert not np.array_equal(uj.cpu().numpy(), u0)
