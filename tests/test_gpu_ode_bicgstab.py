"""GPU tests of the implicit step with the advection inside the implicit operator (ode_step(solver="bicgstab")
/ ecm2_ode_step_bicgstab): T = M_alpha + c dt (K_beta + C), K = K_beta + C, jacobi_of = M_alpha + c dt K_beta,
the stage solves by the device BiCGSTAB -- against oracle/ode.py's step with a closure that solves with the
numpy restatement tests/bicgstab_ref.py.  The setup, the bars (increment relerr < 1e-9, essential values
bitwise, stage-solve counts) and the cases mirror
tests/test_gpu_ode_source.py::test_step_with_convection_in_K_matches_oracle, with the convection scale 20
(the scale of the solver's parity cases, tests/test_bicgstab_reference.py)."""
import ctypes

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import ode as ODE
import conv_ref as CR
import bicgstab_ref as BR
from helpers import coeff_function, nonaligned, relerr

pytestmark = pytest.mark.gpu

TYPES = [21, 22, 23, 32, 33, 34]
CONV_MARKER = [0, 1, 1]
CONV_ALPHA = 20.0
_CONV = {}


def _alpha(P):
    return 2.0 + np.sin(P[..., 0]) * np.cos(P[..., 1])


def _beta(P):
    return coeff_function(P)


def _convective(order):
    """The mesh of test_step_with_convection_in_K_matches_oracle (5 x 4 x 6, non-aligned, attributes 1 + e mod
    3) and the numpy checker of the convection term with the velocity (y, -x, x): once per order."""
    if order not in _CONV:
        m = E.Mesh.MakeCartesian3D(5, 4, 6)
        m.set_vertices(nonaligned(m.vertices()))
        m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32))
        fes = E.H1Space(m, order)
        conv = CR.ConvRef(order, O.default_q1d(order), fes.gather_map(), fes.ndofs, m.element_nodes())
        keep = CR.marker_keep(m.GetAttributes(), CONV_MARKER)
        assert 0 < keep.sum() < fes.ne
        P = O.quad_points(m.element_nodes(), O.default_q1d(order))
        _CONV[order] = (m, fes, conv, CR.reference_velocity(conv.P), keep, P)
    return _CONV[order]


def _form(fes, P, alpha_fn, scale_beta, v, conv_alpha):
    import torch
    ne = fes.ne
    f = E.BilinearForm(fes)
    if conv_alpha is not None:
        f.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(torch.as_tensor(v).cuda()), conv_alpha), CONV_MARKER)
    if alpha_fn is not None:
        f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(torch.as_tensor(alpha_fn(P).reshape(ne, -1)).cuda())))
    f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(
        torch.as_tensor(scale_beta * _beta(P).reshape(ne, -1)).cuda())))
    f.Assemble()
    return f


def _oracle(m, fes, order, P, alpha_fn, scale_beta):
    a = alpha_fn(P) if alpha_fn is not None else None
    return O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, order, alpha=a, beta=scale_beta * _beta(P))


@pytest.mark.parametrize("ode_type,order,sourced", [(t, 2, False) for t in TYPES] + [(23, 3, False), (22, 2, True)])
def test_step_with_implicit_convection_matches_oracle(ode_type, order, sourced):
    import torch
    m, fes, conv, v, keep, P = _convective(order)
    dt = 0.05
    cdt = E.ode_implicit_coeff(ode_type) * dt
    T = _form(fes, P, _alpha, cdt, v, cdt * CONV_ALPHA)
    S = _form(fes, P, _alpha, cdt, v, None)
    K = _form(fes, P, None, 1.0, v, CONV_ALPHA)
    assert T.ConvectionInfo() == (True, int(keep.sum()), True) and K.ConvectionInfo() == (True, int(keep.sum()), True)
    Sr = _oracle(m, fes, order, P, _alpha, cdt)
    Kr = _oracle(m, fes, order, P, None, 1.0)
    ess = np.asarray(fes.boundary_dofs())
    X = fes.dof_coords()
    u0 = 37.0 + 20.0 * np.exp(-4.0 * np.sum((X - 0.5) ** 2, axis=1))
    bh = _oracle(m, fes, order, P, _alpha, 0.0).mult(40.0 * np.cos(3.0 * X[:, 0])) if sourced else None
    pa_k = conv.pa_data(v, CONV_ALPHA, keep)
    pa_t = conv.pa_data(v, cdt * CONV_ALPHA, keep)
    t_mult = lambda x: Sr.mult(x) + conv.mult(v, x, keep=keep, pa=pa_t)
    dinv = BR.jacobi_vector(Sr.diagonal(), ess)

    def solve(us):
        rhs = -(Kr.mult(us) + conv.mult(v, us, keep=keep, pa=pa_k))
        if sourced:
            rhs += bh
        rhs[ess] = 0.0
        res = BR.bicgstab(t_mult, rhs, ess, dinv, rel_tol=1e-13, max_iter=5000)
        assert res.converged
        return res.x

    ur = u0.copy()
    for _ in range(2):
        ur = ODE.step(ode_type, solve, ur, dt)
    u = torch.as_tensor(u0).cuda()
    essd = torch.as_tensor(ess).cuda()
    kw = {"source": torch.as_tensor(bh).cuda()} if sourced else {}
    Top, Sop, Kop = E.Operator(T), E.Operator(S), E.Operator(K)
    iters = 0
    for _ in range(2):
        ns, it, conv_ok = E.ode_step(ode_type, Top, Kop, dt, u, ess=essd, rel_tol=1e-13, max_iter=5000, solver="bicgstab",
                                     jacobi_of=Sop, **kw)
        iters += it
        assert conv_ok and ns == {21: 1, 32: 1, 22: 2, 33: 2, 23: 3, 34: 3}[ode_type]
    uh = u.cpu().numpy()
    assert np.array_equal(uh[ess], u0[ess])
    # the implicit operator's convective share is far above the bar
    share = np.abs(conv.mult(v, u0, keep=keep, pa=pa_t)).max() / np.abs(Sr.mult(u0)).max()
    err = relerr(uh - u0, ur - u0)
    print(f"type {ode_type} p={order} source={sourced}: {err:.2e}, {iters} BiCGSTAB iterations (|c dt C u0| / |S u0| = {share:.2e})")
    assert share > 1e-3
    assert err < 1e-9


@pytest.mark.parametrize("ode_type", [21, 34])
def test_default_arguments_are_the_pcg_step_bitwise(ode_type):
    """ode_step with the default arguments == solver="pcg" spelled out == the C entry point ecm2_ode_step
    called directly: the PCG path is untouched."""
    import torch
    m, fes, conv, v, keep, P = _convective(2)
    dt = 0.05
    cdt = E.ode_implicit_coeff(ode_type) * dt
    T = E.Operator(_form(fes, P, _alpha, cdt, v, None))
    K = E.Operator(_form(fes, P, None, 1.0, v, 1.7))
    essd = torch.as_tensor(np.asarray(fes.boundary_dofs())).cuda()
    u0 = torch.as_tensor(np.random.default_rng(3).uniform(30, 40, fes.ndofs)).cuda()
    ua, ub, uc = u0.clone(), u0.clone(), u0.clone()
    ra = E.ode_step(ode_type, T, K, dt, ua, ess=essd, rel_tol=1e-12, max_iter=2000)
    rb = E.ode_step(ode_type, T, K, dt, ub, ess=essd, rel_tol=1e-12, max_iter=2000, solver="pcg", jacobi_of=None)
    ns, it, cv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    E._check(E._par_lib().ecm2_ode_step(ode_type, T._h, K._h, dt, E._dev_ptr(uc), E._dev_ptr(essd), int(essd.numel()),
                                        1e-12, 2000, 1, ctypes.byref(ns), ctypes.byref(it), ctypes.byref(cv),
                                        E._stream()))
    assert ra == rb == (ns.value, it.value, bool(cv.value)) and ra[2]
    assert torch.equal(ua, ub) and torch.equal(ua, uc) and not torch.equal(ua, u0)
    with pytest.raises(E.ECM2Error):
        E.ode_step(ode_type, T, K, dt, ua, ess=essd, solver="gmres")
    with pytest.raises(E.ECM2Error):
        E.ode_step(ode_type, T, K, dt, ua, ess=essd, jacobi_of=T)
