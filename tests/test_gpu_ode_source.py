"""GPU tests of the sourced implicit step M du/dt = -K u + b (ecm2_ode_step_source) with b assembled
by the device linear form: against the oracle's stepping (the setup of
tests/test_solvers.py::test_ode_step_matches_oracle and its bound for the same kind of comparison),
the null source, the uniform-heating closed form of examples/rf_heat_step.cpp, a loopback-group
operator, and the step whose explicit operator K carries a ConvectionIntegrator (non-symmetric K, symmetric
T) against the same stepping with the numpy checker of the term (tests/conv_ref.py)."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import ode as ODE
import lform_ref as R
import conv_ref as CR
from helpers import coeff_function, nonaligned, relerr

pytestmark = pytest.mark.gpu

TYPES = [21, 22, 23, 32, 33, 34]
ORDER = 2
_SETUP = {}


# ---- the setup of tests/test_solvers.py::test_ode_step_matches_oracle ----
def _mesh(kind):
    assert kind == "cart"
    m = E.Mesh.MakeCartesian3D(5, 4, 6)
    m.set_vertices(nonaligned(m.vertices()))
    return m


def _elem_rank(m, kind, nranks):
    return E.partition_slabs_z(m, nranks)


def _alpha(P):
    return 2.0 + np.sin(P[..., 0]) * np.cos(P[..., 1])


def _beta(P):
    return coeff_function(P)


def _quad_form(form, ne, P, alpha_fn, beta_fn, scale_beta):
    import torch
    if alpha_fn is not None:
        form.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(
            torch.as_tensor(alpha_fn(P).reshape(ne, -1)).cuda())))
    if beta_fn is not None:
        form.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(
            torch.as_tensor(scale_beta * beta_fn(P).reshape(ne, -1)).cuda())))
    form.Assemble()
    return form


def _serial(m, fes, order, alpha_fn, beta_fn, scale_beta=1.0):
    P = O.quad_points(m.element_nodes(), O.default_q1d(order))
    return _quad_form(E.BilinearForm(fes), fes.ne, P, alpha_fn, beta_fn, scale_beta)


def _group(m, fes, order, er, nranks, alpha_fn, beta_fn, scale_beta=1.0):
    forms, parts = [], []
    for r in range(nranks):
        part = E.Partition(fes, er, r, nranks)
        P = E.quadrature_points_subset(m, O.default_q1d(order), part.elems)
        forms.append(_quad_form(E.ParBilinearForm(part), part.ne_local, P, alpha_fn, beta_fn, scale_beta))
        parts.append(part)
    return E.ParGroup(forms), parts


def _oracle(m, fes, order, alpha_fn, beta_fn, scale_beta=1.0):
    P = O.quad_points(m.element_nodes(), O.default_q1d(order))
    a = alpha_fn(P) if alpha_fn is not None else None
    b = scale_beta * beta_fn(P) if beta_fn is not None else None
    return O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, order, alpha=a, beta=b)


def _to_group(vec_global, parts):
    return np.concatenate([vec_global[p.owned_global] for p in parts])


def _from_group(vec_group, parts, n):
    out = np.zeros(n)
    o = 0
    for p in parts:
        out[p.owned_global] = vec_group[o: o + p.n_owned]
        o += p.n_owned
    return out


def _group_ess(ess_global, parts):
    """Global essential dofs -> indices in the group's concatenated true vector."""
    idx, o = [], 0
    for p in parts:
        pos = np.nonzero(np.isin(p.owned_global, ess_global))[0]
        idx.append(pos + o)
        o += p.n_owned
    return np.concatenate(idx).astype(np.int32)


def _source(m, fes):
    """b = LF(JOULE with sigma(T)) + LF(GRIDFUNC_AFFINE) assembled on the device, shared and left
    unchanged: (device vector, host copy)."""
    import torch
    if "b" not in _SETUP:
        X = fes.dof_coords()
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
        lf = E.LinearForm(fes)
        lf.AddDomainIntegrator(E.DomainLFIntegrator(E.JouleHeatingCoefficient(
            dev(R.phi_field(X)), R.SIGMA0, R.SIGMA_SLOPE, R.T_REF, dev(R.temp_field(X)))))
        lf.AddDomainIntegrator(E.DomainLFIntegrator(E.AffineGridFunctionCoefficient(dev(R.temp_field(X)), 0.8, 0.02,
                                                                                     R.T_REF)))
        b = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda")
        lf.Assemble(b)
        torch.cuda.synchronize()
        _SETUP["b"] = (b, b.cpu().numpy())
    return _SETUP["b"]


def _space():
    if "space" not in _SETUP:
        m = _mesh("cart")
        _SETUP["space"] = (m, E.H1Space(m, ORDER))
    return _SETUP["space"]


@pytest.mark.parametrize("ode_type", TYPES)
def test_sourced_step_matches_oracle(ode_type):
    """Two steps with the device-assembled source == oracle/ode.py's step with the closure
    rhs = -K u + b, rhs[ess] = 0; essential values stay bitwise unchanged."""
    import torch
    m, fes = _space()
    dt = 0.05
    c = E.ode_implicit_coeff(ode_type)
    T = _serial(m, fes, ORDER, _alpha, _beta, scale_beta=c * dt)
    K = _serial(m, fes, ORDER, None, _beta)
    Tr = _oracle(m, fes, ORDER, _alpha, _beta, scale_beta=c * dt)
    Kr = _oracle(m, fes, ORDER, None, _beta)
    ess = fes.boundary_dofs()
    X = fes.dof_coords()
    u0 = 37.0 + 20.0 * np.exp(-4.0 * np.sum((X - 0.5) ** 2, axis=1))
    bd, bh = _source(m, fes)
    # the device source is the linear form's (its own parity is tests/test_gpu_lform.py's)
    ref = R.LFRef(ORDER, ORDER + 1, fes.gather_map(), fes.ndofs, enodes=m.element_nodes())
    assert relerr(bh, ref.assemble([
        ({"kind": "joule", "phi": R.phi_field(X), "sigma": R.SIGMA0, "slope": R.SIGMA_SLOPE, "t_ref": R.T_REF,
          "T": R.temp_field(X)}, None),
        ({"kind": "affine", "field": R.temp_field(X), "scale": 0.8, "slope": 0.02, "t_ref": R.T_REF}, None)])) < 1e-12

    def solve(us):
        rhs = -Kr.mult(us) + bh
        rhs[ess] = 0.0
        return Tr.pcg(rhs, ess, rel_tol=1e-13, max_iter=5000)[0]

    ur = u0.copy()
    for _ in range(2):
        ur = ODE.step(ode_type, solve, ur, dt)
    u = torch.as_tensor(u0).cuda()
    essd = torch.as_tensor(ess).cuda()
    for _ in range(2):
        ns, it, conv = E.ode_step(ode_type, E.Operator(T), E.Operator(K), dt, u, ess=essd, rel_tol=1e-13,
                                  max_iter=5000, source=bd)
        assert conv and ns == {21: 1, 32: 1, 22: 2, 33: 2, 23: 3, 34: 3}[ode_type]
    uh = u.cpu().numpy()
    assert np.array_equal(uh[ess], u0[ess])
    err = relerr(uh - u0, ur - u0)
    print(f"type {ode_type}: {err:.2e}")
    assert err < 1e-9


_CONV = {}


def _convective(order):
    """The setup above with a mesh of its own carrying the attributes 1 + e mod 3, and the numpy checker of
    the convection term with the per-point reference velocity (y, -x, x): computed once per order."""
    if order not in _CONV:
        m = _mesh("cart")
        m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32))
        fes = E.H1Space(m, order)
        conv = CR.ConvRef(order, O.default_q1d(order), fes.gather_map(), fes.ndofs, m.element_nodes())
        keep = CR.marker_keep(m.GetAttributes(), CONV_MARKER)
        assert 0 < keep.sum() < fes.ne
        _CONV[order] = (m, fes, conv, CR.reference_velocity(conv.P), keep)
    return _CONV[order]


CONV_MARKER = [0, 1, 1]
CONV_ALPHA = 1.7


@pytest.mark.parametrize("ode_type,order,sourced", [(t, 2, False) for t in TYPES] + [(23, 3, False), (22, 2, True)])
def test_step_with_convection_in_K_matches_oracle(ode_type, order, sourced):
    """The non-symmetric explicit operator: T = M_alpha + c dt K_beta stays symmetric, K = K_beta +
    Convection(per-point velocity, marked) -- two steps against oracle/ode.py's step with the closure
    rhs = -(K_beta u + C u) [+ b], rhs[ess] = 0, C u from tests/conv_ref.py.  Order 3 steps the sheet
    kernel, order 2 the thread-per-element one; the bar, the bitwise essential values and the stage-solve
    counts are those of test_sourced_step_matches_oracle."""
    import torch
    m, fes, conv, v, keep = _convective(order)
    dt = 0.05
    c = E.ode_implicit_coeff(ode_type)
    T = _serial(m, fes, order, _alpha, _beta, scale_beta=c * dt)
    P = O.quad_points(m.element_nodes(), O.default_q1d(order))
    Kf = E.BilinearForm(fes)
    Kf.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(torch.as_tensor(v).cuda()), CONV_ALPHA), CONV_MARKER)
    K = _quad_form(Kf, fes.ne, P, None, _beta, 1.0)
    assert K.ConvectionInfo() == (True, int(keep.sum()), True)
    Tr = _oracle(m, fes, order, _alpha, _beta, scale_beta=c * dt)
    Kr = _oracle(m, fes, order, None, _beta)
    ess = fes.boundary_dofs()
    X = fes.dof_coords()
    u0 = 37.0 + 20.0 * np.exp(-4.0 * np.sum((X - 0.5) ** 2, axis=1))
    # (any frozen true-dof vector serves as the source: a smooth load through the oracle's mass)
    bh = _oracle(m, fes, order, _alpha, None).mult(40.0 * np.cos(3.0 * X[:, 0])) if sourced else None

    def solve(us):
        rhs = -(Kr.mult(us) + conv.mult(v, us, CONV_ALPHA, keep))
        if sourced:
            rhs += bh
        rhs[ess] = 0.0
        return Tr.pcg(rhs, ess, rel_tol=1e-13, max_iter=5000)[0]

    ur = u0.copy()
    for _ in range(2):
        ur = ODE.step(ode_type, solve, ur, dt)
    u = torch.as_tensor(u0).cuda()
    essd = torch.as_tensor(ess).cuda()
    kw = {"source": torch.as_tensor(bh).cuda()} if sourced else {}
    for _ in range(2):
        ns, it, conv_ok = E.ode_step(ode_type, E.Operator(T), E.Operator(K), dt, u, ess=essd, rel_tol=1e-13,
                                     max_iter=5000, **kw)
        assert conv_ok and ns == {21: 1, 32: 1, 22: 2, 33: 2, 23: 3, 34: 3}[ode_type]
    uh = u.cpu().numpy()
    assert np.array_equal(uh[ess], u0[ess])
    # the term is not a bystander: its share of the first slope's right-hand side is far above the bar
    share = np.abs(conv.mult(v, u0, CONV_ALPHA, keep)).max() / np.abs(Kr.mult(u0)).max()
    err = relerr(uh - u0, ur - u0)
    print(f"type {ode_type} p={order} source={sourced}: {err:.2e} (|C u0| / |K u0| = {share:.2e})")
    assert share > 1e-3
    assert err < 1e-9


@pytest.mark.parametrize("ode_type", [21, 23, 34])
def test_null_source_is_the_homogeneous_step(ode_type):
    """source=None and a zero source vector reproduce ode_step bitwise."""
    import torch
    m, fes = _space()
    dt = 0.05
    c = E.ode_implicit_coeff(ode_type)
    T = E.Operator(_serial(m, fes, ORDER, _alpha, _beta, scale_beta=c * dt))
    K = E.Operator(_serial(m, fes, ORDER, None, _beta))
    essd = torch.as_tensor(fes.boundary_dofs()).cuda()
    u0 = torch.as_tensor(np.random.default_rng(3).uniform(30, 40, fes.ndofs)).cuda()
    outs = []
    for src in ("plain", None, torch.zeros(fes.ndofs, dtype=torch.float64, device="cuda")):
        u = u0.clone()
        if isinstance(src, str):
            r = E.ode_step(ode_type, T, K, dt, u, ess=essd, rel_tol=1e-12, max_iter=2000)
        else:
            r = E.ode_step(ode_type, T, K, dt, u, ess=essd, rel_tol=1e-12, max_iter=2000, source=src)
        outs.append((u, r))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    assert torch.equal(outs[0][0], outs[2][0]) and outs[0][1] == outs[2][1]
    # a source vector of the wrong size never reaches the kernels
    with pytest.raises(E.ECM2Error):
        E.ode_step(ode_type, T, K, dt, u0.clone(), ess=essd, source=torch.zeros(3, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("ode_type", [21, 23, 34])
def test_uniform_heating_closed_form(ode_type):
    """phi = a . x, sigma and rho c constant, no essential dofs, u0 uniform: K u0 = 0 and
    b = sigma |a|^2 M_1 1, so every stage slope is the constant vector and
    u1 = u0 + dt sigma |a|^2 / rho c at every dof; sum b = sigma |a|^2 (unit cube)."""
    import torch
    m = E.Mesh.MakeCartesian3D(4, 4, 4)
    fes = E.H1Space(m, ORDER)
    a = np.array([1.5, -0.7, 0.4])
    sigma, rho_c, k, dt, u_init = 0.6, 3.6, 0.5, 0.25, 37.0
    c = E.ode_implicit_coeff(ode_type)
    phi = torch.as_tensor(fes.dof_coords() @ a).cuda()
    lf = E.LinearForm(fes)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.JouleHeatingCoefficient(phi, sigma)))
    b = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda")
    lf.Assemble(b)
    assert abs(float(b.sum()) - sigma * (a @ a)) < 1e-12 * sigma * (a @ a)
    Tf, Kf = E.BilinearForm(fes), E.BilinearForm(fes)
    Tf.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(rho_c)))
    Tf.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(c * dt * k)))
    Kf.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(k)))
    Tf.Assemble()
    Kf.Assemble()
    u = torch.full((fes.ndofs,), u_init, dtype=torch.float64, device="cuda")
    ns, it, conv = E.ode_step(ode_type, E.Operator(Tf), E.Operator(Kf), dt, u, rel_tol=1e-13, max_iter=2000, source=b)
    assert conv
    rise = dt * sigma * (a @ a) / rho_c
    err = float((u - u_init - rise).abs().max()) / rise
    print(f"type {ode_type}: {err:.2e}")
    assert err < 1e-9


def test_group_operator_takes_the_permuted_source():
    """SDIRK33 on a 3-rank loopback group with b permuted by Partition.owned_global == the serial
    device step."""
    import torch
    m, fes = _space()
    nranks, dt, ode_type = 3, 0.02, 23
    c = E.ode_implicit_coeff(ode_type)
    er = _elem_rank(m, "cart", nranks)
    Tg, parts = _group(m, fes, ORDER, er, nranks, _alpha, _beta, scale_beta=c * dt)
    Kg, _ = _group(m, fes, ORDER, er, nranks, None, _beta)
    Ts = _serial(m, fes, ORDER, _alpha, _beta, scale_beta=c * dt)
    Ks = _serial(m, fes, ORDER, None, _beta)
    ess = fes.boundary_dofs()
    bd, bh = _source(m, fes)
    u0 = np.random.default_rng(3).uniform(30, 40, fes.ndofs)
    us = torch.as_tensor(u0).cuda()
    E.ode_step(ode_type, E.Operator(Ts), E.Operator(Ks), dt, us, ess=torch.as_tensor(ess).cuda(), rel_tol=1e-13,
               max_iter=5000, source=bd)
    ug = torch.as_tensor(_to_group(u0, parts)).cuda()
    E.ode_step(ode_type, E.Operator(Tg), E.Operator(Kg), dt, ug, ess=torch.as_tensor(_group_ess(ess, parts)).cuda(),
               rel_tol=1e-13, max_iter=5000, source=torch.as_tensor(_to_group(bh, parts)).cuda())
    ugh = _from_group(ug.cpu().numpy(), parts, fes.ndofs)
    assert relerr(ugh - u0, us.cpu().numpy() - u0) < 1e-9
