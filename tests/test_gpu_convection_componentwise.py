"""GPU parity of the convection term, componentwise: C x, C^T x and the term's qdata against the
extended-precision reference (tests/conv_ref.py in numpy.longdouble, Lagrange product tables),

    max_i |y_i - y_hp,i| / (u S_i) <= C_CONV        (qdata against Pabs: C_CONV_QD),      u = 2^-53,

S the same sums over the magnitudes of every factor (hp_ref.constant; where S_i = 0 the entry must be
exactly 0).  This is the tight bar of the term: unlike relerr < 1e-12 on x ~ U[0, 1) it holds on the
temperature fields the ODE step applies K to, for which C x cancels four to five digits (C 1 = 0), and a
1e-12 relative error of the qdata at one point is 340 - 400 units of MultTranspose and 9000 of the qdata
criterion (tests/test_conv_reference.py, which also derives the two constants from the float64
checker's own error -- never from a device result).  tests/test_gpu_convection.py stays as the coverage
of the paths and the ABI.

Cases (tests/conv_cases.py): `perturbed` and `fichera` at p = 1..4 with p + 1 and p + 2 points -- all eight
(D, Q) instantiations, thread-per-element and sheet -- and `cube8` with its ragged marker at p = 2, 4;
each with C alone, constant and per-point velocity, marked and unmarked, both directions, the four
states; the explicit operator K = Diffusion(beta) + Convection the ODE step applies; and the Jacobian
geometry (SetJacobians) on the trilinear `perturbed` mesh and on the curved fichera-q2 / fichera-q3 meshes,
the branch of the setup kernel the drop-in binding takes.  y is preset to NaN; ConvectionInfo's active
count is asserted, so that a case cannot fall to another path.  Run with -s for every case's constants."""
import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import conv_cases as CC
import hp_ref as HP
from cw_cases import STATES
from helpers import k_of_T, relerr, temperature

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    E.load_library()
    yield
    torch.cuda.synchronize()


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def vcoeff(v):
    return E.VectorCoefficient(v if np.ndim(v) == 1 else dev(v))


def make_form(g, vname=None, marked=False, beta=None, mass=False):
    """The form of one geometry: corners or SetJacobians, then Diffusion(beta per point), the unit mass
    and / or the convection integrator."""
    q1d = 0 if g.q1d == g.p + 2 else g.q1d
    if g.kind == "jacobians":
        f = E.BilinearForm(g.fes, q1d=q1d, geometry="jacobians")
        f.SetJacobians(dev(g.J))
    else:
        f = E.BilinearForm(g.fes, q1d=q1d)
    if mass:
        f.AddDomainIntegrator(E.MassIntegrator())
    if beta is not None:
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(dev(beta.reshape(g.ne, -1)))))
    if vname is not None:
        f.AddDomainIntegrator(E.ConvectionIntegrator(vcoeff(g.velocity(vname)), CC.CALPHA),
                              list(CC.MARKER) if marked else None)
    f.Assemble()
    if vname is not None:
        n_act = g.n_active(marked)
        assert f.ConvectionInfo() == (True, n_act, n_act > 0)
    return f


def mult(f, x, transpose=False):
    xd = dev(x)
    y = torch.full_like(xd, float("nan"))   # (Mult overwrites)
    (f.MultTranspose if transpose else f.Mult)(xd, y)
    return host(y)


def check_term(g):
    """C alone: the qdata and both products of every (velocity, marker) on the four states."""
    nq = g.q1d ** 3
    for vname in ("const", "points"):
        for marked in (False, True):
            f = make_form(g, vname, marked)
            pa_hp, Pabs = g.qdata_ref(vname, marked)
            qd = f.qdata(E.CONVECTION)
            assert qd.shape == (g.ne, 3, nq)
            if marked:
                assert np.all(qd[~g.keep] == 0.0)          # excluded elements: exact zeros
            assert np.all(qd[Pabs == 0] == 0.0)
            c_qd = HP.constant(qd.ravel(), pa_hp.ravel(), Pabs.ravel())
            consts = {}
            for tr in (False, True):
                ref = g.mult_ref(vname, marked, tr)
                consts[tr] = {s: HP.constant(mult(f, g.x[s], tr), *ref[s]) for s in STATES}
            print("\n%-30s %-6s %-8s Mult %s | MultT %s | qdata %5.2f   (C_CONV %g, C_CONV_QD %g)" % (
                CC.case_id((g.kind, g.name, g.p, g.q1d)), vname, "marked" if marked else "all",
                " ".join("%5.2f" % consts[False][s] for s in STATES),
                " ".join("%5.2f" % consts[True][s] for s in STATES), c_qd, HP.C_CONV, HP.C_CONV_QD))
            assert c_qd <= HP.C_CONV_QD, (vname, marked, c_qd)
            for tr in (False, True):
                assert max(consts[tr].values()) <= HP.C_CONV, (vname, marked, tr, consts[tr])


@pytest.mark.parametrize("case", CC.CORNER_CASES, ids=[CC.case_id(c) for c in CC.CORNER_CASES])
def test_convection_componentwise(case):
    """Corner geometry: every (D, Q) kernel, forward and transposed, and the setup kernel's trilinear branch."""
    g = CC.geometry(*case)
    if case[1] == "cube8":
        assert g.n_active(True) == 347
        # axis-aligned: the off-diagonal Jacobian entries and their bounds are exactly zero
        assert np.all(g.hi.Jabs[..., ~np.eye(3, dtype=bool)] == 0)
    check_term(g)


@pytest.mark.parametrize("case", CC.JACOBIAN_CASES, ids=[CC.case_id(c) for c in CC.JACOBIAN_CASES])
def test_convection_componentwise_jacobian_geometry(case):
    """SetJacobians (GeometricFactors::JACOBIANS, what the drop-in binding passes): the setup kernel's
    Jacobian branch on a trilinear and on the curved meshes, against ConvRef.from_jacobians."""
    check_term(CC.geometry(*case))


@pytest.mark.parametrize("case", CC.JACOBIAN_CASES, ids=[CC.case_id(c) for c in CC.JACOBIAN_CASES])
def test_jacobian_geometry_identities(case):
    """With no CPU operator at all, constant v: C 1 = 0 within C_CONV u S, and the device's C (g . X)
    against the device's own alpha (v . g) M_1 1 (M_1 the unit mass form on the same Jacobians) to 1e-12
    in max norm: adj(J) v . J^T g = det J (v . g) at every point, whatever the geometry."""
    g = CC.geometry(*case)
    f = make_form(g, "const")
    one = np.ones(g.ndofs)
    c1 = HP.constant(mult(f, one), np.zeros(g.ndofs, HP.LD), g.hi.bound(CC.VCONST, one, CC.CALPHA))
    gvec = np.array([0.4, -1.1, 0.7])
    lhs = mult(f, g.X @ gvec)
    rhs = CC.CALPHA * (CC.VCONST @ gvec) * mult(make_form(g, mass=True), one)
    err = relerr(lhs, rhs)
    print(f"\n{CC.case_id(case)}: |C 1|_i / (u S_i) <= {c1:.2f}; C (g . X) against alpha (v . g) M_1 1: {err:.2e}")
    assert c1 <= HP.C_CONV
    assert np.abs(rhs).max() > 1e-4 and err < 1e-12


@pytest.mark.parametrize("p", [2, 4])
def test_explicit_operator_diffusion_plus_convection(p):
    """K = Diffusion(beta) + Convection, the operator the ODE step applies (one case per kernel family:
    thread-per-element and sheet; per-point velocity, marked, beta = k(T) per point as in cw_cases):
    |y - (y_vol,hp + y_conv,hp)|_i <= u (C S_vol,i + C_CONV S_conv,i) on the four states, the add
    pass's few extra roundings inside each constant's 4x headroom."""
    g = CC.geometry("corners", "perturbed", p, p + 2)
    beta = k_of_T(temperature(O.quad_points(g.en, g.q1d)))
    vol = HP.cached(("conv-K", p), lambda: HP.HPRef(g.en, g.gm, g.ndofs, p, g.q1d, beta=beta))
    f = make_form(g, "points", True, beta=beta)
    for tr in (False, True):
        ref = g.mult_ref("points", True, tr)
        for s in STATES:
            y_hp = vol.mult(g.x[s]) + ref[s][0]
            S = HP.C * vol.bound(g.x[s]) + HP.C_CONV * ref[s][1]
            c = HP.constant(mult(f, g.x[s], tr), y_hp, S)
            print(f"\nK p={p} transpose={tr} {s}: {c:.3f} of the combined bound")
            assert c <= 1.0, (tr, s, c)
