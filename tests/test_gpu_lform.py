"""GPU tests of the device linear form: LinearForm.Assemble against the numpy restatement of
DLFEvalAssemble3D + the source coefficients (tests/lform_ref.py, pinned by
tests/test_lform_reference.py), relerr < helpers.RTOL (the project's parity bar; the sources are
non-negative, so nothing cancels; the helper's own float64 error is below 1e-14).

Meshes, the smallest that reach every code path: 2 x 1 x 1 (fewer elements than one workgroup),
5 x 4 x 4 perturbed (80 non-affine elements: more than one workgroup at every order -- a workgroup
holds 64 / 28 / 16 / 10 / 7 elements at Q1D = 2..6 -- with a partial last one), fichera refined once
(56 elements, unstructured sharing), and the curved fichera-q2 mesh for the Jacobian mode."""
import ctypes

import numpy as np
import pytest

import helpers
import ecm2_amd as E
import oracle as O
import lform_ref as R
from helpers import RTOL, relerr

pytestmark = pytest.mark.gpu


def _coeff(src):
    """The Python mirror's coefficient of a lform_ref source (device tensors)."""
    import torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64)).cuda()
    k = src["kind"]
    if k == "constant":
        return E.ConstantCoefficient(src["value"])
    if k == "quad":
        return E.QuadratureCoefficient(dev(src["values"]))
    if k == "gridfunc":
        return E.GridFunctionCoefficient(dev(src["field"]))
    if k == "affine":
        return E.AffineGridFunctionCoefficient(dev(src["field"]), src["scale"], src["slope"], src["t_ref"])
    T = dev(src["T"]) if src.get("T") is not None else None
    return E.JouleHeatingCoefficient(dev(src["phi"]), src["sigma"], src["slope"], src["t_ref"], T)


def _assemble(lf, ndofs):
    import torch
    b = torch.full((ndofs,), float("nan"), dtype=torch.float64, device="cuda")  # (Assemble overwrites)
    lf.Assemble(b)
    torch.cuda.synchronize()
    return b


_SPACES = {}


def _space(name, p, q1d):
    """(mesh, fes, reference, dof coordinates, quadrature points), shared and left unchanged."""
    key = (name, p, q1d)
    if key not in _SPACES:
        m = R.MESHES[name](E)
        fes = E.H1Space(m, p, E.NUMBERING_ENTITY)
        ref = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, enodes=m.element_nodes())
        _SPACES[key] = (m, fes, ref, fes.dof_coords(), O.quad_points(m.element_nodes(), q1d))
    return _SPACES[key]


@pytest.mark.parametrize("name,p,dq", R.CASES)
def test_assemble_matches_reference(name, p, dq):
    """Every coefficient kind, p = 1..4 with the default rule (p + 1) and p + 2, corner geometry."""
    q1d = p + dq
    m, fes, ref, X, P = _space(name, p, q1d)
    for kind in R.KINDS:
        src = R.make_source(kind, X, P)
        lf = E.LinearForm(fes, q1d=0 if dq == 1 else q1d)
        assert lf.info() == {"ne": fes.ne, "ndofs": fes.ndofs, "d1d": p + 1, "q1d": q1d, "n_integrators": 0}
        lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(src)))
        b = _assemble(lf, fes.ndofs).cpu().numpy()
        err = relerr(b, ref.assemble([(src, None)]))
        print(f"{name} p={p} q1d={q1d} {kind}: {err:.2e}")
        assert err < RTOL, (kind, err)


@pytest.mark.parametrize("q1d", [3, 4])
def test_jacobian_mode_on_curved_mesh(tmp_path, q1d):
    """Geometry from MFEM-layout Jacobians (the curved fichera-q2 mesh), p = 2, every kind."""
    import torch
    p = 2
    mesh, fes, J, X = helpers.curved_fichera(tmp_path, p, q1d)
    ref = R.LFRef(p, q1d, fes.gather_map(), fes.ndofs, J=J)
    Jd = torch.as_tensor(np.ascontiguousarray(J)).cuda()
    quad = np.random.default_rng(5).uniform(0.5, 2.0, (fes.ne, q1d ** 3))
    for kind in R.KINDS:
        src = {"kind": "quad", "values": quad} if kind == "quad" else R.make_source(kind, X, None)
        lf = E.LinearForm(fes, q1d=q1d, geometry="jacobians")
        lf.SetJacobians(Jd)
        lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(src)))
        err = relerr(_assemble(lf, fes.ndofs).cpu().numpy(), ref.assemble([(src, None)]))
        print(f"curved q1d={q1d} {kind}: {err:.2e}")
        assert err < RTOL, (kind, err)
    # the same form switched to corner geometry and back: the last call wins
    lf = E.LinearForm(fes, q1d=q1d, geometry="nodes")
    lf.SetJacobians(Jd)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.ConstantCoefficient(1.0)))
    assert relerr(_assemble(lf, fes.ndofs).cpu().numpy(),
                  ref.assemble([({"kind": "constant", "value": 1.0}, None)])) < RTOL


@pytest.mark.parametrize("p,q1d", [(1, 2), (2, 3), (3, 5)])
def test_markers_and_integrator_order(p, q1d):
    """A marked integrator (attributes 1 and 2) equals the reference with f zeroed on the excluded
    elements; two integrators sum in the order they were added."""
    m, fes, ref, X, P = _space("perturbed", p, q1d)
    attr = m.GetAttributes()
    s1, s2 = R.make_source("joule_T", X, P), R.make_source("affine", X, P)
    for marker in ([1, 0], [0, 1]):
        keep = R.marker_keep(attr, marker)
        lf = E.LinearForm(fes, q1d=q1d)
        lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(s1)), elem_marker=marker)
        b = _assemble(lf, fes.ndofs).cpu().numpy()
        f0 = ref.point_values(s1) * keep[:, None]
        assert relerr(b, ref.reduce(ref.element_vectors(f0))) < RTOL
        assert relerr(b, ref.assemble([(s1, keep)])) < RTOL
        # dofs of excluded elements only are exactly zero
        only_excluded = np.setdiff1d(fes.gather_map()[~keep].ravel(), fes.gather_map()[keep].ravel())
        assert only_excluded.size and np.all(b[only_excluded] == 0.0)
    lf = E.LinearForm(fes, q1d=q1d)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(s2)))
    lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(s1)), elem_marker=[0, 1])
    assert lf.info()["n_integrators"] == 2
    b = _assemble(lf, fes.ndofs).cpu().numpy()
    assert relerr(b, ref.assemble([(s2, None), (s1, R.marker_keep(attr, [0, 1]))])) < RTOL


def test_reassemble_after_field_change_and_determinism():
    """Assemble re-reads the coefficients' tensors: changing phi in place gives the new answer; two
    Assembles of the same inputs are bitwise equal (no atomics)."""
    import torch
    p, q1d = 2, 3
    m, fes, ref, X, P = _space("perturbed", p, q1d)
    src = R.make_source("joule_T", X, P)
    c = _coeff(src)
    lf = E.LinearForm(fes)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(c))
    lf.AddDomainIntegrator(E.DomainLFIntegrator(_coeff(R.make_source("gridfunc", X, P))))
    b1 = _assemble(lf, fes.ndofs)
    b2 = _assemble(lf, fes.ndofs)
    assert torch.equal(b1, b2)
    phi2 = np.cos(1.1 * X[:, 0]) * X[:, 1] + 0.3 * X[:, 2]
    c.phi.copy_(torch.as_tensor(phi2).cuda())
    b3 = _assemble(lf, fes.ndofs).cpu().numpy()
    want = ref.assemble([(dict(src, phi=phi2), None), (R.make_source("gridfunc", X, P), None)])
    assert relerr(b3, want) < RTOL
    assert relerr(b1.cpu().numpy(), want) > 1e-3  # (the answer did change)


@pytest.mark.parametrize("name,p", [("perturbed", 1), ("perturbed", 2), ("fichera", 3), ("perturbed", 4)])
def test_gridfunc_equals_mass_mult(name, p):
    """GRIDFUNC at Q1D = p + 2 is the device BilinearForm's mass Mult of the same field."""
    import torch
    m, fes, ref, X, P = _space(name, p, p + 2)
    g = torch.as_tensor(R.temp_field(X)).cuda()
    lf = E.LinearForm(fes, q1d=p + 2)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.GridFunctionCoefficient(g)))
    b = _assemble(lf, fes.ndofs).cpu().numpy()
    form = E.BilinearForm(fes, q1d=p + 2)
    form.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    form.Assemble()
    y = torch.empty_like(g)
    form.Mult(g, y)
    torch.cuda.synchronize()
    assert relerr(b, y.cpu().numpy()) < RTOL


def test_documented_errors():
    """Unsupported (p, Q1D): ECM2_ERR_UNSUPPORTED; vector / matrix kinds and JOULE on a bilinear
    form: ECM2_ERR_ARG."""
    import torch
    m, fes, ref, X, P = _space("small", 1, 2)
    for p, q1d in [(1, 4), (2, 5), (5, 6), (4, 7)]:
        with pytest.raises(E.ECM2Error) as ei:
            E.LinearForm(E.H1Space(m, p), q1d=q1d)
        assert ei.value.code == 5, (p, q1d)
    lf = E.LinearForm(fes)
    lib = E.load_library()
    phi = torch.zeros(fes.ndofs, dtype=torch.float64, device="cuda")
    params = (ctypes.c_double * 6)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    add = lib.ecm2_linear_form_add_domain_integrator
    for kind in (E.COEFF_QUAD_VECTOR, E.COEFF_QUAD_SYMMATRIX, E.COEFF_QUAD_MATRIX, E.COEFF_CONST_VECTOR,
                 E.COEFF_CONST_SYMMATRIX, E.COEFF_CONST_MATRIX, E.COEFF_GRIDFUNC_PERFUSION, 12, -1):
        rc = add(lf._h, kind, ctypes.c_void_p(phi.data_ptr()), None, ctypes.cast(params, ctypes.c_void_p), None, 0)
        assert rc == 1, kind
    assert lf.info()["n_integrators"] == 0
    # data2 belongs to JOULE alone
    assert add(lf._h, E.COEFF_GRIDFUNC, ctypes.c_void_p(phi.data_ptr()), ctypes.c_void_p(phi.data_ptr()), None, None, 0) == 1
    with pytest.raises(E.ECM2Error):
        lf.AddDomainIntegrator(E.DomainLFIntegrator(E.VectorCoefficient([1.0, 2.0, 3.0])))
    # JOULE on a bilinear form
    form = E.BilinearForm(fes)
    for integ in (E.MASS, E.DIFFUSION):
        rc = lib.ecm2_pa_form_add_integrator(form._h, integ, E.COEFF_JOULE, ctypes.c_void_p(phi.data_ptr()),
                                             ctypes.cast(params, ctypes.c_void_p))
        assert rc == 1 and b"JOULE" in lib.ecm2_last_error()
    with pytest.raises(E.ECM2Error):
        form.AddDomainIntegrator(E.MassIntegrator(E.JouleHeatingCoefficient(phi)))
    # a marked integrator without attributes for every element's marker entry
    lf2 = E.LinearForm(fes)
    lf2.AddDomainIntegrator(E.DomainLFIntegrator(E.ConstantCoefficient(1.0)), elem_marker=[])
    with pytest.raises(E.ECM2Error) as ei:
        lf2.Assemble(torch.empty(fes.ndofs, dtype=torch.float64, device="cuda"))
    assert ei.value.code == 1
