"""CPU tests of the linear form's host side: the C ABI declares and exports the new entry points,
the default rule is DomainLFIntegrator's, the Python mirror has the reference's names, and without a
GPU the form fails loudly (no CPU fallback).  No compute entry point runs here."""
import ctypes

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E

NEW_SYMBOLS = ["ecm2_linear_form_default_q1d", "ecm2_linear_form_create", "ecm2_linear_form_set_element_nodes",
               "ecm2_linear_form_set_jacobians", "ecm2_linear_form_set_attributes",
               "ecm2_linear_form_add_domain_integrator", "ecm2_linear_form_assemble", "ecm2_linear_form_info",
               "ecm2_linear_form_destroy", "ecm2_ode_step_source"]


def test_linear_form_symbols_declared_and_exported():
    lib = E.load_library()
    declared = E.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert "#define ECM2_COEFF_JOULE 11" in open(E.HEADER_PATH).read()
    assert E.COEFF_JOULE == 11


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_default_rule_is_domain_lf_integrators(p):
    """DomainLFIntegrator(Q, a = 2, b = 0): order 2 p, p + 1 Gauss-Legendre points."""
    lib = E.load_library()
    lib.ecm2_linear_form_default_q1d.restype = ctypes.c_int
    assert lib.ecm2_linear_form_default_q1d(p) == p + 1
    assert E.linear_form_default_q1d(p) == p + 1


def test_python_names_exist():
    for name in ("LinearForm", "DomainLFIntegrator", "JouleHeatingCoefficient", "linear_form_default_q1d"):
        assert hasattr(E, name), name
    for meth in ("SetJacobians", "AddDomainIntegrator", "Assemble", "info"):
        assert callable(getattr(E.LinearForm, meth))
    import inspect
    assert "source" in inspect.signature(E.ode_step).parameters
    c = E.JouleHeatingCoefficient(None, sigma=0.6, slope=0.01, t_ref=37.0)
    assert (c.sigma, c.slope, c.t_ref, c.T) == (0.6, 0.01, 37.0, None)
    assert E.DomainLFIntegrator(c).coeff is c


def test_linear_form_fails_loudly_without_gpu():
    """No CPU fallback: creating a linear form without a device must raise ECM2_ERR_HIP."""
    lib = E.load_library()
    if lib.ecm2_device_count() > 0:
        pytest.skip("a GPU is visible")
    gm = np.zeros((1, 8), np.int32)
    h = ctypes.c_void_p()
    lib.ecm2_linear_form_create.restype = ctypes.c_int
    rc = lib.ecm2_linear_form_create(1, 1, 1, ctypes.c_void_p(gm.ctypes.data), 0, ctypes.byref(h))
    assert rc == 2  # ECM2_ERR_HIP
    assert b"no HIP device" in lib.ecm2_last_error()
    m = E.Mesh.MakeCartesian3D(2, 1, 1)
    with pytest.raises(E.ECM2Error) as ei:
        E.LinearForm(E.H1Space(m, 1))
    assert ei.value.code == 2


def test_sources_are_checked_before_the_gpu():
    """The Python mirror refuses non-scalar sources and misfit fields before a pointer reaches a kernel."""
    torch = pytest.importorskip("torch")
    lf = E.LinearForm.__new__(E.LinearForm)  # (no device: only the argument checks run)
    lf._keep, lf._marked = [], False
    lf.info = lambda: {"ne": 6, "ndofs": 125, "d1d": 3, "q1d": 3, "n_integrators": 0}
    bad = [E.VectorCoefficient([1.0, 2.0, 3.0]), E.MatrixCoefficient(np.eye(3)),
           E.PerfusionCoefficient(None, 1.0, 0.1, 0.5),
           E.JouleHeatingCoefficient(torch.zeros(125, dtype=torch.float64)),      # a host tensor
           E.JouleHeatingCoefficient(None),
           E.GridFunctionCoefficient(torch.zeros(125, dtype=torch.float32))]
    for c in bad:
        with pytest.raises(E.ECM2Error):
            lf.AddDomainIntegrator(E.DomainLFIntegrator(c))
    lf._h = None
    # a Joule coefficient is not a bilinear form's coefficient
    with pytest.raises(E.ECM2Error):
        E._integrator_args(E.JouleHeatingCoefficient(None), [], 6, 27, 125)
