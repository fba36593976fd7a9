"""The convection term's public interface without a device: the C entry points are declared in the header
and exported by the library, and the Python mirror has the integrator kind, the class and the methods."""
import ctypes

import ecm2_amd as E


def test_convection_symbols_are_declared_and_exported():
    lib = E.load_library()
    declared = E.declared_symbols()
    for name in ("ecm2_pa_form_integrator_add_mult_transpose", "ecm2_pa_form_convection_info"):
        assert name in declared, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    assert "#define ECM2_CONVECTION 2" in open(E.HEADER_PATH).read()


def test_python_mirror_has_the_convection_integrator():
    assert E.CONVECTION == 2 and E.ConvectionIntegrator.kind == 2
    ci = E.ConvectionIntegrator(E.VectorCoefficient([1.0, 0.0, 0.0]))
    assert ci.alpha == 1.0 and E.ConvectionIntegrator(ci.coeff, 2.5).alpha == 2.5
    for method in ("ConvectionInfo", "IntegratorAddMultTransposePA", "MultTranspose"):
        assert callable(getattr(E.BilinearForm, method))
