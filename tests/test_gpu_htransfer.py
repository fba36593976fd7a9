"""GPU tests of the device h-refinement transfer operator (HRefinementTransfer / ecm2_transfer_create_h:
FiniteElementSpace::RefinementOperator, fem/fespace.cpp:1833-2120, in the kernels of csrc/k_transfer.hip) against
the 80-bit evaluation of tests/hmg_ref.py, componentwise: |y_i - y_80bit,i| <= C_HXFER u S_i with S = |P| |x| and
|P|^T |x| (C_HXFER measured by tests/test_hmg_reference.py).  Every output is preset to NaN, so an entry that is not
written fails; every result is computed twice and must be bitwise equal."""
import ctypes

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import hmg_cases as HC
import hmg_ref as HR
import hp_ref as HP
import mg_cases as MC
from helpers import relerr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 5


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _check(P, mult, mult_transpose, R, label):
    """Both directions of a device transfer against the 80-bit reference R on the pair's inputs."""
    import torch
    nc, nf = P.lf.ndofs, P.hf.ndofs
    for kind, (xc, xf) in P.inputs.items():
        yf, yf2, yc, yc2 = _nan(nf), _nan(nf), _nan(nc), _nan(nc)
        mult(_dev(xc), yf)
        mult(_dev(xc), yf2)
        mult_transpose(_dev(xf), yc)
        mult_transpose(_dev(xf), yc2)
        c1 = HP.constant(yf.cpu().numpy(), R.mult(xc), R.bound_mult(xc))
        c2 = HP.constant(yc.cpu().numpy(), R.mult_transpose(xf), R.bound_mult_transpose(xf))
        print(f"{label} p {P.p} {kind}: constants {c1:.2f} (Mult), {c2:.2f} (MultTranspose)")
        assert c1 <= HR.C_HXFER and c2 <= HR.C_HXFER
        assert torch.equal(yf, yf2) and torch.equal(yc, yc2)


@pytest.mark.parametrize("name,p", HC.TRANSFER_CASES)
def test_componentwise(name, p):
    P = HC.pair(name, p)
    T = E.HRefinementTransfer(P.lf, P.hf)
    assert (T.width, T.height) == (P.lf.ndofs, P.hf.ndofs) and T.plan_bytes > 0
    _check(P, T.Mult, T.MultTranspose, P.ref(HR.LD), name)


def test_info_reports_equal_orders_and_the_fine_count():
    P = HC.pair("moved322", 2)
    T = E.HRefinementTransfer(P.lf, P.hf)
    v = [ctypes.c_int() for _ in range(5)]
    assert E._par_lib().ecm2_transfer_info(T._h, *[ctypes.byref(a) for a in v], None) == 0
    assert [a.value for a in v] == [P.hf.ne, 2, 2, P.lf.ndofs, P.hf.ndofs]


def test_embedding_that_is_a_permutation_of_the_fine_elements():
    """The fine elements in another order than 8 i + k: the fine map's rows, parent and octant permuted alike.  The
    owners change with the order; the result is the reference's fed the same embedding."""
    P = HC.pair("moved322", 2)
    lib = E._par_lib()
    perm = np.random.default_rng(5).permutation(P.hf.ne)
    assert not np.array_equal(perm, np.arange(P.hf.ne))
    gc = P.lf.gather_map()
    gf = np.ascontiguousarray(P.hf.gather_map()[perm])
    parent, octant = np.ascontiguousarray(P.parent[perm]), np.ascontiguousarray(P.octant[perm])
    h = ctypes.c_void_p()
    assert lib.ecm2_transfer_create_h(2, P.lf.ne, P.lf.ndofs, E._np_ptr(gc), P.hf.ne, P.hf.ndofs, E._np_ptr(gf),
                                      E._np_ptr(parent), E._np_ptr(octant), ctypes.byref(h)) == 0
    try:
        mult = lambda x, y: E._check(lib.ecm2_transfer_mult(h, E._dev_ptr(x), E._dev_ptr(y), E._stream()))
        multt = lambda x, y: E._check(lib.ecm2_transfer_mult_transpose(h, E._dev_ptr(x), E._dev_ptr(y), E._stream()))
        _check(P, mult, multt, P.ref(HR.LD, gf, parent, octant), "moved322 permuted")
        import torch
        torch.cuda.synchronize()
    finally:
        lib.ecm2_transfer_destroy(h)


@pytest.mark.parametrize("p", [1, 2, 4])
def test_galerkin_identity_through_the_device_forms(p):
    """Flat lattice, constant coefficients: P^T (A_f (P x)) = A_c x to 1e-12 through the real forms on the two
    meshes -- an octant or axis mix-up cannot pass this."""
    m = MC.lattice((3, 3, 2), False)
    f = HC.refined(m)
    lf, hf = E.H1Space(m, p), E.H1Space(f, p)
    T = E.HRefinementTransfer(lf, hf)
    forms = []
    for fes in (lf, hf):
        a = E.BilinearForm(fes)
        a.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(1.0)))
        a.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        a.Assemble()
        forms.append(a)
    x = _dev(np.random.default_rng(4).uniform(0, 1, lf.ndofs))
    want, px, apx, got = _nan(lf.ndofs), _nan(hf.ndofs), _nan(hf.ndofs), _nan(lf.ndofs)
    forms[0].Mult(x, want)
    T.Mult(x, px)
    forms[1].Mult(px, apx)
    T.MultTranspose(apx, got)
    err = relerr(got.cpu().numpy(), want.cpu().numpy())
    print(f"p {p}: relerr {err:.2e}")
    assert err <= 1e-12


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


def test_refusals_and_the_next_valid_call_works():
    P = HC.pair("moved322", 1)
    P2 = HC.pair("moved322", 2)
    assert _code(lambda: E.HRefinementTransfer(P.lf, P2.hf)) == ERR_ARG       # unequal orders
    assert _code(lambda: E.HRefinementTransfer(P.lf, P.lf)) == ERR_ARG        # hfes.ne != 8 lfes.ne
    assert _code(lambda: E.HRefinementTransfer(P.hf, P.lf)) == ERR_ARG
    # a missing octant: two children of one parent at the same place
    lib = E._par_lib()
    octant = P.octant.copy()
    octant[9] = octant[8]
    h = ctypes.c_void_p()
    gc, gf = P.lf.gather_map(), P.hf.gather_map()
    assert lib.ecm2_transfer_create_h(1, P.lf.ne, P.lf.ndofs, E._np_ptr(gc), P.hf.ne, P.hf.ndofs, E._np_ptr(gf),
                                      E._np_ptr(P.parent), E._np_ptr(octant), ctypes.byref(h)) == ERR_UNSUPPORTED
    assert not h.value
    T = E.HRefinementTransfer(P.lf, P.hf)
    # vectors of the wrong size are refused before the call
    with pytest.raises(E.ECM2Error):
        T.Mult(_nan(P.lf.ndofs), _nan(P.lf.ndofs))
    with pytest.raises(E.ECM2Error):
        T.MultTranspose(_nan(P.lf.ndofs), _nan(P.lf.ndofs))
    _check(P, T.Mult, T.MultTranspose, P.ref(HR.LD), "after the refusals")
