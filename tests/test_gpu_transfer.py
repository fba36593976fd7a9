"""GPU tests of the device p-refinement transfer operator (PRefinementTransfer / ecm2_transfer_*:
TensorProductPRefinementTransferOperator, fem/transfer.cpp:2223-2592, in the kernels of csrc/k_transfer.hip) against
the 80-bit evaluation of tests/mg_ref.py, componentwise: |y_i - y_80bit,i| <= C_XFER u S_i with S = |B| (x) |B| (x) |B|
|x| (C_XFER measured by tests/test_mg_reference.py).  Every output is preset to NaN, so an entry that is not
written fails; every result is computed twice and must be bitwise equal."""
import os

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import hp_ref as HP
import mg_cases as MC
import mg_ref as MR
from helpers import GOLDEN, relerr, temperature

pytestmark = pytest.mark.gpu

PAIRS = [(pc, pf) for pc in (1, 2, 3) for pf in range(pc + 1, 5)]
ERR_ARG, ERR_UNSUPPORTED = 1, 5


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _check_pair(lf, hf, label):
    """Both directions of the device transfer between two spaces against the 80-bit reference."""
    import torch
    T = E.PRefinementTransfer(lf, hf)
    R = MR.Transfer(lf.gather_map(), lf.ndofs, lf.order, hf.gather_map(), hf.ndofs, hf.order, MR.LD)
    rng = np.random.default_rng(9)
    for kind in ("temperature", "random"):
        xc = temperature(lf.dof_coords()) if kind == "temperature" else rng.uniform(-1, 1, lf.ndofs)
        xf = temperature(hf.dof_coords()) if kind == "temperature" else rng.uniform(-1, 1, hf.ndofs)
        yf, yf2, yc, yc2 = _nan(hf.ndofs), _nan(hf.ndofs), _nan(lf.ndofs), _nan(lf.ndofs)
        T.Mult(_dev(xc), yf)
        T.Mult(_dev(xc), yf2)
        T.MultTranspose(_dev(xf), yc)
        T.MultTranspose(_dev(xf), yc2)
        c1 = HP.constant(yf.cpu().numpy(), R.mult(xc), R.bound_mult(xc))
        c2 = HP.constant(yc.cpu().numpy(), R.mult_transpose(xf), R.bound_mult_transpose(xf))
        print(f"{label} p {lf.order} -> {hf.order} {kind}: constants {c1:.2f} (Mult), {c2:.2f} (MultTranspose)")
        assert c1 <= MR.C_XFER and c2 <= MR.C_XFER
        assert torch.equal(yf, yf2) and torch.equal(yc, yc2)
    return T


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_all_pairs_componentwise(pc, pf):
    m = MC.lattice((3, 2, 2), True)
    _check_pair(E.H1Space(m, pc), E.H1Space(m, pf), "moved 3x2x2")


@pytest.mark.parametrize("dims", [(5, 4, 3), (9, 4, 2)])
def test_element_counts_around_a_wave(dims):
    """5 x 4 x 3: 60 elements (less than a wave), 693 fine dofs (odd); 9 x 4 x 2: 72 elements (a wave and a part of
    the next, more than one workgroup of the p 1 -> 2 kernels)."""
    m = MC.lattice(dims, True)
    _check_pair(E.H1Space(m, 1), E.H1Space(m, 2), "moved %dx%dx%d" % dims)


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
def test_fichera(pc, pf):
    """Seven elements whose shared faces have differing local orientations."""
    m = E.Mesh(os.path.join(GOLDEN, "fichera.mesh"))
    _check_pair(E.H1Space(m, pc), E.H1Space(m, pf), "fichera")


def test_mixed_numberings_and_sfc_order():
    m = MC.lattice((4, 3, 3), True)
    _check_pair(E.H1Space(m, 1, E.NUMBERING_ENTITY), E.H1Space(m, 2, E.NUMBERING_STRUCTURED), "entity -> structured")
    _check_pair(E.H1Space(m, 2, E.NUMBERING_STRUCTURED), E.H1Space(m, 3, E.NUMBERING_ENTITY), "structured -> entity")
    s = MC.lattice((4, 4, 4), True, sfc=True)
    _check_pair(E.H1Space(s, 1), E.H1Space(s, 2), "sfc 4x4x4")
    _check_pair(E.H1Space(s, 2), E.H1Space(s, 4), "sfc 4x4x4")


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
def test_galerkin_identity_through_the_device_forms(pc, pf):
    """Flat 4^3 lattice, constant coefficient: P^T (A_f (P x)) = A_c x to 1e-12 through the real forms -- two
    spaces that disagree about an element's orientation would not pass."""
    import torch
    m = MC.lattice((4, 4, 4), False)
    lf, hf = E.H1Space(m, pc), E.H1Space(m, pf)
    T = E.PRefinementTransfer(lf, hf)
    forms = []
    for fes in (lf, hf):
        f = E.BilinearForm(fes)
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(1.0)))
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.Assemble()
        forms.append(f)
    x = _dev(np.random.default_rng(4).uniform(0, 1, lf.ndofs))
    want, px, apx, got = _nan(lf.ndofs), _nan(hf.ndofs), _nan(hf.ndofs), _nan(lf.ndofs)
    forms[0].Mult(x, want)
    T.Mult(x, px)
    forms[1].Mult(px, apx)
    T.MultTranspose(apx, got)
    err = relerr(got.cpu().numpy(), want.cpu().numpy())
    print(f"p {pc} -> {pf}: relerr {err:.2e}")
    assert err <= 1e-12


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


def test_refusals_and_the_next_valid_call_works():
    m = MC.lattice((3, 2, 2), True)
    f1, f2, f3 = E.H1Space(m, 1), E.H1Space(m, 2), E.H1Space(m, 3)
    assert _code(lambda: E.PRefinementTransfer(f2, f1)) == ERR_ARG
    assert _code(lambda: E.PRefinementTransfer(f2, f2)) == ERR_ARG
    assert _code(lambda: E.PRefinementTransfer(f1, E.H1Space(MC.lattice((3, 2, 1), True), 2))) == ERR_ARG
    assert _code(lambda: E.PRefinementTransfer(f1, E.H1Space(m, 5))) == ERR_UNSUPPORTED
    T = E.PRefinementTransfer(f1, f2)
    # vectors of the wrong size are refused before the call
    with pytest.raises(E.ECM2Error):
        T.Mult(_nan(f1.ndofs), _nan(f3.ndofs))
    with pytest.raises(E.ECM2Error):
        T.MultTranspose(_nan(f1.ndofs), _nan(f1.ndofs))
    _check_pair(f1, f2, "after the refusals")
