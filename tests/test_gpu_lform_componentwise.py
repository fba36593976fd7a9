"""GPU parity of the device linear form, componentwise: LinearForm.Assemble against the
extended-precision reference (tests/lform_ref.py in numpy.longdouble),

    max_i |b_i - b_hp,i| / (u S_i) <= C_LF  (Joule sources: C_LF_JOULE),      u = 2^-53,

S = R^T |B|^T |B|^T |B|^T (W F |det J|) the same sums over the magnitudes of every factor
(LFRef.bound; hp_ref.constant: where S_i = 0 the entry must be exactly 0).  Unlike relerr < 1e-12 it
sees every entry, not the largest ones only (the electrode potential's Joule heat spans 50 decades), and
it holds on the inputs the model feeds the form, whose sums cancel: kelvin fields through the affine law,
a signed per-point source, potentials with an offset.  tests/test_lform_reference.py derives the two
constants from the float64 checker's own error -- never from a device result -- and shows what the
criterion sees.  tests/test_gpu_lform.py stays as the coverage of the paths and the ABI.

Cases (tests/rhs_cases.py): `perturbed` at p = 1..4 with p + 1 and p + 2 points (all eight kernels, more
than one workgroup each), `fichera` at p = 2, 4, `small` at p = 1, `perturbed` translated by (10, -7, 3)
at p = 2 and the curved fichera-q2 mesh in Jacobian mode; sixteen source states each, and on `perturbed`
a marked integrator and two integrators (order kept, bounds added).  b is preset to NaN, every dof is
checked, every Assemble runs twice and must repeat bitwise.  Run with -s for every case's constants."""
import numpy as np
import pytest

import ecm2_amd as E
import hp_ref as HP
import rhs_cases as RC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    E.load_library()
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float64)).cuda()


def coeff(src):
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


def make_form(sp, integ):
    q1d = 0 if sp.q1d == sp.p + 1 else sp.q1d
    if sp.J is not None:
        lf = E.LinearForm(sp.fes, q1d=sp.q1d, geometry="jacobians")
        lf.SetJacobians(dev(sp.J))
    else:
        lf = E.LinearForm(sp.fes, q1d=q1d)
    assert lf.info()["q1d"] == sp.q1d
    for src, keep in integ:
        lf.AddDomainIntegrator(E.DomainLFIntegrator(coeff(src)), elem_marker=None if keep is None else RC.LF_MARKER)
    return lf


def assemble_twice(lf, n):
    out = []
    for _ in range(2):
        b = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")   # (Assemble overwrites)
        lf.Assemble(b)
        out.append(b)
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]), "two Assembles differ"
    return out[0].cpu().numpy()


@pytest.mark.parametrize("case", RC.LF_SPACES, ids=[RC.lf_id(c) for c in RC.LF_SPACES])
def test_linear_form_componentwise(case):
    """Every source state of the space (and on `perturbed` the marked and the two-integrator case) within
    its family's constant; the linear potential's heat also against sigma |a|^2 (M 1)_hp within the same
    bound."""
    sp = RC.lf_space(*case)
    row, over = {}, {}
    for cname in RC.lf_cases(sp.name):
        integ = sp.integrators(cname)
        b = assemble_twice(make_form(sp, integ), sp.ndofs)
        b_hp, L = sp.limit(cname)
        frac = HP.constant(b, b_hp, L)
        # reported in units of u S: the fraction of the allowance times the family's constant
        c_fam = HP.C_LF_JOULE if sp.family(cname) == "joule" else HP.C_LF
        row[cname] = frac if cname == "two" else frac * c_fam
        if frac > 1.0:
            over[cname] = row[cname]
        if cname == "marked":
            S = sp.ref("marked")[1]
            assert np.any(S == 0) and np.all(b[S == 0] == 0.0)       # dofs of excluded elements only
        if cname == "joule_linear" and sp.name != "small":
            ident = HP.constant(b, sp.linear_potential_rhs(), sp.ref(cname)[1])
            row["linear=M1"] = ident
            if ident > HP.C_LF_JOULE:
                over["linear=M1"] = ident
    print("\n%-18s %s   (C_LF %g, C_LF_JOULE %g; `two`: fraction of the added bounds)" % (
        RC.lf_id(case), " ".join("%s %.2f" % kv for kv in row.items()), HP.C_LF, HP.C_LF_JOULE))
    assert not over, over
