"""GPU parity of the Robin face terms, componentwise, against the extended-precision references
(tests/bdr_ref.py and tests/hp_ref.py in numpy.longdouble):

    |y_i - y_hp,i| <= u (C S_vol,i + C_BDR S_bdr,i)      the bilinear form s (M_alpha + K_beta) + H,
    |d_i - d_hp,i| <= u (C_DIAG dS_vol,i + C_BDR_DIAG dS_bdr,i)      its diagonal,
    |qd - qd_hp| <= C_BDR_QD u W |h| Dabs,   |b_i - b_hp,i| <= C_BDR u S_i      qdata, face linear form,

u = 2^-53, every S the same sums over the magnitudes of every factor.  The volume half is scaled by a
power of two s so that S_vol,i <= S_bdr,i on every dof of a marked face (tests/rhs_cases.py; asserted
in tests/test_bdr_reference.py, which also derives the constants from the float64 checker's own error,
never from a device result): a face error cannot hide behind the volume term, as it can under relerr <
1e-12 over all dofs.  States: uniform(-1, 1), the temperature in celsius and in kelvin, 310.15 + a . x.
tests/test_gpu_boundary.py stays as the coverage of the paths and the ABI.

Outputs are preset to NaN, every dof is checked, every result is computed twice and must repeat bitwise
-- but what sums with atomics: the p >= 3 volume diagonal, the atomic scatter and the workgroup-per-element
kernel (KERNEL_WPE adds every element entry to y with an atomic), which are held to the bound only.  Run
with -s for every case's constants."""
import numpy as np
import pytest

import ecm2_amd as E
import bdr_ref as R
import hp_ref as HP
import lform_ref as LR
import rhs_cases as RC
from cw_cases import STATES

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
LD = np.longdouble


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


def modes(p):
    return ([E.KERNEL_TPE] if p <= 2 else []) + [E.KERNEL_LINE, E.KERNEL_WPE, E.KERNEL_UNFUSED]


def coeff(h):
    return E.ConstantCoefficient(float(h)) if np.ndim(h) == 0 else E.QuadratureCoefficient(dev(h))


def make_form(r, fr, detj=None, **kw):
    """s (M_alpha + K_beta) + the case's boundary integrators at the rule r.q1d."""
    f = E.BilinearForm(r.space.fes, **kw)
    f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(fr["scale"] * RC.ALPHA)))
    f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(fr["scale"] * RC.BETA)))
    f.SetBoundary(0 if r.q1d == r.p + 1 else r.q1d)
    if detj is not None:
        f.SetBoundaryDetJ(dev(detj))
    for h, mk in fr["integ"]:
        f.AddBoundaryIntegrator(E.MassIntegrator(coeff(h)), mk)
    f.Assemble()
    nbe, ni, nact, q = f.BoundaryInfo()
    assert (nbe, ni, nact, q) == (r.lo.nbe, len(fr["integ"]), int(fr["keep"].sum()), r.q1d)
    return f


def twice(run, bitwise, what=""):
    a, b = run(), run()
    torch.cuda.synchronize()
    if bitwise:
        assert torch.equal(a, b), ("two runs differ", what)
    return host(a)


def mult(f, xd):
    y = torch.full_like(xd, float("nan"))   # (Mult overwrites)
    f.Mult(xd, y)
    return y


def diagonal(f, n):
    d = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    f.AssembleDiagonal(d)
    return d


def check_form(r, cname, runs):
    """H x on the four states and the diagonal under the two-term criterion; returns the worst fractions."""
    sp, fr = r.space, r.form_ref(cname)
    worst = [0.0, 0.0]
    for kw in runs:
        atomic = kw.get("scatter") == "atomic" or kw["kernel"] == E.KERNEL_WPE
        f = make_form(r, fr, **kw)
        for s in STATES:
            xd = dev(sp.x[s])
            y = twice(lambda: mult(f, xd), not atomic, (cname, kw, s))
            c = RC.two_term_constant(y, fr["y_hp"][s], fr["S_vol"][s], fr["S_bdr"][s], HP.C)
            worst[0] = max(worst[0], c)
            assert c <= 1.0, (cname, kw, s, c)
        d = twice(lambda: diagonal(f, sp.ndofs), r.p <= 2 and not atomic, (cname, kw, "diagonal"))
        cd = HP.constant(d, fr["d_hp"], LD(HP.C_DIAG) * fr["dS_vol"] + LD(HP.C_BDR_DIAG) * fr["dS_bdr"])
        worst[1] = max(worst[1], cd)
        assert cd <= 1.0, (cname, kw, cd)
    return worst


@pytest.mark.parametrize("case", RC.BDR_RULES, ids=[RC.bdr_id(c) for c in RC.BDR_RULES])
def test_mult_and_diagonal_componentwise(case):
    """Both face rules, the three marker cases; the two-integrator overlapping-marker case in every
    kernel mode and with the atomic scatter.  p <= 2 reaches k_bdr_apply_tpf, p >= 3 k_bdr_apply_grp."""
    r = RC.bdr_rule(*case)
    for cname in r.cases():
        runs = [dict(kernel=E.KERNEL_AUTO)]
        if cname == "two":
            runs = [dict(kernel=k) for k in modes(r.p)] + [dict(kernel=E.KERNEL_AUTO, scatter="atomic")]
        wy, wd = check_form(r, cname, runs)
        print("\n%-18s %-8s volume scale %-9g Mult %.3f diagonal %.3f of u (C S_vol + C_BDR S_bdr) "
              "(C %g, C_DIAG %g, C_BDR %g, C_BDR_DIAG %g)" % (RC.bdr_id(case), cname, r.form_ref(cname)["scale"], wy, wd,
                                                              HP.C, HP.C_DIAG, HP.C_BDR, HP.C_BDR_DIAG))


def test_structured_numbering_componentwise():
    """8 x 8 x 8, p = 2, structured (lattice) numbering: the regular-block kernel's output plus the face
    pass, the two-integrator case on the kelvin state, and the diagonal."""
    r = RC.bdr_rule("cube8", 2, 3)
    sp, fr = r.space, r.form_ref("two")
    f = make_form(r, fr)
    xd = dev(sp.x["kelvin"])
    c = RC.two_term_constant(twice(lambda: mult(f, xd), True), fr["y_hp"]["kelvin"], fr["S_vol"]["kelvin"],
                             fr["S_bdr"]["kelvin"], HP.C)
    cd = HP.constant(twice(lambda: diagonal(f, sp.ndofs), True), fr["d_hp"],
                     LD(HP.C_DIAG) * fr["dS_vol"] + LD(HP.C_BDR_DIAG) * fr["dS_bdr"])
    print(f"\ncube8 structured p=2: Mult {c:.3f}, diagonal {cd:.3f} of the two-term bound (volume scale {fr['scale']:g})")
    assert c <= 1.0 and cd <= 1.0


QD_CASES = [("perturbed", 2, 3), ("perturbed", 3, 5), ("fichera", 1, 2), ("fichera", 4, 5), ("translated", 2, 3)]


@pytest.mark.parametrize("case", QD_CASES, ids=[RC.bdr_id(c) for c in QD_CASES])
def test_boundary_qdata_componentwise(case):
    """BoundaryQData against pa_data within C_BDR_QD u W |h| Dabs, exact zeros on the excluded faces: from
    the corners, then from a caller's detJ array (the corners' detJ times a smooth positive factor; Dabs =
    |detJ|); the face linear form takes the same array."""
    r = RC.bdr_rule(*case)
    sp, fr = r.space, r.form_ref("two")
    factor = 1.0 + 0.25 * np.cos(r.Pf[..., 0])
    detj = r.lo.detJ * factor
    hi2 = R.BdrRef(r.p, r.q1d, sp.bmap, sp.battr, sp.ndofs, detj=detj, dtype=LD)
    out = []
    for hi, dj in ((r.hi, None), (hi2, detj)):
        f = make_form(r, fr, detj=dj)
        for i, (h, mk) in enumerate(fr["integ"]):
            qd = f.BoundaryQData(i)
            assert np.all(qd[~R.marker_keep(r.lo.attr, mk)] == 0.0)
            c = HP.constant(qd.ravel(), hi.pa_data(h, mk).ravel(), hi.pa_bound(h, mk).ravel())
            out.append(c)
            assert c <= HP.C_BDR_QD, (i, dj is not None, c)
    lf = E.LinearForm(sp.fes)
    lf.SetBoundary(r.q1d)
    lf.SetBoundaryDetJ(dev(detj))
    for g, mk in fr["integ"]:
        lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
    cb = HP.constant(twice(lambda: lf_assemble(lf, sp.ndofs), True), hi2.assemble(fr["integ"]), hi2.assemble_bound(fr["integ"]))
    print("\n%-18s qdata corners %.2f %.2f, detJ array %.2f %.2f (C_BDR_QD %g); linear form on the array %.2f (C_BDR %g)" % (
        RC.bdr_id(case), *out, HP.C_BDR_QD, cb, HP.C_BDR))
    assert cb <= HP.C_BDR


def lf_assemble(lf, n):
    b = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")  # (Assemble overwrites)
    lf.Assemble(b)
    return b


@pytest.mark.parametrize("name,p", RC.BDR_SPACES, ids=["%s-p%d" % c for c in RC.BDR_SPACES])
def test_face_linear_form_componentwise(name, p):
    """BoundaryLFIntegrator at the default, p + 1 and p + 2 rules: g = h T_b per point with T_b in kelvin
    on two overlapping markers, a signed g unmarked and on one attribute; then a domain integrator (the
    kelvin temperature as a grid function) plus the boundary ones within C_LF S_dom + C_BDR S_bdr."""
    sp = RC.bdr_space(name, p)
    row = []
    for q1d in RC.lf_rules(name, p):
        r = RC.bdr_rule(name, p, q1d)
        for cname in r.lf_cases():
            integ, b_hp, S = r.lform_ref(cname)
            lf = E.LinearForm(sp.fes)
            lf.SetBoundary(0 if q1d == R.lf_default_q1d(p) else q1d)
            for g, mk in integ:
                lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
            c = HP.constant(twice(lambda: lf_assemble(lf, sp.ndofs), True), b_hp, S)
            row.append("q%d %s %.2f" % (q1d, cname, c))
            assert c <= HP.C_BDR, (q1d, cname, c)
    # domain (default rule p + 1) + boundary (default rule), the boundary added after the domain part
    r = RC.bdr_rule(name, p, R.lf_default_q1d(p))
    integ, b_bdr, S_bdr = r.lform_ref("hTb")
    src = {"kind": "gridfunc", "field": sp.x["kelvin"]}
    dom = HP.cached(("rhs-bdr-dom", name, p), lambda: LR.LFRef(p, p + 1, sp.gm, sp.ndofs, enodes=sp.mesh.element_nodes(),
                                                                dtype=LD, edge_form=True))
    b_dom, S_dom = HP.cached(("rhs-bdr-dom-ref", name, p), lambda: (dom.assemble([(src, None)]), dom.bound([(src, None)])))
    lf = E.LinearForm(sp.fes)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.GridFunctionCoefficient(dev(src["field"]))))
    for g, mk in integ:
        lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
    c = HP.constant(twice(lambda: lf_assemble(lf, sp.ndofs), True), b_dom + b_bdr, LD(HP.C_LF) * S_dom + LD(HP.C_BDR) * S_bdr)
    print("\n%-14s %s | domain + boundary %.3f of u (C_LF S_dom + C_BDR S_bdr)   (C_BDR %g)" % (
        "%s-p%d" % (name, p), ", ".join(row), c, HP.C_BDR))
    assert c <= 1.0
