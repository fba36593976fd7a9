"""GPU tests of the Robin boundary terms: BilinearForm.AddBoundaryIntegrator(MassIntegrator(h)) and
LinearForm.AddBoundaryIntegrator(BoundaryLFIntegrator(g)) against the oracle's volume operator plus
the numpy restatement of the reference's face kernels (tests/bdr_ref.py, pinned by
tests/test_bdr_reference.py: its own float64 error is below 1e-15).  Bar: relerr < helpers.RTOL
(1e-12, the project's parity bar); fields and coefficients are positive, so the boundary term does
not cancel against the volume one.

Meshes, the smallest that reach every path: 2 x 1 x 1 (10 faces, fewer than any workgroup),
5 x 4 x 3 with every vertex moved (94 non-planar faces: more than one workgroup of the thread-per-face
kernel, 64, and of the lane-group kernel, 8, and a multiple of neither), fichera refined once (96
faces, unstructured sharing, the file's 24 attributes), and 8 x 8 x 8 with the structured numbering."""
import os
import subprocess

import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import bioheat as BH
import bdr_ref as R
from helpers import ROOT, RTOL, relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALPHA, BETA = 2.0, 0.7   # the volume form M_alpha + K_beta


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
    """Every kernel mode the order allows (the volume rule is the default p + 2)."""
    return ([E.KERNEL_TPE] if p <= 2 else []) + [E.KERNEL_LINE, E.KERNEL_WPE, E.KERNEL_UNFUSED]


_SPACES, _REFS = {}, {}


def space(name, p, numbering=E.NUMBERING_ENTITY):
    """Mesh, space, positive input, and the volume reference (computed once, left unchanged)."""
    key = (name, p, numbering)
    if key not in _SPACES:
        if name == "cube8":
            m = E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3)
        else:
            m = R.MESHES[name](E)
        fes = E.H1Space(m, p, numbering)
        X = fes.dof_coords()
        x = R.positive_field(X)
        op = O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=ALPHA, beta=BETA)
        _SPACES[key] = dict(mesh=m, fes=fes, X=X, x=x, op=op, y_vol=op.mult(x), d_vol=op.diagonal())
    return _SPACES[key]


def bref(name, p, q1d, numbering=E.NUMBERING_ENTITY):
    key = (name, p, q1d, numbering)
    if key not in _REFS:
        s = space(name, p, numbering)
        m, fes = s["mesh"], s["fes"]
        _REFS[key] = R.BdrRef(p, q1d, fes.boundary_map(), m.GetBdrAttributes(), fes.ndofs, bnodes=m.boundary_nodes())
    return _REFS[key]


def marker_cases(mesh, q1d):
    """name -> [(h, marker)]: unmarked constant; one attribute, per-point h; two integrators whose
    masks overlap (a constant on the odd attributes and 3, per-point values on 3 and up)."""
    n = int(mesh.GetBdrAttributes().max())
    hq = R.h_points(R.face_points(mesh.boundary_nodes(), q1d))
    one = [1 if a + 1 == 3 else 0 for a in range(n)]
    odd3 = [1 if (a + 1) % 2 == 1 or a + 1 == 3 else 0 for a in range(n)]
    hi = [1 if a + 1 >= 3 else 0 for a in range(n)]
    return {"unmarked": [(12.5, None)], "one": [(hq, one)], "two": [(12.5, odd3), (hq, hi)]}


def coeff(h):
    return E.ConstantCoefficient(h) if np.ndim(h) == 0 else E.QuadratureCoefficient(dev(h))


def make_form(s, integ, bq=0, **kw):
    f = E.BilinearForm(s["fes"], **kw)
    f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(ALPHA)))
    f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(BETA)))
    if integ is not None:
        f.SetBoundary(bq)
        for h, mk in integ:
            f.AddBoundaryIntegrator(E.MassIntegrator(coeff(h)), mk)
    f.Assemble()
    return f


def mult(f, x):
    y = torch.full_like(x, float("nan"))   # (Mult overwrites)
    f.Mult(x, y)
    return y


def diagonal(f, n):
    d = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    f.AssembleDiagonal(d)
    return d


CASES = [("small", 1), ("small", 2)] + [(n, p) for n in ("perturbed", "fichera") for p in (1, 2, 3, 4)]


@pytest.mark.parametrize("dq", [1, 2])
@pytest.mark.parametrize("name,p", CASES)
def test_mult_and_diagonal(name, p, dq):
    """A x = oracle Mult + checker H x and diag A = oracle diagonal + checker diagonal: both face
    rules (p + 1, p + 2), constant and per-point h, unmarked / one attribute / two overlapping
    integrators; the two-integrator case in every kernel mode and with the atomic scatter."""
    s = space(name, p)
    q1d = p + dq
    ref = bref(name, p, q1d)
    xd = dev(s["x"])
    for cname, integ in marker_cases(s["mesh"], q1d).items():
        y_ref = ref.mult(integ, s["x"], s["y_vol"])
        d_ref = ref.diagonal(integ, s["d_vol"])
        runs = [dict(kernel=E.KERNEL_AUTO)]
        if cname == "two":
            runs = [dict(kernel=k) for k in modes(p)] + [dict(kernel=E.KERNEL_AUTO, scatter="atomic")]
        for kw in runs:
            f = make_form(s, integ, bq=0 if dq == 1 else q1d, **kw)
            nbe, ni, nact, q = f.BoundaryInfo()
            keep = np.zeros(nbe, bool)
            for _, mk in integ:
                keep |= R.marker_keep(ref.attr, mk)
            assert (nbe, ni, nact, q) == (ref.nbe, len(integ), int(keep.sum()), q1d)
            assert f.EnergyParts() == 0
            ey = relerr(host(mult(f, xd)), y_ref)
            ed = relerr(host(diagonal(f, s["fes"].ndofs)), d_ref)
            print(f"{name} p={p} q1d={q1d} {cname} {kw}: mult {ey:.2e} diag {ed:.2e} "
                  f"(boundary share {relerr(y_ref, s['y_vol']):.2e})")
            assert ey < RTOL and ed < RTOL, (cname, kw, ey, ed)


def test_structured_numbering():
    """8 x 8 x 8, p = 2, structured (lattice) numbering: the regular-block kernel's output plus the
    face pass."""
    s = space("cube8", 2, E.NUMBERING_STRUCTURED)
    ref = bref("cube8", 2, 3, E.NUMBERING_STRUCTURED)
    integ = marker_cases(s["mesh"], 3)["two"]
    f = make_form(s, integ)
    assert relerr(host(mult(f, dev(s["x"]))), ref.mult(integ, s["x"], s["y_vol"])) < RTOL
    assert relerr(host(diagonal(f, s["fes"].ndofs)), ref.diagonal(integ, s["d_vol"])) < RTOL


@pytest.mark.parametrize("name,p,dq", [("perturbed", 2, 1), ("perturbed", 3, 2), ("fichera", 1, 1), ("fichera", 4, 1)])
def test_boundary_qdata(name, p, dq):
    """BoundaryQData against the checker's pa_data: corner geometry, then a given detJ array (the
    corners' detJ times a smooth positive factor, so a swap of the two sources shows); zeros on the
    faces the marker excludes."""
    s = space(name, p)
    q1d = p + dq
    ref = bref(name, p, q1d)
    m = s["mesh"]
    integ = marker_cases(m, q1d)["two"]
    f = make_form(s, integ, bq=q1d)
    for i, (h, mk) in enumerate(integ):
        qd = f.BoundaryQData(i)
        assert relerr(qd, ref.pa_data(h, mk)) < RTOL
        assert np.all(qd[~R.marker_keep(ref.attr, mk)] == 0.0)
    factor = 1.0 + 0.25 * np.cos(R.face_points(m.boundary_nodes(), q1d)[..., 0])
    detj = ref.detJ * factor
    ref2 = R.BdrRef(p, q1d, ref.bmap, ref.attr, ref.ndofs, detj=detj)
    f2 = E.BilinearForm(s["fes"])
    f2.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(ALPHA)))
    f2.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(BETA)))
    f2.SetBoundary(q1d)
    f2.SetBoundaryDetJ(dev(detj))
    for h, mk in integ:
        f2.AddBoundaryIntegrator(E.MassIntegrator(coeff(h)), mk)
    f2.Assemble()
    for i, (h, mk) in enumerate(integ):
        assert relerr(f2.BoundaryQData(i), ref2.pa_data(h, mk)) < RTOL
    assert relerr(f2.BoundaryQData(1), ref.pa_data(*integ[1])) > 1e-3   # the array, not the corners
    assert relerr(host(mult(f2, dev(s["x"]))), ref2.mult(integ, s["x"], s["y_vol"])) < RTOL
    # the linear form takes the same array
    lf = E.LinearForm(s["fes"])
    lf.SetBoundary(q1d)
    lf.SetBoundaryDetJ(dev(detj))
    for g, mk in integ:
        lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
    assert relerr(host(lf_assemble(lf, s["fes"].ndofs)), ref2.assemble(integ)) < RTOL


def lf_assemble(lf, n):
    b = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")  # (Assemble overwrites)
    lf.Assemble(b)
    return b


@pytest.mark.parametrize("name,p", CASES)
def test_linear_form(name, p):
    """BoundaryLFIntegrator: boundary-only forms at the default, p + 1 and p + 2 rules (constant and
    per-point g, markers), then domain + two boundary integrators with the order of addition kept."""
    import lform_ref as LR
    s = space(name, p)
    m, fes = s["mesh"], s["fes"]
    for q1d in sorted({R.lf_default_q1d(p), p + 1, p + 2}):
        ref = bref(name, p, q1d)
        for cname, integ in marker_cases(m, q1d).items():
            lf = E.LinearForm(fes)
            lf.SetBoundary(0 if q1d == R.lf_default_q1d(p) else q1d)
            for g, mk in integ:
                lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
            err = relerr(host(lf_assemble(lf, fes.ndofs)), ref.assemble(integ))
            print(f"{name} p={p} q1d={q1d} {cname}: {err:.2e}")
            assert err < RTOL, (q1d, cname, err)
    # domain (default rule p + 1) + boundary (default rule), the boundary added after the domain part
    qb = R.lf_default_q1d(p)
    ref = bref(name, p, qb)
    integ = marker_cases(m, qb)["two"]
    dref = LR.LFRef(p, p + 1, fes.gather_map(), fes.ndofs, enodes=m.element_nodes())
    src = {"kind": "constant", "value": 2.5}
    lf = E.LinearForm(fes)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.ConstantCoefficient(2.5)))
    for g, mk in integ:
        lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(coeff(g)), mk)
    b1 = lf_assemble(lf, fes.ndofs)
    assert relerr(host(b1), ref.assemble(integ, dref.assemble([(src, None)]))) < RTOL
    assert torch.equal(b1, lf_assemble(lf, fes.ndofs))   # bitwise repeatable


@pytest.mark.parametrize("p", [2, 3])
def test_determinism(p):
    """No atomics in the face passes: two Mults, a Mult after a second Assemble, the Mult of a second
    form built the same way, and two diagonals are bitwise equal (partial-sum scatter)."""
    s = space("perturbed", p)
    integ = marker_cases(s["mesh"], p + 1)["two"]
    xd = dev(s["x"])
    f = make_form(s, integ)
    y1, y2 = mult(f, xd), mult(f, xd)
    assert torch.equal(y1, y2)
    f.Assemble()
    assert torch.equal(y1, mult(f, xd))
    assert torch.equal(diagonal(f, s["fes"].ndofs), diagonal(f, s["fes"].ndofs))
    g = make_form(s, integ)
    assert torch.equal(y1, mult(g, xd))


def test_no_boundary_integrator_is_a_no_op():
    """A form with the boundary set but no boundary integrator, and one whose only boundary integrator
    has an all-zero marker, give bitwise the Mult and diagonal of the form without boundary data."""
    for p in (2, 3):
        s = space("perturbed", p)
        xd = dev(s["x"])
        n = s["fes"].ndofs
        plain = make_form(s, None)
        y0, d0 = mult(plain, xd), diagonal(plain, n)
        empty = make_form(s, [])
        assert empty.BoundaryInfo()[1:3] == (0, 0)
        zero = make_form(s, [(12.5, [0] * 6)])
        assert zero.BoundaryInfo()[1:3] == (1, 0)
        for f in (empty, zero):
            assert torch.equal(y0, mult(f, xd))
            # (the p >= 3 volume diagonal is summed with atomics: two forms agree to rounding only)
            d = diagonal(f, n)
            assert torch.equal(d0, d) if p == 2 else relerr(host(d), host(d0)) < 1e-14
        lf0 = E.LinearForm(s["fes"])
        lf0.AddDomainIntegrator(E.DomainLFIntegrator(E.ConstantCoefficient(2.5)))
        lf1 = E.LinearForm(s["fes"])
        lf1.AddDomainIntegrator(E.DomainLFIntegrator(E.ConstantCoefficient(2.5)))
        lf1.AddBoundaryIntegrator(E.BoundaryLFIntegrator(E.ConstantCoefficient(3.0)), [0] * 6)
        assert torch.equal(lf_assemble(lf0, n), lf_assemble(lf1, n))


def test_pcg_on_the_snapshot_kernel_with_robin():
    """8 x 8 x 8, p = 2, structured numbering, the diffusion coefficient a GridFunctionCoefficient (the
    coefficient-snapshot kernel, which folds (A d, d) into its Mult when there is no boundary term),
    Robin on attribute 3, Dirichlet on attribute 5; Jacobi-PCG at rel_tol 1e-10 from x = 0.  CGSolver
    stops at (B r, r) <= rel_tol^2 (B r0, r0); checked with the REFERENCE operator (oracle Mult +
    checker H, constrained rows) and the reference diagonal D:
        sqrt(r^T D^-1 r) <= 2 rel_tol sqrt(b^T D^-1 b),  r = b - A_ref u
    (the factor 2 covers the recurrence-vs-true-residual gap and the 1e-12 operator parity, both orders
    of magnitude below 1e-10).  Fails if the energy fold drops d^T H d or the Jacobi diagonal lacks the
    face term."""
    p, q1d, rel_tol = 2, 4, 1e-10
    m = E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3)
    fes = E.H1Space(m, p, E.NUMBERING_STRUCTURED)
    X, gm = fes.dof_coords(), fes.gather_map()
    kfield = 0.5 * (1.0 + 0.4 * np.sin(2.0 * X[:, 0]) * np.cos(X[:, 1]) + 0.2 * X[:, 2])
    kq = BH.temperature_at_quadrature(kfield, gm, p, q1d)
    op = O.OracleOperator(m.element_nodes(), gm, fes.ndofs, p, alpha=None, beta=kq)
    ref = R.BdrRef(p, p + 1, fes.boundary_map(), m.GetBdrAttributes(), fes.ndofs, bnodes=m.boundary_nodes())
    robin = [(40.0, [0, 0, 1, 0, 0, 0])]
    ess = np.unique(fes.boundary_map()[m.GetBdrAttributes() == 5])
    kd = dev(kfield)

    plain = E.BilinearForm(fes)
    plain.AddDomainIntegrator(E.DiffusionIntegrator(E.GridFunctionCoefficient(kd)))
    plain.Assemble()
    assert plain.CoefficientSnapshot() and plain.EnergyParts() > 0   # the fold is on without a boundary term

    f = E.BilinearForm(fes)
    f.AddDomainIntegrator(E.DiffusionIntegrator(E.GridFunctionCoefficient(kd)))
    f.AddBoundaryIntegrator(E.MassIntegrator(E.ConstantCoefficient(40.0)), robin[0][1])
    f.Assemble()
    assert f.CoefficientSnapshot()
    assert f.EnergyParts() == 0

    b = R.positive_field(X)
    b[ess] = 0.0
    u = torch.zeros(fes.ndofs, dtype=torch.float64, device="cuda")
    iters, _ = f.PCG(dev(b), u, ess=dev(ess, torch.int32), rel_tol=rel_tol, max_iter=2000, jacobi=True)
    assert E.pcg_last_converged() and 0 < iters < 2000
    uh = host(u)

    def a_ref(v):
        v0 = v.copy()
        v0[ess] = 0.0
        y = ref.mult(robin, v0, op.mult(v0))
        y[ess] = v[ess]
        return y

    D = ref.diagonal(robin, op.diagonal())
    D[ess] = 1.0
    r = b - a_ref(uh)
    lhs, rhs = np.sqrt(r @ (r / D)), np.sqrt(b @ (b / D))
    print(f"PCG {iters} iterations: sqrt(r D^-1 r) = {lhs:.3e}, rel_tol sqrt(b D^-1 b) = {rel_tol * rhs:.3e}")
    assert lhs <= 2.0 * rel_tol * rhs
    # and the operator the solver applied is the reference's
    assert relerr(host(mult(f, dev(uh))), ref.mult(robin, uh, op.mult(uh))) < RTOL


def _code(fn):
    with pytest.raises(E.ECM2Error) as ei:
        fn()
    code = ei.value.code
    del ei   # (the exception's traceback holds this frame and fn's forms: no cycle left for a later GC)
    return code


def test_errors(tmp_path):
    s = space("perturbed", 2)
    fes = s["fes"]
    f = E.BilinearForm(fes)
    # a boundary integrator before set_boundary (the C ABI; the Python mirror sets the boundary itself)
    one = np.array([1.0])
    rc = E._lib.ecm2_pa_form_add_boundary_integrator(f._h, E.MASS, E.COEFF_CONSTANT, one.ctypes.data, None, 0)
    assert rc == 3, rc                                                   # ECM2_ERR_STATE
    lf = E.LinearForm(fes)
    rc = E._lib.ecm2_linear_form_add_boundary_integrator(lf._h, E.COEFF_CONSTANT, one.ctypes.data, None, 0)
    assert rc == 3, rc
    # an unsupported rule
    assert _code(lambda: f.SetBoundary(5)) == 5                           # ECM2_ERR_UNSUPPORTED (p + 3)
    assert _code(lambda: f.SetBoundary(2)) == 5
    assert _code(lambda: lf.SetBoundary(5)) == 5
    f.SetBoundary()
    # a diffusion boundary integrator
    assert _code(lambda: f.AddBoundaryIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(1.0)))) == 5
    # an unsupported coefficient kind
    T = dev(s["x"])
    assert _code(lambda: f.AddBoundaryIntegrator(E.MassIntegrator(E.GridFunctionCoefficient(T)))) == 1   # ECM2_ERR_ARG
    assert _code(lambda: lf.AddBoundaryIntegrator(E.BoundaryLFIntegrator(E.GridFunctionCoefficient(T)))) == 1
    # an attribute beyond the marker
    f.AddBoundaryIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)), [1, 1])
    f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    assert _code(f.Assemble) == 1
    # set_boundary on a distributed local form (n_owned < ndofs): the C++ class itself, there is no
    # C entry point that reaches it (tests/cpp/bdr_local_check.cpp)
    pkg = os.path.join(ROOT, "cardiac-ablation-ecm2_amd")
    exe = os.path.join(str(tmp_path), "bdr_local_check")
    subprocess.run(["make", "-s", "-C", pkg, f"OBJ={tmp_path}", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "PASS", r.stdout + r.stderr
