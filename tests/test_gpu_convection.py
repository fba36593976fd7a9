"""GPU tests of the convection term: BilinearForm.AddDomainIntegrator(ConvectionIntegrator(v, alpha)[, marker])
against the oracle's volume operator plus the numpy restatement of the reference's convection kernels
(tests/conv_ref.py, pinned by tests/test_conv_reference.py: its own float64 error is below 2e-15).  Bar:
relerr < helpers.RTOL (1e-12, the project's parity bar); x is uniform random in [0, 1), the parity tests'
non-cancelling input; y is preset to NaN (Mult overwrites).

This file is the coverage of the paths and the ABI: every volume kernel mode and scatter behind the term,
the E-vector entry points, determinism, the Assemble-time state, the wrapper, the refusals and the
example.  The tight bar -- C x, C^T x and the qdata componentwise against an extended-precision reference,
on the temperature fields the solver applies the operator to, and the Jacobian geometry -- is
tests/test_gpu_convection_componentwise.py's.

Meshes, the smallest at which each path can go wrong: 2 x 1 x 1 (fewer elements than a wave or a sheet
group), 5 x 4 x 3 with every vertex moved (60 non-affine elements: one partial wave), fichera refined once
(56 elements, unstructured sharing), and 8 x 8 x 8 (1 x 0.7 x 1.3, structured numbering) whose marker
selects the 320 elements of five z layers -- more than one workgroup of every kernel (64 elements, or 16 /
10 / 7 sheets).  A z layer of that mesh has 64 elements, so no count of whole layers avoids a multiple of
64; a second marker there adds 27 elements of a sixth layer (347: a multiple of none of 64, 16, 10, 7)."""
import os
import subprocess

import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
import bdr_ref as BR
import conv_ref as R
from conv_cases import cube8_attributes
from helpers import ROOT, RTOL, relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALPHA, BETA = 2.0, 0.7          # the volume form M_alpha + K_beta
CALPHA = 1.7                    # ConvectionIntegrator's alpha
VCONST = np.array([0.8, -0.3, 0.5])


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
    """Every volume kernel mode the order allows (the default rule p + 2)."""
    return ([E.KERNEL_TPE] if p <= 2 else []) + [E.KERNEL_LINE, E.KERNEL_WPE, E.KERNEL_UNFUSED]


_MESH, _SPACES, _REFS, _CX = {}, {}, {}, {}


def mesh_of(name):
    """The mesh with the element attributes the marked cases use (set once)."""
    if name not in _MESH:
        if name == "cube8":
            m = E.Mesh.MakeCartesian3D(8, 8, 8, 1.0, 0.7, 1.3)
            m.SetAttributes(cube8_attributes())
        else:
            m = BR.MESHES[name](E)
            m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32) if name != "small" else np.array([1, 2], np.int32))
        _MESH[name] = m
    return _MESH[name]


MARKER = {"small": [0, 1], "perturbed": [0, 1, 1], "fichera": [0, 1, 1], "cube8": [0, 1, 0]}
NUMBERING = {"cube8": E.NUMBERING_STRUCTURED}


def space(name, p):
    key = (name, p)
    if key not in _SPACES:
        m = mesh_of(name)
        fes = E.H1Space(m, p, NUMBERING.get(name, E.NUMBERING_ENTITY))
        rng = np.random.default_rng(11)
        _SPACES[key] = dict(name=name, p=p, mesh=m, fes=fes, x=rng.uniform(0.0, 1.0, fes.ndofs),
                            w=rng.uniform(0.0, 1.0, fes.ndofs), attr=m.GetAttributes())
    return _SPACES[key]


def refs(name, p, q1d):
    """The checker, the oracle's volume operator and its Mult of x for one (mesh, p, rule): computed once."""
    key = (name, p, q1d)
    if key not in _REFS:
        s = space(name, p)
        m, fes = s["mesh"], s["fes"]
        cr = R.ConvRef(p, q1d, fes.gather_map(), fes.ndofs, m.element_nodes())
        op = O.OracleOperator(m.element_nodes(), fes.gather_map(), fes.ndofs, p, alpha=ALPHA, beta=BETA, q1d=q1d)
        _REFS[key] = dict(cr=cr, op=op, y_vol=op.mult(s["x"]), vpts=R.reference_velocity(cr.P))
    return _REFS[key]


def velocity(name, p, q1d, vname):
    return VCONST if vname == "const" else refs(name, p, q1d)["vpts"]


def keep_of(name, p, marker):
    return None if marker is None else R.marker_keep(space(name, p)["attr"], marker)


def cx_ref(name, p, q1d, vname, marker, transpose, vec="x"):
    """C x (or C^T x) of the checker, cached (marker as a tuple or None)."""
    key = (name, p, q1d, vname, marker, transpose, vec)
    if key not in _CX:
        r = refs(name, p, q1d)
        _CX[key] = r["cr"].mult(velocity(name, p, q1d, vname), space(name, p)[vec], CALPHA,
                                keep_of(name, p, marker), transpose)
    return _CX[key]


def vcoeff(v):
    return E.VectorCoefficient(v if np.ndim(v) == 1 else dev(v))


def make_form(s, q1d, conv=None, volume=True, assemble=True, **kw):
    """q1d: the form's rule; conv: (velocity, marker) or None."""
    f = E.BilinearForm(s["fes"], q1d=0 if q1d == s["p"] + 2 else q1d, **kw)
    if volume:
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(ALPHA)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(BETA)))
    if conv is not None:
        v, marker = conv
        f.AddDomainIntegrator(E.ConvectionIntegrator(vcoeff(v), CALPHA), None if marker is None else list(marker))
    if assemble:
        f.Assemble()
    return f


def mult(f, x, transpose=False):
    y = torch.full_like(x, float("nan"))   # (Mult overwrites)
    (f.MultTranspose if transpose else f.Mult)(x, y)
    return y


CASES = [(n, p, dq) for n in ("small", "perturbed", "fichera", "cube8") for p in (1, 2, 3, 4) for dq in (1, 2)]


def test_cube8_active_counts():
    """The marked counts against the kernels' workgroup sizes (64 elements; 256 // Q^2 sheets, Q = 4, 5, 6)."""
    attr = cube8_attributes()
    layers = int(R.marker_keep(attr, [0, 1, 0]).sum())
    ragged = int(R.marker_keep(attr, [0, 1, 1]).sum())
    groups = [64] + [256 // (q * q) for q in (4, 5, 6)]
    assert layers == 320 and all(layers > g for g in groups)
    assert ragged == 347 and all(ragged > g and ragged % g != 0 for g in groups)


@pytest.mark.parametrize("name,p,dq", CASES)
def test_mult_and_mult_transpose(name, p, dq):
    """A x and A^T x for A = C alone and A = M + K + C: both rules, constant and per-point (y, -x, x)
    velocity, unmarked and marked; ConvectionInfo reports the active count."""
    s = space(name, p)
    q1d = p + dq
    r = refs(name, p, q1d)
    xd = dev(s["x"])
    markers = [None, tuple(MARKER[name])] + ([(0, 1, 1)] if name == "cube8" else [])
    for vname in ("const", "points"):
        v = velocity(name, p, q1d, vname)
        for marker in markers:
            n_act = s["fes"].ne if marker is None else int(keep_of(name, p, marker).sum())
            for volume in (False, True):
                f = make_form(s, q1d, (v, marker), volume=volume)
                assert f.ConvectionInfo() == (True, n_act, n_act > 0)
                assert f.EnergyParts() == 0
                for tr in (False, True):
                    y_ref = cx_ref(name, p, q1d, vname, marker, tr) + (r["y_vol"] if volume else 0.0)
                    err = relerr(host(mult(f, xd, tr)), y_ref)
                    print(f"{name} p={p} q1d={q1d} {vname} marker={marker} volume={volume} transpose={tr}: {err:.2e}")
                    assert err < RTOL, (vname, marker, volume, tr, err)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_volume_kernel_modes_and_atomic_scatter(p):
    """One marked case per order (perturbed, per-point velocity, the default rule) behind every volume
    kernel mode the order allows and behind the atomic scatter: the term is added after whichever ran."""
    name, q1d = "perturbed", p + 2
    s, r = space(name, p), refs(name, p, p + 2)
    marker = tuple(MARKER[name])
    v = velocity(name, p, q1d, "points")
    xd = dev(s["x"])
    for kw in [dict(kernel=k) for k in modes(p)] + [dict(kernel=E.KERNEL_AUTO, scatter="atomic")]:
        f = make_form(s, q1d, (v, marker), **kw)
        for tr in (False, True):
            err = relerr(host(mult(f, xd, tr)), cx_ref(name, p, q1d, "points", marker, tr) + r["y_vol"])
            print(f"p={p} {kw} transpose={tr}: {err:.2e}")
            assert err < RTOL, (kw, tr, err)


@pytest.mark.parametrize("name,p,dq", [(n, p, dq) for n in ("perturbed", "cube8") for p in (1, 2, 3, 4) for dq in (1, 2)])
def test_duality_on_the_device(name, p, dq):
    """<w, C x> - <C^T w, x> is bounded by 1e-12 sum_i |w_i| |C x|_i: the transposed kernel is the
    transpose of the forward one."""
    s = space(name, p)
    q1d = p + dq
    marker = tuple(MARKER[name])
    f = make_form(s, q1d, (velocity(name, p, q1d, "points"), marker), volume=False)
    cx = host(mult(f, dev(s["x"])))
    ctw = host(mult(f, dev(s["w"]), True))
    lhs, bound = abs(s["w"] @ cx - ctw @ s["x"]), 1e-12 * (np.abs(s["w"]) @ np.abs(cx))
    print(f"{name} p={p} q1d={q1d}: |<w, Cx> - <C^T w, x>| = {lhs:.3e}, bound {bound:.3e}")
    assert bound > 0 and lhs <= bound


@pytest.mark.parametrize("name,p,dq", [("small", 1, 2), ("perturbed", 2, 2), ("perturbed", 2, 1), ("fichera", 3, 1),
                                       ("perturbed", 4, 2), ("cube8", 2, 2), ("cube8", 3, 2)])
def test_evector_entry_points_and_qdata(name, p, dq):
    """IntegratorAddMultPA / IntegratorAddMultTransposePA (ye += on E-vectors over all elements: the rows of
    excluded elements stay) and qdata(CONVECTION) ([ne][3][nq], zeros on excluded elements) against the checker."""
    s = space(name, p)
    q1d = p + dq
    cr = refs(name, p, q1d)["cr"]
    marker = tuple(MARKER[name])
    keep = keep_of(name, p, marker)
    v = velocity(name, p, q1d, "points")
    f = make_form(s, q1d, (v, marker))
    pa = cr.pa_data(v, CALPHA, keep)
    qd = f.qdata(E.CONVECTION)
    assert qd.shape == pa.shape and relerr(qd, pa) < RTOL
    assert np.all(qd[~keep] == 0.0)
    rng = np.random.default_rng(3)
    xe = rng.uniform(0.0, 1.0, (cr.ne, cr.nd))
    ye0 = rng.uniform(0.0, 1.0, (cr.ne, cr.nd))
    for tr, fn in ((False, f.IntegratorAddMultPA), (True, f.IntegratorAddMultTransposePA)):
        ye = dev(ye0)
        fn(E.CONVECTION, dev(xe), ye)
        ref = ye0 + (cr.apply_t if tr else cr.apply)(pa, xe)
        got = host(ye)
        assert relerr(got, ref) < RTOL, (tr, relerr(got, ref))
        assert np.array_equal(got[~keep], ye0[~keep])
    # the symmetric integrators' transposed entry point is their plain apply
    a, b = dev(ye0), dev(ye0)
    f.IntegratorAddMultPA(E.DIFFUSION, dev(xe), a)
    f.IntegratorAddMultTransposePA(E.DIFFUSION, dev(xe), b)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name,p", [("perturbed", 2), ("perturbed", 3), ("cube8", 2)])
def test_determinism(name, p):
    """No atomics in the term's two passes: two Mults, a Mult after a second Assemble and the Mult of a
    second form built the same way are bitwise equal (partial-sum scatter of the volume part)."""
    s = space(name, p)
    conv = (velocity(name, p, p + 2, "points"), tuple(MARKER[name]))
    xd = dev(s["x"])
    f = make_form(s, p + 2, conv)
    for tr in (False, True):
        y1 = mult(f, xd, tr)
        assert torch.equal(y1, mult(f, xd, tr))
        f.Assemble()
        assert torch.equal(y1, mult(f, xd, tr))
        assert torch.equal(y1, mult(make_form(s, p + 2, conv), xd, tr))


@pytest.mark.parametrize("p", [2, 3])
def test_marker_that_selects_nothing_is_a_no_op(p):
    """A convection integrator whose marker keeps no element leaves Mult, MultTranspose and AssembleDiagonal
    bitwise those of the form without it, and launches nothing."""
    s = space("perturbed", p)
    xd = dev(s["x"])
    n = s["fes"].ndofs
    plain = make_form(s, p + 2)
    zero = make_form(s, p + 2, (VCONST, (0, 0, 0)))
    assert plain.ConvectionInfo() == (False, 0, False)
    assert zero.ConvectionInfo() == (True, 0, False)
    assert torch.equal(mult(plain, xd), mult(zero, xd))
    assert torch.equal(mult(plain, xd, True), mult(zero, xd, True))
    assert torch.equal(mult(plain, xd), mult(plain, xd, True))   # without convection MultTranspose is Mult
    d0 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    d1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    plain.AssembleDiagonal(d0)
    zero.AssembleDiagonal(d1)
    # (the p >= 3 volume diagonal is summed with atomics: two forms agree to rounding only)
    assert torch.equal(d0, d1) if p == 2 else relerr(host(d1), host(d0)) < 1e-14


def test_velocity_is_read_at_assemble():
    """Assemble-time state: overwriting the velocity tensor after Assemble changes nothing until the next one."""
    name, p, q1d = "perturbed", 2, 4
    s = space(name, p)
    v = velocity(name, p, q1d, "points")
    vt = dev(v)
    f = E.BilinearForm(s["fes"])
    f.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(vt), CALPHA))
    f.Assemble()
    xd = dev(s["x"])
    y1 = mult(f, xd)
    vt.mul_(-2.0)
    torch.cuda.synchronize()
    assert torch.equal(y1, mult(f, xd))
    assert relerr(f.qdata(E.CONVECTION), refs(name, p, q1d)["cr"].pa_data(v, CALPHA)) < RTOL
    f.Assemble()
    assert relerr(host(mult(f, xd)), -2.0 * cx_ref(name, p, q1d, "points", None, False)) < RTOL


def test_operator_wrapper_includes_the_term():
    name, p, q1d = "fichera", 3, 5
    s, r = space(name, p), refs(name, p, 5)
    marker = tuple(MARKER[name])
    f = make_form(s, q1d, (velocity(name, p, q1d, "points"), marker))
    op = E.Operator(f)
    xd = dev(s["x"])
    y = torch.full_like(xd, float("nan"))
    op.Mult(xd, y)
    assert relerr(host(y), cx_ref(name, p, q1d, "points", marker, False) + r["y_vol"]) < RTOL
    assert torch.equal(y, mult(f, xd))
    z = dev(s["w"])
    f.AddMult(xd, z, -0.5)
    assert relerr(host(z), s["w"] - 0.5 * host(y)) < RTOL


def _code(fn):
    with pytest.raises(E.ECM2Error) as ei:
        fn()
    code = ei.value.code
    del ei   # (the exception's traceback holds this frame and fn's forms: no cycle left for a later GC)
    return code


def test_refusals():
    s = space("perturbed", 2)
    fes = s["fes"]
    n = fes.ndofs
    vc = E.VectorCoefficient(VCONST)
    # AssembleDiagonal (ECM2_ERR_UNSUPPORTED), and so Jacobi-PCG; the energy is not folded
    f = make_form(s, 4, (VCONST, None))
    d = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert _code(lambda: f.AssembleDiagonal(d)) == 5
    assert "ConvectionIntegrator" in E._lib.ecm2_last_error().decode()
    assert f.EnergyParts() == 0
    b, u = dev(s["x"]), torch.zeros(n, dtype=torch.float64, device="cuda")
    assert _code(lambda: f.PCG(b, u, jacobi=True)) == 5
    # a scalar coefficient (ECM2_ERR_ARG)
    g = E.BilinearForm(fes)
    assert _code(lambda: g.AddDomainIntegrator(E.ConvectionIntegrator(E.ConstantCoefficient(1.0)))) == 1
    assert _code(lambda: g.AddDomainIntegrator(E.ConvectionIntegrator(E.GridFunctionCoefficient(dev(s["x"]))))) == 1
    # mass keeps refusing vector kinds
    assert _code(lambda: g.AddDomainIntegrator(E.MassIntegrator(vc))) == 1
    # a second convection integrator
    g.AddDomainIntegrator(E.ConvectionIntegrator(vc))
    assert _code(lambda: g.AddDomainIntegrator(E.ConvectionIntegrator(vc, 2.0))) == 5
    # an unsupported rule: p + 3 points
    h = E.BilinearForm(fes, q1d=5)
    assert _code(lambda: h.AddDomainIntegrator(E.ConvectionIntegrator(vc))) == 5
    # an attribute beyond the marker (at Assemble)
    k = E.BilinearForm(fes)
    k.AddDomainIntegrator(E.ConvectionIntegrator(vc), [1, 1])
    assert _code(k.Assemble) == 1
    # the E-vector entry points and the qdata of an integrator that is not there
    plain = make_form(s, 4)
    assert _code(lambda: plain.qdata(E.CONVECTION)) == 1
    # a distributed form
    part = E.Partition(fes, np.zeros(fes.ne, np.int32), 0, 1)
    pf = E.ParBilinearForm(part)
    assert _code(lambda: pf.AddDomainIntegrator(E.ConvectionIntegrator(vc))) == 5
    assert _code(lambda: pf.AddDomainIntegrator(E.ConvectionIntegrator(vc), [1, 1, 1])) == 5


@pytest.mark.parametrize("args", [(), ("1", "3"), ("3", "5"), ("4", "5")])
def test_example_convect_on_gpu(args):
    examples = os.path.join(ROOT, "examples")
    binary = os.path.join(examples, "convect_heat")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary, *args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("PASS")
    assert "converged 1" in r.stdout
