"""GPU parity, componentwise: every kernel path's Mult and AssembleDiagonal against the extended-
precision reference (tests/hp_ref.py),

    max_i |y_i - y_hp,i| / (u S_i) <= C      (diagonal: C_DIAG),      u = 2^-53,

S the same sums over the magnitudes of every factor.  Unlike the global relerr <= 1e-12 of the other
parity tests this holds for inputs whose sums cancel -- the temperature fields the solver applies the
operator to (celsius, kelvin, linear; K x cancels 5 to 18 digits per entry there) -- and it is as tight
as the arithmetic: a 1e-12 relative error at one quadrature point is 190 - 620 units
(test_hp_reference.py).  C and C_DIAG come from the CPU oracle's own constants, never from a device
result.  The case matrix (tests/cw_cases.py) takes the existing suite's smallest mesh for every path and
asserts the kernel, the layout and the path-specific facts, so that a case cannot fall to another
path.  Run with -s for every case's constants.  Also here: the host refusal of an unaligned x in the
device PCG."""
import numpy as np
import pytest

import ecm2_amd as E
import hp_ref as HP
import cw_cases as CW

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


def coefficient(spec, ne, field):
    """The device coefficient of a form's mass / diff entry (cw_cases.Space.form)."""
    if spec[0] == "quad":
        return E.QuadratureCoefficient(dev(np.asarray(spec[1]).reshape(ne, -1)))
    if spec[0] == "affine":
        return E.AffineGridFunctionCoefficient(field, *spec[1:])
    assert spec[0] == "perfusion", spec
    return E.PerfusionCoefficient(field, *spec[1:])


def add_integrators(form, f, ne, field):
    if f["mass"] is not None:
        form.AddDomainIntegrator(E.MassIntegrator(coefficient(f["mass"], ne, field)))
    if f["diff"] is not None:
        form.AddDomainIntegrator(E.DiffusionIntegrator(coefficient(f["diff"], ne, field)))


def serial_apply(case, fname, sp, f):
    """The assembled serial form with its path asserted: (mult(x) -> y, diagonal() -> d), host arrays."""
    fes = sp.fes
    Td = dev(sp.T)
    form = E.BilinearForm(fes, kernel=case.kernel, **case.kw)
    add_integrators(form, f, fes.ne, Td)
    form.Assemble()
    info = form.info()
    assert info["kernel"] == case.resolved, info
    assert info["layout"] == case.layout(fname), info
    has_diff = f["diff"] is not None
    if case.flags.get("snapshot"):
        on, mvals, at_pt = form.SnapshotInfo()
        assert on and form.CoefficientSnapshot()
        assert mvals == {"Ks": 0, "MKs": 1, "PKs": 2}[fname] and at_pt == (fname == "PKs")
        assert form.FluxDiagonal()                      # axis-aligned: the diagonal flux product
        Td.fill_(1.0e3)                                 # the operator keeps the Assemble-time field
    if case.flags.get("lattice") and has_diff:          # every block a lattice brick: the two-wave kernel
        lat, units, _ = form.AddressingInfo()
        lslot, _ = form.PlanInfo()
        assert (lat if case.numbering == CW.STRUCTURED else lslot) == units == fes.ne // 64
    if case.resolved == E.KERNEL_LINE:
        nb, depth = form.BrickInfo()
        if fname in ("MK", "MKphys") and case.mesh in ("na645", "cart4"):
            assert nb > 0 and depth == 1                # 2 x 2 x 1 bricks (+ leftover elements on na645)
        elif f["mass"] is None or not has_diff:
            assert nb == 0                              # a single integrator: the per-element line kernel
        if case.mesh == "cart4" and has_diff:
            assert form.FluxDiagonal()

    def mult(x):
        y = torch.full((fes.ndofs,), float("nan"), dtype=torch.float64, device="cuda")
        form.Mult(dev(x), y)
        return host(y)

    def diagonal():
        d = torch.full((fes.ndofs,), float("nan"), dtype=torch.float64, device="cuda")
        form.AssembleDiagonal(d)
        return host(d)
    return mult, diagonal


def group_apply(case, fname, sp, f):
    """The loopback group of z-slabs (OVERLAP decomposition, overlapped schedule), gathered to the
    global dof order."""
    m, fes, nr = sp.mesh, sp.fes, case.flags["group"]
    er = E.partition_slabs_z(m, nr)
    nq = sp.q1d ** 3
    forms, parts = [], []
    for r in range(nr):
        part = E.Partition(fes, er, r, nr, decomposition="overlap")
        pf = E.ParBilinearForm(part, schedule="overlap")
        for kind, integ in (("mass", E.MassIntegrator), ("diff", E.DiffusionIntegrator)):
            if f[kind] is not None:
                assert f[kind][0] == "quad"
                vals = np.asarray(f[kind][1]).reshape(fes.ne, nq)[part.elems]
                pf.AddDomainIntegrator(integ(E.QuadratureCoefficient(dev(vals))))
        pf.Assemble()
        info = pf.info()
        assert info["kernel"] == case.resolved and info["layout"] == case.layout(fname), info
        forms.append(pf)
        parts.append(part)
    group = E.ParGroup(forms)
    assert sum(p.n_owned for p in parts) == fes.ndofs

    def gather(outs):
        torch.cuda.synchronize()
        y = np.full(fes.ndofs, np.nan)
        for part, t in zip(parts, outs):
            y[part.owned_global] = t.cpu().numpy()
        return y

    def nan_outputs():
        return [torch.full((p.n_owned,), float("nan"), dtype=torch.float64, device="cuda") for p in parts]

    def mult(x):
        ys = nan_outputs()
        group.Mult([dev(x[p.owned_global]) for p in parts], ys)
        return gather(ys)

    def diagonal():
        ds = nan_outputs()
        group.AssembleDiagonal(ds)
        return gather(ds)
    return mult, diagonal


@pytest.mark.parametrize("case,fname", CW.CASE_FORMS, ids=["%s-%s" % (c.id, f) for c, f in CW.CASE_FORMS])
def test_mult_and_diagonal_componentwise(case, fname):
    sp = CW.space(case.mesh, case.p, case.numbering)
    f = sp.form(fname)
    mult, diagonal = (group_apply if "group" in case.flags else serial_apply)(case, fname, sp, f)
    consts = {s: HP.constant(mult(sp.x[s]), f["y_hp"][s], f["S"][s]) for s in CW.STATES}
    c_diag = HP.constant(diagonal(), f["d_hp"], f["dS"])
    print("\n%-34s %-7s Mult %s | diag %6.2f   (C %g, C_DIAG %g)" % (
        case.id, fname, " ".join("%s %5.2f" % (s, consts[s]) for s in CW.STATES), c_diag, HP.C, HP.C_DIAG))
    assert max(consts.values()) <= HP.C, consts
    assert c_diag <= HP.C_DIAG, c_diag


@pytest.mark.parametrize("entry", ["form", "operator"])
def test_pcg_refuses_unaligned_x(entry):
    """The device PCG's update kernels move two entries of the caller's x per access: a contiguous view
    at an odd element offset (8-byte aligned only) is refused on the host with ECM2_ERR_ARG before
    anything is enqueued -- the buffer is untouched -- and the aligned call still solves."""
    sp = CW.space("na543", 2)
    f = sp.form("MK")
    fes = sp.fes
    form = E.BilinearForm(fes)
    add_integrators(form, f, fes.ne, None)
    form.Assemble()
    solver = form if entry == "form" else E.Operator(form)
    n = fes.ndofs
    b = dev(np.random.default_rng(6).uniform(-1, 1, n))
    buf = torch.full((n + 2,), 7.0, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[1:n + 1]
    assert x.is_contiguous() and x.data_ptr() % 16 == 8
    with pytest.raises(E.ECM2Error) as ei:
        solver.PCG(b, x, rel_tol=1e-10, max_iter=500)
    assert ei.value.code == 1 and "16-byte" in str(ei.value)          # ECM2_ERR_ARG
    assert bool((host(buf) == 7.0).all())
    xa = buf[:n]
    assert xa.data_ptr() % 16 == 0
    it, nrm = solver.PCG(b, xa, rel_tol=1e-10, max_iter=500)
    assert E.pcg_last_converged() and 0 < it < 500
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    form.Mult(xa, y)
    res = host(y) - host(b)
    assert np.abs(res).max() <= 1e-8 * np.abs(host(b)).max()
