"""GPU tests of the device BiCGSTAB (Operator.BiCGSTAB / ecm2_operator_bicgstab: BiCGSTABSolver::Mult,
linalg/solvers.cpp:1579-1805, in the fused passes of csrc/k_bicgstab.hip) against the numpy restatement
tests/bicgstab_ref.py on the cases of tests/bicgstab_cases.py -- whose self-gap under three summation orders
(tests/test_bicgstab_reference.py: <= 1e-14 of max|x|, equal iteration counts) is the condition under which
the project's 1e-12 bar may be applied to x after a fixed number of iterations."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import oracle as O
import bicgstab_cases as BC
from helpers import coeff_function, nonaligned, relerr

pytestmark = pytest.mark.gpu

_DEV = {}


def _device(name, marked):
    """(case, Operator(T), Operator(symmetric part), b, ess) on the device, built once per case."""
    import torch
    key = (name, marked)
    if key not in _DEV:
        c = BC.case(name, marked)
        T, S = c.device_forms()
        _DEV[key] = (c, E.Operator(T), E.Operator(S), torch.as_tensor(c.b).cuda(), torch.as_tensor(c.ess).cuda())
    return _DEV[key]


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


@pytest.mark.parametrize("name,marked", BC.CASES)
def test_fixed_work_matches_reference(name, marked):
    """Six iterations (max_iter = 6: not converged), the same work as the reference's: x to 1e-12."""
    import torch
    c, T, S, b, ess = _device(name, marked)
    ref = BC.reference(name, marked, 6)
    assert ref.final_iter == 6 and not ref.converged
    x = torch.empty(c.n, dtype=torch.float64, device="cuda")
    it, nrm = T.BiCGSTAB(b, x, ess=ess, rel_tol=1e-12, max_iter=6, jacobi_of=S)
    err = relerr(x.cpu().numpy(), ref.x)
    print(f"{name} marked={marked}: iterations {it}, ||r|| {nrm:.3e} (reference {ref.final_norm:.3e}), relerr(x) {err:.2e}")
    assert it == 6 and not E.bicgstab_last_converged()
    assert err <= 1e-12


@pytest.mark.parametrize("name,marked", BC.CASES)
def test_converged_matches_reference(name, marked):
    import torch
    c, T, S, b, ess = _device(name, marked)
    ref = BC.reference(name, marked, 1000)
    assert ref.converged
    x = torch.empty(c.n, dtype=torch.float64, device="cuda")
    it, nrm = T.BiCGSTAB(b, x, ess=ess, rel_tol=1e-12, max_iter=1000, jacobi_of=S)
    xh = x.cpu().numpy()
    tol_goal = np.linalg.norm(c.b) * 1e-12
    res_dev, res_ref = c.true_residual(xh), c.true_residual(ref.x)
    err = relerr(xh, ref.x)
    print(f"{name} marked={marked}: iterations {it} (reference {ref.final_iter}), final_norm {nrm:.3e} (tol_goal "
          f"{tol_goal:.3e}), true residual {res_dev:.2e} (reference {res_ref:.2e}), relerr(x) {err:.2e}")
    assert E.bicgstab_last_converged()
    assert abs(it - ref.final_iter) <= 1
    assert nrm < tol_goal
    assert res_dev <= 4.0 * res_ref
    assert err <= 1e-10


def _sym_setup():
    import torch
    if "sym" not in _DEV:
        m = E.Mesh.MakeCartesian3D(4, 4, 8)
        m.set_vertices(nonaligned(m.vertices()))
        fes = E.H1Space(m, 2)
        q1d = O.default_q1d(2)
        alpha = lambda P: 2.0 + np.sin(P[..., 0]) * np.cos(P[..., 1])

        def add(form, ne, P):
            form.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(torch.as_tensor(alpha(P).reshape(ne, -1)).cuda())))
            form.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(
                torch.as_tensor(0.05 * coeff_function(P).reshape(ne, -1)).cuda())))
            form.Assemble()
            return form
        serial = add(E.BilinearForm(fes), fes.ne, O.quad_points(m.element_nodes(), q1d))
        er = E.partition_slabs_z(m, 2)
        forms, parts = [], []
        for r in range(2):
            part = E.Partition(fes, er, r, 2)
            forms.append(add(E.ParBilinearForm(part), part.ne_local, E.quadrature_points_subset(m, q1d, part.elems)))
            parts.append(part)
        _DEV["sym"] = (m, fes, serial, E.ParGroup(forms), parts)
    return _DEV["sym"]


@pytest.mark.parametrize("kind", ["serial", "group"])
def test_symmetric_form_agrees_with_pcg(kind):
    """A form without convection: BiCGSTAB's x == Operator.PCG's to 1e-10, serial and through a 2-slab
    loopback group (4 x 4 x 8, p = 2), whose dots over the concatenated true vectors are already global."""
    import torch
    m, fes, serial, group, parts = _sym_setup()
    n = fes.ndofs
    ess = np.asarray(fes.boundary_dofs())
    b = np.random.default_rng(4).uniform(0, 1, n)
    if kind == "serial":
        op, bd, essd = E.Operator(serial), torch.as_tensor(b).cuda(), torch.as_tensor(ess).cuda()
    else:
        op = E.Operator(group)
        bd = torch.as_tensor(np.concatenate([b[p.owned_global] for p in parts])).cuda()
        idx, o = [], 0
        for p in parts:
            idx.append(np.nonzero(np.isin(p.owned_global, ess))[0] + o)
            o += p.n_owned
        essd = torch.as_tensor(np.concatenate(idx).astype(np.int32)).cuda()
    assert op.size == n
    xp, xb = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    op.PCG(bd, xp, ess=essd, rel_tol=1e-13, max_iter=2000)
    it, nrm = op.BiCGSTAB(bd, xb, ess=essd, rel_tol=1e-13, max_iter=2000, jacobi_of=op)
    assert E.pcg_last_converged() and E.bicgstab_last_converged() and 0 < it < 200
    err = relerr(xb.cpu().numpy(), xp.cpu().numpy())
    print(f"{kind}: BiCGSTAB {it} iterations, against PCG {err:.2e}")
    assert err <= 1e-10


def test_stops():
    import torch
    c, T, S, b, ess = _device("p2", False)
    n = c.n
    x = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    # b = 0: ||r_0|| <= tol_goal, 0 iterations, converged, x = 0
    it, nrm = T.BiCGSTAB(torch.zeros_like(b), x, ess=ess, jacobi_of=S)
    assert (it, nrm) == (0, 0.0) and E.bicgstab_last_converged() and not x.any()
    # every dof essential: the constrained operator is the identity -- alpha = 1, s = 0, x = b bitwise
    every = torch.arange(n, dtype=torch.int32, device="cuda")
    x.fill_(7.0)
    it, nrm = T.BiCGSTAB(b, x, ess=every, jacobi_of=S)
    assert (it, nrm) == (1, 0.0) and E.bicgstab_last_converged() and torch.equal(x, b)
    # max_iter = 1
    it, nrm = T.BiCGSTAB(b, x, ess=ess, max_iter=1, jacobi_of=S)
    assert it == 1 and not E.bicgstab_last_converged() and nrm >= np.linalg.norm(c.b) * 1e-12
    ref = BC.case("p2", False).solve(rel_tol=1e-12, max_iter=1)
    assert relerr(x.cpu().numpy(), ref.x) <= 1e-12 and abs(nrm - ref.final_norm) <= 1e-10 * ref.final_norm


def test_nonfinite_is_numeric_error_and_the_next_solve_works():
    import torch
    c, T, S, b, ess = _device("p2", False)
    ref = BC.reference("p2", False, 1000)
    x = torch.empty(c.n, dtype=torch.float64, device="cuda")

    def good():
        it, _ = T.BiCGSTAB(b, x, ess=ess, rel_tol=1e-12, jacobi_of=S)
        assert E.bicgstab_last_converged() and abs(it - ref.final_iter) <= 1
        assert relerr(x.cpu().numpy(), ref.x) <= 1e-10

    # NaN in b: ||r_0|| is not finite
    bad = b.clone()
    bad[c.n // 2] = float("nan")
    assert _code(lambda: T.BiCGSTAB(bad, x, ess=ess, jacobi_of=S)) == 8
    assert not E.bicgstab_last_converged()
    good()
    # a form with zero coefficients: v = 0, alpha = rho_1 / 0, ||s|| is not finite (found on the device)
    Z = E.BilinearForm(c.fes)
    Z.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(0.0)))
    Z.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(0.0)))
    Z.Assemble()
    assert _code(lambda: E.Operator(Z).BiCGSTAB(b, x)) == 8
    assert not E.bicgstab_last_converged()
    good()


def test_refusals():
    import torch
    c, T, S, b, ess = _device("p2", False)
    n = c.n
    # a misaligned x (a view at an odd element offset), before anything is enqueued
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    assert _code(lambda: T.BiCGSTAB(b, buf[1:], ess=ess, jacobi_of=S)) == 1
    assert not buf.any()
    # a preconditioner's operator of another size
    _, _, S3, _, _ = _device("p3", False)
    assert S3.size != n
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    assert _code(lambda: T.BiCGSTAB(b, x, ess=ess, jacobi_of=S3)) == 1
    # the diagonal of the convective form itself is refused, as the reference aborts in AssembleDiagonalPA
    assert _code(lambda: T.BiCGSTAB(b, x, ess=ess, jacobi_of=T)) == 5
    # operators whose dots need communication: an RCCL rank's form and a member of a loopback group
    m, fes, serial, group, parts = _sym_setup()
    part = E.Partition(fes, np.zeros(fes.ne, np.int32), 0, 1)
    pf = E.ParBilinearForm(part)
    pf.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    pf.Assemble()
    bb = torch.ones(fes.ndofs, dtype=torch.float64, device="cuda")
    xx = torch.empty_like(bb)
    assert _code(lambda: E.Operator(pf).BiCGSTAB(bb, xx)) == 5
    # (a member operator needs contiguous sends: z slabs of the lattice numbering)
    fes_s = E.H1Space(m, 2, E.NUMBERING_STRUCTURED)
    er = E.partition_slabs_z(m, 2)
    forms = []
    for r in range(2):
        f = E.ParBilinearForm(E.Partition(fes_s, er, r, 2, decomposition="overlap"))
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.Assemble()
        forms.append(f)
    member = E.Operator(E.ParGroup(forms), member=0)
    bm = torch.ones(member.size, dtype=torch.float64, device="cuda")
    assert _code(lambda: member.BiCGSTAB(bm, torch.empty_like(bm))) == 5


def test_two_solves_are_bitwise_equal():
    import torch
    c, T, S, b, ess = _device("p3", True)
    outs = []
    for _ in range(2):
        x = torch.empty(c.n, dtype=torch.float64, device="cuda")
        outs.append((T.BiCGSTAB(b, x, ess=ess, rel_tol=1e-12, jacobi_of=S), x))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", ["p2", "p3"])
def test_without_preconditioner(name):
    import torch
    c, T, S, b, ess = _device(name, False)
    ref = BC.reference(name, False, 1000)
    x = torch.empty(c.n, dtype=torch.float64, device="cuda")
    it, nrm = T.BiCGSTAB(b, x, ess=ess, rel_tol=1e-12, max_iter=2000)
    err = relerr(x.cpu().numpy(), ref.x)
    print(f"{name}: {it} iterations without a preconditioner ({ref.final_iter} with), relerr(x) {err:.2e}")
    assert E.bicgstab_last_converged() and nrm < np.linalg.norm(c.b) * 1e-12
    assert err <= 1e-10


def test_example_implicit_convect_on_gpu():
    import os
    import subprocess
    examples = os.path.join(helpers.ROOT, "examples")
    binary = os.path.join(examples, "implicit_convect_heat")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("PASS")
