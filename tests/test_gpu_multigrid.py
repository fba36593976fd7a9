"""GPU tests of the device multigrid cycle (Multigrid / ecm2_multigrid_*: Multigrid's V-cycle, fem/multigrid.cpp:
106-232, with GeometricMultigrid's constrained prolongations, :296-309) and of the PCG it preconditions
(Operator.PCG(prec=Multigrid) / ecm2_operator_pcg_mg: CGSolver::Mult, linalg/solvers.cpp:869-1004) against the numpy
restatement tests/mg_ref.py on the cases of tests/mg_cases.py.

The fixed-work bound (DESIGN.md section 4e's method): the reference's spread of x after six iterations, and of one
cycle's y, under its three summation orders is <= 4.95e-16 of max|x| on every case and for both coarse solves
(tests/test_mg_reference.py measures and asserts <= 1e-13), so the device is held to 1e-12 of max|x|.
Every output is preset to NaN; the smoothers take the reference's eigenvalue estimates, so both sides do the same
work."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import mg_cases as MC
from helpers import relerr

pytestmark = pytest.mark.gpu

FIXED = 1e-12
COARSE8 = (0.0, 8)   # a coarse PCG of exactly 8 iterations
ERR_ARG, ERR_UNSUPPORTED, ERR_NUMERIC = 1, 5, 8
_DEV = {}


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


class Dev:
    """One case on the device: per level the Operator, the essential list and the smoother; the transfers; b."""

    def __init__(self, name, eig_scale=1.0):
        import torch
        c = self.c = MC.case(name, eig_scale)
        self.ops = [E.Operator(l.device_form()) for l in c.levels]
        self.ess = [torch.as_tensor(l.ess).cuda() for l in c.levels]
        self.sm = [E.ChebyshevSmoother(A, ess=e, order=MC.SMOOTHER_ORDER, max_eig_estimate=l.max_eig)
                   for A, e, l in zip(self.ops, self.ess, c.levels)]
        self.tr = [E.PRefinementTransfer(a.fes, b.fes) for a, b in zip(c.levels[:-1], c.levels[1:])]
        self.A, self.ess_f = self.ops[-1], self.ess[-1]
        self.b = torch.as_tensor(c.b).cuda()

    def mg(self, coarse_pcg=None):
        return E.Multigrid(self.ops, self.sm, self.tr, self.ess, coarse_pcg=coarse_pcg)


def _device(name, eig_scale=1.0):
    if (name, eig_scale) not in _DEV:
        _DEV[name, eig_scale] = Dev(name, eig_scale)
    return _DEV[name, eig_scale]


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


@pytest.mark.parametrize("name", MC.CYCLE_CASES)
@pytest.mark.parametrize("coarse", [None, COARSE8])
def test_cycle_matches_reference(name, coarse):
    import torch
    d = _device(name)
    B = d.mg(coarse)
    want = d.c.cycle(coarse)(d.c.b)
    y, y2 = _nan(d.c.n), _nan(d.c.n)
    B.Mult(d.b, y)
    B.Mult(d.b, y2)
    yh = y.cpu().numpy()
    err = relerr(yh, want)
    print(f"{name} coarse {coarse}: relerr(y) {err:.2e}")
    assert err <= FIXED
    assert torch.equal(y, y2)
    # the essential entries are the reference's
    ess = d.c.fine.ess
    assert np.abs(yh[ess] - want[ess]).max() <= FIXED * np.abs(want).max()
    assert torch.equal(d.b.cpu(), torch.as_tensor(d.c.b))


@pytest.mark.parametrize("name", MC.CYCLE_CASES)
def test_cycle_is_symmetric(name):
    import torch
    d = _device(name)
    B = d.mg()
    rng = np.random.default_rng(3)
    u, v = torch.as_tensor(rng.uniform(0, 1, d.c.n)).cuda(), torch.as_tensor(rng.uniform(0, 1, d.c.n)).cuda()
    y = _nan(d.c.n)
    B.Mult(u, y)
    fwd = float(v @ y)
    B.Mult(v, y)
    tr = float(u @ y)
    print(f"{name}: symmetry {abs(fwd - tr) / abs(fwd):.2e}")
    assert abs(fwd - tr) <= 1e-13 * abs(fwd)


@pytest.mark.parametrize("name", MC.CYCLE_CASES)
@pytest.mark.parametrize("coarse", [None, COARSE8])
def test_pcg_fixed_work_matches_reference(name, coarse):
    d = _device(name)
    ref = MC.reference(name, "mg", coarse, 6)
    assert ref.final_iter == 6 and not ref.converged
    x = _nan(d.c.n)
    it, nrm = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=6, prec=d.mg(coarse))
    err = relerr(x.cpu().numpy(), ref.x)
    print(f"{name} coarse {coarse}: iterations {it}, final_norm {nrm:.3e} (reference {ref.final_norm:.3e}), relerr(x) {err:.2e}")
    assert it == 6 and not E.pcg_last_converged()
    assert err <= FIXED


@pytest.mark.parametrize("name", MC.CASES)
def test_pcg_iteration_counts(name):
    """Coarse (a): the reference's count.  ex26's coarse PCG: at most the reference's count + 1 -- the inner stop at
    1e-2 may fall one inner iteration to either side under rounding, which changes the preconditioner slightly; no
    more than that one outer iteration is allowed for."""
    d = _device(name)
    n_a, n_b = MC.COUNTS[name][2], MC.COUNTS[name][3]
    ref = MC.reference(name, "mg", None, 1000)
    assert ref.final_iter == n_a
    x = _nan(d.c.n)
    it, nrm = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=1000, prec=d.mg())
    assert E.pcg_last_converged()
    err = relerr(x.cpu().numpy(), ref.x)
    print(f"{name} coarse smoother: {it} iterations (reference {n_a}), relerr(x) {err:.2e}")
    assert it == n_a and err <= 1e-10
    x = _nan(d.c.n)
    itb, _ = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=1000, prec=d.mg(MC.EX26_COARSE))
    assert E.pcg_last_converged()
    errb = relerr(x.cpu().numpy(), ref.x)
    print(f"{name} coarse PCG {MC.EX26_COARSE}: {itb} iterations (reference {n_b}), relerr(x) {errb:.2e}")
    assert itb <= n_b + 1 and errb <= 1e-10


def test_stops():
    """tests/test_gpu_chebyshev.py::test_stops through the new path."""
    import torch
    d = _device("moved543")
    n, A, b, ess = d.c.n, d.A, d.b, d.ess_f
    for coarse in (None, MC.EX26_COARSE):
        B = d.mg(coarse)
        # b = 0: nom = 0 <= r0, 0 iterations, converged, x = 0
        x = _nan(n)
        it, nrm = A.PCG(torch.zeros_like(b), x, ess=ess, prec=B)
        assert (it, nrm) == (0, 0.0) and E.pcg_last_converged() and not x.any()
        # max_iter = 1
        x = _nan(n)
        it, nrm = A.PCG(b, x, ess=ess, max_iter=1, prec=B)
        ref = d.c.solve("mg", coarse, rel_tol=1e-12, max_iter=1)
        assert it == 1 and not E.pcg_last_converged()
        assert relerr(x.cpu().numpy(), ref.x) <= 1e-12 and abs(nrm - ref.final_norm) <= 1e-10 * ref.final_norm
    # every dof essential on every level: the constrained operators are the identity, the smoothers multiples of
    # it and the constrained transfers zero -- x = b after one iteration
    every = [torch.arange(l.n, dtype=torch.int32, device="cuda") for l in d.c.levels]
    sm = [E.ChebyshevSmoother(Ak, ess=e, order=2) for Ak, e in zip(d.ops, every)]
    Be = E.Multigrid(d.ops, sm, d.tr, every)
    x = _nan(n)
    it, nrm = A.PCG(b, x, ess=every[-1], prec=Be)
    assert it == 1 and E.pcg_last_converged()
    assert relerr(x.cpu().numpy(), d.c.b) <= 1e-14
    # eigenvalue estimates far too small on every level: the smoothers, and so the cycle, are indefinite,
    # (B b, b) < 0 and the solve stops before the loop with final_norm = the negative (B b, b), not converged
    ds = _device("moved543", 1.0 / 8.0)
    for coarse in (None, COARSE8):
        ref = ds.c.solve("mg", coarse, rel_tol=1e-12)
        assert ref.stop == "neg0" and ref.final_norm < 0
        x = _nan(n)
        it, nrm = ds.A.PCG(ds.b, x, ess=ds.ess_f, rel_tol=1e-12, prec=ds.mg(coarse))
        print(f"coarse {coarse}: nom {nrm:.6f} (reference {ref.final_norm:.6f})")
        assert it == 0 and not E.pcg_last_converged()
        assert nrm < 0 and abs(nrm - ref.final_norm) <= 1e-12 * abs(ref.final_norm)


@pytest.mark.parametrize("coarse", [None, MC.EX26_COARSE])
def test_nonfinite_is_numeric_error_and_the_next_solve_works(coarse):
    d = _device("moved543")
    B = d.mg(coarse)
    ref = MC.reference("moved543", "mg", coarse, 1000)
    x = _nan(d.c.n)
    bad = d.b.clone()
    bad[d.c.n // 2] = float("nan")
    assert _code(lambda: d.A.PCG(bad, x, ess=d.ess_f, prec=B)) == ERR_NUMERIC
    assert not E.pcg_last_converged()
    it, _ = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, prec=B)
    assert E.pcg_last_converged() and abs(it - ref.final_iter) <= 1
    assert relerr(x.cpu().numpy(), ref.x) <= 1e-10


@pytest.mark.parametrize("coarse", [None, MC.EX26_COARSE])
def test_two_solves_are_bitwise_equal(coarse):
    import torch
    d = _device("moved433")
    B = d.mg(coarse)
    outs = []
    for _ in range(2):
        x = _nan(d.c.n)
        outs.append((d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, prec=B), x))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])


def test_refusals():
    import torch
    d = _device("moved433")
    n = d.c.n
    B = d.mg()
    # misaligned vectors, before anything is enqueued
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    assert _code(lambda: d.A.PCG(d.b, buf[1:], ess=d.ess_f, prec=B)) == ERR_ARG
    assert _code(lambda: B.Mult(d.b, buf[1:])) == ERR_ARG
    assert not buf.any()
    # sizes that do not chain: a level left out, transfers in the wrong order, a smoother of another level
    assert _code(lambda: E.Multigrid([d.ops[0], d.ops[2]], [d.sm[0], d.sm[2]], [d.tr[0]], [d.ess[0], d.ess[2]])) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr[::-1], d.ess)) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm[::-1], d.tr, d.ess)) == ERR_ARG
    # lists whose lengths do not match the levels: refused before the call into the library
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr[:1], d.ess)) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr + d.tr[:1], d.ess)) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm[:2], d.tr, d.ess)) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr, d.ess[:2])) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops[:2], d.sm, d.tr, d.ess)) == ERR_ARG
    # fewer than one level
    assert _code(lambda: E.Multigrid([], [], [], [])) == ERR_ARG
    # a cycle of another size as the preconditioner
    assert _code(lambda: d.A.PCG(d.b, _nan(n), ess=d.ess_f, prec=_device("moved543").mg())) == ERR_ARG
    # the next valid call works
    y = _nan(n)
    B.Mult(d.b, y)
    assert bool(torch.isfinite(y).all())


def test_loopback_group_and_distributed_operators_are_refused():
    """A loopback group's vectors are its members' concatenated true vectors, not the L-vectors that the transfers
    and the essential lists number, so the cycle would act in the wrong numbering: refused at a level and as the
    PCG's operator.  A group member's dots need communication: refused as well."""
    import torch
    m = E.Mesh.MakeCartesian3D(4, 4, 8)
    fes = E.H1Space(m, 2, E.NUMBERING_STRUCTURED)
    er = E.partition_slabs_z(m, 2)
    forms = []
    for r in range(2):
        f = E.ParBilinearForm(E.Partition(fes, er, r, 2, decomposition="overlap"))
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.Assemble()
        forms.append(f)
    group = E.ParGroup(forms)
    opg, member = E.Operator(group), E.Operator(group, member=0)
    serial = E.BilinearForm(fes)
    serial.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    serial.Assemble()
    ops = E.Operator(serial)
    assert opg.size == ops.size
    Sg = E.ChebyshevSmoother(opg, order=2, max_eig_estimate=1.5)
    Ss = E.ChebyshevSmoother(ops, order=2, max_eig_estimate=1.5)
    assert _code(lambda: E.Multigrid([opg], [Sg], [], [None])) == ERR_UNSUPPORTED
    B = E.Multigrid([ops], [Ss], [], [None])
    b = torch.ones(ops.size, dtype=torch.float64, device="cuda")
    x = _nan(ops.size)
    assert _code(lambda: opg.PCG(b, x, prec=B)) == ERR_UNSUPPORTED
    assert bool(torch.isnan(x).all())
    # a member, with a serial smoother of its size (a p = 1 lattice of as many dofs)
    dims = next((i, j, k) for i in range(1, 33) for j in range(1, 33) for k in range(1, 33)
                if (i + 1) * (j + 1) * (k + 1) == member.size)
    sf = E.BilinearForm(E.H1Space(E.Mesh.MakeCartesian3D(*dims), 1))
    sf.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
    sf.Assemble()
    opm = E.Operator(sf)
    Sm = E.ChebyshevSmoother(opm, order=2, max_eig_estimate=1.5)
    assert _code(lambda: E.Multigrid([member], [Sm], [], [None])) == ERR_UNSUPPORTED
    Bm = E.Multigrid([opm], [Sm], [], [None])
    xm = _nan(member.size)
    assert _code(lambda: member.PCG(torch.ones(member.size, dtype=torch.float64, device="cuda"), xm, prec=Bm)) == ERR_UNSUPPORTED
    assert bool(torch.isnan(xm).all())
    # the serial path still works: one level, the smoother as the whole cycle
    it, _ = ops.PCG(b, x, rel_tol=1e-10, prec=B)
    assert E.pcg_last_converged() and it > 0
