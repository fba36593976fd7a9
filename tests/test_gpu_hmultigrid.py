"""GPU tests of the multigrid cycle over h- and p-transfers (Multigrid with HRefinementTransfer and
PRefinementTransfer levels mixed) and of the PCG it preconditions, against the numpy restatement tests/hmg_ref.py on
the hierarchy cases of tests/hmg_cases.py: (h0, 1) -> (h1, 1) -> (h1, 2), the coarsest level its smoother applied once.

The fixed-work bound: the reference's spread of x after six iterations, and of one cycle's y, under its three
summation orders is <= 3.6e-16 of the max (tests/test_hmg_reference.py measures it and asserts that it stays 100 x
below hmg_ref.CYCLE_TOL), so the device is held to CYCLE_TOL = 1e-12 of max|x|.  Every output is preset to NaN; the
smoothers take the reference's eigenvalue estimates, so both sides do the same work."""
import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import hmg_cases as HC
import hmg_ref as HR
import mg_cases as MC
from helpers import relerr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 1, 5
_DEV = {}


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


class Dev:
    """One hierarchy on the device: per level the Operator, the essential list and the smoother; the transfers; b."""

    def __init__(self, name):
        import torch
        c = self.c = HC.hcase(name)
        self.ops = [E.Operator(l.device_form()) for l in c.levels]
        self.ess = [torch.as_tensor(l.ess).cuda() for l in c.levels]
        self.sm = [E.ChebyshevSmoother(A, ess=e, order=MC.SMOOTHER_ORDER, max_eig_estimate=l.max_eig)
                   for A, e, l in zip(self.ops, self.ess, c.levels)]
        self.tr = [E.HRefinementTransfer(c.levels[0].fes, c.levels[1].fes),
                   E.PRefinementTransfer(c.levels[1].fes, c.levels[2].fes)]
        self.A, self.ess_f = self.ops[-1], self.ess[-1]
        self.b = torch.as_tensor(c.b).cuda()

    def mg(self, p_only=False):
        k = 1 if p_only else 0
        return E.Multigrid(self.ops[k:], self.sm[k:], self.tr[k:], self.ess[k:])


def _device(name):
    if name not in _DEV:
        _DEV[name] = Dev(name)
    return _DEV[name]


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


@pytest.mark.parametrize("name", HC.H_CASES)
def test_three_level_cycle_matches_reference(name):
    import torch
    d = _device(name)
    B = d.mg()
    want = d.c.cycle()(d.c.b)
    y, y2 = _nan(d.c.n), _nan(d.c.n)
    B.Mult(d.b, y)
    B.Mult(d.b, y2)
    err = relerr(y.cpu().numpy(), want)
    print(f"{name}: relerr(y) {err:.2e}")
    assert err <= HR.CYCLE_TOL
    assert torch.equal(y, y2)
    assert torch.equal(d.b.cpu(), torch.as_tensor(d.c.b))


@pytest.mark.parametrize("name", HC.H_CASES)
def test_pcg_fixed_work_matches_reference(name):
    import torch
    d = _device(name)
    ref = HC.reference(name, 6)
    assert ref.final_iter == 6 and not ref.converged
    x, x2 = _nan(d.c.n), _nan(d.c.n)
    it, nrm = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=6, prec=d.mg())
    d.A.PCG(d.b, x2, ess=d.ess_f, rel_tol=1e-12, max_iter=6, prec=d.mg())
    err = relerr(x.cpu().numpy(), ref.x)
    print(f"{name}: iterations {it}, final_norm {nrm:.3e} (reference {ref.final_norm:.3e}), relerr(x) {err:.2e}")
    assert it == 6 and not E.pcg_last_converged()
    assert err <= HR.CYCLE_TOL
    assert torch.equal(x, x2)


@pytest.mark.parametrize("name", HC.H_CASES)
def test_pcg_iteration_counts(name):
    d = _device(name)
    ref = HC.reference(name, 1000)
    assert ref.final_iter == HC.COUNTS[name][2]
    x = _nan(d.c.n)
    it, _ = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=1000, prec=d.mg())
    assert E.pcg_last_converged()
    err = relerr(x.cpu().numpy(), ref.x)
    x = _nan(d.c.n)
    itp, _ = d.A.PCG(d.b, x, ess=d.ess_f, rel_tol=1e-12, max_iter=1000, prec=d.mg(p_only=True))
    print(f"{name}: h+p cycle {it} iterations (reference {HC.COUNTS[name][2]}), p cycle {itp} ({HC.COUNTS[name][1]}), relerr(x) {err:.2e}")
    assert it == HC.COUNTS[name][2] and itp == HC.COUNTS[name][1] and err <= 1e-10


def test_all_p_hierarchy_is_bitwise_the_hand_built_cycle():
    """A p-only cycle holds its transfer through the common base class: its result is, bit for bit, the two-level
    V-cycle put together here from the same device pieces one call at a time (MultigridBase::Cycle's steps, the
    vector passes as single IEEE operations in torch)."""
    import torch
    d = _device("hmoved433")
    (A0, A1), (S0, S1), (e0, e1), P = d.ops[1:], d.sm[1:], [e.long() for e in d.ess[1:]], d.tr[1]
    n0, n1 = A0.size, A1.size

    def cmult(A, ess, y):                    # ConstrainedOperator::ConstrainedMult, DIAG_ONE
        w = y.clone()
        w[ess] = 0.0
        out = _nan(y.numel())
        A.Mult(w, out)
        out[ess] = y[ess]
        return out

    def smooth(S, x):
        out = _nan(x.numel())
        S.Mult(x, out)
        return out
    x = d.b
    y = smooth(S1, x)                        # pre-smoothing from the zero guess
    r = x - cmult(A1, e1, y)
    r[e1] = 0.0
    xc = _nan(n0)
    P.MultTranspose(r, xc)
    xc[e0] = 0.0
    yc = smooth(S0, xc)                      # the coarsest level: its smoother once
    yc[e0] = 0.0
    z = _nan(n1)
    P.Mult(yc, z)
    z[e1] = 0.0
    y = y + z
    r = x - cmult(A1, e1, y)                 # post-smoothing
    y = y + smooth(S1, r)
    got = _nan(n1)
    d.mg(p_only=True).Mult(x, got)
    assert torch.equal(got, y)


def test_refusals_and_the_next_valid_call_works():
    import torch
    d = _device("hmoved433")
    n = d.c.n
    # sizes that do not chain: the h-transfer between the two levels of the fine mesh, the transfers swapped
    assert _code(lambda: E.Multigrid(d.ops[1:], d.sm[1:], d.tr[:1], d.ess[1:])) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr[::-1], d.ess)) == ERR_ARG
    assert _code(lambda: E.Multigrid(d.ops, d.sm, d.tr[:1], d.ess)) == ERR_ARG
    # something that is no transfer
    with pytest.raises(E.ECM2Error):
        E.Multigrid(d.ops, d.sm, [d.tr[0], d.sm[0]], d.ess)
    y = _nan(n)
    d.mg().Mult(d.b, y)
    assert bool(torch.isfinite(y).all())


def test_loopback_group_is_refused_below_an_h_transfer():
    """A loopback group's concatenated true vectors are not the L-vectors an h-transfer numbers: refused as a level."""
    import torch
    m = E.Mesh.MakeCartesian3D(4, 4, 8)
    f = HC.refined(m)
    lf, hf = E.H1Space(m, 2, E.NUMBERING_STRUCTURED), E.H1Space(f, 2)
    T = E.HRefinementTransfer(lf, hf)
    er = E.partition_slabs_z(m, 2)
    forms = []
    for r in range(2):
        a = E.ParBilinearForm(E.Partition(lf, er, r, 2, decomposition="overlap"))
        a.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        a.Assemble()
        forms.append(a)
    opg = E.Operator(E.ParGroup(forms))
    ops = []
    for fes in (lf, hf):
        a = E.BilinearForm(fes)
        a.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        a.Assemble()
        ops.append(E.Operator(a))
    assert opg.size == ops[0].size
    Sg = E.ChebyshevSmoother(opg, order=2, max_eig_estimate=1.5)
    sm = [E.ChebyshevSmoother(o, order=2, max_eig_estimate=1.5) for o in ops]
    assert _code(lambda: E.Multigrid([opg, ops[1]], [Sg, sm[1]], [T], [None, None])) == ERR_UNSUPPORTED
    B = E.Multigrid(ops, sm, [T], [None, None])
    b = torch.ones(ops[1].size, dtype=torch.float64, device="cuda")
    x = _nan(ops[1].size)
    it, _ = ops[1].PCG(b, x, rel_tol=1e-10, prec=B)
    assert E.pcg_last_converged() and it > 0
