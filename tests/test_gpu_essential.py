"""GPU tests of inhomogeneous essential data on the device: the elimination (Operator.EliminateRHS /
Operator.FormLinearSystem: ConstrainedOperator::EliminateRHS and Operator::FormLinearSystem, linalg/operator.cpp:
559-584, 114-129, in csrc/k_ess.hip) and the warm-started solves (iterative_mode = true: CGSolver::Mult and
BiCGSTABSolver::Mult from r = b - A~ x, linalg/solvers.cpp:875-884, 1618-1627) against the numpy restatement
tests/ess_ref.py on the cases of tests/cheb_cases.py, tests/mg_cases.py and tests/bicgstab_cases.py.

Data (ess_ref.Problem): x_D = 37 + 20 exp(-10 |p - 1/2|^2) on the boundary dofs, b eliminated; the starts "lift" (x_D
on the list, 0 elsewhere) and "far" (free entries 37 + 20 U[0, 1)).  The fixed-work bound is the project's 1e-12 of
max|x| under the self-gap condition tests/test_ess_reference.py pins (<= 1e-14 under three summation orders; the
BiCGSTAB case p3 marked misses it from the lift, 4.8e-14, and is left out of that comparison alone)."""
import ctypes

import numpy as np
import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import ess_ref as ER
import bicgstab_cases as BC
import mg_cases as MC
from helpers import relerr
from test_ess_reference import ADMITTED_BICGSTAB, CG_CASES, FIXED_POINT_BICGSTAB, FIXED_POINT_CG

pytestmark = pytest.mark.gpu

FIXED = 1e-12
ERR_ARG = 1
_DEV = {}


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _nan(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _code(fn):
    try:
        fn()
    except E.ECM2Error as e:
        return e.code
    return 0


class Dev:
    """One problem on the device: the operator, the essential list (None without one), the eliminated b and what the
    solver takes beside them (PCG: prec; BiCGSTAB: jacobi_of)."""

    def __init__(self, kind, key, solver):
        self.P = P = ER.problem(kind, key)
        self.solver = solver
        self.kw = {}
        if kind == "cg":
            self.A = E.Operator(P.c.device_form())
        elif kind == "bicgstab":
            T, S = P.c.device_forms()
            self.A, self.S = E.Operator(T), E.Operator(S)
            self.kw = {"jacobi_of": self.S}
        else:
            mc = P.c.mc
            self.ops = [E.Operator(l.device_form()) for l in mc.levels]
            self.lev_ess = [_t(l.ess) for l in mc.levels]
            self.sm = [E.ChebyshevSmoother(A, ess=e, order=MC.SMOOTHER_ORDER, max_eig_estimate=l.max_eig)
                       for A, e, l in zip(self.ops, self.lev_ess, mc.levels)]
            self.tr = [E.PRefinementTransfer(a.fes, b.fes) for a, b in zip(mc.levels[:-1], mc.levels[1:])]
            self.A = self.ops[-1]
            self.kw = {"prec": E.Multigrid(self.ops, self.sm, self.tr, self.lev_ess)}
        self.ess = _t(P.ess.astype(np.int32)) if P.ess.size else None
        if solver == "cheb":
            self.kw = {"prec": E.ChebyshevSmoother(self.A, ess=self.ess, order=2, max_eig_estimate=P.c.max_eig)}
        self.b = _t(P.b)
        self.n = P.c.n

    def ref_kind(self):
        """What ess_ref.Problem.solve takes for this solver, and the reference's cache tag."""
        if self.solver == "cheb":
            return self.P.c.smoother(2), "cheb2"
        if self.solver == "mg":
            return self.P.c.mc.cycle(), "mg"
        return self.solver, None

    def reference(self, start, max_iter, **kw):
        kind, tag = self.ref_kind()
        return self.P.reference(kind, start, max_iter, tag=tag, **kw)

    def solve(self, x, **kw):
        """(iterations, final_norm, converged) of the device solve of the eliminated system."""
        if self.solver == "bicgstab":
            it, nrm = self.A.BiCGSTAB(self.b, x, ess=self.ess, **self.kw, **kw)
            return it, nrm, E.bicgstab_last_converged()
        it, nrm = self.A.PCG(self.b, x, ess=self.ess, **self.kw, **kw)
        return it, nrm, E.pcg_last_converged()


def _dev(kind, key, solver):
    if (kind, key, solver) not in _DEV:
        _DEV[kind, key, solver] = Dev(kind, key, solver)
    return _DEV[kind, key, solver]


JACOBI = [("cg", k, "jacobi") for k in CG_CASES]
FIXED_FORMS = JACOBI + [("cg", "k2", "cheb"), ("mg", MC.CASES[0], "mg")] + [("bicgstab", k, "bicgstab") for k in ADMITTED_BICGSTAB]
CONVERGED_FORMS = JACOBI + [("bicgstab", k, "bicgstab") for k in BC.CASES]
FIXED_POINT_FORMS = [("cg", k, "jacobi") for k in FIXED_POINT_CG] + [("bicgstab", k, "bicgstab") for k in FIXED_POINT_BICGSTAB]
_ids = lambda v: "-".join(str(t) for t in v) if isinstance(v, tuple) else str(v)


# ---- elimination ----
@pytest.mark.parametrize("name", CG_CASES)
def test_eliminate_rhs_is_the_composition_of_public_calls(name):
    """k1: fewer entries than one workgroup; k2: an odd n (the tail lane); k3: the line kernel; mk2: a heat stage."""
    import torch
    d = _dev("cg", name, "jacobi")
    c, P = d.P.c, d.P
    x = _t(P.starts["far"])
    b = _t(c.b)
    b0 = b.clone()
    d.A.EliminateRHS(x, b, d.ess)
    # the same operations through public calls: w built in torch, Operator.Mult, b - z, the overwrite
    w = torch.zeros_like(x)
    w[d.ess.long()] = x[d.ess.long()]
    z = _nan(d.n)
    d.A.Mult(w, z)
    want = b0 - z
    want[d.ess.long()] = x[d.ess.long()]
    torch.cuda.synchronize()
    assert torch.equal(b, want)
    assert torch.equal(x, _t(P.starts["far"]))
    err = relerr(b.cpu().numpy(), ER.eliminate_rhs(c.mult, P.ess, P.starts["far"], c.b))
    print(f"{name}: EliminateRHS against the reference {err:.2e}")
    assert err <= FIXED
    # (the problem's own b is this elimination: the lift and the far start share their essential entries)
    assert relerr(b.cpu().numpy(), P.b) <= FIXED


def test_no_essential_dofs_leaves_b_bitwise_unchanged():
    import torch
    d = _dev("cg", "mk2_free", "jacobi")
    assert d.ess is None
    x, b = _t(d.P.starts["far"]), _t(d.P.c.b)
    b0, x0 = b.clone(), x.clone()
    d.A.EliminateRHS(x, b, None)
    assert torch.equal(b, b0) and torch.equal(x, x0)
    d.A.FormLinearSystem(None, x, b, copy_interior=True)
    assert torch.equal(b, b0) and torch.equal(x, x0)
    # (copy_interior = False: every entry is off the list)
    d.A.FormLinearSystem(None, x, b)
    assert torch.equal(b, b0) and not x.any()


@pytest.mark.parametrize("copy_interior", [False, True])
def test_form_linear_system(copy_interior):
    import torch
    d = _dev("cg", "k2", "jacobi")
    c, P = d.P.c, d.P
    x, b = _t(P.starts["far"]), _t(c.b)
    be = b.clone()
    d.A.EliminateRHS(x, be, d.ess)
    d.A.FormLinearSystem(d.ess, x, b, copy_interior=copy_interior)
    Xr, Br = ER.form_linear_system(c.mult, P.ess, P.starts["far"], c.b, copy_interior)
    assert torch.equal(b, be)
    assert np.array_equal(x.cpu().numpy(), Xr)     # (copies and zeros: bitwise)
    assert np.array_equal(Xr, P.starts["far" if copy_interior else "lift"])
    assert relerr(b.cpu().numpy(), Br) <= FIXED


def test_loopback_group_elimination_and_warm_start_match_the_serial_form():
    """The 2-slab loopback group (4 x 4 x 8, p = 2) in its concatenated numbering against the serial form."""
    import torch
    import test_gpu_bicgstab as TB
    m, fes, serial, group, parts = TB._sym_setup()
    n = fes.ndofs
    ess = np.asarray(fes.boundary_dofs())
    rng = np.random.default_rng(8)
    x, b = 37.0 + 20.0 * rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    own = np.concatenate([p.owned_global for p in parts])
    idx, o = [], 0
    for p in parts:
        idx.append(np.nonzero(np.isin(p.owned_global, ess))[0] + o)
        o += p.n_owned
    A, G = E.Operator(serial), E.Operator(group)
    assert G.size == n
    xs, bs, es = _t(x), _t(b), _t(ess.astype(np.int32))
    xg, bg, eg = _t(x[own]), _t(b[own]), _t(np.concatenate(idx).astype(np.int32))
    A.FormLinearSystem(es, xs, bs)
    G.FormLinearSystem(eg, xg, bg)
    err = relerr(bg.cpu().numpy(), bs.cpu().numpy()[own])
    print(f"group EliminateRHS against the serial form {err:.2e}")
    assert err <= FIXED and torch.equal(xg, xs[_t(own).long()])
    A.PCG(bs, xs, ess=es, rel_tol=1e-12, iterative_mode=True)
    assert E.pcg_last_converged()
    it, _ = G.PCG(bg, xg, ess=eg, rel_tol=1e-12, iterative_mode=True)
    assert E.pcg_last_converged() and it > 0
    assert relerr(xg.cpu().numpy(), xs.cpu().numpy()[own]) <= 1e-10
    assert torch.equal(xg[eg.long()], _t(x[own])[eg.long()])


def test_distributed_operators_eliminate_and_warm_start():
    """One RCCL rank (the Mult and the dots collective) and a member of a loopback group: the elimination against
    the composition of public calls, the warm-started PCG against the cold one."""
    import torch
    m = E.Mesh.MakeCartesian3D(4, 4, 8)
    fes = E.H1Space(m, 2, E.NUMBERING_STRUCTURED)

    def assembled(part, **kw):
        f = E.ParBilinearForm(part, **kw)
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.ConstantCoefficient(0.05)))
        f.Assemble()
        return f
    rank = E.Operator(assembled(E.Partition(fes, np.zeros(fes.ne, np.int32), 0, 1), rccl_id=E.rccl_unique_id()))
    er = E.partition_slabs_z(m, 2)
    member = E.Operator(E.ParGroup([assembled(E.Partition(fes, er, r, 2, decomposition="overlap")) for r in range(2)]),
                        member=0)
    for op in (rank, member):
        n = op.size
        rng = np.random.default_rng(9)
        ess = _t(np.arange(0, n, 7, dtype=np.int32))
        x0, b0 = _t(37.0 + 20.0 * rng.uniform(0, 1, n)), _t(rng.uniform(0, 1, n))
        x, b = x0.clone(), b0.clone()
        op.FormLinearSystem(ess, x, b)
        w = torch.zeros_like(x0)
        w[ess.long()] = x0[ess.long()]
        z = _nan(n)
        op.Mult(w, z)
        want = b0 - z
        want[ess.long()] = x0[ess.long()]
        torch.cuda.synchronize()
        assert torch.equal(b, want) and torch.equal(x, w)
        cold = _nan(n)
        op.PCG(b, cold, ess=ess, rel_tol=1e-12)
        assert E.pcg_last_converged()
        it, _ = op.PCG(b, x, ess=ess, rel_tol=1e-12, iterative_mode=True)
        assert E.pcg_last_converged() and it > 0
        assert relerr(x.cpu().numpy(), cold.cpu().numpy()) <= 1e-10
        assert torch.equal(x[ess.long()], x0[ess.long()])


def test_refusals_leave_the_vectors_untouched():
    import torch
    d = _dev("cg", "k2", "jacobi")
    n = d.n
    x = _t(d.P.starts["far"])
    x0 = x.clone()
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    # a misaligned b (a view at an odd element offset), a misaligned x, x is b: before anything is enqueued
    for call in (lambda: d.A.EliminateRHS(x, buf[1:], d.ess), lambda: d.A.FormLinearSystem(d.ess, x, buf[1:]),
                 lambda: d.A.EliminateRHS(x, x, d.ess), lambda: d.A.FormLinearSystem(d.ess, x, x)):
        assert _code(call) == ERR_ARG
        assert not buf.any() and torch.equal(x, x0)
    b = _t(d.P.c.b)
    b0 = b.clone()
    xb = torch.ones(n + 1, dtype=torch.float64, device="cuda")
    assert _code(lambda: d.A.FormLinearSystem(d.ess, xb[1:], b)) == ERR_ARG
    assert torch.equal(b, b0) and bool((xb == 1.0).all())
    # iterative_mode reads b two entries at a time: a misaligned b is refused, x keeps its start
    buf[1:] = d.b
    bb = buf.clone()
    assert _code(lambda: d.A.PCG(buf[1:], x, ess=d.ess, iterative_mode=True)) == ERR_ARG
    assert _code(lambda: d.A.BiCGSTAB(buf[1:], x, ess=d.ess, iterative_mode=True)) == ERR_ARG
    assert torch.equal(x, x0) and torch.equal(buf, bb)
    # (the cold solve copies b: it takes the same view)
    it, _ = d.A.PCG(buf[1:], _nan(n), ess=d.ess)
    assert E.pcg_last_converged() and it > 0


# ---- warm start ----
@pytest.mark.parametrize("start", ER.STARTS)
@pytest.mark.parametrize("form", FIXED_FORMS, ids=_ids)
def test_warm_start_fixed_work_matches_reference(form, start):
    """Six iterations (max_iter = 6: not converged) from the start, the same work as the reference's: x to 1e-12,
    the essential entries bitwise x_D."""
    d = _dev(*form)
    P = d.P
    ref = d.reference(start, 6)
    assert ref.final_iter == 6 and not ref.converged
    x = _t(P.starts[start])
    it, nrm, conv = d.solve(x, rel_tol=1e-12, max_iter=6, iterative_mode=True)
    xh = x.cpu().numpy()
    err = relerr(xh, ref.x)
    print(f"{form} {start}: iterations {it}, final_norm {nrm:.3e} (reference {ref.final_norm:.3e}), relerr(x) {err:.2e}")
    assert it == 6 and not conv
    assert err <= FIXED
    assert np.array_equal(xh[P.ess], P.xd[P.ess])


@pytest.mark.parametrize("start", ER.STARTS)
@pytest.mark.parametrize("form", CONVERGED_FORMS, ids=_ids)
def test_warm_start_converged_matches_reference(form, start):
    d = _dev(*form)
    P = d.P
    ref = d.reference(start, 1000)
    assert ref.converged
    x = _t(P.starts[start])
    it, nrm, conv = d.solve(x, rel_tol=1e-12, max_iter=1000, iterative_mode=True)
    xh = x.cpu().numpy()
    res_dev, res_ref = P.true_residual(xh), P.true_residual(ref.x)
    err = relerr(xh, ref.x)
    cold = _nan(d.n)
    _, _, cold_conv = d.solve(cold, rel_tol=1e-12, max_iter=1000)
    gap = relerr(xh, cold.cpu().numpy())
    print(f"{form} {start}: iterations {it} (reference {ref.final_iter}), true residual {res_dev:.2e} (reference "
          f"{res_ref:.2e}), relerr(x) {err:.2e}, against the cold solve {gap:.2e}")
    assert conv and cold_conv
    assert abs(it - ref.final_iter) <= 1
    assert res_dev <= 4.0 * res_ref
    assert err <= 1e-10
    assert gap <= 1e-10
    assert np.array_equal(xh[P.ess], P.xd[P.ess])


def _goal(d):
    """The cold solve's goal as an absolute tolerance, read from the reference: rel_tol sqrt(nom_0) (PCG),
    rel_tol ||r_0|| (BiCGSTAB)."""
    cold = d.reference(None, 1000)
    return cold, 1e-12 * cold.initial_norm


@pytest.mark.parametrize("form", FIXED_POINT_FORMS, ids=_ids)
def test_fixed_point_returns_at_once(form):
    """From the converged solution with the cold solve's goal as abs_tol: 0 iterations, converged, x untouched.
    (The cases end their cold solve at <= 0.6 of the goal: tests/test_ess_reference.py.)"""
    import torch
    d = _dev(*form)
    cold, goal = _goal(d)
    x = _nan(d.n)
    it, nrm, conv = d.solve(x, rel_tol=1e-12, max_iter=1000)
    assert conv and abs(it - cold.final_iter) <= 1
    x0 = x.clone()
    it, nrm, conv = d.solve(x, rel_tol=0.0, abs_tol=goal, max_iter=1000, iterative_mode=True)
    print(f"{form}: fixed point: {it} iterations, norm {nrm:.3e} against the goal {goal:.3e}")
    assert it == 0 and conv and nrm <= goal
    assert torch.equal(x, x0)


@pytest.mark.parametrize("form", FIXED_POINT_FORMS, ids=_ids)
def test_near_start_saves_iterations_under_an_absolute_tolerance(form):
    """From the converged solution times 1 + 1e-3 sin(i) with the cold solve's goal as abs_tol: the reference's
    warm count +- 1, which tests/test_ess_reference.py asserts is below the cold count."""
    d = _dev(*form)
    P = d.P
    cold, goal = _goal(d)
    start = P.near(cold.x)
    ref = d.reference(("near", start), 1000, rel_tol=0.0, abs_tol=goal)
    assert ref.converged and ref.final_iter < cold.final_iter
    x = _t(start)
    it, nrm, conv = d.solve(x, rel_tol=0.0, abs_tol=goal, max_iter=1000, iterative_mode=True)
    print(f"{form}: near start {it} iterations (reference {ref.final_iter}, cold {cold.final_iter})")
    assert conv and abs(it - ref.final_iter) <= 1
    assert relerr(x.cpu().numpy(), cold.x) <= 1e-10


# ---- flag 0 is the old solver ----
def _raw(fn, A, mid, ess, b, x, tail, flag=None):
    """An entry point called as the C ABI declares it: (iterations, final_norm)."""
    it, nrm = ctypes.c_int(), ctypes.c_double()
    args = [A._h] + mid + [E._dev_ptr(ess), int(ess.numel()), E._dev_ptr(b), E._dev_ptr(x), 1e-12, 0.0, 1000] + tail
    args += [ctypes.byref(it), ctypes.byref(nrm), E._stream()] + ([] if flag is None else [flag])
    E._check(fn(*args))
    return it.value, nrm.value


def test_ex_entry_points_with_flag_zero_are_the_old_solvers():
    """Bitwise the x, the iteration count and the norm of the old entry points, from an x filled with NaN (it is
    overwritten, not read)."""
    import torch
    lib = E._par_lib()
    k2, mg, p2 = _dev("cg", "k2", "jacobi"), _dev("mg", MC.CASES[0], "mg"), _dev("bicgstab", ("p2", False), "bicgstab")
    cheb = _dev("cg", "k2", "cheb")
    runs = [
        (lib.ecm2_operator_pcg, lib.ecm2_operator_pcg_ex, k2, [], [1]),
        (lib.ecm2_operator_pcg_prec, lib.ecm2_operator_pcg_prec_ex, cheb, [cheb.kw["prec"]._h], []),
        (lib.ecm2_operator_pcg_mg, lib.ecm2_operator_pcg_mg_ex, mg, [mg.kw["prec"]._h], []),
        (lib.ecm2_operator_bicgstab, lib.ecm2_operator_bicgstab_ex, p2, [p2.S._h], []),
    ]
    for old, new, d, mid, tail in runs:
        xo, xn = _nan(d.n), _nan(d.n)
        ro = _raw(old, d.A, mid, d.ess, d.b, xo, tail)
        rn = _raw(new, d.A, mid, d.ess, d.b, xn, tail, 0)
        assert ro == rn and ro[0] > 0, (ro, rn)
        assert torch.equal(xo, xn) and bool(torch.isfinite(xn).all())
        # ... and the flag set, from a zero start, is the cold solve too: A~ 0 = 0, so r = b - 0 has b's bits
        xz = torch.zeros(d.n, dtype=torch.float64, device="cuda")
        rz = _raw(new, d.A, mid, d.ess, d.b, xz, tail, 1)
        assert rz == ro and torch.equal(xz, xo)
