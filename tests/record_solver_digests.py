"""The cases of tests/test_gpu_solver_bitwise.py and the recorder of their digests.

    python3 tests/record_solver_digests.py [out.json]
    python3 tests/record_solver_digests.py --prec [out.json]
    python3 tests/record_solver_digests.py --sweep [out.json]

runs every case on cuda:0 through the public Python API, twice, and writes the SHA-256 of the float64
bytes of each result with the exact iteration count, final norm and converged flag (default:
tests/golden/solver_digests.json).  A case whose two runs differ is refused: nothing non-deterministic
enters the set (no case uses scatter = atomic).  The committed file was recorded from the build of the
commit before the device PCG and the device BiCGSTAB got one loop driver and one workspace
(csrc/solvers.cpp, LoopCtl): that commit's solvers are the reference the shared pieces must reproduce bit
for bit.

Inputs use no libm function: the vertices are moved by polynomials, the coefficients are polynomials of
the coordinates, b, u and the source are seeded uniform draws.  The shapes are the smallest at which each
shared piece can still go wrong:
  serial   5 x 4 x 3, p = 2 (693 dofs, odd: the tail lane of the 16-byte passes), mass + diffusion per
           point: the thread-per-element kernel, EnergyParts() == 0 -- PCG's (A d, d) is a dot pass (the
           energy-folded path is pinned by ts_epilogue_digests.json); with Jacobi, without, and with no
           essential dofs (the constrained Mult's shortcut)
  group    4 x 4 x 8, p = 2, two z slabs as one operator on the concatenated true vectors (not distributed)
  member   member 0 of the same slabs (structured numbering, overlap): distributed -- the dots through
           sum_scalars and the stand-alone stopping-test kernel
  bcg      the serial form + convection (y, -x, x): with Jacobi from the symmetric part, without a
           preconditioner (s serves as shat), and 4 x 3 x 3, p = 3 (the line kernel) with the convection
           marked on two of three attributes, without a preconditioner.  (The p = 3 setup with Jacobi is
           left out: it is not deterministic.  The diagonal of a form on the line kernel is summed by
           atomic adds onto the L-vector (csrc/k_line.hip, the sum-factorised diagonal), so dinv and with
           it x differ in the last bits from one process to the next -- three fresh processes of the
           reference build gave three different digests, while two runs in one process agreed.)
  ode      one step of SDIRK33 (23) and SDIRK34 (34) on the serial mesh, PCG stages on the symmetric forms
           and BiCGSTAB stages on the convective ones; 23 / BiCGSTAB with a source
Each solver setup runs fixed work (rel_tol = 0), max_iter = 1 (the loop ends before any wait) and a
converging solve.  SEQUENCE: solves of different sizes and methods in one process, each equal to the
digest of the same solve alone (the workspace they share grows, shrinks in use, and changes method).

--prec: the second group and the second file, tests/golden/solver_prec_digests.json -- the PCG with a Chebyshev
smoother and the PCG with a multigrid cycle as its preconditioner, under the same rules.  The committed file
was recorded from the build of commit 9b6518a, the last one in which these two and the Jacobi PCG were three
copies of CGSolver::Mult's loop (csrc/solvers.cpp pcg_solve, pcg_solve_prec, pcg_solve_mg): that commit's
solvers are the reference the one loop must reproduce bit for bit.  The recorder ran in two fresh processes
there, and the two files were byte-identical; no case had to be dropped.  Every case stays at p <= 2, whose
diagonal (the smoothers' and the coarse PCG's dinv) is summed without atomics.
  cheb-o1, -o2, -o3   the serial p = 2 form above, ChebyshevSmoother of order 1 (the entry pass sums betanom
           itself, no term loop), 2 (one term, the last) and 3 (a middle term that stores t), the largest
           eigenvalue by the power method from the library's own start vector: max_eig and the steps are
           part of the digest, which pins power_method on the shared workspace
  cheb-o2-noess       no essential dofs: the essential kernels are not launched
  cheb-o2-energy      the snapshot form of record_ts_epilogue_digests.build_form on 4 x 4 x 4 (729 dofs),
           EnergyParts() == 1: (A d, d) folded into the Mult inside the preconditioned loop; fixed and conv
  mg-smoother, mg-coarse   levels p = 1 -> 2 on the serial mesh (120 -> 693 dofs), mass + diffusion on both,
           order-2 smoothers, pre = post = 1; the coarsest level's smoother, or a coarse PCG (1e-2, 200): the
           nested workspace and the synchronise-and-look before each cycle
  ode-23-cheb         one SDIRK33 step, the stage solves preconditioned by an order-2 smoother
PREC_SEQUENCE: a nested solve, a depth-0 Jacobi solve, a preconditioned one and a BiCGSTAB on one workspace.

--sweep: the third group and the third file, tests/golden/solver_sweep_digests.json -- what the shapes above cannot
reach in the solvers' 16-byte vector passes.  At 693 to 1,377 dofs no thread of a grid-stride pass (1,024 workgroups
of 256, two entries per trip) makes a second trip round its loop, and all but one workgroup of a flat pass is partly
empty; a second trip needs more than 2 x 256 x 1,024 = 524,288 entries.  One shape: 41 x 41 x 40 elements, p = 2,
83 x 83 x 81 = 558,009 dofs (odd: the tail lane too), the moved vertices and polynomial coefficients of the serial
form (per-point qdata, the thread-per-element kernel, the partial scatter: no atomics).  Fixed work only (rel_tol =
0, three iterations): the Jacobi PCG; the PCG with an order-3 smoother (max_eig and the power steps in the digest);
the PCG with the p = 1 -> 2 cycle whose coarsest level is its smoother; BiCGSTAB with Jacobi from the symmetric part
on the form plus convection.  The committed file was recorded from the build of commit 18e996c, the last one in
which every pass had a 16-byte body and a scalar copy of it for the tail entry: the recorder ran in two fresh
processes there, and the two files were byte-identical; no case had to be dropped."""
import hashlib
import json
import os
import sys

import numpy as np

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_digests.json")
DIGESTS_PREC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_prec_digests.json")
DIGESTS_SWEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_sweep_digests.json")
CDT = 0.4359 * 0.05
CONV_SCALE = 20.0
MARKER = [0, 1, 1]
MESHES = {"p1": (5, 4, 3, 1), "p2": (5, 4, 3, 2), "p3": (4, 3, 3, 3), "s1": (41, 41, 40, 1), "s2": (41, 41, 40, 2)}
# solver runs per setup: name -> (rel_tol, max_iter) for PCG and for BiCGSTAB
PCG_RUNS = {"fixed": (0.0, 6), "one": (0.0, 1), "conv": (1e-10, 1000)}
BCG_RUNS = {"fixed": (0.0, 5), "one": (0.0, 1), "conv": (1e-12, 1000)}
PCG_SERIAL = ["jacobi", "plain", "noess"]
PCG_PAR = ["group", "member"]
BCG_SETUPS = ["p2-jacobi", "p2-plain", "p3-plain"]
ODE_CASES = [(23, "pcg", False), (34, "pcg", False), (23, "bicgstab", True), (34, "bicgstab", False)]
SEQUENCE = ["bcg-p3-plain-conv", "pcg-jacobi-conv", "pcg-group-conv", "bcg-p2-jacobi-conv", "bcg-p3-plain-conv"]
# the second group: the PCG with a Chebyshev smoother or a multigrid cycle as its preconditioner
MG_RUNS = {"fixed": (0.0, 4), "one": (0.0, 1), "conv": (1e-10, 1000)}
CHEB_SETUPS = {"o1": PCG_RUNS, "o2": PCG_RUNS, "o3": PCG_RUNS, "o2-noess": PCG_RUNS,
               "o2-energy": {r: PCG_RUNS[r] for r in ("fixed", "conv")}}
MG_SETUPS = ["smoother", "coarse"]
MG_COARSE_PCG = (1e-2, 200)
PREC_SEQUENCE = ["mg-coarse-conv", "pcg-jacobi-conv", "cheb-o3-conv", "bcg-p2-jacobi-conv", "mg-coarse-conv"]
# the third group: one shape above the grid-stride passes' first trip, fixed work
SWEEP_NDOFS = 83 * 83 * 81
SWEEP_ITERS = 3
SWEEP_SETUPS = ["pcg-jacobi", "cheb-o3", "mg-smoother", "bcg-jacobi"]
_CACHE = {}


def all_cases():
    ids = ["pcg-%s-%s" % (s, r) for s in PCG_SERIAL + PCG_PAR for r in PCG_RUNS]
    ids += ["bcg-%s-%s" % (s, r) for s in BCG_SETUPS for r in BCG_RUNS]
    ids += ["ode-%d-%s" % (t, s) for t, s, _ in ODE_CASES]
    return ids


def prec_cases():
    ids = ["cheb-%s-%s" % (s, r) for s, runs in CHEB_SETUPS.items() for r in runs]
    ids += ["mg-%s-%s" % (s, r) for s in MG_SETUPS for r in MG_RUNS]
    return ids + ["ode-23-cheb"]


def sweep_cases():
    return ["sweep-" + s for s in SWEEP_SETUPS]


def sha(t):
    a = np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64)
    return hashlib.sha256(a.tobytes()).hexdigest()


def move(V):
    V = np.array(V, dtype=np.float64, copy=True)
    x, y, z = V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()
    V[:, 0] = x + 0.05 * y * (1.0 - y) * z
    V[:, 1] = y + 0.04 * x * (2.0 - x)
    V[:, 2] = z + 0.03 * x * y
    return V


def alpha_poly(P):
    return 2.0 + 0.5 * P[..., 0] * (1.0 - P[..., 1])


def beta_poly(P):
    return 1.0 + 0.5 * P[..., 2]


def velocity_poly(P):
    return np.stack([P[..., 1], -P[..., 0], P[..., 0]], -1)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def serial_setup(E, torch, name):
    """(mesh, fes, quadrature points, essential dofs on the device) of a serial mesh."""
    def make():
        nx, ny, nz, p = MESHES[name]
        m = E.Mesh.MakeCartesian3D(nx, ny, nz)
        m.set_vertices(move(m.vertices()))
        m.SetAttributes(1 + (np.arange(m.GetNE()) % 3).astype(np.int32))
        fes = E.H1Space(m, p)
        ess = torch.as_tensor(np.asarray(fes.boundary_dofs(), dtype=np.int32)).cuda()
        return m, fes, m.quadrature_points(p + 2), ess
    return _cached(("serial", name), make)


def serial_form(E, torch, name, mass, diff_scale, conv_alpha, marked=False):
    """mass * Mass(alpha) + Diffusion(diff_scale beta) [+ Convection(v, conv_alpha)], assembled, with the kernel
    and the dot path asserted."""
    def make():
        m, fes, P, _ = serial_setup(E, torch, name)
        ne = fes.ne
        f = E.BilinearForm(fes)
        if mass:
            f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(_dev(torch, alpha_poly(P).reshape(ne, -1)))))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(_dev(torch, diff_scale * beta_poly(P).reshape(ne, -1)))))
        if conv_alpha is not None:
            ci = E.ConvectionIntegrator(E.VectorCoefficient(_dev(torch, velocity_poly(P))), conv_alpha)
            if marked:
                f.AddDomainIntegrator(ci, MARKER)
            else:
                f.AddDomainIntegrator(ci)
        f.Assemble()
        info = f.info()
        assert info["kernel"] == (E.KERNEL_TPE if MESHES[name][3] <= 2 else E.KERNEL_LINE), info
        assert f.EnergyParts() == 0 and not f.CoefficientSnapshot()   # (A d, d) by the dot pass
        kept = int(np.count_nonzero(np.asarray(MARKER)[m.GetAttributes() - 1])) if marked else ne
        assert f.ConvectionInfo() == ((True, kept, True) if conv_alpha is not None else (False, 0, False)), f.ConvectionInfo()
        if marked:
            assert 0 < kept < ne
        return f
    return _cached(("form", name, mass, diff_scale, conv_alpha, marked), make)


def par_setup(E, torch, kind):
    """(operator, b, ess) of the 2-slab group (kind "group") or of its member 0 ("member")."""
    def make():
        m = E.Mesh.MakeCartesian3D(4, 4, 8)
        m.set_vertices(move(m.vertices()))
        member = kind == "member"
        fes = E.H1Space(m, 2, E.NUMBERING_STRUCTURED if member else E.NUMBERING_ENTITY)
        er = E.partition_slabs_z(m, 2)
        forms, parts = [], []
        for r in range(2):
            part = E.Partition(fes, er, r, 2, decomposition="overlap")
            P = E.quadrature_points_subset(m, 4, part.elems)
            f = E.ParBilinearForm(part)
            f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(_dev(torch, alpha_poly(P).reshape(part.ne_local, -1)))))
            f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(_dev(torch, CDT * beta_poly(P).reshape(part.ne_local, -1)))))
            f.Assemble()
            forms.append(f)
            parts.append(part)
        group = E.ParGroup(forms)
        bdr = np.asarray(fes.boundary_dofs())
        bg = np.random.default_rng(23).uniform(0.0, 1.0, fes.ndofs)
        if member:
            op = E.Operator(group, member=0)
            own = parts[0].owned_global
            assert op.size == len(own) < fes.ndofs
            b, ess = bg[own], np.nonzero(np.isin(own, bdr))[0]
        else:
            op = E.Operator(group)
            assert op.size == fes.ndofs == 9 * 9 * 17
            b = np.concatenate([bg[p.owned_global] for p in parts])
            idx, o = [], 0
            for p in parts:
                idx.append(np.nonzero(np.isin(p.owned_global, bdr))[0] + o)
                o += p.n_owned
            ess = np.concatenate(idx)
        assert 0 < len(ess) < op.size
        return op, _dev(torch, b), _dev(torch, ess.astype(np.int32))
    return _cached(("par", kind), make)


def run_pcg(E, torch, setup, run):
    rel_tol, max_iter = PCG_RUNS[run]
    if setup in PCG_SERIAL:
        _, fes, _, ess = serial_setup(E, torch, "p2")
        assert fes.ndofs == 693
        form = serial_form(E, torch, "p2", True, CDT, None)
        op = _cached(("op", "pcg"), lambda: E.Operator(form))
        assert isinstance(op.form, E.BilinearForm) and op.size == 693
        b = _cached(("b", "p2"), lambda: _dev(torch, np.random.default_rng(11).uniform(0.0, 1.0, 693)))
        ess = None if setup == "noess" else ess
        jacobi = setup != "plain"
    else:
        op, b, ess = par_setup(E, torch, setup)
        jacobi = True
    x = torch.full((op.size,), float("nan"), dtype=torch.float64, device="cuda")
    it, nrm = op.PCG(b, x, ess=ess, rel_tol=rel_tol, max_iter=max_iter, jacobi=jacobi)
    conv = E.pcg_last_converged()
    if run == "conv":
        assert conv and 1 < it < max_iter, (it, conv)
    else:
        assert it == max_iter and not conv, (it, conv)
    return {"x": sha(x), "iterations": it, "final_norm": float(nrm).hex(), "converged": conv}


def bcg_setup(E, torch, setup):
    """(T, jacobi_of or None, b, ess) of a BiCGSTAB setup."""
    name = setup[:2]
    marked = name == "p3"
    _, fes, _, ess = serial_setup(E, torch, name)
    T = serial_form(E, torch, name, True, CDT, CDT * CONV_SCALE, marked)
    Top = _cached(("op", "bcgT", name, marked), lambda: E.Operator(T))
    Sop = None
    if not setup.endswith("plain"):
        S = serial_form(E, torch, name, True, CDT, None)
        Sop = _cached(("op", "bcgS", name), lambda: E.Operator(S))
    b = _cached(("b", name), lambda: _dev(torch, np.random.default_rng(11).uniform(0.0, 1.0, fes.ndofs)))
    assert isinstance(Top.form, E.BilinearForm) and Top.size == fes.ndofs
    return Top, Sop, b, ess


def run_bcg(E, torch, setup, run):
    rel_tol, max_iter = BCG_RUNS[run]
    Top, Sop, b, ess = bcg_setup(E, torch, setup)
    x = torch.full((Top.size,), float("nan"), dtype=torch.float64, device="cuda")
    it, nrm = Top.BiCGSTAB(b, x, ess=ess, rel_tol=rel_tol, max_iter=max_iter, jacobi_of=Sop)
    conv = E.bicgstab_last_converged()
    if run == "conv":
        assert conv and 1 < it < max_iter, (it, conv)
    else:
        assert it == max_iter and not conv, (it, conv)
    return {"x": sha(x), "iterations": it, "final_norm": float(nrm).hex(), "converged": conv}


def run_ode(E, torch, ode_type, solver, sourced):
    _, fes, _, ess = serial_setup(E, torch, "p2")
    dt = 0.05
    cdt = E.ode_implicit_coeff(ode_type) * dt
    bicg = solver == "bicgstab"
    T = E.Operator(serial_form(E, torch, "p2", True, cdt, cdt * CONV_SCALE if bicg else None))
    K = E.Operator(serial_form(E, torch, "p2", False, 1.0, CONV_SCALE if bicg else None))
    X = fes.dof_coords()
    u = _dev(torch, 37.0 + 20.0 * X[:, 0] * (1.0 - X[:, 1]) + 5.0 * X[:, 2] * X[:, 2])
    kw = {"source": _dev(torch, np.random.default_rng(31).uniform(0.0, 40.0, fes.ndofs))} if sourced else {}
    if bicg:
        kw.update(solver="bicgstab", jacobi_of=E.Operator(serial_form(E, torch, "p2", True, cdt, None)))
    ns, it, conv = E.ode_step(ode_type, T, K, dt, u, ess=ess, rel_tol=1e-10, max_iter=500, **kw)
    assert conv and ns == 3 and it > ns, (ns, it, conv)
    return {"u": sha(u), "solves": ns, "iterations": it, "converged": conv}


def _solve_result(E, x, it, nrm, run, max_iter, **more):
    conv = E.pcg_last_converged()
    if run == "conv":
        assert conv and 1 < it < max_iter, (it, conv)
    else:
        assert it == max_iter and not conv, (it, conv)
    return dict({"x": sha(x), "iterations": it, "final_norm": float(nrm).hex(), "converged": conv}, **more)


def _power_smoother(E, op, ess, order):
    """An order-`order` smoother with the power method's estimate from the library's own start vector."""
    sm = E.ChebyshevSmoother(op, ess=ess, order=order)
    assert sm.order == order == len(sm.coeffs) and sm.power_steps > 0, (sm.order, sm.power_steps)
    return sm


def run_cheb(E, torch, setup, run):
    rel_tol, max_iter = CHEB_SETUPS[setup][run]
    order = int(setup[1])
    if setup.endswith("energy"):
        import record_ts_epilogue_digests as TS
        fes, form, _keep = _cached(("energy",), lambda: TS.build_form(E, torch, (4, 4, 4), "structured", "bioheat"))
        assert fes.ndofs == 729 and form.EnergyParts() == 1   # (A d, d) folded into the Mult
        ess = _cached(("energy", "ess"), lambda: torch.as_tensor(np.asarray(fes.boundary_dofs(), dtype=np.int32)).cuda())
        op = _cached(("op", "energy"), lambda: E.Operator(form))
        b = _cached(("b", "energy"), lambda: _dev(torch, np.random.default_rng(13).uniform(0.0, 1.0, 729)))
    else:
        _, fes, _, ess = serial_setup(E, torch, "p2")
        form = serial_form(E, torch, "p2", True, CDT, None)   # (asserts EnergyParts() == 0: the dot pass)
        op = _cached(("op", "pcg"), lambda: E.Operator(form))
        b = _cached(("b", "p2"), lambda: _dev(torch, np.random.default_rng(11).uniform(0.0, 1.0, 693)))
        ess = None if setup.endswith("noess") else ess
    assert op.size == fes.ndofs and op.size % 2 == 1
    sm = _power_smoother(E, op, ess, order)
    x = torch.full((op.size,), float("nan"), dtype=torch.float64, device="cuda")
    it, nrm = op.PCG(b, x, ess=ess, rel_tol=rel_tol, max_iter=max_iter, prec=sm)
    return _solve_result(E, x, it, nrm, run, max_iter, max_eig=float(sm.max_eig).hex(), power_steps=sm.power_steps)


def run_mg(E, torch, setup, run):
    rel_tol, max_iter = MG_RUNS[run]
    names = ["p1", "p2"]
    fess = [serial_setup(E, torch, nm)[1] for nm in names]
    esss = [serial_setup(E, torch, nm)[3] for nm in names]
    assert [f.ndofs for f in fess] == [120, 693]
    ops = [_cached(("op", "mg", nm), lambda nm=nm: E.Operator(serial_form(E, torch, nm, True, CDT, None))) for nm in names]
    tr = _cached(("mg", "transfer"), lambda: E.PRefinementTransfer(fess[0], fess[1]))
    assert (tr.width, tr.height) == (120, 693)
    sms = [_power_smoother(E, op, ess, 2) for op, ess in zip(ops, esss)]
    B = E.Multigrid(ops, sms, [tr], esss, pre=1, post=1, coarse_pcg=MG_COARSE_PCG if setup == "coarse" else None)
    b = _cached(("b", "p2"), lambda: _dev(torch, np.random.default_rng(11).uniform(0.0, 1.0, 693)))
    x = torch.full((693,), float("nan"), dtype=torch.float64, device="cuda")
    it, nrm = ops[1].PCG(b, x, ess=esss[1], rel_tol=rel_tol, max_iter=max_iter, prec=B)
    return _solve_result(E, x, it, nrm, run, max_iter, max_eig=[float(s.max_eig).hex() for s in sms])


def run_ode_cheb(E, torch, ode_type):
    _, fes, _, ess = serial_setup(E, torch, "p2")
    dt = 0.05
    cdt = E.ode_implicit_coeff(ode_type) * dt
    T = E.Operator(serial_form(E, torch, "p2", True, cdt, None))
    K = E.Operator(serial_form(E, torch, "p2", False, 1.0, None))
    X = fes.dof_coords()
    u = _dev(torch, 37.0 + 20.0 * X[:, 0] * (1.0 - X[:, 1]) + 5.0 * X[:, 2] * X[:, 2])
    sm = _power_smoother(E, T, ess, 2)
    ns, it, conv = E.ode_step(ode_type, T, K, dt, u, ess=ess, rel_tol=1e-10, max_iter=500, prec=sm)
    assert conv and ns == 3 and it > ns, (ns, it, conv)
    return {"u": sha(u), "solves": ns, "iterations": it, "converged": conv, "max_eig": float(sm.max_eig).hex()}


def run_sweep(E, torch, setup):
    """One fixed-work solve at SWEEP_NDOFS dofs."""
    n = SWEEP_NDOFS
    _, fes, _, ess = serial_setup(E, torch, "s2")
    assert fes.ndofs == n and n % 2 == 1 and n > 2 * 256 * 1024
    op = _cached(("op", "sweep"), lambda: E.Operator(serial_form(E, torch, "s2", True, CDT, None)))
    b = _cached(("b", "s2"), lambda: _dev(torch, np.random.default_rng(11).uniform(0.0, 1.0, n)))
    x = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    if setup == "bcg-jacobi":
        Top = _cached(("op", "sweepT"), lambda: E.Operator(serial_form(E, torch, "s2", True, CDT, CDT * CONV_SCALE)))
        it, nrm = Top.BiCGSTAB(b, x, ess=ess, rel_tol=0.0, max_iter=SWEEP_ITERS, jacobi_of=op)
        conv = E.bicgstab_last_converged()
        assert it == SWEEP_ITERS and not conv, (it, conv)
        return {"x": sha(x), "iterations": it, "final_norm": float(nrm).hex(), "converged": conv}
    more = {}
    if setup == "pcg-jacobi":
        kw = {"jacobi": True}
    elif setup == "cheb-o3":
        sm = _power_smoother(E, op, ess, 3)
        kw, more = {"prec": sm}, {"max_eig": float(sm.max_eig).hex(), "power_steps": sm.power_steps}
    else:
        assert setup == "mg-smoother", setup
        fes1, ess1 = serial_setup(E, torch, "s1")[1], serial_setup(E, torch, "s1")[3]
        op1 = _cached(("op", "sweep1"), lambda: E.Operator(serial_form(E, torch, "s1", True, CDT, None)))
        tr = _cached(("sweep", "transfer"), lambda: E.PRefinementTransfer(fes1, fes))
        assert (tr.width, tr.height) == (42 * 42 * 41, n)
        sms = [_power_smoother(E, o, e, 2) for o, e in ((op1, ess1), (op, ess))]
        kw = {"prec": E.Multigrid([op1, op], sms, [tr], [ess1, ess], pre=1, post=1)}
        more = {"max_eig": [float(s.max_eig).hex() for s in sms]}
    it, nrm = op.PCG(b, x, ess=ess, rel_tol=0.0, max_iter=SWEEP_ITERS, **kw)
    return _solve_result(E, x, it, nrm, "fixed", SWEEP_ITERS, **more)


def run_case(E, torch, cid):
    kind, rest = cid.split("-", 1)
    if kind == "sweep":
        return run_sweep(E, torch, rest)
    if cid == "ode-23-cheb":
        return run_ode_cheb(E, torch, 23)
    if kind == "ode":
        t, solver = rest.split("-")
        return run_ode(E, torch, int(t), solver, dict(((a, b), c) for a, b, c in ODE_CASES)[(int(t), solver)])
    setup, run = rest.rsplit("-", 1)
    return {"pcg": run_pcg, "bcg": run_bcg, "cheb": run_cheb, "mg": run_mg}[kind](E, torch, setup, run)


def run_sequence(E, torch, sequence=SEQUENCE):
    """The results of a sequence's solves, run one after the other."""
    return [run_case(E, torch, cid) for cid in sequence]


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import helpers  # noqa: F401  (registers the package as ecm2_amd)
    import torch
    import ecm2_amd as E
    E.load_library()
    prec, sweep = "--prec" in argv[1:], "--sweep" in argv[1:]
    args = [a for a in argv[1:] if a not in ("--prec", "--sweep")]
    out = args[0] if args else (DIGESTS_SWEEP if sweep else DIGESTS_PREC if prec else DIGESTS)
    cases, sequence = (prec_cases(), PREC_SEQUENCE) if prec else (all_cases(), SEQUENCE)
    if sweep:   # (one shape, fixed work: no sequence)
        cases, sequence = sweep_cases(), []
    digests, refused = {}, []
    for cid in cases:
        first, second = run_case(E, torch, cid), run_case(E, torch, cid)
        print(cid, first, flush=True)
        if first != second:
            refused.append(cid)
            print("  REFUSED: the second run gave", second, flush=True)
            continue
        digests[cid] = first
    alone = dict(digests)
    if prec:   # the sequence's solves of the first group: their digests in the first file
        with open(DIGESTS) as fh:
            alone.update(json.load(fh))
    seq = run_sequence(E, torch, sequence)
    for cid, got in zip(sequence, seq):
        assert got == alone[cid], ("sequence", cid, got, alone[cid])
    assert not seq or seq[0] == seq[-1]
    print("sequence equals the solves run alone")
    with open(out, "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out, "refused:", refused)


if __name__ == "__main__":
    main(sys.argv)
