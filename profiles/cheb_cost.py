#!/usr/bin/env python3
"""Cost of the Chebyshev-preconditioned PCG against Jacobi-PCG on the configs[3] shape (Cartesian 108^3 elements,
H1 p = 2, structured numbering, 10.2M dofs; bench.py's bioheat coefficients, the snapshot kernel), boundary
dofs essential, for two operators:
  (a) "k"   Diffusion(gamma dt k(T)) alone -- the RF-potential shape, no mass to bound the condition number;
  (b) "mk"  the headline Mass(rho c_eff(x)) + Diffusion(gamma dt k(T)).
Each solver -- Jacobi-PCG (the baseline: the same run's untouched code path), Chebyshev-PCG of orders 2 and 3 with
the power method's default estimate -- solves a seeded right-hand side to rel_tol 1e-10, three repetitions after a
warm-up solve, HIP events around each call; recorded: iterations, ms per solve (median and the three values) and
ms per iteration (ms per solve / iterations: the solve's setup and read-backs inside).  The smoother's
construction (the diagonal and ten power steps) is timed beside them, once.
Reported, not gated.  One MI355X; prints one JSON line per operator.

Usage: python profiles/cheb_cost.py [n = 108] [reps = 3]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_pkg  # noqa: E402

REL_TOL = 1e-10


def timed_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 108
    reps = int(args[1]) if len(args) > 1 else 3
    E = _load_pkg()
    E.load_library()
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    fes = E.H1Space(mesh, 2, E.NUMBERING_STRUCTURED)
    nd = fes.ndofs
    ess = torch.as_tensor(np.asarray(fes.boundary_dofs())).cuda()
    b = torch.empty(nd, dtype=torch.float64, device="cuda")
    b.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(3))
    b[ess.long()] = 0.0
    keep = []
    for name in ("k", "mk"):
        a, T = bench.bioheat_coefficients(E, torch, mesh, fes)
        keep += [a, T]
        mass, diff = bench.bench_integrators(E)
        f = E.BilinearForm(fes)
        if name == "mk":
            f.AddDomainIntegrator(mass(a))
        f.AddDomainIntegrator(diff(T))
        f.Assemble()
        A = E.Operator(f)
        res = {"operator": name, "elements": fes.ne, "ndofs": nd, "rel_tol": REL_TOL, "reps": reps,
               "snapshot": f.CoefficientSnapshot(), "energy_parts": f.EnergyParts(), "solvers": {}}
        xs = {}
        solvers = [("jacobi", None)]
        for order in (2, 3):
            ms, S = timed_call(lambda: E.ChebyshevSmoother(A, ess=ess, order=order))
            res.setdefault("smoother_setup_ms", {})[f"order{order}"] = round(ms, 3)
            res["max_eig"], res["power_steps"] = S.max_eig, S.power_steps
            solvers.append((f"chebyshev{order}", S))
        for label, S in solvers:
            x = torch.empty_like(b)
            solve = lambda: A.PCG(b, x, ess=ess, rel_tol=REL_TOL, max_iter=5000, jacobi=True, prec=S)
            solve()  # warm-up: workspaces, code objects
            times, its = [], None
            for _ in range(reps):
                ms, (it, nrm) = timed_call(solve)
                assert E.pcg_last_converged() and (its is None or its == it)
                times.append(ms)
                its = it
            med = statistics.median(times)
            res["solvers"][label] = {"iterations": its, "solve_ms": round(med, 3), "solve_ms_all": [round(t, 3) for t in times],
                                     "iteration_ms": round(med / its, 5), "final_norm": nrm}
            xs[label] = x
        top = float(xs["jacobi"].abs().max())
        res["x_against_jacobi"] = {k: float((v - xs["jacobi"]).abs().max()) / top for k, v in xs.items() if k != "jacobi"}
        jac = res["solvers"]["jacobi"]["solve_ms"]
        res["solve_time_against_jacobi"] = {k: round(v["solve_ms"] / jac, 4) for k, v in res["solvers"].items()}
        y = torch.empty_like(b)
        for _ in range(3):
            f.Mult(b, y)
        res["mult_ms"] = round(statistics.median(timed_call(lambda: [f.Mult(b, y) for _ in range(10)])[0] / 10
                                                 for _ in range(5)), 5)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
