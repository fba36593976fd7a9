#!/usr/bin/env python3
"""Cost of the PCG preconditioned by the p-multigrid V-cycle against Jacobi-PCG, boundary dofs
essential, rel_tol 1e-10, the seeded right-hand side of profiles/cheb_cost.py:
  C4  Cartesian 108^3 elements, H1 p = 2, levels 1 -> 2 (structured numbering; bench.py's bioheat coefficients on
      every level): "k" Diffusion alone, "mk" Mass + Diffusion;
  C5  Cartesian 68^3 elements, H1 p = 4, levels 1 -> 2 -> 4: "k".
Each solver -- Jacobi-PCG (the baseline: the same run's untouched path), the V-cycle PCG with the coarsest level's
smoother as the coarse solve and with ex26's coarse PCG (1e-2, 200) -- after a warm-up solve, three repetitions,
HIP events around each call; recorded: iterations, ms per solve (median and the three values), ms per iteration.
The set-up (forms aside: the smoothers' diagonals and power steps, the transfer plans) is timed beside them, and
each transfer direction (profiles/transfer_cost.py's transfer_times) and the fine Mult alone (20 calls).  Reported,
not gated.  One MI355X; one JSON line per solve.

Usage: python profiles/mg_cost.py [c4|c5|all] [reps = 3] [n (overrides the shape's elements per side)] [--lib=path]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from transfer_cost import call_ms, load, timed_call, transfer_times  # noqa: E402

REL_TOL = 1e-10
EX26_COARSE = (1e-2, 200)
SHAPES = {"c4": (108, (1, 2), ("k", "mk")), "c5": (68, (1, 2, 4), ("k",))}


def run(E, shape, reps, n_override):
    n, orders, operators = SHAPES[shape]
    n = n_override or n
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    spaces = [E.H1Space(mesh, p, E.NUMBERING_STRUCTURED) for p in orders]
    fes = spaces[-1]
    nd = fes.ndofs
    ess = [torch.as_tensor(np.asarray(s.boundary_dofs())).cuda() for s in spaces]
    b = torch.empty(nd, dtype=torch.float64, device="cuda")
    b.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(3))
    b[ess[-1].long()] = 0.0
    keep = []
    for name in operators:
        ops = []
        for s in spaces:
            a, T = bench.bioheat_coefficients(E, torch, mesh, s)
            keep.extend([a, T])
            mass, diff = bench.bench_integrators(E)
            f = E.BilinearForm(s)
            if name == "mk":
                f.AddDomainIntegrator(mass(a))
            f.AddDomainIntegrator(diff(T))
            f.Assemble()
            ops.append(E.Operator(f))
        A = ops[-1]
        res = {"shape": shape, "operator": name, "elements": fes.ne, "orders": list(orders),
               "ndofs": [s.ndofs for s in spaces], "rel_tol": REL_TOL, "reps": reps, "solvers": {}}
        ms_s, sm = timed_call(lambda: [E.ChebyshevSmoother(o, ess=e, order=2) for o, e in zip(ops, ess)])
        ms_t, tr = timed_call(lambda: [E.PRefinementTransfer(lo, hi) for lo, hi in zip(spaces[:-1], spaces[1:])])
        res["setup_ms"] = {"smoothers": round(ms_s, 3), "transfer_plans": round(ms_t, 3)}
        res["max_eig"] = [s.max_eig for s in sm]
        res["plan_bytes"] = [t.plan_bytes for t in tr]
        solvers = [("jacobi", None), ("vcycle_smoother", E.Multigrid(ops, sm, tr, ess)),
                   ("vcycle_pcg", E.Multigrid(ops, sm, tr, ess, coarse_pcg=EX26_COARSE))]
        xs = {}
        for label, B in solvers:
            x = torch.empty_like(b)
            solve = lambda: A.PCG(b, x, ess=ess[-1], rel_tol=REL_TOL, max_iter=5000, jacobi=True, prec=B)
            solve()  # warm-up: workspaces, code objects
            times, its = [], None
            for _ in range(reps):
                ms, (it, nrm) = timed_call(solve)
                assert E.pcg_last_converged() and (its is None or its == it)
                times.append(ms)
                its = it
            med = statistics.median(times)
            res["solvers"][label] = {"iterations": its, "solve_ms": round(med, 3),
                                     "solve_ms_all": [round(t, 3) for t in times], "iteration_ms": round(med / its, 5)}
            xs[label] = x
        top = float(xs["jacobi"].abs().max())
        res["x_against_jacobi"] = {k: float((v - xs["jacobi"]).abs().max()) / top for k, v in xs.items() if k != "jacobi"}
        jac = res["solvers"]["jacobi"]["solve_ms"]
        res["solve_time_against_jacobi"] = {k: round(v["solve_ms"] / jac, 4) for k, v in res["solvers"].items()}
        # the transfer's two directions (profiles/transfer_cost.py) and the fine Mult alone at the finest pair (the
        # rocprofv3 run reads the same calls per kernel)
        transfer_times(tr[-1], spaces[-2], spaces[-1], res)
        yf = torch.empty_like(b)
        res["mult_ms"] = call_ms(lambda: A.Mult(b, yf))
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        del solvers, sm, tr, ops, xs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "all"
    reps = int(args[1]) if len(args) > 1 else 3
    n_override = int(args[2]) if len(args) > 2 else 0
    E = load(sys.argv[1:])
    for shape in (("c4", "c5") if which == "all" else (which,)):
        run(E, shape, reps, n_override)


if __name__ == "__main__":
    main()
