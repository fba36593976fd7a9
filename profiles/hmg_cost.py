#!/usr/bin/env python3
"""Cost of the PCG preconditioned by the h+p multigrid V-cycle against Jacobi-PCG and against
the p-only cycle with ex26's coarse PCG (section 4f), profiles/mg_cost.py's protocol: boundary dofs essential, rel_tol
1e-10, the seeded right-hand side, Diffusion alone with bench.py's bioheat coefficient on every level; after a
warm-up solve, three repetitions, HIP events around each call; recorded: iterations, ms per solve (median and the
three values), ms per iteration.
  C4  (27^3, 1) -> (54^3, 1) -> (108^3, 1) -> (108^3, 2)
  C5  (17^3, 1) -> (34^3, 1) -> (68^3, 1) -> (68^3, 2) -> (68^3, 4)
The meshes are a Cartesian mesh and its uniform refinements, so every space is in the entity numbering and the
refined meshes' element order (child k of element i at 8 i + k) -- not section 4f's structured lattice; the same run's
Jacobi-PCG and p-only cycles are therefore timed on the same finest space.  Solvers: "jacobi"; "p_vcycle_pcg" (the
levels of the finest mesh, ex26's coarse PCG (1e-2, 200): section 4f's form); "p_vcycle_smoother" (the same levels,
the coarsest smoothed once); "hp_vcycle" (all levels, the coarsest smoothed once).  Then the two h-transfer kernels
alone at the (n/2, 1) -> (n, 1) pair (profiles/transfer_cost.py's transfer_times): ms per call and the bytes that
must move.  Reported, not gated.  One MI355X; one JSON line per shape.

Usage: python profiles/hmg_cost.py [c4|c5|all] [reps = 3] [n0 (overrides the coarsest mesh's elements per side)]
       python profiles/hmg_cost.py kernels [n0]     (the two kernels at the C4 pair alone: what a rocprofv3
                                                     --kernel-trace --stats run wraps)
       --lib=path times another build of the library"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from transfer_cost import load, timed_call, transfer_times  # noqa: E402

REL_TOL = 1e-10
EX26_COARSE = (1e-2, 200)
SHAPES = {"c4": (27, 2, (2,)), "c5": (17, 2, (2, 4))}   # n0, refinements, the orders above p = 1 on the finest mesh


def hierarchy(E, n0, refinements):
    meshes = [E.Mesh.MakeCartesian3D(n0, n0, n0)]
    for _ in range(refinements):
        m = meshes[-1].Copy()
        m.UniformRefinement()
        meshes.append(m)
    return meshes


def run(E, shape, reps, n0_override):
    n0, refinements, top = SHAPES[shape]
    n0 = n0_override or n0
    meshes = hierarchy(E, n0, refinements)
    spaces = [E.H1Space(m, 1) for m in meshes] + [E.H1Space(meshes[-1], p) for p in top]
    level_mesh = meshes + [meshes[-1]] * len(top)
    fes = spaces[-1]
    nd = fes.ndofs
    ess = [torch.as_tensor(np.asarray(s.boundary_dofs())).cuda() for s in spaces]
    b = torch.empty(nd, dtype=torch.float64, device="cuda")
    b.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(3))
    b[ess[-1].long()] = 0.0
    keep, ops = [], []
    for m, s in zip(level_mesh, spaces):
        a, T = bench.bioheat_coefficients(E, torch, m, s)
        keep.extend([a, T])
        _, diff = bench.bench_integrators(E)
        f = E.BilinearForm(s)
        f.AddDomainIntegrator(diff(T))
        f.Assemble()
        ops.append(E.Operator(f))
    A = ops[-1]
    res = {"shape": shape, "operator": "k", "elements": [s.ne for s in spaces], "orders": [s.order for s in spaces],
           "ndofs": [s.ndofs for s in spaces], "rel_tol": REL_TOL, "reps": reps, "kernel": f.info()["kernel"], "solvers": {}}
    ms_s, sm = timed_call(lambda: [E.ChebyshevSmoother(o, ess=e, order=2) for o, e in zip(ops, ess)])
    nh = refinements
    ms_t, tr = timed_call(lambda: [E.HRefinementTransfer(lo, hi) for lo, hi in zip(spaces[:nh], spaces[1:nh + 1])]
                          + [E.PRefinementTransfer(lo, hi) for lo, hi in zip(spaces[nh:-1], spaces[nh + 1:])])
    res["setup_ms"] = {"smoothers": round(ms_s, 3), "transfer_plans": round(ms_t, 3)}
    res["max_eig"] = [s.max_eig for s in sm]
    res["plan_bytes"] = [t.plan_bytes for t in tr]
    solvers = [("jacobi", None),
               ("p_vcycle_pcg", E.Multigrid(ops[nh:], sm[nh:], tr[nh:], ess[nh:], coarse_pcg=EX26_COARSE)),
               ("p_vcycle_smoother", E.Multigrid(ops[nh:], sm[nh:], tr[nh:], ess[nh:])),
               ("hp_vcycle", E.Multigrid(ops, sm, tr, ess))]
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
    top_x = float(xs["jacobi"].abs().max())
    res["x_against_jacobi"] = {k: float((v - xs["jacobi"]).abs().max()) / top_x for k, v in xs.items() if k != "jacobi"}
    jac = res["solvers"]["jacobi"]["solve_ms"]
    res["solve_time_against_jacobi"] = {k: round(v["solve_ms"] / jac, 4) for k, v in res["solvers"].items()}
    transfer_times(tr[nh - 1], spaces[nh - 1], spaces[nh], res)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)


def kernels_only(E, n0):
    meshes = hierarchy(E, n0, 1)
    res = {"shape": "kernels"}
    lo, hi = E.H1Space(meshes[0], 1), E.H1Space(meshes[1], 1)
    transfer_times(E.HRefinementTransfer(lo, hi), lo, hi, res)
    print(json.dumps(res), flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "all"
    E = load(sys.argv[1:])
    if which == "kernels":
        return kernels_only(E, int(args[1]) if len(args) > 1 else 54)
    reps = int(args[1]) if len(args) > 1 else 3
    n0_override = int(args[2]) if len(args) > 2 else 0
    for shape in (("c4", "c5") if which == "all" else (which,)):
        run(E, shape, reps, n0_override)


if __name__ == "__main__":
    main()
