#!/usr/bin/env python3
"""Cost of the device elimination and the gain of a warm start.  Reported, not gated.

elim: on configs[3] (Cartesian 108^3, p = 2, 10.2M dofs) and configs[4] (68^3, p = 4) with bench.py's timed form
(Mass + Diffusion, structured numbering) and the boundary dofs essential, Operator.EliminateRHS against one
Operator.Mult of the same form in the same process: HIP events around each call after a warm-up, the median of
`reps` (the elimination ends with a stream synchronisation, inside the events).

warm: examples/rf_electrode.cpp's problem at n^3 elements (default 32), p = 2: phi = 30 on x = 0, 0 on x = 1,
sigma = 1 + x, Jacobi-PCG to rel_tol 1e-12 from the lifted data; then sigma changes by 1 % (sigma' = 1.01 + x: as
after a re-assembly of sigma(T)) and the potential is solved again to the first solve's absolute goal, cold (x = the
lifted data) and warm (x = the previous potential): the two iteration counts and times.

One MI355X; one JSON line per part.  Usage: python profiles/ess_cost.py [elim|warm|all] [reps = 5] [n = 32]"""
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

SHAPES = {"c4": (108, 2), "c5": (68, 4)}


def timed_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def elim(E, shape, reps):
    n, order = SHAPES[shape]
    mesh, fes = bench.cartesian_space(E, n, n, n, order, "structured", "affine")
    keep = []
    form = bench.bench_form(E, torch, mesh, fes, keep)
    A = E.Operator(form)
    ess = torch.as_tensor(np.asarray(fes.boundary_dofs())).cuda()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda").uniform_(0.0, 1.0, generator=g)
    b0 = torch.empty_like(x).uniform_(0.0, 1.0, generator=g)
    b, y = b0.clone(), torch.empty_like(x)
    calls = {"mult_ms": lambda: A.Mult(x, y), "eliminate_rhs_ms": lambda: A.EliminateRHS(x, b, ess)}
    res = {"part": "elim", "shape": shape, "ndofs": fes.ndofs, "n_ess": int(ess.numel()), "order": order,
           "kernel": form.info()["kernel"], "reps": reps}
    for key, fn in calls.items():
        for _ in range(3):
            fn()
        times = [timed_call(fn)[0] for _ in range(reps)]
        res[key] = round(statistics.median(times), 4)
        res[key + "_all"] = [round(t, 4) for t in times]
    res["eliminate_over_mult"] = round(res["eliminate_rhs_ms"] / res["mult_ms"], 3)
    # one Mult plus the memset of w, b -= z (3 streams) and two list kernels
    res["vector_stream_bytes"] = 8 * fes.ndofs * 4
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)


def warm(E, n, reps):
    order, V0 = 2, 30.0
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    fes = E.H1Space(mesh, order)
    attr = mesh.GetBdrAttributes()
    marker = np.zeros(int(attr.max()), np.int32)
    marker[[5 - 1, 3 - 1]] = 1      # Make3D's sides x = 0 and x = 1
    ess_h = fes.essential_dofs(marker)
    X = fes.dof_coords()
    lift = np.zeros(fes.ndofs)
    lift[ess_h] = np.where(X[ess_h, 0] < 0.5, V0, 0.0)
    ess = torch.as_tensor(ess_h).cuda()
    P = mesh.quadrature_points(order + 2)

    def operator(shift):
        f = E.BilinearForm(fes)
        q = torch.as_tensor((shift + P[..., 0]).reshape(fes.ne, -1)).cuda()
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.QuadratureCoefficient(q)))
        f.Assemble()
        return E.Operator(f), (f, q)

    def solve(A, x0, **kw):
        x = torch.as_tensor(x0).cuda() if isinstance(x0, np.ndarray) else x0.clone()
        b = torch.zeros_like(x)
        A.FormLinearSystem(ess, x, b, copy_interior=True)
        ms, (it, nrm) = timed_call(lambda: A.PCG(b, x, ess=ess, max_iter=5000, iterative_mode=True, **kw))
        assert E.pcg_last_converged()
        return x, it, nrm, ms
    A0, keep0 = operator(1.0)
    solve(A0, lift, rel_tol=1e-12)  # warm-up: workspaces, code objects
    phi0, it0, _, ms0 = solve(A0, lift, rel_tol=1e-12)
    # the first solve's goal as an absolute tolerance: rel_tol sqrt(nom_0), nom_0 from a solve that stops at once
    _, _, norm0, _ = solve(A0, lift, rel_tol=1.0)
    goal = 1e-12 * norm0
    A1, keep1 = operator(1.01)
    res = {"part": "warm", "n": n, "ndofs": fes.ndofs, "n_ess": int(ess.numel()), "abs_tol": goal,
           "first_solve": {"iterations": it0, "ms": round(ms0, 3)}}
    for label, start in (("cold", lift), ("warm", phi0)):
        runs = [solve(A1, start, rel_tol=0.0, abs_tol=goal) for _ in range(reps)]
        res[label] = {"iterations": runs[0][1], "ms": round(statistics.median(r[3] for r in runs), 3)}
        res[label + "_x"] = runs[0][0]
    top = float(res["cold_x"].abs().max())
    res["warm_against_cold"] = float((res.pop("warm_x") - res.pop("cold_x")).abs().max()) / top
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res), flush=True)


def main():
    args = sys.argv[1:]
    which = args[0] if args else "all"
    reps = int(args[1]) if len(args) > 1 else 5
    n = int(args[2]) if len(args) > 2 else 32
    E = _load_pkg()
    E.load_library()
    if which in ("elim", "all"):
        for shape in SHAPES:
            elim(E, shape, reps)
    if which in ("warm", "all"):
        warm(E, n, reps)


if __name__ == "__main__":
    main()
