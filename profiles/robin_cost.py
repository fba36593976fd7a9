#!/usr/bin/env python3
"""Cost of the Robin boundary term on the configs[3] form (Cartesian 108^3 elements, H1 p = 2,
structured numbering, 10.2M dofs; bench.py's Mass(rho c_eff(x)) + Diffusion(gamma dt k(T))): the Mult
and the marginal Jacobi-PCG iteration, HIP-event timed, without a boundary term, with Robin on one
side (attribute 3: 11,664 faces) and on all six (69,984 faces against 1,259,712 elements).  Reported,
not gated (boundary section).  One MI355X; prints one JSON line.

Usage: python profiles/robin_cost.py [n = 108] [reps = 50] [--mult-only]
  --mult-only: the three forms' Mults alone, for a kernel trace of the face kernels taken in a run of
  its own (rocprofv3 --kernel-trace --stats -- python profiles/robin_cost.py 108 20 --mult-only)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_pkg  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    mult_only = "--mult-only" in sys.argv
    n = int(args[0]) if len(args) > 0 else 108
    reps = int(args[1]) if len(args) > 1 else 50
    E = _load_pkg()
    E.load_library()
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    fes = E.H1Space(mesh, 2, E.NUMBERING_STRUCTURED)
    keep = []
    h = 25.0
    cases = {"none": None, "one_side": [0, 0, 1, 0, 0, 0], "all_sides": [1] * 6}
    x = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5)
    y = torch.empty_like(x)
    b = torch.empty_like(x).uniform_(0.5, 1.5)
    res = {"elements": fes.ne, "ndofs": fes.ndofs, "boundary_faces": mesh.GetNBE(), "cases": {}}
    for name, marker in cases.items():
        a, T = bench.bioheat_coefficients(E, torch, mesh, fes)
        keep += [a, T]
        mass, diff = bench.bench_integrators(E)
        f = E.BilinearForm(fes)
        f.AddDomainIntegrator(mass(a))
        f.AddDomainIntegrator(diff(T))
        if marker is not None:
            f.AddBoundaryIntegrator(E.MassIntegrator(E.ConstantCoefficient(h)), marker)
        f.Assemble()
        out = {"active_faces": f.BoundaryInfo()[2], "energy_parts": f.EnergyParts(),
               "mult_ms": round(timed(lambda: f.Mult(x, y), reps), 5)}
        if not mult_only:
            # marginal iteration: two fixed-length solves (rel_tol 0 never stops early)
            u = torch.zeros_like(x)
            k1, k2 = 10, 40
            solve = lambda k: f.PCG(b, u, rel_tol=0.0, max_iter=k, jacobi=True)
            t1 = timed(lambda: solve(k1), 5)
            t2 = timed(lambda: solve(k2), 5)
            out["pcg_iteration_ms"] = round((t2 - t1) / (k2 - k1), 5)
        res["cases"][name] = out
        del f
    base = res["cases"]["none"]
    for name in ("one_side", "all_sides"):
        c = res["cases"][name]
        c["mult_extra_ms"] = round(c["mult_ms"] - base["mult_ms"], 5)
        c["faces_over_elements"] = round(c["active_faces"] / fes.ne, 5)
        if not mult_only:
            c["pcg_iteration_extra_ms"] = round(c["pcg_iteration_ms"] - base["pcg_iteration_ms"], 5)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
