#!/usr/bin/env python3
"""Cost of a device BiCGSTAB iteration on the configs[3] form (Cartesian 108^3 elements, H1 p = 2, structured
numbering, 10.2M dofs; bench.py's Mass(rho c_eff(x)) + Diffusion(gamma dt k(T)), the snapshot kernel) with the
blood-pool slab convection of profiles/convection_cost.py (the lowest ~10% of the z layers) inside the
operator, Jacobi from the symmetric form: the marginal iteration -- (time of a solve stopped at max_iter = N2
- one stopped at N1) / (N2 - N1), HIP events around the calls -- against two marginal Jacobi-PCG iterations
(two Mults) of the same form without convection, the timed windows alternated in one run after a warm-up.
The yardstick is the PCG, not the code under test.  Beside them the same run's stream rates and the bytes
each fused pass must move (8 n B per vector stream):
  bcg_update_p 6 streams, (r~, v) 2, bcg_update_s 5, (t, s) + (t, t) 2, bcg_update_xr 8: 23 in all.
The passes' own times come from a kernel trace taken in a run of its own:
  rocprofv3 --kernel-trace --stats -- python profiles/bicgstab_cost.py 108 5 --solve-only
Reported, not gated.  One MI355X; prints one JSON line.

Usage: python profiles/bicgstab_cost.py [n = 108] [rounds = 7] [--solve-only]"""
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

VEL = [0.8, -0.3, 0.5]
ALPHA = 3.8e6 * 1e-3   # rho_b c_b times a stage's c dt: the convection inside T = M + c dt (K + C)
N1, N2 = 5, 25
STREAMS = {"k_bcg_update_p": 6, "k_bcg_dot (r~, v)": 2, "k_bcg_update_s": 5, "k_bcg_dot (t, s), (t, t)": 2,
           "k_bcg_update_xr": 8}


def timed_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    solve_only = "--solve-only" in sys.argv
    n = int(args[0]) if len(args) > 0 else 108
    rounds = int(args[1]) if len(args) > 1 else 7
    E = _load_pkg()
    E.load_library()
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    layers = max(1, round(0.1 * n))
    attr = np.ones(n ** 3, np.int32)
    attr[: layers * n * n] = 2          # lexicographic elements: the lowest z layers
    mesh.SetAttributes(attr)
    fes = E.H1Space(mesh, 2, E.NUMBERING_STRUCTURED)
    keep = []
    forms = {}
    for name in ("sym", "conv"):
        a, T = bench.bioheat_coefficients(E, torch, mesh, fes)
        keep += [a, T]
        mass, diff = bench.bench_integrators(E)
        f = E.BilinearForm(fes)
        f.AddDomainIntegrator(mass(a))
        f.AddDomainIntegrator(diff(T))
        if name == "conv":
            f.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(VEL), ALPHA), [0, 1])
        f.Assemble()
        forms[name] = f
    S, A = E.Operator(forms["sym"]), E.Operator(forms["conv"])
    nd = fes.ndofs
    ess = torch.as_tensor(np.asarray(fes.boundary_dofs())).cuda()
    b = torch.empty(nd, dtype=torch.float64, device="cuda").uniform_(0.0, 1.0)
    x = torch.empty_like(b)
    # never converged inside the window: rel_tol far below what N2 iterations reach
    bicg = lambda it: A.BiCGSTAB(b, x, ess=ess, rel_tol=1e-200, max_iter=it, jacobi_of=S)
    pcg = lambda it: S.PCG(b, x, ess=ess, rel_tol=1e-200, max_iter=it, jacobi=True)
    res = {"elements": fes.ne, "ndofs": nd, "active_elements": forms["conv"].ConvectionInfo()[1],
           "snapshot": forms["sym"].CoefficientSnapshot(), "energy_parts": forms["sym"].EnergyParts(), "n1": N1, "n2": N2}
    if solve_only:
        for _ in range(rounds):
            res["bicgstab_iterations"] = bicg(N2)[0]
        print(json.dumps(res))
        return
    for _ in range(2):   # warm-up: workspaces, code objects
        bicg(N1)
        pcg(2 * N1)
    t = {"b1": [], "b2": [], "p1": [], "p2": []}
    for _ in range(rounds):   # alternated windows
        t["b1"].append(timed_call(lambda: bicg(N1)))
        t["p1"].append(timed_call(lambda: pcg(2 * N1)))
        t["b2"].append(timed_call(lambda: bicg(N2)))
        t["p2"].append(timed_call(lambda: pcg(2 * N2)))
    assert bicg(N2)[0] == N2 and pcg(2 * N2)[0] == 2 * N2
    med = {k: statistics.median(v) for k, v in t.items()}
    res["bicgstab_iteration_ms"] = round((med["b2"] - med["b1"]) / (N2 - N1), 5)
    res["two_pcg_iterations_ms"] = round((med["p2"] - med["p1"]) / (N2 - N1), 5)
    res["ratio"] = round(res["bicgstab_iteration_ms"] / res["two_pcg_iterations_ms"], 4)
    y = torch.empty_like(b)
    mult = {}
    for name, f in forms.items():
        for _ in range(3):
            f.Mult(b, y)
        mult[name] = round(statistics.median(timed_call(lambda: [f.Mult(b, y) for _ in range(10)]) / 10 for _ in range(5)), 5)
    res["mult_ms"] = mult
    copy, read = bench.stream_copy_peak(E, torch)
    res["stream_copy_gbs"], res["stream_read_gbs"] = copy, read
    res["pass_bytes"] = {k: 8 * nd * s for k, s in STREAMS.items()}
    res["pass_ms_at_stream_copy"] = {k: round(8 * nd * s / (copy * 1e9) * 1e3, 5) for k, s in STREAMS.items()}
    res["vector_streams"] = sum(STREAMS.values())
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
