#!/usr/bin/env python3
"""Cost of the convection term on the configs[3] form (Cartesian 108^3 elements, H1 p = 2, structured
numbering, 10.2M dofs; bench.py's Mass(rho c_eff(x)) + Diffusion(gamma dt k(T)), the snapshot kernel): the
Mult, HIP-event timed, without the term, with a ConvectionIntegrator whose marker selects nothing (it must
time like the plain form: the same launches), on a blood-pool slab of about 10% of the elements (the lowest
z layers) and on all elements; the convection-only form (memset + apply + add); and, in the same run, the
full per-point-layout volume Mult (bench.py --geometry full) and the stream rates, against which the bytes
the two passes must move are set:
  apply: per active element 24 Q^3 B of qdata, 4 ND B of map, 8 ND B of E-vector written; 8 B per touched dof of x
  add:   per active element 8 ND B of E-vector read and 4 ND B of CSR entries; 24 B per touched dof (row, y read and written)
Reported, not gated.  One MI355X; prints one JSON line.

Usage: python profiles/convection_cost.py [n = 108] [reps = 50] [--mult-only]
  --mult-only: the slab and all-elements forms' Mults alone, for a kernel trace of k_conv_apply_tpe and
  k_conv_add taken in a run of its own (rocprofv3 --kernel-trace --stats -- python profiles/convection_cost.py
  108 20 --mult-only)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import _load_pkg  # noqa: E402

VEL, ALPHA = [0.8, -0.3, 0.5], 3.8e6   # a uniform flow; rho_b c_b


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
    layers = max(1, round(0.1 * n))
    attr = np.ones(n ** 3, np.int32)
    attr[: layers * n * n] = 2          # lexicographic elements: the lowest z layers
    mesh.SetAttributes(attr)
    p, q1d = 2, 4
    fes = E.H1Space(mesh, p, E.NUMBERING_STRUCTURED)
    nd, nq = (p + 1) ** 3, q1d ** 3
    keep = []
    cases = {"none": "absent", "empty_marker": [0, 0], "slab": [0, 1], "all": None}
    if mult_only:
        cases = {"slab": [0, 1], "all": None}
    x = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5)
    y = torch.empty_like(x)
    res = {"elements": fes.ne, "ndofs": fes.ndofs, "p": p, "q1d": q1d, "slab_layers": layers, "cases": {}}
    gm = fes.gather_map()
    for name, marker in cases.items():
        a, T = bench.bioheat_coefficients(E, torch, mesh, fes)
        keep += [a, T]
        mass, diff = bench.bench_integrators(E)
        f = E.BilinearForm(fes)
        f.AddDomainIntegrator(mass(a))
        f.AddDomainIntegrator(diff(T))
        if marker != "absent":
            f.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(VEL), ALPHA), marker)
        f.Assemble()
        n_act = f.ConvectionInfo()[1]
        out = {"active_elements": n_act, "snapshot": f.CoefficientSnapshot(), "energy_parts": f.EnergyParts(),
               "mult_ms": round(timed(lambda: f.Mult(x, y), reps), 5),
               "mult_transpose_ms": round(timed(lambda: f.MultTranspose(x, y), reps), 5)}
        if n_act:
            rows = int(np.unique(gm[: n_act]).size) if marker is not None else fes.ndofs  # (the slab: the first elements)
            out["touched_dofs"] = rows
            out["apply_bytes"] = n_act * (24 * nq + 4 * nd + 8 * nd) + 8 * rows
            out["add_bytes"] = n_act * (8 * nd + 4 * nd) + 24 * rows
        res["cases"][name] = out
        del f
    if not mult_only:
        # the convection-only form: memset of y, the apply, the add
        c = E.BilinearForm(fes)
        c.AddDomainIntegrator(E.ConvectionIntegrator(E.VectorCoefficient(VEL), ALPHA))
        c.Assemble()
        res["convection_only_mult_ms"] = round(timed(lambda: c.Mult(x, y), reps), 5)
        res["memset_ms"] = round(timed(lambda: y.zero_(), reps), 5)
        del c
        # the same run's full per-point-layout volume Mult (56 B per point) and the stream rates
        full = bench.bench_form(E, torch, mesh, fes, keep, compress_geometry=False, coefficient_snapshot=False)
        res["full_layout_mult_ms"] = round(timed(lambda: full.Mult(x, y), reps), 5)
        res["full_layout_qdata_bytes"] = full.qdata_bytes()
        del full
        copy, read = bench.stream_copy_peak(E, torch)
        res["stream_copy_gbs"], res["stream_read_gbs"] = copy, read
        base = res["cases"]["none"]
        for name in ("empty_marker", "slab", "all"):
            cs = res["cases"][name]
            cs["mult_extra_ms"] = round(cs["mult_ms"] - base["mult_ms"], 5)
            if "apply_bytes" in cs:
                cs["bytes_at_stream_read_ms"] = round((cs["apply_bytes"] + cs["add_bytes"]) / (read * 1e9) * 1e3, 5)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
