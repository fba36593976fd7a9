#!/usr/bin/env python3
"""Time of one device LinearForm.Assemble at the C4 size (Cartesian 108^3 elements, H1 p = 2,
structured numbering, 10.2M dofs) with the Joule source sigma(T) |grad phi|^2 -- beside the bytes it
must move, this run's own STREAM rates, and the Mult of a Pennes form on the same space for scale
(linear-form section).  One MI355X; prints one JSON line.

Usage: python profiles/lform_assemble_time.py [n = 108] [order = 2] [reps = 20]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
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
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 108
    order = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    E = _load_pkg()
    E.load_library()
    mesh = E.Mesh.MakeCartesian3D(n, n, n)
    fes = E.H1Space(mesh, order, E.NUMBERING_STRUCTURED)
    X = fes.dof_coords()
    phi = torch.as_tensor(np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1]) + 0.7 * X[:, 2] * X[:, 0]).cuda()
    T = torch.as_tensor(37.0 + 20.0 * np.exp(-10.0 * ((X - 0.3) ** 2).sum(1))).cuda()
    del X
    lf = E.LinearForm(fes)
    lf.AddDomainIntegrator(E.DomainLFIntegrator(E.JouleHeatingCoefficient(phi, 0.6, 0.015, 37.0, T)))
    b = torch.empty(fes.ndofs, dtype=torch.float64, device="cuda")
    asm_ms = timed(lambda: lf.Assemble(b), reps)
    assert bool(torch.isfinite(b).all()) and float(b.min()) >= 0.0

    # the Pennes stage operator on the same space: Mass(rho c) + Diffusion(c dt k(T))
    form = E.BilinearForm(fes)
    form.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(3.6e6)))
    form.AddDomainIntegrator(E.DiffusionIntegrator(E.AffineGridFunctionCoefficient(T, 0.5, 0.0012, 37.0)))
    form.Assemble()
    x = torch.empty_like(b).uniform_(-1.0, 1.0)
    y = torch.empty_like(b)
    mult_ms = timed(lambda: form.Mult(x, y), reps)

    # this run's STREAM rates (the library's 16-byte nontemporal kernels, as bench.py --full)
    a = torch.empty((1 << 30) // 8, dtype=torch.float64, device="cuda").uniform_()
    c = torch.empty_like(a)
    copy_ms = timed(lambda: E.stream_copy(a, c), reps)
    del c
    out = torch.empty(256 * 64 * 256, dtype=torch.float64, device="cuda")
    read_ms = timed(lambda: E.stream_read(a, out), reps)
    copy_gbs, read_gbs = 2.0 * (1 << 30) / copy_ms / 1e6, (1 << 30) / read_ms / 1e6

    ne, nd, ndofs = fes.ne, fes.nd, fes.ndofs
    parts = {"fields (phi, T), once": 16 * ndofs, "gather map": 4 * ne * nd, "corners": 192 * ne,
             "E-vector write + read": 16 * ne * nd, "CSR offsets + indices": 4 * (ndofs + 1) + 4 * ne * nd,
             "b": 8 * ndofs}
    nbytes = sum(parts.values())
    res = {"elements": ne, "order": order, "ndofs": ndofs, "q1d": lf.info()["q1d"], "assemble_ms": round(asm_ms, 4),
           "mult_ms": round(mult_ms, 4), "assemble_over_mult": round(asm_ms / mult_ms, 2),
           "bytes": nbytes, "bytes_parts": parts, "achieved_gbs": round(nbytes / asm_ms / 1e6, 1),
           "stream_copy_gbs": round(copy_gbs, 1), "stream_read_gbs": round(read_gbs, 1),
           "frac_of_stream": round(nbytes / asm_ms / 1e6 / max(copy_gbs, read_gbs), 3),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
