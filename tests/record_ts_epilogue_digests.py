"""The cases of tests/test_gpu_ts_epilogue_bitwise.py and the recorder of their digests.

    python3 tests/record_ts_epilogue_digests.py [out.json]

runs every case on cuda:0 through the public Python API and writes the SHA-256 of the float64 bytes
of each result (default: tests/golden/ts_epilogue_digests.json).  The committed file was recorded from
the build of the commit before the snapshot kernel k_apply_tpe_ts got its lattice epilogue (DPP face
merges, branch-free store): that commit's Mult is the reference the kernel must reproduce bit for bit.

Inputs use no libm function (the host's sin / exp cannot matter): x and b are uniform draws, the
coefficients polynomials of the coordinates.  Meshes (p = 2), the smallest that reach each path of the
epilogue: 4x4x4 one brick, three idle waves; 8x8x4 one workgroup, x and y across waves; 4x4x8 and 8x8x8
z across waves and across workgroups (partial slots); 12x12x12 27 bricks, the last workgroup with 3 of 4
waves on.  Numberings: structured (regular blocks, RM 1) and the reference's entity numbering
(lattice-map blocks, RM 3).  Forms: the benchmark's bioheat form (mass per point, MM 1), ex16 (mass per
element, MM 2), Pennes (MM 2 and the laws at the point), diffusion alone (MM 0), bioheat on a sheared
affine mesh (the general flux product)."""
import hashlib
import json
import os
import sys

import numpy as np

MESHES = [(4, 4, 4), (8, 8, 4), (4, 4, 8), (8, 8, 8), (12, 12, 12)]
NUMBERINGS = ["structured", "entity"]
FORMS = ["bioheat", "ex16", "pennes", "diffusion", "bioheat_sheared"]
# form -> SnapshotInfo() (snapshot, mass values, laws at the point), FluxDiagonal()
EXPECT = {"bioheat": ((True, 1, False), True), "ex16": ((True, 2, False), True), "pennes": ((True, 2, True), True),
          "diffusion": ((True, 0, False), True), "bioheat_sheared": ((True, 1, False), False)}
PERFUSION = (3.6e6, 0.05 * 3.6e3, 6.4e-3, 0.02, 37.0, 50.0)
K_LAW = (0.05, 0.0012, 37.0)
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ts_epilogue_digests.json")


def case_id(mesh, numbering, form):
    return "%dx%dx%d-%s-%s" % (mesh + (numbering, form))


def all_cases():
    return [(m, n, f) for m in MESHES for n in NUMBERINGS for f in FORMS]


def alpha_poly(P):
    return 3.6e6 * (1.0 + 0.1 * P[..., 0] * (1.0 - P[..., 0]) + 0.05 * P[..., 1] * P[..., 2])


def temperature_poly(X):
    return 37.0 + 20.0 * (X[:, 0] * X[:, 1] + X[:, 2] * X[:, 2])


def sha(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return hashlib.sha256(a.tobytes()).hexdigest()


def build_form(E, torch, mesh_n, numbering, form):
    """The assembled form of a case, with the snapshot kernel asserted: (fes, form, tensors to keep)."""
    nx, ny, nz = mesh_n
    entity = numbering == "entity"
    mesh = E.Mesh.MakeCartesian3D(nx, ny, nz, 1.0, ny / nx, nz / nx, sfc_ordering=entity)
    if form == "bioheat_sheared":
        V = mesh.vertices()
        V[:, 0] += 0.25 * V[:, 1]
        mesh.set_vertices(V)
    fes = E.H1Space(mesh, 2, E.NUMBERING_ENTITY if entity else E.NUMBERING_STRUCTURED)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    T = dev(temperature_poly(fes.dof_coords()))
    keep = [T]
    f = E.BilinearForm(fes, element_order="faces" if entity else "auto")
    if form in ("bioheat", "bioheat_sheared"):
        a = dev(alpha_poly(mesh.quadrature_points(4)).reshape(fes.ne, -1))
        keep.append(a)
        f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(a)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.AffineGridFunctionCoefficient(T, *K_LAW)))
    elif form == "ex16":
        ua = 0.05 * (0.5 + 0.01 * T)
        keep.append(ua)
        f.AddDomainIntegrator(E.MassIntegrator(E.ConstantCoefficient(1.0)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.GridFunctionCoefficient(ua)))
    elif form == "pennes":
        f.AddDomainIntegrator(E.MassIntegrator(E.PerfusionCoefficient(T, *PERFUSION)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.AffineGridFunctionCoefficient(T, *K_LAW)))
    else:
        assert form == "diffusion", form
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.AffineGridFunctionCoefficient(T, *K_LAW)))
    f.Assemble()
    # the snapshot kernel ran, on the block class of the numbering, writing partial slots' plan
    info = f.info()
    nblk = fes.ne // 64
    assert info["kernel"] == E.KERNEL_TPE and info["layout"] == E.QLAYOUT_AFFINE, info
    assert f.CoefficientSnapshot() and f.SnapshotInfo() == EXPECT[form][0], f.SnapshotInfo()
    assert f.FluxDiagonal() == EXPECT[form][1]
    lat, units, _ = f.AddressingInfo()
    lslot, _ = f.PlanInfo()
    assert units == nblk and (lslot == nblk and lat == 0 if entity else lat == nblk), (lat, units, lslot)
    assert f.EnergyParts() == (nblk + 3) // 4   # PCG folds its (A d, d) into the Mult: the kernel's energy path
    return fes, f, keep


def run_case(E, torch, mesh_n, numbering, form):
    """{"mult", "pcg_x", "pcg_norm"} digests of a case; the repeat and the zero-vector checks are asserted
    here (they need no recorded value)."""
    fes, f, keep = build_form(E, torch, mesh_n, numbering, form)
    n = fes.ndofs
    seed = 1000 * MESHES.index(mesh_n) + 10 * FORMS.index(form) + NUMBERINGS.index(numbering)
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(rng.uniform(-1, 1, n)).cuda()
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    f.Mult(x, y)
    y2 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    f.Mult(x, y2)
    torch.cuda.synchronize()
    yh, y2h = y.cpu().numpy(), y2.cpu().numpy()
    assert yh.tobytes() == y2h.tobytes(), "two Mults of one x differ"
    z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    f.Mult(torch.zeros(n, dtype=torch.float64, device="cuda"), z)
    torch.cuda.synchronize()
    assert z.cpu().numpy().tobytes() == bytes(8 * n), "A 0 is not all +0.0"
    b = torch.as_tensor(rng.uniform(-1, 1, n)).cuda()
    ess = torch.as_tensor(fes.boundary_dofs()).to(device="cuda", dtype=torch.int32)
    xs = torch.empty(n, dtype=torch.float64, device="cuda")
    it, nrm = f.PCG(b, xs, ess=ess, rel_tol=0.0, max_iter=5, jacobi=True)
    torch.cuda.synchronize()
    assert it == 5, it
    return {"mult": sha(yh), "pcg_x": sha(xs.cpu().numpy()), "pcg_norm": float(nrm).hex()}


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import helpers  # noqa: F401  (registers the package as ecm2_amd)
    import torch
    import ecm2_amd as E
    E.load_library()
    out = argv[1] if len(argv) > 1 else DIGESTS
    digests = {}
    for m, nb, fm in all_cases():
        digests[case_id(m, nb, fm)] = run_case(E, torch, m, nb, fm)
        print(case_id(m, nb, fm), digests[case_id(m, nb, fm)]["mult"][:16], flush=True)
    with open(out, "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main(sys.argv)
