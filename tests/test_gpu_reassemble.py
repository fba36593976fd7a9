"""Re-assembly of one BilinearForm after its setters: the lifetime of the fused kernels' scatter plans.

One serial form is walked through SetCoefficientSnapshot / SetGeometryCompression / SetKernel and
re-assembled after each; every assembly must be the operator of the oracle and, on the fused
partial-scatter kernels (deterministic), bit for bit the operator of a fresh form constructed with
the same settings -- a plan, a launch argument or a qdata layout left over from the previous assembly
would show as a difference.  Shapes: the smallest at which the plans differ in kind.

The p >= 3 forms' AssembleDiagonal is not one of those kernels: kern::diagonal adds element
contributions with FP64 atomics, so two forms' diagonals differ in the last bits (on the line-kernel
case the walked and the fresh form already differed at step 1 with the library as it was before the
plan objects).  Their diagonals are compared at RTOL; their Mult, and everything at p = 2, bit for bit.
"""
import numpy as np
import pytest

import ecm2_amd as E
import oracle as O
from helpers import RTOL, alpha_bioheat, relerr, temperature

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    E.load_library()
    yield
    torch.cuda.synchronize()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=torch.float64)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


# (mesh, numbering, element order, p, kernel of the default assembly)
CASES = {
    # 8 blocks in two workgroups, every block regular: the snapshot kernel at step 1
    "p2_regular": ((8, 8, 8), E.NUMBERING_STRUCTURED, "auto", 2, E.KERNEL_TPE),
    # 120 elements: a partial last block, a derived element order, map-addressed blocks
    "p2_entity_faces": ((6, 5, 4), E.NUMBERING_ENTITY, "faces", 2, E.KERNEL_TPE),
    # 32 elements in eight 2 x 2 x 1 bricks
    "p4_bricks": ((4, 4, 2), E.NUMBERING_STRUCTURED, "auto", 4, E.KERNEL_LINE),
}

# the walk: (kernel, geometry compression, coefficient snapshot) of each assembly
STEPS = [
    (E.KERNEL_AUTO, True, True),
    (E.KERNEL_AUTO, True, False),
    (E.KERNEL_AUTO, False, False),   # another qdata layout kind: the thread-per-element plan is rebuilt
    (E.KERNEL_WPE, False, False),
    (E.KERNEL_AUTO, True, True),
]
SCALE, SLOPE, TREF = 0.05, 0.0012, 37.0


def _state(form):
    return form.info(), form.CoefficientSnapshot(), form.ScatterInfo(), form.AddressingInfo(), form.BrickInfo()


@pytest.mark.parametrize("case", list(CASES))
def test_reassemble_walk(case):
    dims, numbering, eo, order, kernel0 = CASES[case]
    mesh = E.Mesh.MakeCartesian3D(*dims, 1.0, 0.7, 1.3)
    fes = E.H1Space(mesh, order, numbering)
    en = mesh.element_nodes()
    q1d = O.default_q1d(order)
    T = temperature(fes.dof_coords())
    Td = dev(T)
    a = alpha_bioheat(O.quad_points(en, q1d))
    ad = dev(a.reshape(fes.ne, -1))
    beta = SCALE * (1.0 + SLOPE * (O.interp_evector(T[fes.gather_map()], order, q1d) - TREF))
    op = O.OracleOperator(en, fes.gather_map(), fes.ndofs, order, alpha=a, beta=beta)
    x = np.random.default_rng(23).uniform(-1, 1, fes.ndofs)
    xd = dev(x)
    y_ref, d_ref = op.mult(x), op.diagonal()

    def integrators(f):
        f.AddDomainIntegrator(E.MassIntegrator(E.QuadratureCoefficient(ad)))
        f.AddDomainIntegrator(E.DiffusionIntegrator(E.AffineGridFunctionCoefficient(Td, SCALE, SLOPE, TREF)))

    def outputs(f):
        y = torch.full((fes.ndofs,), float("nan"), dtype=torch.float64, device="cuda")
        d = torch.full_like(y, float("nan"))
        f.Mult(xd, y)
        f.AssembleDiagonal(d)
        return y, d

    form = E.BilinearForm(fes, element_order=eo)
    integrators(form)
    prev = STEPS[0]
    ys = []
    for i, step in enumerate(STEPS):
        kernel, compress, snap = step
        if snap != prev[2]:
            form.SetCoefficientSnapshot(snap)
        if compress != prev[1]:
            form.SetGeometryCompression(compress)
        if kernel != prev[0]:
            form.SetKernel(kernel)
        prev = step
        form.Assemble()
        y, d = outputs(form)
        ys.append(y)
        ey, ed = relerr(host(y), y_ref), relerr(host(d), d_ref)
        print(f"{case} step {i + 1}: kernel {form.info()['kernel']} layout {form.info()['layout']} "
              f"snapshot {form.CoefficientSnapshot()} mult {ey:.2e} diagonal {ed:.2e}")
        assert ey <= RTOL
        assert ed < 1e-13
        if case == "p2_regular":
            assert form.CoefficientSnapshot() == snap
        if kernel == E.KERNEL_AUTO:
            assert form.info()["kernel"] == kernel0
            fresh = E.BilinearForm(fes, kernel=kernel, element_order=eo, compress_geometry=compress,
                                   coefficient_snapshot=snap)
            integrators(fresh)
            fresh.Assemble()
            assert _state(form) == _state(fresh)
            yf, df = outputs(fresh)
            assert torch.equal(y, yf)
            if kernel0 == E.KERNEL_TPE:
                assert torch.equal(d, df)
            else:  # atomics in the diagonal (see above)
                assert relerr(host(d), host(df)) <= RTOL
        else:
            assert form.info()["kernel"] == E.KERNEL_WPE
    assert torch.equal(ys[4], ys[0])
    # a setter leaves the form unassembled
    form.SetKernel(E.KERNEL_AUTO)
    with pytest.raises(E.ECM2Error):
        form.Mult(xd, ys[0])
