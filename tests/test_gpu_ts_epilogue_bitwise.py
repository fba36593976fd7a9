"""GPU: the snapshot kernel k_apply_tpe_ts with the lattice epilogue (DPP face merges, one wait for the
z permutes, a branch-free partial-slot store; csrc/k_tpe.hip tpe_assemble_store_lattice) writes, bit for
bit, what the kernel wrote with the generic epilogue.

The epilogue performs the same floating-point additions in the same order, so the comparison is of
bytes, not of norms: tests/golden/ts_epilogue_digests.json holds the SHA-256 of the float64 bytes of
every case's results, recorded by tests/record_ts_epilogue_digests.py (which also defines the cases and
asserts, through info() / SnapshotInfo() / AddressingInfo() / PlanInfo() / EnergyParts(), that the
snapshot kernel on the intended block class is what ran) from the build of the commit before the
change.  Per case: the Mult; the energy path -- x and the final norm of a 5-iteration Jacobi-PCG, whose
(A d, d) the kernel folds into the Mult; two Mults of one x equal; A 0 all +0.0 bytes.  scatter =
atomic is left out: it keeps the generic epilogue and is not deterministic."""
import json

import pytest

import ecm2_amd as E
import record_ts_epilogue_digests as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    E.load_library()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def digests():
    with open(R.DIGESTS) as fh:
        return json.load(fh)


def test_every_case_has_a_digest(digests):
    assert sorted(digests) == sorted(R.case_id(*c) for c in R.all_cases())


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("numbering", R.NUMBERINGS)
@pytest.mark.parametrize("mesh", R.MESHES, ids=lambda m: "%dx%dx%d" % m)
def test_snapshot_kernel_bitwise(digests, mesh, numbering, form):
    got = R.run_case(E, torch, mesh, numbering, form)
    want = digests[R.case_id(mesh, numbering, form)]
    print(R.case_id(mesh, numbering, form), got)
    assert got["mult"] == want["mult"], "Mult differs from the recorded bytes"
    assert got["pcg_x"] == want["pcg_x"], "x after 5 PCG iterations differs from the recorded bytes"
    assert got["pcg_norm"] == want["pcg_norm"], "final PCG norm differs"
