"""GPU: the device PCG and the device BiCGSTAB on their shared loop driver, control struct, partial sums and
workspace (csrc/solvers.cpp SolverWork / LoopDriver, csrc/dev_common.hpp loop_set_done / park_partial /
sum_partials_fixed) compute, bit for bit, what they computed as two separate copies of that protocol.

The shared pieces perform the same floating-point additions in the same order, so the comparison is of
bytes: tests/golden/solver_digests.json holds the SHA-256 of the float64 bytes of every case's x (or u) with
the exact iteration count, final norm and converged flag, recorded by tests/record_solver_digests.py (which
also defines the cases, asserts which path ran, and refuses a case whose two runs differ) from the build of
the commit before the change.  One setup is left out as not deterministic (p = 3 with Jacobi: the line kernel's
diagonal is summed by atomic adds; the recorder's docstring has the evidence); p = 3 runs without a
preconditioner.  The sequence test runs solves of both methods and of different sizes one after
the other in this process, on the workspace they share: each equals the digest of the same solve alone, the
repeat equals the first."""
import json

import pytest

import ecm2_amd as E
import record_solver_digests as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    E.load_library()
    yield
    torch.cuda.synchronize()
    R._CACHE.clear()


@pytest.fixture(scope="module")
def digests():
    with open(R.DIGESTS) as fh:
        return json.load(fh)


def test_every_case_has_a_digest(digests):
    assert sorted(digests) == sorted(R.all_cases())


@pytest.mark.parametrize("cid", R.all_cases())
def test_solver_bitwise(digests, cid):
    got = R.run_case(E, torch, cid)
    print(cid, got)
    assert got == digests[cid], "differs from the recorded bytes"


def test_sequence_on_the_shared_workspace(digests):
    got = R.run_sequence(E, torch)
    for cid, g in zip(R.SEQUENCE, got):
        print(cid, g)
        assert g == digests[cid], cid + " in the sequence differs from the same solve alone"
    assert got[0] == got[-1]


# The PCG with a Chebyshev smoother and with a multigrid cycle on the one CGSolver loop they share with the Jacobi
# PCG (csrc/solvers.cpp pcg_loop): tests/golden/solver_prec_digests.json, recorded by the same recorder (--prec)
# from the build of the last commit in which the three were separate copies of that loop.
@pytest.fixture(scope="module")
def prec_digests():
    with open(R.DIGESTS_PREC) as fh:
        return json.load(fh)


def test_every_prec_case_has_a_digest(prec_digests):
    assert sorted(prec_digests) == sorted(R.prec_cases())


@pytest.mark.parametrize("cid", R.prec_cases())
def test_prec_solver_bitwise(prec_digests, cid):
    got = R.run_case(E, torch, cid)
    print(cid, got)
    assert got == prec_digests[cid], "differs from the recorded bytes"


def test_prec_sequence_on_the_shared_workspace(digests, prec_digests):
    """A nested solve (the cycle's coarse PCG), a depth-0 Jacobi solve, a preconditioned one and a BiCGSTAB."""
    alone = dict(digests, **prec_digests)
    got = R.run_sequence(E, torch, R.PREC_SEQUENCE)
    for cid, g in zip(R.PREC_SEQUENCE, got):
        print(cid, g)
        assert g == alone[cid], cid + " in the sequence differs from the same solve alone"
    assert got[0] == got[-1]


# What the shapes above cannot reach in the 16-byte vector passes (a second trip round a grid-stride loop, full flat
# workgroups): tests/golden/solver_sweep_digests.json, one fixed-work solve per method at 558,009 dofs, recorded by the
# same recorder (--sweep) from the build of the last commit in which every pass had a pair body and a scalar copy of it.
@pytest.fixture(scope="module")
def sweep_digests():
    with open(R.DIGESTS_SWEEP) as fh:
        return json.load(fh)


def test_every_sweep_case_has_a_digest(sweep_digests):
    assert sorted(sweep_digests) == sorted(R.sweep_cases())


@pytest.mark.parametrize("cid", R.sweep_cases())
def test_sweep_solver_bitwise(sweep_digests, cid):
    got = R.run_case(E, torch, cid)
    print(cid, got)
    assert got == sweep_digests[cid], "differs from the recorded bytes"
