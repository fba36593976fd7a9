"""GPU: the one pair of transfer kernel templates (csrc/k_transfer.hip, k_prolong / k_restrict over both kinds)
computes, bit for bit, what the separate p- and h-refinement kernels computed.

The templates perform the same floating-point additions in the same order -- per output entry the x sum, the y
sum, the z sum, each ascending from 0.0, then the children in ascending octant order, then the transposed-map sum
-- so the comparison is of bytes: tests/golden/transfer_digests.json holds the SHA-256 of the float64 bytes of
Mult's and MultTranspose's result of every case, recorded by tests/record_transfer_digests.py (which also defines the
cases and refuses a case whose two runs differ) from the build of the commit before the change.  If a digest
differs the arithmetic order changed: the file is not to be recorded again from the code under test."""
import json

import pytest

import helpers  # noqa: F401
import ecm2_amd as E
import record_transfer_digests as R

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
def test_transfer_bitwise(digests, cid):
    got = R.run_case(E, torch, cid)
    print(cid, got)
    assert got == digests[cid], "differs from the recorded bytes"
