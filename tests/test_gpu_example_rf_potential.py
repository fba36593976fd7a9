"""GPU test of examples/rf_potential.cpp (the C ABI alone): the RF potential problem solved with Jacobi-PCG and
with the Chebyshev-preconditioned PCG -- exit status 0 (both converged, the solutions agree, the manufactured
solution is met, the smoother saves a quarter of the iterations) and both iteration counts printed."""
import os
import re
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu


def test_example_rf_potential_on_gpu():
    examples = os.path.join(helpers.ROOT, "examples")
    binary = os.path.join(examples, "rf_potential")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    jac = re.search(r"Jacobi-PCG iterations: (\d+)", r.stdout)
    cheb = re.search(r"Chebyshev-PCG iterations: (\d+)", r.stdout)
    assert jac and cheb
    assert 0 < int(cheb.group(1)) <= 0.75 * int(jac.group(1))
    assert r.stdout.rstrip().endswith("PASS")
