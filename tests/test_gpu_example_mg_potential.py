"""GPU test of examples/mg_potential.cpp (the C ABI alone): the RF potential problem at p = 4 solved with Jacobi-PCG,
with the Chebyshev-preconditioned PCG and with the PCG preconditioned by the 1 -> 2 -> 4 V-cycle with ex26's settings
-- exit status 0 (all converged, the solutions agree, the manufactured solution is met, V-cycle < Chebyshev <
Jacobi in iterations) and the three iteration counts printed."""
import os
import re
import subprocess

import pytest

import helpers

pytestmark = pytest.mark.gpu


def test_example_mg_potential_on_gpu():
    examples = os.path.join(helpers.ROOT, "examples")
    binary = os.path.join(examples, "mg_potential")
    if not os.access(binary, os.X_OK):
        subprocess.run(["make", "-s", "-C", examples], check=True, timeout=300)
    r = subprocess.run([binary], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = [re.search(rf"{k}-PCG iterations: (\d+)", r.stdout) for k in ("Jacobi", "Chebyshev", "V-cycle")]
    assert all(counts)
    jac, cheb, mg = (int(c.group(1)) for c in counts)
    assert 0 < mg < cheb < jac
    assert r.stdout.rstrip().endswith("PASS")
